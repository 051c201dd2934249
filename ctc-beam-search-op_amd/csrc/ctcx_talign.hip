// ctcx_talign.hip — the forced Viterbi alignment of targets the caller supplies
// (include/ctcext.h, "Target alignments"): the recursion of the path alignments
// over many short label rows per item, with the walk back, the token times and
// the token scores in the same kernel.  A translation unit of its own: the
// decode objects neither see nor depend on it.
//
// Work split (ctcx_target_align<T, Fmt, G, Staged>): that of ctcx_targets.hip.
// A target of m labels lives in a segment of G lanes (8, 16, 32 or 64): slot
// j < m holds the pair (blank state 2j, label state 2j + 1), slot m the final
// blank.  A workgroup of 256 threads holds 256 / G consecutive targets of ONE
// item, so the item's frame count bounds every loop of every lane alike.  One
// DPP wave_shr:1 a frame brings the label state of the slot in front.  The
// logits come through the double-buffered LDS tile of lp = x - norm (Staged)
// or are gathered lane by lane, one frame ahead.
//
// Forward.  Per state two strict compares, two selects and one add, in the
// definition's order; frame 0 is the definition's v_0, written, not computed.
// Nothing is renormalised: the values are the definition's, bit for bit.  A
// lane makes three decision bits a frame -- bit 0 for its blank state (0 stay,
// 1 from the label in front), bits 1..2 for its label state (0 stay, 1 from its
// blank, 2 the skip) -- shifts them into a register and stores one word per
// kTalignWordFrames frames at bp[workgroup][frame / 10][thread]: the workgroup's
// store is 1 KiB, coalesced.
//
// Walk back.  A lane reads back only words it stored itself, so program order
// is all the ordering there is: no second launch, no fence.  Slot m chooses the
// end state and the segment takes it from there; the state is uniform in the
// segment.  A step takes the owner lane's word (state >> 1) by a shuffle inside
// the segment, shifts the frame's bits out and subtracts the decision.  Each
// lane loads its word of the ten frames before while these ten are consumed.
// Slot j keeps start[j] and end[j] as the walk passes its label state, slot m
// counts the trailing blanks.  With an alignment row asked for, lane f mod G
// holds frame f's class, and the segment stores G consecutive frames at once.
//
// Scores.  Slot j adds lp[f][y[j]] over its span in frame order -- one rounded
// subtraction, one rounded add -- and keeps the minimum.  The spans of a target
// are disjoint: at most `frames` gathers per target.
//
// Nothing is trusted: frames are clamped to [0, Tmax]; a length outside
// [0, max_target] or a label outside [0, C) makes the target NaN before any
// logit is read with it; every logit read is frame f < frames <= Tmax of item
// b, class c < C; a shuffle's source is masked into the segment; every store
// goes to the target's own cells or the thread's own words.
#include "ctcx_talign.h"

#include "ctcx_lse.h"
#include "ctcx_paths.h"   // kPathsIn*

namespace {

static_assert(kPathsInNative == 0 && kPathsInF16 == 1 && kPathsInBF16 == 2, "ctcx_lse.h spells the formats out");
static_assert(kTargetsTileBytes == kTargetsThreads * 32, "a thread moves 32 bytes of a tile");
constexpr int kW = kTalignWordFrames;

template <typename T>
__device__ __forceinline__ T qnan() { return (T)__builtin_nanf(""); }

template <typename T, int Fmt, int G, bool Staged>
__global__ __launch_bounds__(kTargetsThreads) void ctcx_target_align(CtcxTalignParams q) {
  const CtcxTargetsParams& p = q.t;
  constexpr int kPerWg = kTargetsThreads / G;            // targets of a workgroup
  constexpr int kMove = kTargetsTileBytes / (int)sizeof(T) / kTargetsThreads;   // tile elements a thread moves
  const int tid = threadIdx.x;
  const int j = tid & (G - 1);                           // the slot
  const int seg0 = (tid & 63) & ~(G - 1);                // the segment's first lane in the wave
  const int64_t nblk = (p.N + kPerWg - 1) / kPerWg;
  const int64_t b = blockIdx.x / nblk;                   // (uniform)
  const int64_t n = (blockIdx.x - b * nblk) * kPerWg + tid / G;
  const T NINF = ninf<T>();
  const int Tmax = (int)p.Tmax;
  int frames = p.frames[b];
  frames = frames < 0 ? 0 : frames > Tmax ? Tmax : frames;   // (uniform)
  const bool valid = n < p.N;

  // the target: its length, this slot's label and flag (as ctcx_target_scores)
  bool nan = p.status && p.status[b] != 0;
  int m = 0;
  uint32_t lab = 0;
  bool skip = false;
  if (valid) {
    const int64_t ti = p.shared ? n : b * p.N + n;
    const int32_t len = p.target_length[ti];
    if (len < 0 || len > p.L) nan = true;
    m = nan ? 0 : len;
    if (j < m) {   // (L < G: slot j is element j of the row)
      int64_t v, u = -1;
      if (p.labels_i64) {
        const int64_t* const y = (const int64_t*)p.targets + ti * p.L;
        v = y[j];
        if (j > 0) u = y[j - 1];
      } else {
        const int32_t* const y = (const int32_t*)p.targets + ti * p.L;
        v = y[j];
        if (j > 0) u = y[j - 1];
      }
      const bool bad = v < 0 || v >= p.C;
      lab = bad ? 0u : (uint32_t)v;
      skip = j > 0 && v != u;
      nan |= bad;
    }
  }
  {   // one bad label or length makes the whole segment's target NaN
    const uint64_t seg = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1)) << seg0;
    nan = (__ballot(nan) & seg) != 0;
  }
  if (nan) m = 0;
  const bool live = valid && !nan && j <= m;   // the slots with a blank state
  const bool has_label = valid && !nan && j < m;

  // ---- forward
  const int64_t nwords = ctcx_talign_words(p.Tmax);
  uint32_t* const bp = q.bp + (size_t)blockIdx.x * (size_t)nwords * kTargetsThreads + tid;   // word k at bp[k * 256]
  T aB = j == 0 ? (T)0 : NINF, aL = NINF;   // ("frame -1": what frames == 0 ends with)
  uint32_t acc = 0;
  int shift = 0;
  auto step = [&](int f, T lpB, T lpL) {
    const T got = from_prev_lane(aL);   // (every lane: the DPP move is no place to diverge)
    const T pl = j == 0 ? NINF : got;
    const T oB = aB, oL = aL;
    if (f == 0) {   // (uniform) v_0
      aB = live && j == 0 ? lpB : NINF;
      aL = has_label && j == 0 ? lpL : NINF;
    } else {
      const bool b1 = pl > oB;
      const T bestB = b1 ? pl : oB;
      const bool l1 = oB > oL;
      const T mid = l1 ? oB : oL;
      const bool l2 = skip && pl > mid;
      const T bestL = l2 ? pl : mid;
      aB = live ? bestB + lpB : NINF;
      aL = has_label ? bestL + lpL : NINF;
      acc |= ((b1 ? 1u : 0u) | (l2 ? 4u : l1 ? 2u : 0u)) << shift;
    }
    shift += 3;
    if (shift == 3 * kW) {
      bp[(size_t)(f / kW) * kTargetsThreads] = acc;
      acc = 0;
      shift = 0;
    }
  };

  const T* const nb = (const T*)p.norm + b;
  const uint32_t blank = (uint32_t)p.blank_index;
  if constexpr (Staged) {
    __shared__ T tile[2][kTargetsTileBytes / sizeof(T)];
    const int C = (int)p.C;
    const int F = ctcx_targets_tile(p.C, sizeof(T) == 8);   // >= kTargetsMinTile: the host chose this route
    const int cells = F * C;                               // <= kMove * kTargetsThreads
    int fi[kMove], ci[kMove];   // where this thread's elements of a tile lie: (frame in the tile, class)
#pragma unroll
    for (int e = 0; e < kMove; ++e) {
      const int i = e * kTargetsThreads + tid;
      fi[e] = i < cells ? i / C : F;   // (F: no element)
      ci[e] = i < cells ? i - fi[e] * C : 0;
    }
    T hold[kMove];
    auto load = [&](int f0) {   // tile [f0, f0 + F) into registers, as lp
#pragma unroll
      for (int e = 0; e < kMove; ++e) {
        const int f = f0 + fi[e];
        hold[e] = (T)0;
        if (fi[e] < F && f < frames) {
          const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + b * p.xst_b);
          hold[e] = row_at<T, Fmt>(row, (uint32_t)ci[e]) - nb[(int64_t)f * p.B];
        }
      }
    };
    auto store = [&](int buf) {
#pragma unroll
      for (int e = 0; e < kMove; ++e) tile[buf][e * kTargetsThreads + tid] = hold[e];
    };
    if (frames > 0) {
      load(0);
      store(0);
    }
    __syncthreads();
    for (int f0 = 0, buf = 0; f0 < frames; f0 += F, buf ^= 1) {
      const bool more = f0 + F < frames;   // (uniform)
      if (more) load(f0 + F);
      const T* const t = tile[buf];
      const int nf = frames - f0 < F ? frames - f0 : F;
      for (int k = 0; k < nf; ++k) step(f0 + k, t[k * C + (int)blank], t[k * C + (int)lab]);
      if (more) store(buf ^ 1);
      __syncthreads();   // tile k is read, tile k + 1 is whole
    }
  } else {
    auto gather = [&](int f, T& v, T& vb, T& vn) {
      const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + b * p.xst_b);   // uniform
      v = row_at<T, Fmt>(row, lab);
      vb = row_at<T, Fmt>(row, blank);
      vn = nb[(int64_t)f * p.B];
    };
    T cur = (T)0, curB = (T)0, curN = (T)0;
    if (frames > 0) gather(0, cur, curB, curN);
    for (int f = 0; f < frames; ++f) {
      T nxt = cur, nxtB = curB, nxtN = curN;
      if (f + 1 < frames) gather(f + 1, nxt, nxtB, nxtN);
      step(f, curB - curN, cur - curN);
      cur = nxt;
      curB = nxtB;
      curN = nxtN;
    }
  }
  if (shift > 0) bp[(size_t)((frames - 1) / kW) * kTargetsThreads] = acc;   // (frames > 0) the last, partial word

  // ---- the end state: slot m holds the final blank, the slot in front of it the last label
  const T got = from_prev_lane(aL);
  int s = -1;   // the walk's state; -1: unaligned
  if (j == m) {
    T logp = aB;
    int end_state = 2 * m;
    if (m > 0 && got > aB) {
      logp = got;
      end_state = 2 * m - 1;
    }
    if (nan) logp = qnan<T>();
    if (logp > NINF) s = end_state;
    if (valid) {
      ((T*)p.out)[b * p.N + n] = logp;
      if (!(logp > NINF)) q.trailing_blank[b * p.N + n] = 0;
    }
  }
  s = __shfl(s, seg0 + m, 64);   // (m <= L < G)
  const bool aligned = valid && s >= 0;
  if (!aligned) s = -1;

  // ---- walk back
  int st = -1, en = -1, trail = 0, cls = -1;
  const bool want_ali = q.alignment != nullptr;   // (uniform)
  int32_t* const ali = want_ali && valid ? q.alignment + (b * p.N + n) * p.Tmax : nullptr;
  if (frames > 0) {
    int k = (frames - 1) / kW;
    uint32_t wnext = bp[(size_t)k * kTargetsThreads];
    for (; k >= 0; --k) {
      const uint32_t w = wnext;
      if (k > 0) wnext = bp[(size_t)(k - 1) * kTargetsThreads];
      const int hi = frames - 1 - k * kW < kW - 1 ? frames - 1 - k * kW : kW - 1;
      for (int r = hi; r >= 0; --r) {
        const int f = k * kW + r;
        const int owner = (s < 0 ? 0 : s >> 1) & (G - 1);
        const uint32_t word = (uint32_t)__shfl((int)w, seg0 + owner, 64);
        const bool odd = (s & 1) != 0;
        if (aligned) {
          if (odd && owner == j) {
            if (en < 0) en = f;
            st = f;
          }
          if (j == m && s == 2 * m) ++trail;
        }
        if (want_ali) {
          const int c = __shfl((int)lab, seg0 + owner, 64);
          if ((f & (G - 1)) == j) cls = !aligned ? -1 : odd ? c : (int)blank;
          if ((f & (G - 1)) == 0 && ali && f + j < frames) ali[f + j] = cls;
        }
        if (aligned && f > 0) {
          const uint32_t bits = word >> (3 * r);
          const int d = odd ? (int)((bits >> 1) & 3u) : (int)(bits & 1u);
          s = s - d < 0 ? 0 : s - d;
        }
      }
    }
  }
  if (ali)
    for (int64_t i = frames + j; i < p.Tmax; i += G) ali[i] = -1;

  // ---- the times, and the scores of each slot's span
  if (!valid) return;
  const int64_t cell = (b * p.N + n) * p.L + j;
  const bool timed = aligned && j < m && st >= 0 && st <= en && en < frames;
  if (j < p.L) {
    q.start[cell] = timed ? st : -1;
    q.end[cell] = timed ? en : -1;
  }
  if (aligned && j == m) q.trailing_blank[b * p.N + n] = trail;
  if (q.logp_sum || q.logp_min) {
    T sum = qnan<T>(), mn = qnan<T>();
    if (timed) {
      for (int f = st; f <= en; ++f) {
        const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + b * p.xst_b);
        const T lp = row_at<T, Fmt>(row, lab) - nb[(int64_t)f * p.B];
        if (f == st) {
          sum = mn = lp;
        } else {
          sum = sum + lp;
          if (lp < mn) mn = lp;
        }
      }
    }
    if (j < p.L) {
      if (q.logp_sum) ((T*)q.logp_sum)[cell] = sum;
      if (q.logp_min) ((T*)q.logp_min)[cell] = mn;
    }
  }
}

template <typename T, int Fmt, int G>
hipError_t launch_segment(const CtcxTalignParams& q, hipStream_t s) {
  const int64_t nblk = (q.t.N + kTargetsThreads / G - 1) / (kTargetsThreads / G);
  if (q.t.B * nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(q.t.B * nblk)), block(kTargetsThreads);
  if (q.t.staged) hipLaunchKernelGGL((ctcx_target_align<T, Fmt, G, true>), grid, block, 0, s, q);
  else hipLaunchKernelGGL((ctcx_target_align<T, Fmt, G, false>), grid, block, 0, s, q);
  return hipGetLastError();
}

template <typename T, int Fmt>
hipError_t launch_all(const CtcxTalignParams& q, hipStream_t s) {
  switch (ctcx_targets_segment(q.t.L)) {
    case 8: return launch_segment<T, Fmt, 8>(q, s);
    case 16: return launch_segment<T, Fmt, 16>(q, s);
    case 32: return launch_segment<T, Fmt, 32>(q, s);
    case 64: return launch_segment<T, Fmt, 64>(q, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

static_assert(ctcx_talign_bytes(1, 1, 7, 10) == 1024 && ctcx_talign_bytes(1, 33, 7, 11) == 2 * 2 * 1024 &&
                  ctcx_talign_bytes(2, 5, 63, 1) == 2 * 2 * 1024 && ctcx_talign_bytes(1, 1, 64, 1) == -1,
              "a workgroup stores 1 KiB per ten frames");

hipError_t ctcx_launch_target_align(const CtcxTalignParams& q, hipStream_t s) {
  const CtcxTargetsParams& p = q.t;
  if (p.B <= 0 || p.N <= 0) return hipSuccess;
  if (p.Tmax < 0 || p.Tmax > 0x7fffffffLL || p.C <= 0 || p.C > 0x7fffffffLL || p.blank_index < 0 ||
      p.blank_index >= p.C || !p.target_length || (p.L > 0 && !p.targets) || !p.frames || !p.out ||
      (p.Tmax > 0 && (!p.x || !p.norm || !q.bp)) || (p.L > 0 && (!q.start || !q.end)) || !q.trailing_blank ||
      (p.xfmt != kPathsInNative && (p.f64 || (p.xfmt != kPathsInF16 && p.xfmt != kPathsInBF16))) ||
      !ctcx_targets_segment(p.L) || (p.staged && !ctcx_targets_tile(p.C, p.f64)))
    return hipErrorInvalidValue;
  if (p.f64) return launch_all<double, kPathsInNative>(q, s);
  if (p.xfmt == kPathsInF16) return launch_all<float, kPathsInF16>(q, s);
  if (p.xfmt == kPathsInBF16) return launch_all<float, kPathsInBF16>(q, s);
  return launch_all<float, kPathsInNative>(q, s);
}
