// ctcx_targets.hip — the CTC log-likelihood log p(y | x) of targets the caller
// supplies (include/ctcext.h, "Target scores"): the forward recursion of the
// path scores over many short label rows per item, a packed trellis.  A
// translation unit of its own: the decode objects neither see nor depend on it.
//
// Work split (ctcx_target_scores<T, Fmt, G, Staged>).  A target of m labels
// lives in a segment of G lanes, G the smallest of 8, 16, 32, 64 with
// max_target + 1 slots: slot j < m holds the pair (blank state 2j, label state
// 2j + 1) in two registers, slot m the final blank, the slots above idle with
// -inf.  A wave holds 64 / G targets; a workgroup of 256 threads holds 256 / G
// consecutive targets of ONE item, so the item's frame count bounds the time
// loop of every lane alike and the barriers below are uniform.  The grid is
// batch * ceil(n_targets / (256 / G)); a segment past n_targets runs empty and
// writes nothing.
//
// Neighbour exchange.  A slot needs one foreign value a frame: the label state
// of the slot in front, of the frame before.  One DPP wave_shr:1 moves it (two
// for a double) in all lanes at once; a segment's head lane drops what crossed
// the segment border for -inf.  The head's blank state starts at 0 ("frame
// -1"), which makes the first step the definition's alpha_0.  The s - 2
// permission (y[j] != y[j - 1]) is one flag per lane, set once.
//
// Logit movement, staged (Staged = true).  The workgroup stages tiles of F
// whole rows of its item into LDS (F = ctcx_targets_tile): element i of a tile
// is (frame i / C, class i % C), thread t moves elements t, t + 256, ..., so
// the global loads run along the class axis through the caller's strides and
// the LDS stores are conflict-free.  What is stored is lp = x - norm, the
// definition's one rounded subtraction, widened from the two-byte formats on
// the way.  Two buffers: the loads of tile k + 1 are issued before tile k is
// consumed and held in registers (eight floats or four doubles a thread), and
// stored behind it; one barrier per tile, none per frame.  A lane reads
// lp[f][label] and lp[f][blank] (a broadcast) from LDS: the logits leave HBM
// once per workgroup, not once per target.
//
// Logit movement, gathered (Staged = false): every lane reads its label's
// logit, the blank's and the normaliser from global memory, one frame ahead in
// registers, as ctcx_path_scores_reg does.  Segments, exchange and arithmetic
// are the same.
//
// Arithmetic: ctcx_lse.h's lse2 / lse3, the path-scores kernels' own.  Every
// kPathsRenorm frames a float32 segment takes the maximum of its finite states
// (a butterfly over its G lanes), subtracts it and adds it to a double that is
// uniform in the segment and goes back in at the end.  No band test: a state
// outside the band is -inf and stays so through the guarded sums.
//
// Nothing is trusted: frames are clamped to [0, Tmax]; a length outside
// [0, max_target] or a label outside [0, C) makes the target NaN before any
// logit is read with it; every logit read is frame f < frames <= Tmax of item
// b, class c < C.
#include "ctcx_targets.h"

#include "ctcx_lse.h"
#include "ctcx_paths.h"   // kPathsRenorm, kPathsIn*

namespace {

constexpr int kR = kPathsRenorm;
static_assert((kR & (kR - 1)) == 0, "the frame test below masks");
static_assert(kPathsInNative == 0 && kPathsInF16 == 1 && kPathsInBF16 == 2, "ctcx_lse.h spells the formats out");
static_assert(kTargetsTileBytes == kTargetsThreads * 32, "a thread moves 32 bytes of a tile");

// the maximum of v over the G lanes of the segment, in every lane of it
template <int G>
__device__ __forceinline__ float segment_max(float v) {
#pragma unroll
  for (int k = 1; k < G; k <<= 1) v = fmaxf(v, __shfl_xor(v, k, 64));
  return v;
}

template <typename T, int Fmt, int G, bool Staged>
__global__ __launch_bounds__(kTargetsThreads) void ctcx_target_scores(CtcxTargetsParams p) {
  constexpr int kPerWg = kTargetsThreads / G;            // targets of a workgroup
  constexpr int kMove = kTargetsTileBytes / (int)sizeof(T) / kTargetsThreads;   // tile elements a thread moves
  const int tid = threadIdx.x;
  const int j = tid & (G - 1);                           // the slot
  const int64_t nblk = (p.N + kPerWg - 1) / kPerWg;
  const int64_t b = blockIdx.x / nblk;                   // (uniform)
  const int64_t n = (blockIdx.x - b * nblk) * kPerWg + tid / G;
  const T NINF = ninf<T>();
  const int Tmax = (int)p.Tmax;
  int frames = p.frames[b];
  frames = frames < 0 ? 0 : frames > Tmax ? Tmax : frames;   // (uniform)
  const bool valid = n < p.N;

  // the target: its length, this slot's label and flag
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
    const uint64_t seg = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1)) << ((tid & 63) & ~(G - 1));
    nan = (__ballot(nan) & seg) != 0;
  }
  const bool has_label = !nan && j < m;
  const bool counts = valid && !nan && j <= m;   // the slots whose states a renormalisation looks at

  T aB = j == 0 ? (T)0 : NINF, aL = NINF;
  double shift = 0;   // what the renormalisations took out (uniform in the segment)
  auto step = [&](int f, T lpB, T lpL) {
    const T got = from_prev_lane(aL);   // (every lane: the DPP move is no place to diverge)
    const T pl = j == 0 ? NINF : got;
    const T oB = aB, oL = aL;
    aB = lse2(oB, pl) + lpB;
    aL = has_label ? lse3(oL, oB, skip ? pl : NINF) + lpL : NINF;
    if constexpr (sizeof(T) == 4) {
      if ((f & (kR - 1)) == kR - 1) {
        const float mine = counts ? fmaxf(finite_or_ninf(aB), finite_or_ninf(aL)) : NINF;
        const float top = segment_max<G>(mine);
        if (top > NINF) {
          aB -= top;
          aL -= top;
          shift += (double)top;
        }
      }
    }
  };

  const T* const nb = (const T*)p.norm + b;
  const uint32_t blank = (uint32_t)p.blank_index;
  if constexpr (Staged) {
    __shared__ T tile[2][kTargetsTileBytes / sizeof(T)];
    const int C = (int)p.C;
    const int F = ctcx_targets_tile(p.C, sizeof(T) == 8);   // >= kTargetsMinTile: the host chose this route
    const int cells = F * C;                               // <= kMove * kTargetsThreads
    // where this thread's elements of a tile lie: (frame in the tile, class)
    int fi[kMove], ci[kMove];
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

  // slot m holds the final blank, the slot in front of it the last label
  const T got = from_prev_lane(aL);
  if (valid && j == (nan ? 0 : m)) {
    T* const out = (T*)p.out + b * p.N + n;
    *out = nan ? (T)__builtin_nanf("") : (T)((double)lse2(aB, j == 0 ? NINF : got) + shift);
  }
}

template <typename T, int Fmt, int G>
hipError_t launch_segment(const CtcxTargetsParams& p, hipStream_t s) {
  const int64_t nblk = (p.N + kTargetsThreads / G - 1) / (kTargetsThreads / G);
  if (p.B * nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(p.B * nblk)), block(kTargetsThreads);
  if (p.staged) hipLaunchKernelGGL((ctcx_target_scores<T, Fmt, G, true>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((ctcx_target_scores<T, Fmt, G, false>), grid, block, 0, s, p);
  return hipGetLastError();
}

template <typename T, int Fmt>
hipError_t launch_all(const CtcxTargetsParams& p, hipStream_t s) {
  switch (ctcx_targets_segment(p.L)) {
    case 8: return launch_segment<T, Fmt, 8>(p, s);
    case 16: return launch_segment<T, Fmt, 16>(p, s);
    case 32: return launch_segment<T, Fmt, 32>(p, s);
    case 64: return launch_segment<T, Fmt, 64>(p, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

static_assert(ctcx_targets_segment(7) == 8 && ctcx_targets_segment(8) == 16 && ctcx_targets_segment(15) == 16 &&
                  ctcx_targets_segment(16) == 32 && ctcx_targets_segment(31) == 32 && ctcx_targets_segment(32) == 64 &&
                  ctcx_targets_segment(63) == 64 && ctcx_targets_segment(64) == 0,
              "a segment has a slot for the final blank");

hipError_t ctcx_launch_target_scores(const CtcxTargetsParams& p, hipStream_t s) {
  if (p.B <= 0 || p.N <= 0) return hipSuccess;
  if (p.Tmax < 0 || p.C <= 0 || p.C > 0x7fffffffLL || p.blank_index < 0 || p.blank_index >= p.C || !p.target_length ||
      (p.L > 0 && !p.targets) || !p.frames || !p.out || (p.Tmax > 0 && (!p.x || !p.norm)) ||
      (p.xfmt != kPathsInNative && (p.f64 || (p.xfmt != kPathsInF16 && p.xfmt != kPathsInBF16))) ||
      !ctcx_targets_segment(p.L) || (p.staged && !ctcx_targets_tile(p.C, p.f64)))
    return hipErrorInvalidValue;
  if (p.f64) return launch_all<double, kPathsInNative>(p, s);
  if (p.xfmt == kPathsInF16) return launch_all<float, kPathsInF16>(p, s);
  if (p.xfmt == kPathsInBF16) return launch_all<float, kPathsInBF16>(p, s);
  return launch_all<float, kPathsInNative>(p, s);
}

// (ctcx_prefix.hip's ctcx_prefix_tails is this kernel's twin: the same segments, exchange, staging and
// renormalisation, with two stores a frame.  A change of the recursion above belongs there as well.)
