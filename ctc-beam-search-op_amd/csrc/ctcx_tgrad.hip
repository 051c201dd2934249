// ctcx_tgrad.hip — CTC forward-backward over targets the caller supplies
// (include/ctcext.h, "Target gradients"): the scores log p(y_n | x) and the
// slab G[b] = sum_n w[b][n] * d log p(y_n | x) / d x[b], in one kernel.  A
// translation unit of its own: a twin of the packed trellis of
// ctcx_targets.hip, not an edit of it; ctcx_targets.o, ctcx_prefix.o and
// ctcx_talign.o are not touched by it.
//
// Work split (ctcx_target_grads<T, Fmt, G, Staged>).  As in the target scores a
// target of m labels lives in a segment of G lanes (8, 16, 32, 64), slot j < m
// the pair (blank state 2j, label state 2j + 1), slot m the final blank, and a
// workgroup of 256 threads holds 256 / G consecutive targets of ONE item.  The
// workgroup owns its targets over all frames, so forward, backward and the
// reduction over classes run in one launch with workgroup barriers only.  An
// item with more targets has several groups: one launch a group, in order on
// the stream, the grid one workgroup an item.  Group 0 stores every cell of the
// slab (zeros past the item's frames and for an item without a finite row), a
// later group reads, adds and writes.  No two workgroups in flight touch the
// same cell, there is no atomic, and every sum has a fixed order: the same
// bits on every run.
//
// 1. Forward with checkpoints.  Time runs in tiles of K frames
//    (ctcx_tgrad_tile: 16 for float32, 8 for float64, shorter where K staged
//    rows would not fit).  Before a tile every lane stores its pair and the
//    double the renormalisations took out to the workspace: two coalesced
//    stores of the compute dtype and one of a double a tile, 1 / K of what
//    storing every alpha would cost.  The arithmetic is the target scores':
//    lse2 / lse3 of ctcx_lse.h, one DPP wave_shr:1 a frame, float32
//    renormalised every kPathsRenorm frames -- which is a tile's last frame, so
//    all alpha of a tile are relative to the checkpoint's shift.
// 2. Backward by tiles, from the last tile down.  The tile's checkpoint is
//    reloaded and its K frames of alpha recomputed into two LDS planes
//    [K][257] (the last tile keeps them from the forward).  beta runs down the
//    tile with the mirrored move (wave_shl:1, twice: the next slot's blank and
//    label state), renormalised at frames f = 0 mod 16, a tile's first.  Each
//    alpha is overwritten with the lane's weighted occupancy in the
//    probability domain, w_n * exp(alpha + beta - lp - logp_n): the exponent is
//    summed in double with the three shifts, a state whose alpha + beta is
//    -inf gives exactly 0, and so does every state of a row without a finite
//    score.
// 3. Class-major reduce per tile.  Once per workgroup a prologue builds in LDS
//    the list of the distinct classes among the label states (the lanes that
//    hold a class first, compacted by ballot) and for every lane the next lane
//    with the same class.  After the beta sweep the 256 threads are K frames
//    by 256 / K slices: a thread walks the chains of its slice's classes for
//    its frame in lane order.  The blank column sums all 256 blank states: a
//    slice sums K lanes, one thread a frame adds the slices in order.  The
//    term -W_g * exp(lp[f][c]) (W_g: the weights of the group's finite rows,
//    summed in segment order) covers all classes: staged, it replaces lp in the
//    row tile, the chains add into the tile and the tile leaves as coalesced
//    stores; gathered, it is a coalesced sweep of the row in place followed by
//    the sparse adds.
//
// Logit movement: staged (class counts of ctcx_targets_tile) the K rows of a
// tile pass through one LDS buffer as lp = x - norm, loaded along the class
// axis through the caller's strides; gathered, a lane holds its label's and the
// blank's lp of the tile's K frames in registers.  Both serve the recomputed
// forward and the beta sweep of a tile from one load.
//
// Nothing is trusted: frames are clamped to [0, Tmax]; lengths and labels are
// checked before a logit is read with them; every logit read and every slab
// cell is frame f < Tmax of item b < B, class c < C; every LDS index is below
// its array's extent by the bounds stated where it is formed.
#include "ctcx_tgrad.h"

#include "ctcx_lse.h"
#include "ctcx_paths.h"   // kPathsRenorm, kPathsIn*

namespace {

constexpr int kR = kPathsRenorm;
static_assert((kR & (kR - 1)) == 0 && kR % kTgradK32 == 0, "a tile holds at most one renormalisation, at its last frame");
static_assert(kPathsInNative == 0 && kPathsInF16 == 1 && kPathsInBF16 == 2, "ctcx_lse.h spells the formats out");
static_assert(kTargetsTileBytes == kTargetsThreads * 32, "a thread moves 32 bytes of a tile");
static_assert((kTgradK32 & (kTgradK32 - 1)) == 0 && (kTgradK64 & (kTgradK64 - 1)) == 0, "the reduce masks");

template <int G>
__device__ __forceinline__ float segment_max(float v) {
#pragma unroll
  for (int k = 1; k < G; k <<= 1) v = fmaxf(v, __shfl_xor(v, k, 64));
  return v;
}

// lane l receives lane l + 1's v, lane 63 -inf (wave_shl:1)
__device__ __forceinline__ float from_next_lane(float v) {
  return __int_as_float(dpp_keep<0x130>(__float_as_int(ninf<float>()), __float_as_int(v)));
}
__device__ __forceinline__ double from_next_lane(double v) {
  const double o = ninf<double>();
  return __hiloint2double(dpp_keep<0x130>(__double2hiint(o), __double2hiint(v)),
                          dpp_keep<0x130>(__double2loint(o), __double2loint(v)));
}

constexpr uint16_t kNoLane = 0xffff;

template <typename T, int Fmt, int G, bool Staged>
__global__ __launch_bounds__(kTargetsThreads) void ctcx_target_grads(CtcxTgradParams pp) {
  const CtcxTargetsParams& p = pp.t;
  constexpr int kThreads = kTargetsThreads;
  constexpr int kPerWg = kThreads / G;
  constexpr int KMAX = sizeof(T) == 8 ? kTgradK64 : kTgradK32;
  constexpr int kMove = kTargetsTileBytes / (int)sizeof(T) / kThreads;
  __shared__ T sA[2][KMAX * kTgradPlane];   // alpha, then the occupancies: [state][frame of the tile][lane]
  __shared__ T sTile[Staged ? kTargetsTileBytes / sizeof(T) : 1];
  __shared__ T sPart[kThreads];             // the blank column's partial sums: [frame][slice]
  __shared__ T sW[kPerWg];
  __shared__ int sLab[kThreads];            // a lane's class where its label state counts, or -1
  __shared__ uint16_t sNext[kThreads], sHeads[kThreads];
  __shared__ int sCnt[kThreads / 64];

  const int tid = threadIdx.x;
  const int j = tid & (G - 1);
  const int64_t b = blockIdx.x;                          // (uniform; b < B)
  const int64_t n = pp.group * kPerWg + tid / G;
  const T NINF = ninf<T>();
  const int Tmax = (int)p.Tmax;
  const int C = (int)p.C;
  int frames = p.frames[b];
  frames = frames < 0 ? 0 : frames > Tmax ? Tmax : frames;   // (uniform)
  const bool valid = n < p.N;
  const bool first = pp.group == 0;
  const int K = pp.tile;   // a power of two, <= ctcx_tgrad_tile <= KMAX: the launcher checked

  // the target: its length, this slot's label and flag (the target scores' prologue)
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
  {
    const uint64_t seg = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1)) << ((tid & 63) & ~(G - 1));
    nan = (__ballot(nan) & seg) != 0;
  }
  if (nan) m = 0;
  const bool has_label = !nan && j < m;
  const bool counts = valid && !nan && j <= m;
  // the s + 2 permission out of this slot's label state: the next slot's flag (j < m: slot j + 1 is the segment's)
  const bool skip_next = (__shfl_down((int)skip, 1, 64) != 0) && j < m;

  const T* const nb = (const T*)p.norm + b;
  const uint32_t blank = (uint32_t)p.blank_index;

  // the tile's logits: staged, element i of the tile is (frame i / C, class i % C), as the target scores stage it
  int fi[kMove], ci[kMove];
  if constexpr (Staged) {
    const int cells = K * C;   // <= kMove * kThreads: K <= ctcx_targets_tile
#pragma unroll
    for (int e = 0; e < kMove; ++e) {
      const int i = e * kThreads + tid;
      fi[e] = i < cells ? i / C : K;   // (K: no element)
      ci[e] = i < cells ? i - fi[e] * C : 0;
    }
  }
  T gB[KMAX], gL[KMAX];   // gathered: lp of the blank and of this slot's label, by frame of the tile
  auto tile_in = [&](int f0, int nf) {
    if constexpr (Staged) {
      __syncthreads();   // the tile before is read
#pragma unroll
      for (int e = 0; e < kMove; ++e) {
        const int f = f0 + fi[e];
        T v = (T)0;
        if (fi[e] < nf) {   // (f < frames)
          const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + b * p.xst_b);
          v = row_at<T, Fmt>(row, (uint32_t)ci[e]) - nb[(int64_t)f * p.B];
        }
        sTile[e * kThreads + tid] = v;
      }
      __syncthreads();
    } else {
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        gB[k] = gL[k] = (T)0;
        if (k < nf) {   // (f0 + k < frames)
          const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)(f0 + k) * p.xst_t + b * p.xst_b);
          const T nrm = nb[(int64_t)(f0 + k) * p.B];
          gB[k] = row_at<T, Fmt>(row, blank) - nrm;
          gL[k] = row_at<T, Fmt>(row, lab) - nrm;
        }
      }
    }
  };
  auto lp_at = [&](int k, T& lpB, T& lpL) {   // (k < nf <= K)
    if constexpr (Staged) {
      lpB = sTile[k * C + (int)blank];
      lpL = sTile[k * C + (int)lab];
    } else {
      lpB = gB[k];
      lpL = gL[k];
    }
  };

  // the checkpoints of this item: record k holds the pairs before frame k * K
  const int64_t nck = ((int64_t)Tmax + K - 1) / K;
  T* const ck = (T*)pp.ws + b * nck * 2 * kThreads + tid;
  double* const cks = (double*)((char*)pp.ws + p.B * nck * 2 * kThreads * sizeof(T)) + b * nck * kThreads + tid;

  T aB = j == 0 ? (T)0 : NINF, aL = NINF;
  double shift = 0, shift0 = 0;   // what the renormalisations took out; shift0: at the head of the running tile
  auto alpha_tile = [&](int f0, int nf, bool keep) {
    shift0 = shift;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < nf) {   // (uniform)
        T lpB, lpL;
        lp_at(k, lpB, lpL);
        const T got = from_prev_lane(aL);
        const T pl = j == 0 ? NINF : got;
        const T oB = aB, oL = aL;
        aB = lse2(oB, pl) + lpB;
        aL = has_label ? lse3(oL, oB, skip ? pl : NINF) + lpL : NINF;
        if (keep) {   // (k < KMAX: below the plane's KMAX * 257)
          sA[0][k * kTgradPlane + tid] = aB;
          sA[1][k * kTgradPlane + tid] = aL;
        }
        if constexpr (sizeof(T) == 4) {
          if (((f0 + k) & (kR - 1)) == kR - 1) {
            const float mine = counts ? fmaxf(finite_or_ninf(aB), finite_or_ninf(aL)) : NINF;
            const float top = segment_max<G>(mine);
            if (top > NINF) {
              aB -= top;
              aL -= top;
              shift += (double)top;
            }
          }
        }
      }
    }
  };

  const int f0_last = frames > 0 ? (frames - 1) / K * K : 0;
  for (int f0 = 0; f0 < frames; f0 += K) {
    const int nf = frames - f0 < K ? frames - f0 : K;
    tile_in(f0, nf);
    if (f0 != f0_last) {   // (f0 / K < nck)
      const int64_t r = f0 / K;
      ck[(r * 2) * kThreads] = aB;
      ck[(r * 2 + 1) * kThreads] = aL;
      if constexpr (sizeof(T) == 4) cks[r * kThreads] = shift;
    }
    alpha_tile(f0, nf, f0 == f0_last);
  }

  // the score: slot m holds the final blank, the slot in front of it the last label
  const T got_end = from_prev_lane(aL);
  const double mine_end = (double)lse2(aB, j == 0 ? NINF : got_end) + shift;
  const double logp = __shfl(mine_end, ((tid & 63) & ~(G - 1)) + m, 64);   // (m <= L < G: a lane of the segment)
  if (valid && j == m) ((T*)p.out)[b * p.N + n] = nan ? (T)__builtin_nanf("") : (T)logp;
  if (pp.forward_only) return;

  const bool fin = valid && !nan && ab((T)logp) < -NINF;
  T w = (T)0;
  if (fin) w = pp.weights ? ((const T*)pp.weights)[b * p.N + n] : (T)1;
  if (j == 0) sW[tid / G] = w;
  const bool any = __syncthreads_or(fin) != 0;
  T* const gout = (T*)pp.grad + b * pp.ost_b;
  if (!any) {   // (uniform) nothing to add; group 0 still owns the cells
    if (first)
      for (int f = 0; f < Tmax; ++f)
        for (int c = tid; c < C; c += kThreads) gout[(int64_t)f * pp.ost_t + c] = (T)0;
    return;
  }
  T Wg = (T)0;
#pragma unroll
  for (int s = 0; s < kPerWg; ++s) Wg += sW[s];

  // the classes of the label states: who holds a class first, and every lane's next lane of the same class
  sLab[tid] = has_label && fin ? (int)lab : -1;
  __syncthreads();
  int nheads = 0;
  {
    const int mine = sLab[tid];
    bool head = mine >= 0;
    int nxt = kNoLane;
    if (mine >= 0) {
      for (int t = 0; t < tid; ++t) head &= sLab[t] != mine;
      for (int t = kThreads - 1; t > tid; --t) nxt = sLab[t] == mine ? t : nxt;
    }
    sNext[tid] = (uint16_t)nxt;
    const uint64_t bal = __ballot(head);
    if ((tid & 63) == 0) sCnt[tid >> 6] = __popcll(bal);
    __syncthreads();
    int rank = __popcll(bal & ((1ull << (tid & 63)) - 1));
#pragma unroll
    for (int v = 0; v < kThreads / 64; ++v) {
      if (v < (tid >> 6)) rank += sCnt[v];
      nheads += sCnt[v];
    }
    if (head) sHeads[rank] = (uint16_t)tid;   // (rank < nheads <= 256)
    __syncthreads();
  }

  // backward: beta of the frame behind the last is 0 in the final blank alone
  T bB = counts && j == m ? (T)0 : NINF, bL = NINF;
  double shift_b = 0;
  const int S = kThreads / K, fr = tid & (K - 1), sl = tid / K;   // the reduce: frame of the tile, slice
  for (int f0 = f0_last; frames > 0 && f0 >= 0; f0 -= K) {
    const int nf = frames - f0 < K ? frames - f0 : K;
    if (f0 != f0_last) {
      tile_in(f0, nf);
      const int64_t r = f0 / K;
      aB = ck[(r * 2) * kThreads];
      aL = ck[(r * 2 + 1) * kThreads];
      if constexpr (sizeof(T) == 4) shift = cks[r * kThreads];
      alpha_tile(f0, nf, true);
    }
    const double D = shift0 + shift_b - logp;
#pragma unroll
    for (int k = KMAX - 1; k >= 0; --k) {
      if (k < nf) {   // (uniform)
        T lpB, lpL;
        lp_at(k, lpB, lpL);
        T nB = from_next_lane(bB), nL = from_next_lane(bL);   // (every lane: the DPP move is no place to diverge)
        if (j >= m) nB = nL = NINF;
        const T oB = bB, oL = bL;
        bL = has_label ? lse3(oL, nB, skip_next ? nL : NINF) + lpL : NINF;
        bB = counts ? lse2(oB, oL) + lpB : NINF;
        T* const a0 = &sA[0][k * kTgradPlane + tid];
        T* const a1 = &sA[1][k * kTgradPlane + tid];
        T o0 = (T)0, o1 = (T)0;
        if (fin) {
          if (*a0 + bB > NINF) o0 = w * ex((T)((double)*a0 + (double)bB - (double)lpB + D));
          if (*a1 + bL > NINF) o1 = w * ex((T)((double)*a1 + (double)bL - (double)lpL + D));
        }
        *a0 = o0;
        *a1 = o1;
        if constexpr (sizeof(T) == 4) {
          if (((f0 + k) & (kR - 1)) == 0) {   // (k == 0: K divides kR)
            const float mine = counts ? fmaxf(finite_or_ninf(bB), finite_or_ninf(bL)) : NINF;
            const float top = segment_max<G>(mine);
            if (top > NINF) {
              bB -= top;
              bL -= top;
              shift_b += (double)top;
            }
          }
        }
      }
    }
    __syncthreads();   // the occupancies are whole

    // -W_g exp(lp) over all classes, and the blank column's partial sums
    if constexpr (Staged) {
#pragma unroll
      for (int e = 0; e < kMove; ++e)
        if (fi[e] < nf) sTile[e * kThreads + tid] = -Wg * ex(sTile[e * kThreads + tid]);
    } else {
      for (int k = 0; k < nf; ++k) {
        const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)(f0 + k) * p.xst_t + b * p.xst_b);
        const T nrm = nb[(int64_t)(f0 + k) * p.B];
        T* const o = gout + (int64_t)(f0 + k) * pp.ost_t;
        for (int c = tid; c < C; c += kThreads) {
          const T v = -Wg * ex(row_at<T, Fmt>(row, (uint32_t)c) - nrm);
          o[c] = first ? v : o[c] + v;
        }
      }
    }
    if (fr < nf) {   // (fr < K, sl * K + i < 256, fr * S + sl < 256)
      T s = (T)0;
      for (int i = 0; i < K; ++i) s += sA[0][fr * kTgradPlane + sl * K + i];
      sPart[fr * S + sl] = s;
    }
    __syncthreads();
    if (fr < nf) {
      for (int h = sl; h < nheads; h += S) {
        int t = sHeads[h];
        const int c = sLab[t];   // (a head's class: 0 <= c < C)
        T s = (T)0;
        do {
          s += sA[1][fr * kTgradPlane + t];
          t = sNext[t];
        } while (t != kNoLane);
        if constexpr (Staged) sTile[fr * C + c] += s;
        else gout[(int64_t)(f0 + fr) * pp.ost_t + c] += s;
      }
    }
    __syncthreads();
    if (tid < nf) {
      T s = (T)0;
      for (int v = 0; v < S; ++v) s += sPart[tid * S + v];
      if constexpr (Staged) sTile[tid * C + (int)blank] += s;
      else gout[(int64_t)(f0 + tid) * pp.ost_t + blank] += s;
    }
    __syncthreads();
    if constexpr (Staged) {
#pragma unroll
      for (int e = 0; e < kMove; ++e) {
        if (fi[e] < nf) {   // (f0 + fi < frames <= Tmax, ci < C)
          T* const o = gout + (int64_t)(f0 + fi[e]) * pp.ost_t + ci[e];
          const T v = sTile[e * kThreads + tid];
          *o = first ? v : *o + v;
        }
      }
    }
  }
  if (first)   // the frames past the item's length
    for (int f = frames; f < Tmax; ++f)
      for (int c = tid; c < C; c += kThreads) gout[(int64_t)f * pp.ost_t + c] = (T)0;
}

template <typename T, int Fmt, int G>
hipError_t launch_segment(CtcxTgradParams p, hipStream_t s) {
  int64_t groups = (p.t.N + kTargetsThreads / G - 1) / (kTargetsThreads / G);
  if (groups < 1) groups = 1;   // (no target: one launch, which zero-fills the slab)
  const dim3 grid((unsigned)p.t.B), block(kTargetsThreads);
  for (int64_t g = 0; g < groups; ++g) {
    p.group = g;
    if (p.t.staged) hipLaunchKernelGGL((ctcx_target_grads<T, Fmt, G, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((ctcx_target_grads<T, Fmt, G, false>), grid, block, 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename T, int Fmt>
hipError_t launch_all(const CtcxTgradParams& p, hipStream_t s) {
  switch (ctcx_targets_segment(p.t.L)) {
    case 8: return launch_segment<T, Fmt, 8>(p, s);
    case 16: return launch_segment<T, Fmt, 16>(p, s);
    case 32: return launch_segment<T, Fmt, 32>(p, s);
    case 64: return launch_segment<T, Fmt, 64>(p, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t ctcx_launch_target_grads(const CtcxTgradParams& pp, hipStream_t s) {
  const CtcxTargetsParams& p = pp.t;
  if (p.B <= 0 || p.N < 0 || (p.N == 0 && pp.forward_only)) return hipSuccess;
  if (p.Tmax < 0 || p.Tmax > 0x7fffffffLL || p.B > 0x7fffffffLL || p.C <= 0 || p.C > 0x7fffffffLL || p.blank_index < 0 ||
      p.blank_index >= p.C || (p.N > 0 && (!p.target_length || (p.L > 0 && !p.targets) || !p.out)) || !p.frames ||
      (p.Tmax > 0 && (!p.x || !p.norm || !pp.ws || (!pp.forward_only && !pp.grad))) ||
      (p.xfmt != kPathsInNative && (p.f64 || (p.xfmt != kPathsInF16 && p.xfmt != kPathsInBF16))) ||
      !ctcx_targets_segment(p.L) || (p.staged && !ctcx_targets_tile(p.C, p.f64)) || pp.tile < 1 ||
      (pp.tile & (pp.tile - 1)) != 0 || pp.tile > ctcx_tgrad_tile(p.C, p.f64, p.staged))
    return hipErrorInvalidValue;
  if (p.f64) return launch_all<double, kPathsInNative>(pp, s);
  if (p.xfmt == kPathsInF16) return launch_all<float, kPathsInF16>(pp, s);
  if (p.xfmt == kPathsInBF16) return launch_all<float, kPathsInBF16>(pp, s);
  return launch_all<float, kPathsInNative>(pp, s);
}
