// ctcx_paths.hip — the exact CTC log-likelihood log p(y | x) of every returned
// path (include/ctcext.h, "Path scores"): the forward recursion over the
// 2m + 1 states of the decoded row y, from the row the traceback leaves in the
// workspace (walk 0), the decoder's normaliser and the logits where the decode
// read them.  A translation unit of its own: the decode objects neither see nor
// depend on it.
//
// A trellis: the time axis is serial, the state axis parallel.  One wave64 per
// (item, path) row, and a workgroup is that one wave, so the time loop of the
// register kernels has no barrier.
//
// Work split (ctcx_path_scores_reg<T, Fmt, K>).  The m labels are dealt to the
// lanes in contiguous blocks of K: lane l holds labels [l K, l K + K), and for
// each the pair (blank state 2j, label state 2j + 1) in registers, unrolled.
// The lane of the last label holds the final blank too: slot m of its own block
// where the block has room, the register aF where label m - 1 is its block's
// last.  K is one of kPathsBlocks; a row runs in the smallest instantiation
// with 64 K >= m, every instantiation is launched over all rows (those the
// widths up to max_time can need), and a workgroup whose row belongs to another
// returns at once.  Rows above 64 * kPathsMaxBlock labels run in
// ctcx_path_scores_lds, which keeps the pairs in LDS: the same recursion, one
// wave, slot j on lane j mod 64, in place from the last chunk of 64 slots down,
// with a barrier between a chunk's reads and its writes.
//
// Neighbour exchange.  With contiguous blocks a lane needs one foreign value a
// frame: the previous lane's last label state of the frame before, which feeds
// its first blank (s - 1) and its first label (s - 2).  One DPP wave_shr:1
// moves it (two for a double); lane 0 receives -inf.  Whether the s - 2 step is
// allowed (y[j] != y[j - 1]) is a bit per label, set once per row.
//
// Logit movement.  A lane's labels are fixed, so its gather offsets are: the
// row pointer of the frame is uniform and advances by xst_t.  The K logits, the
// blank's and the normaliser of frame f + 1 are requested before the arithmetic
// of frame f and held in a second set of registers.
//
// Arithmetic.  Log domain; the three-way LSE subtracts the maximum and guards
// an all -inf argument list (the sum of the arguments then: -inf, or the NaN
// that was among them).  float32 uses the hardware exp2 / log2, float64 the
// double exp / log.  Every kPathsRenorm frames a float32 row takes the maximum
// finite state of the wave (a DPP reduction), subtracts it from every state and
// adds it to a double, which goes back in at the end: states stay near 0, where
// float32 is fine, however far the raw alphas have run.
//
// Band.  At frame f only states s <= 2 f + 1 can be finite, and only states
// s >= S - 2 (frames - f) can still reach the end.  A lane whose block lies
// wholly outside skips the frame's arithmetic (the exchange runs in front of
// the branch, in every lane).  A block that has fallen behind the band stays
// behind it, and what its stale states feed lies behind it as well.
//
// Rows of the caller (CtcxPathsParams' tgt fields; the per-row route of the
// target scores, ctcx_targets.h).  The same kernels read row (b, p) from the
// caller's targets in place instead of the walk buffers: labels in reading
// order, int32 or int64.  A length outside [0, tgt_L] makes the row NaN; a row
// of more labels than frames is -inf without a recursion (its labels are
// checked all the same), so every row that runs has m <= frames <= Tmax.
//
// Nothing is trusted: lengths are clamped to [0, Tmax] as the token-scores
// kernel clamps them, a label outside [0, C) makes the row a NaN before any
// logit is read, and every logit read is frame f < frames <= Tmax of item b.
#include "ctcx_paths.h"
#include "ctcx_lse.h"   // ninf, row_at, row_ptr, lse2, lse3, dpp_keep, from_prev_lane, finite_or_ninf

#include <atomic>

namespace {

constexpr int kR = kPathsRenorm;
static_assert((kR & (kR - 1)) == 0, "the frame test below masks");
static_assert(kPathsInNative == 0 && kPathsInF16 == 1 && kPathsInBF16 == 2, "ctcx_lse.h spells the formats out");

// the wave's maximum of v (no NaN), uniform: row_shr 1, 2, 4, 8, row_bcast 15 and 31 gather it in lane 63
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, __int_as_float(dpp_keep<0x111>(__float_as_int(v), __float_as_int(v))));
  v = fmaxf(v, __int_as_float(dpp_keep<0x112>(__float_as_int(v), __float_as_int(v))));
  v = fmaxf(v, __int_as_float(dpp_keep<0x114>(__float_as_int(v), __float_as_int(v))));
  v = fmaxf(v, __int_as_float(dpp_keep<0x118>(__float_as_int(v), __float_as_int(v))));
  v = fmaxf(v, __int_as_float(dpp_keep<0x142>(__float_as_int(v), __float_as_int(v))));
  v = fmaxf(v, __int_as_float(dpp_keep<0x143>(__float_as_int(v), __float_as_int(v))));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// the largest register block of the compute dtype: 24 pairs of doubles with
// their two sets of logits do not fit the register file, so float64 rows above
// 64 * 16 labels take the LDS instantiation
template <typename T>
constexpr int kMaxBlock = sizeof(T) == 8 ? 16 : kPathsMaxBlock;
// the instantiation of a row of m labels: its block size, or 0 for the LDS one
template <typename T>
__host__ __device__ constexpr int block_of(int m) {
  const int k = m <= 64 ? 1 : m <= 128 ? 2 : m <= 256 ? 4 : m <= 512 ? 8 : m <= 1024 ? 16 : m <= 1536 ? 24 : 0;
  return k > kMaxBlock<T> ? 0 : k;
}
static_assert(kPathsBlocks[0] == 1 && kPathsBlocks[1] == 2 && kPathsBlocks[2] == 4 && kPathsBlocks[3] == 8 &&
                  kPathsBlocks[4] == 16 && kPathsBlocks[5] == 24 && kPathsMaxBlock == 24,
              "block_of and launch_all spell kPathsBlocks out");

struct Row {
  int64_t bp, b;
  int m, frames;
  bool empty;        // the row is NaN
  bool infeasible;   // (a target) more labels than frames: the row is -inf (NaN with a bad label), and m reads 0
  int tlen;          // (a target) its labels
  int64_t t0;        // (a target) its first label's index in p.tgt
};
__device__ __forceinline__ Row read_row(const CtcxPathsParams& p) {
  Row r;
  r.bp = blockIdx.x;
  r.b = r.bp / p.P;
  const int pth = (int)(r.bp - r.b * p.P);
  const int Tmax = (int)p.Tmax;
  auto clampT = [&](int v) { return v < 0 ? 0 : v > Tmax ? Tmax : v; };
  r.empty = p.status && p.status[r.b] != 0;
  r.frames = clampT(p.frames[r.b]);
  r.infeasible = false;
  r.t0 = 0;
  r.tlen = 0;
  if (p.tgt_len) {
    const int64_t ti = p.tgt_shared ? pth : r.bp;
    const int32_t len = p.tgt_len[ti];
    r.empty |= len < 0 || len > p.tgt_L;
    r.infeasible = !r.empty && len > r.frames;
    r.m = r.empty || r.infeasible ? 0 : len;
    r.t0 = ti * p.tgt_L;
    r.tlen = r.empty ? 0 : len;
    return r;
  }
  r.m = r.empty ? 0 : clampT(p.len[((int64_t)pth * 2 + 0) * p.B + r.b]);
  return r;
}
// label j of the row: the walk's element m - 1 - j, or the target's j (-1: an int64 label outside [0, C))
__device__ __forceinline__ int row_label(const CtcxPathsParams& p, const Row& r, const int32_t* d_rev, int j) {
  if (!p.tgt_len) return d_rev[r.m - 1 - j];
  if (!p.tgt_i64) return ((const int32_t*)p.tgt)[r.t0 + j];
  const int64_t v = ((const int64_t*)p.tgt)[r.t0 + j];
  return v < 0 || v >= p.C ? -1 : (int)v;
}
// the rows that need no recursion (uniform)
template <typename T>
__device__ __forceinline__ bool row_is_done(const CtcxPathsParams& p, const Row& r, T* out, int lane) {
  if (!r.empty && !r.infeasible) return false;
  bool bad = r.empty;
  if (r.infeasible)   // its labels are checked all the same: a label outside [0, C) makes the row NaN
    for (int j = lane; j < r.tlen; j += 64) {
      const int v = row_label(p, r, nullptr, j);
      bad |= v < 0 || v >= p.C;
    }
  bad = __any(bad);
  if (lane == 0) *out = bad ? (T)__builtin_nanf("") : ninf<T>();
  return true;
}

template <typename T, int Fmt, int K>
__global__ __launch_bounds__(64) void ctcx_path_scores_reg(CtcxPathsParams p) {
  const Row r = read_row(p);
  if (p.force_lds || block_of<T>(r.m) != K) return;   // (uniform) another instantiation's row
  const int lane = threadIdx.x;
  T* const out = (T*)p.path_logp + r.bp;
  if (row_is_done(p, r, out, lane)) return;
  const int m = r.m, frames = r.frames;
  const int32_t* const d_rev = p.seq + (r.bp * 2 + 0) * p.Tmax;   // token j is element m - 1 - j
  const int j0 = lane * K;
  const int nl = m - j0 < 0 ? 0 : m - j0 > K ? K : m - j0;   // labels of this lane
  uint32_t lab[K];
  unsigned skipm = 0;   // bit i: the s - 2 step into label i is allowed
  bool bad = false;
  int prev = (nl > 0 && j0 > 0) ? row_label(p, r, d_rev, j0 - 1) : -1;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    int v = 0;
    if (i < nl) {
      v = row_label(p, r, d_rev, j0 + i);
      bad |= v < 0 || v >= p.C;
      if (j0 + i > 0 && v != prev) skipm |= 1u << i;
      prev = v;
    }
    lab[i] = (uint32_t)v;
  }
  if (__any(bad)) {
    if (lane == 0) *out = (T)__builtin_nanf("");
    return;
  }
  const T NINF = ninf<T>();
  const T* const nb = (const T*)p.norm + r.b;
  const uint32_t blank = (uint32_t)p.blank_index;
  auto gather = [&](int f, T (&v)[K], T& vb, T& vn) {
    const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + r.b * p.xst_b);   // uniform
#pragma unroll
    for (int i = 0; i < K; ++i)
      if (i < nl) v[i] = row_at<T, Fmt>(row, lab[i]);
    vb = row_at<T, Fmt>(row, blank);
    vn = nb[(int64_t)f * p.B];
  };

  // the states of "frame -1": state 0 holds 0, and the recursion's first step gives the definition's alpha_0
  T aB[K], aL[K], aF = NINF;
#pragma unroll
  for (int i = 0; i < K; ++i) aB[i] = aL[i] = NINF;
  if (lane == 0) aB[0] = (T)0;
  const int last_lane = m > 0 ? (m - 1) / K : 0;
  const int li = m - 1 - last_lane * K;   // the last label's slot in its lane; -1: no label
  const bool need_f = li == K - 1;        // (uniform) the final blank has no slot of its own
  const int S = 2 * m + 1;
  const int hi = 2 * (j0 + K) - 1;        // this lane's last label state
  const bool owns = lane == 0 || j0 < m;
  double shift = 0;                        // what the renormalisations took out

  T cur[K], curB = (T)0, curN = (T)0;
#pragma unroll
  for (int i = 0; i < K; ++i) cur[i] = NINF;
  if (frames > 0) gather(0, cur, curB, curN);
  for (int f = 0; f < frames; ++f) {
    T nxt[K], nxtB = curB, nxtN = curN;
#pragma unroll
    for (int i = 0; i < K; ++i) nxt[i] = cur[i];
    if (f + 1 < frames) gather(f + 1, nxt, nxtB, nxtN);
    const T from_prev = from_prev_lane(aL[K - 1]);
    const bool live = owns && j0 <= f && hi >= S - 2 * (frames - f);
    if (live) {
      const T lpB = curB - curN;
      T pl = from_prev;   // alpha_{f-1} of the label state in front of slot i's pair
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const T oB = aB[i], oL = aL[i];
        const T lp = i < nl ? cur[i] - curN : NINF;
        aB[i] = lse2(oB, pl) + lpB;
        aL[i] = lse3(oL, oB, (skipm >> i) & 1u ? pl : NINF) + lp;
        pl = oL;
      }
      if (need_f) aF = lse2(aF, pl) + lpB;
    }
    if constexpr (sizeof(T) == 4) {
      if ((f & (kR - 1)) == kR - 1) {
        float mine = NINF;
        if (live) {
#pragma unroll
          for (int i = 0; i < K; ++i) mine = fmaxf(mine, fmaxf(finite_or_ninf(aB[i]), finite_or_ninf(aL[i])));
          if (need_f) mine = fmaxf(mine, finite_or_ninf(aF));
        }
        const float top = wave_max(mine);   // uniform
        if (top > NINF) {
#pragma unroll
          for (int i = 0; i < K; ++i) {
            aB[i] -= top;
            aL[i] -= top;
          }
          aF -= top;
          shift += (double)top;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < K; ++i) cur[i] = nxt[i];
    curB = nxtB;
    curN = nxtN;
  }
  if (lane == last_lane) {
    T fb = NINF, fl = NINF;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      if (i == li + 1) fb = aB[i];
      if (i == li) fl = aL[i];
    }
    if (need_f) fb = aF;
    *out = (T)((double)lse2(fb, fl) + shift);
  }
}

// The pairs in LDS: sB[j] / sL[j] are states 2j / 2j + 1 (slot m holds the final
// blank), sY[j] label j with the s - 2 permission in the sign bit.
template <typename T, int Fmt>
__global__ __launch_bounds__(64) void ctcx_path_scores_lds(CtcxPathsParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  const Row r = read_row(p);
  if (!p.force_lds && block_of<T>(r.m) != 0) return;   // (uniform) a register instantiation's row
  const int lane = threadIdx.x;
  T* const out = (T*)p.path_logp + r.bp;
  if (row_is_done(p, r, out, lane)) return;
  const int m = r.m, frames = r.frames;
  const int W = (int)ctcx_paths_width(p) + 1;   // m <= Tmax (and a target's <= tgt_L)
  T* const sB = (T*)s_mem;
  T* const sL = sB + W;
  int32_t* const sY = (int32_t*)(sL + W);
  const int32_t* const d_rev = p.seq + (r.bp * 2 + 0) * p.Tmax;
  const T NINF = ninf<T>();
  bool bad = false;
  for (int j = lane; j <= m; j += 64) {
    int v = 0;
    if (j < m) {
      v = row_label(p, r, d_rev, j);
      bad |= v < 0 || v >= p.C;
      if (j > 0 && v != row_label(p, r, d_rev, j - 1)) v |= (int)0x80000000u;
    }
    sY[j] = v;
    sB[j] = j == 0 ? (T)0 : NINF;
    sL[j] = NINF;
  }
  __syncthreads();
  if (__any(bad)) {
    if (lane == 0) *out = (T)__builtin_nanf("");
    return;
  }
  const T* const nb = (const T*)p.norm + r.b;
  const int S = 2 * m + 1;
  double shift = 0;
  for (int f = 0; f < frames; ++f) {
    const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + r.b * p.xst_b);
    const T nrm = nb[(int64_t)f * p.B];
    const T lpB = row_at<T, Fmt>(row, (uint32_t)p.blank_index) - nrm;
    // the band's slots: j <= f, and 2j + 1 >= S - 2 (frames - f)
    const int lo_s = S - 2 * (frames - f);
    const int jlo = lo_s <= 1 ? 0 : lo_s / 2;   // (2j + 1 >= lo_s)
    const int jhi = f < m ? f : m;
    for (int c = jhi / 64; c >= jlo / 64; --c) {
      const int j = c * 64 + lane;
      const bool act = j >= jlo && j <= jhi;
      T oB = NINF, oL = NINF, pl = NINF;
      if (act) {
        oB = sB[j];
        oL = sL[j];
        if (j > 0) pl = sL[j - 1];
      }
      __syncthreads();
      if (act) {
        sB[j] = lse2(oB, pl) + lpB;
        if (j < m) {
          const int y = sY[j];
          const T lp = row_at<T, Fmt>(row, (uint32_t)y & 0x7fffffffu) - nrm;
          sL[j] = lse3(oL, oB, y < 0 ? pl : NINF) + lp;
        }
      }
      __syncthreads();
    }
    if constexpr (sizeof(T) == 4) {
      if ((f & (kR - 1)) == kR - 1) {
        float mine = NINF;
        for (int j = jlo + lane; j <= jhi; j += 64) mine = fmaxf(mine, fmaxf(finite_or_ninf(sB[j]), finite_or_ninf(sL[j])));
        const float top = wave_max(mine);
        if (top > NINF) {
          for (int j = lane; j <= m; j += 64) {
            sB[j] -= top;
            sL[j] -= top;
          }
          shift += (double)top;
        }
        __syncthreads();
      }
    }
  }
  if (lane == 0) *out = (T)((double)lse2(sB[m], m > 0 ? sL[m - 1] : NINF) + shift);
}

template <typename T>
constexpr size_t lds_bytes(int64_t Tmax) { return (size_t)(Tmax + 1) * (2 * sizeof(T) + 4); }

template <typename T, int Fmt>
hipError_t launch_all(const CtcxPathsParams& p, hipStream_t s) {
  const dim3 grid((unsigned)(p.B * p.P)), block(64);
  const int64_t Wd = ctcx_paths_width(p);
  if (!p.force_lds) {
    // every register instantiation a row of at most Tmax labels can need
    hipLaunchKernelGGL((ctcx_path_scores_reg<T, Fmt, 1>), grid, block, 0, s, p);
    if (Wd > 64 * 1) hipLaunchKernelGGL((ctcx_path_scores_reg<T, Fmt, 2>), grid, block, 0, s, p);
    if (Wd > 64 * 2) hipLaunchKernelGGL((ctcx_path_scores_reg<T, Fmt, 4>), grid, block, 0, s, p);
    if (Wd > 64 * 4) hipLaunchKernelGGL((ctcx_path_scores_reg<T, Fmt, 8>), grid, block, 0, s, p);
    if (Wd > 64 * 8) hipLaunchKernelGGL((ctcx_path_scores_reg<T, Fmt, 16>), grid, block, 0, s, p);
    if constexpr (kMaxBlock<T> >= 24)
      if (Wd > 64 * 16) hipLaunchKernelGGL((ctcx_path_scores_reg<T, Fmt, 24>), grid, block, 0, s, p);
    if (Wd <= 64 * kMaxBlock<T>) return hipGetLastError();
  }
  const size_t bytes = lds_bytes<T>(Wd);
  if (bytes > 64 * 1024) {
    // dynamic LDS above the default limit is allowed once per device and instantiation, for the widest row
    // (a host-side attribute of the function: no stream operation, nothing a capture sees)
    static std::atomic<uint64_t> allowed{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(allowed.load() & bit)) {
      e = hipFuncSetAttribute((const void*)ctcx_path_scores_lds<T, Fmt>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes<T>(sizeof(T) == 8 ? kPathsMaxLdsT64 : kPathsMaxLdsT32));
      if (e != hipSuccess) return e;
      allowed.fetch_or(bit);
    }
  }
  hipLaunchKernelGGL((ctcx_path_scores_lds<T, Fmt>), grid, block, bytes, s, p);
  return hipGetLastError();
}

}  // namespace

static_assert(block_of<float>(64) == 1 && block_of<float>(65) == 2 &&
                  block_of<float>(64 * kPathsMaxBlock) == kPathsMaxBlock && block_of<float>(64 * kPathsMaxBlock + 1) == 0 &&
                  block_of<double>(1024) == 16 && block_of<double>(1025) == 0,
              "launch_all's thresholds follow kPathsBlocks");

bool ctcx_path_scores_fits(int64_t Tmax, int32_t f64, int32_t force_lds) {
  const bool lds = force_lds || Tmax > 64 * (f64 ? kMaxBlock<double> : kMaxBlock<float>);
  return !lds || Tmax <= (f64 ? kPathsMaxLdsT64 : kPathsMaxLdsT32);
}

hipError_t ctcx_launch_path_scores(const CtcxPathsParams& p, hipStream_t s) {
  if (p.B <= 0 || p.P <= 0) return hipSuccess;
  if (p.B * p.P > 0x7fffffffLL || p.Tmax < 0 || p.C <= 0 || p.C > 0x7fffffffLL || p.blank_index < 0 ||
      p.blank_index >= p.C || (!p.tgt_len && (!p.seq || !p.len)) || (p.tgt_len && (p.tgt_L < 0 || (p.tgt_L > 0 && !p.tgt))) || !p.frames || !p.path_logp || (p.Tmax > 0 && (!p.x || !p.norm)) ||
      (p.xfmt != kPathsInNative && (p.f64 || (p.xfmt != kPathsInF16 && p.xfmt != kPathsInBF16))) ||
      !ctcx_path_scores_fits(ctcx_paths_width(p), p.f64, p.force_lds))
    return hipErrorInvalidValue;
  if (p.f64) return launch_all<double, kPathsInNative>(p, s);
  if (p.xfmt == kPathsInF16) return launch_all<float, kPathsInF16>(p, s);
  if (p.xfmt == kPathsInBF16) return launch_all<float, kPathsInBF16>(p, s);
  return launch_all<float, kPathsInNative>(p, s);
}
