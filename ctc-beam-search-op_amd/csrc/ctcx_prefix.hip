// ctcx_prefix.hip — the CTC prefix score of every one-label extension of
// prefixes the caller supplies (include/ctcext.h, "Prefix scores"), in two
// kernels.  A translation unit of its own: the decode objects neither see nor
// depend on it, and ctcx_targets.o and ctcx_paths.o are not touched by it.
//
// Kernel A (ctcx_prefix_tails<T, Fmt, G, Staged>) is the forward of the prefix
// g, a forward of its own in the packed trellis of ctcx_targets.hip: a prefix
// of m labels in a segment of G lanes (8, 16, 32 or 64), slot j < m the pair
// (blank state 2j, label state 2j + 1), slot m the final blank; 256 / G
// prefixes of ONE item a workgroup; one DPP wave_shr:1 a frame; the item's rows
// staged through two LDS buffers (Staged) or gathered lane by lane; float32
// renormalised every kPathsRenorm frames.  What it adds: after every frame,
// slot m stores bl_f = alpha_f[2m] and slot m - 1 stores nb_f = alpha_f[2m - 1]
// (slot 0 stores -inf for the empty prefix), as absolute log values -- the
// shift goes back in before the store -- with ordinary vector stores.  It ends
// with one word a prefix: the last label, -1 (empty) or -2 (the row is NaN).
// Prefixes of more than 63 labels take ctcx_prefix_tails_row, one wave per
// prefix with the states in LDS (its comment below).
//
// Kernel B (ctcx_prefix_reduce<T, Fmt, G, CP>) is the extension reduce: for
// every (item, prefix, class) the LSE over frames of phi_{f-1}(c) + lp[f][c].
// Work is split over (item, prefix group, class tile).  A workgroup of 256
// threads is CP classes by 256 / CP time slices: CP = 256 is the wide layout
// (one class a thread, every frame), CP = 32 the narrow one (eight slices,
// slice s takes the frames f = s mod 8), so an alphabet of 29 classes fills a
// workgroup.  A thread reads lp[f][c] in place through the strides, coalesced
// along the class axis, one frame ahead in a register, once for the G prefixes
// of its group; their running (maximum, sum) pairs live in 2G registers.
//
// The group's tails pass through LDS in tiles of kPrefixTile frames: the fill
// turns (bl, nb) into (bl, LSE(bl, nb)) once a (prefix, frame), not once a
// class, and puts phi_{-1} (0 for the empty prefix, else -inf) in front.  Two
// buffers, one barrier a tile.  In a step every lane of a slice reads the same
// pair -- an LDS broadcast -- and one select takes bl for the one class equal to
// g[m - 1] (a bit per prefix, set once).  The online LSE costs one exp a term:
// with d = term - max, e = exp(-|d|) either rescales the sum (d > 0) or is
// added to it.  A NaN term goes into the sum and stays.  The narrow layout
// merges its slices through LDS in slice order, in slice 0's threads.  The
// thread of the blank column writes the end score LSE(bl, nb) of the last
// frame instead.
//
// No matrix instructions: a probability-domain product Phi[N, T] * P[T, C]
// takes one shift a prefix and underflows where the definition is finite.
//
// Nothing is trusted: frames are clamped to [0, Tmax]; Kernel A checks lengths
// and labels before a logit is read with them; Kernel B reads class c < C of
// frame f < frames <= Tmax, tails of frame f < frames, and prefix n < N.
#include "ctcx_prefix.h"

#include <atomic>

#include "ctcx_lse.h"
#include "ctcx_paths.h"   // kPathsRenorm, kPathsIn*

namespace {

constexpr int kR = kPathsRenorm;
static_assert((kR & (kR - 1)) == 0, "the frame test below masks");
static_assert(kPathsInNative == 0 && kPathsInF16 == 1 && kPathsInBF16 == 2, "ctcx_lse.h spells the formats out");
static_assert(kTargetsThreads == kPrefixThreads && kTargetsTileBytes == kTargetsThreads * 32, "a thread moves 32 bytes of a tile");

template <int G>
__device__ __forceinline__ float segment_max(float v) {
#pragma unroll
  for (int k = 1; k < G; k <<= 1) v = fmaxf(v, __shfl_xor(v, k, 64));
  return v;
}

// ---------------------------------------------------------------------------
// Kernel A

template <typename T, int Fmt, int G, bool Staged>
__global__ __launch_bounds__(kPrefixThreads) void ctcx_prefix_tails(CtcxPrefixParams pp) {
  const CtcxTargetsParams& p = pp.t;
  constexpr int kPerWg = kPrefixThreads / G;
  constexpr int kMove = kTargetsTileBytes / (int)sizeof(T) / kPrefixThreads;
  const int tid = threadIdx.x;
  const int j = tid & (G - 1);   // the slot
  const int64_t nblk = (p.N + kPerWg - 1) / kPerWg;
  const int64_t b = blockIdx.x / nblk;   // (uniform)
  const int64_t n = (blockIdx.x - b * nblk) * kPerWg + tid / G;
  const T NINF = ninf<T>();
  const int Tmax = (int)p.Tmax;
  int frames = p.frames[b];
  frames = frames < 0 ? 0 : frames > Tmax ? Tmax : frames;   // (uniform)
  const bool valid = n < p.N;

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
  {   // one bad label or length makes the whole segment's prefix NaN
    const uint64_t seg = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1)) << ((tid & 63) & ~(G - 1));
    nan = (__ballot(nan) & seg) != 0;
  }
  const bool has_label = !nan && j < m;
  const bool counts = valid && !nan && j <= m;
  // the tail slots: slot m stores bl, slot m - 1 stores nb (slot 0 both for the empty prefix)
  const bool st_bl = valid && !nan && j == m, st_nb = valid && !nan && (m == 0 ? j == 0 : j == m - 1);
  T* const tail = (T*)pp.tails + (valid ? (b * p.N + n) * (int64_t)Tmax * 2 : 0);

  T aB = j == 0 ? (T)0 : NINF, aL = NINF;
  double shift = 0;
  auto step = [&](int f, T lpB, T lpL) {
    const T got = from_prev_lane(aL);
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
    // (f < frames <= Tmax)
    if (st_bl) tail[2 * (int64_t)f] = (T)((double)aB + shift);
    if (st_nb) tail[2 * (int64_t)f + 1] = m == 0 ? NINF : (T)((double)aL + shift);
  };

  const T* const nb = (const T*)p.norm + b;
  const uint32_t blank = (uint32_t)p.blank_index;
  if constexpr (Staged) {
    __shared__ T tile[2][kTargetsTileBytes / sizeof(T)];
    const int C = (int)p.C;
    const int F = ctcx_targets_tile(p.C, sizeof(T) == 8);   // >= kTargetsMinTile: the host chose this route
    const int cells = F * C;
    int fi[kMove], ci[kMove];
#pragma unroll
    for (int e = 0; e < kMove; ++e) {
      const int i = e * kPrefixThreads + tid;
      fi[e] = i < cells ? i / C : F;   // (F: no element)
      ci[e] = i < cells ? i - fi[e] * C : 0;
    }
    T hold[kMove];
    auto load = [&](int f0) {
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
      for (int e = 0; e < kMove; ++e) tile[buf][e * kPrefixThreads + tid] = hold[e];
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
      __syncthreads();
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

  // the prefix's word: the last label (slot m - 1 has it), -1 empty, -2 NaN
  if (valid) {
    int32_t* const w = pp.info + b * p.N + n;
    if (j == 0 && (nan || m == 0)) *w = nan ? -2 : -1;
    if (has_label && j == m - 1) *w = (int32_t)lab;
  }
}

template <typename T, int Fmt, int G>
hipError_t tails_segment(const CtcxPrefixParams& p, hipStream_t s) {
  const int64_t nblk = (p.t.N + kPrefixThreads / G - 1) / (kPrefixThreads / G);
  if (p.t.B * nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(p.t.B * nblk)), block(kPrefixThreads);
  if (p.t.staged) hipLaunchKernelGGL((ctcx_prefix_tails<T, Fmt, G, true>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((ctcx_prefix_tails<T, Fmt, G, false>), grid, block, 0, s, p);
  return hipGetLastError();
}

template <typename T, int Fmt>
hipError_t tails_all(const CtcxPrefixParams& p, hipStream_t s) {
  switch (ctcx_targets_segment(p.t.L)) {
    case 8: return tails_segment<T, Fmt, 8>(p, s);
    case 16: return tails_segment<T, Fmt, 16>(p, s);
    case 32: return tails_segment<T, Fmt, 32>(p, s);
    case 64: return tails_segment<T, Fmt, 64>(p, s);
  }
  return hipErrorInvalidValue;
}

// Kernel A, per row (ctcx_prefix_tails_row<T, Fmt>): prefixes of more than
// kTargetsMaxPacked labels.  One wave per prefix, and the workgroup is that
// wave.  The pairs live in LDS: sB[j] / sL[j] are states 2j / 2j + 1 (slot m
// holds the final blank), sY[j] label j with the s - 2 permission in the sign
// bit; slot j runs on lane j mod 64, in place from the last chunk of 64 slots
// down, with a barrier between a chunk's reads and its writes.  Only the band
// runs: slots j <= f, and those that can still reach the tails by the last
// frame.  After every frame lane 0 stores slot m's blank and slot m - 1's
// label state.  A prefix of more labels than frames has -inf tails without a
// recursion (its labels are checked all the same), so every row that runs has
// m <= frames <= Tmax and the LDS holds min(L, Tmax) + 1 slots.
template <typename T>
constexpr size_t row_lds_bytes(int64_t width) { return (size_t)(width + 1) * (2 * sizeof(T) + 4); }

template <typename T, int Fmt>
__global__ __launch_bounds__(64) void ctcx_prefix_tails_row(CtcxPrefixParams pp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  const CtcxTargetsParams& p = pp.t;
  const int lane = threadIdx.x;
  const int64_t bn = blockIdx.x, b = bn / p.N, n = bn - b * p.N;   // (uniform; bn < B * N)
  const T NINF = ninf<T>();
  const int Tmax = (int)p.Tmax;
  int frames = p.frames[b];
  frames = frames < 0 ? 0 : frames > Tmax ? Tmax : frames;
  int32_t* const w = pp.info + bn;
  T* const tail = (T*)pp.tails + bn * (int64_t)Tmax * 2;
  const int64_t ti = p.shared ? n : bn;
  const int64_t len = p.target_length[ti];
  bool bad = (p.status && p.status[b] != 0) || len < 0 || len > p.L;
  const int m = bad ? 0 : (int)len;
  auto label = [&](int j) -> int64_t {   // (j < m <= L)
    return p.labels_i64 ? ((const int64_t*)p.targets)[ti * p.L + j] : (int64_t)((const int32_t*)p.targets)[ti * p.L + j];
  };
  for (int j = lane; j < m; j += 64) {
    const int64_t v = label(j);
    bad |= v < 0 || v >= p.C;
  }
  if (__any(bad)) {
    if (lane == 0) *w = -2;
    return;
  }
  if (lane == 0) *w = m == 0 ? -1 : (int32_t)label(m - 1);
  if (m > frames) {   // (uniform) infeasible at every frame
    for (int i = lane; i < 2 * frames; i += 64) tail[i] = NINF;
    return;
  }
  const int W = (int)(p.L < p.Tmax ? p.L : p.Tmax) + 1;   // m <= min(L, frames) < W
  T* const sB = (T*)s_mem;
  T* const sL = sB + W;
  int32_t* const sY = (int32_t*)(sL + W);
  for (int j = lane; j <= m; j += 64) {
    int v = 0;
    if (j < m) {
      v = (int)label(j);
      if (j > 0 && label(j) != label(j - 1)) v |= (int)0x80000000u;
    }
    sY[j] = v;
    sB[j] = j == 0 ? (T)0 : NINF;
    sL[j] = NINF;
  }
  __syncthreads();
  const T* const nb = (const T*)p.norm + b;
  const int S = 2 * m + 1;
  double shift = 0;
  for (int f = 0; f < frames; ++f) {
    const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + b * p.xst_b);
    const T nrm = nb[(int64_t)f * p.B];
    const T lpB = row_at<T, Fmt>(row, (uint32_t)p.blank_index) - nrm;
    // the band's slots: j <= f, and 2j + 1 >= S - 2 (frames - f)
    const int lo_s = S - 2 * (frames - f);
    const int jlo = lo_s <= 1 ? 0 : lo_s / 2;
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
        const float top = segment_max<64>(mine);
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
    if (lane == 0) {   // (f < frames <= Tmax; one wave: the next frame's writes come behind these reads)
      tail[2 * (int64_t)f] = (T)((double)sB[m] + shift);
      tail[2 * (int64_t)f + 1] = m > 0 ? (T)((double)sL[m - 1] + shift) : NINF;
    }
  }
}

template <typename T, int Fmt>
hipError_t tails_rows(const CtcxPrefixParams& p, hipStream_t s) {
  if (p.t.B * p.t.N > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t bytes = row_lds_bytes<T>(p.t.L < p.t.Tmax ? p.t.L : p.t.Tmax);
  if (bytes > 64 * 1024) {
    // dynamic LDS above the default limit is allowed once per device and instantiation, for the widest row
    // (a host-side attribute of the function: no stream operation, nothing a capture sees)
    static std::atomic<uint64_t> allowed{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(allowed.load() & bit)) {
      e = hipFuncSetAttribute((const void*)ctcx_prefix_tails_row<T, Fmt>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)row_lds_bytes<T>(sizeof(T) == 8 ? kPathsMaxLdsT64 : kPathsMaxLdsT32));
      if (e != hipSuccess) return e;
      allowed.fetch_or(bit);
    }
  }
  hipLaunchKernelGGL((ctcx_prefix_tails_row<T, Fmt>), dim3((unsigned)(p.t.B * p.t.N)), dim3(64), bytes, s, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Kernel B

// one more term into a running (maximum, sum): one exp
template <typename T>
__device__ __forceinline__ void lse_push(T& mx, T& sum, T term) {
  if (!(term == ninf<T>())) {   // (a NaN term passes, and stays in the sum)
    const T d = term == mx ? (T)0 : term - mx;   // (two +inf terms: +inf, not inf - inf)
    const T e = ex(-ab(d));
    const bool up = d > (T)0;
    sum = up ? sum * e + (T)1 : sum + e;
    mx = up ? term : mx;
  }
}
// ... and another pair into it
template <typename T>
__device__ __forceinline__ void lse_merge(T& mx, T& sum, T mx2, T sum2) {
  if (!(mx2 == ninf<T>())) {
    const T d = mx2 == mx ? (T)0 : mx2 - mx;
    const T e = ex(-ab(d));
    const bool up = d > (T)0;
    sum = up ? sum * e + sum2 : sum + sum2 * e;
    mx = up ? mx2 : mx;
  } else {
    sum += sum2;   // (0, or a NaN that has to stay)
  }
}

template <typename T, int Fmt, int G, int CP>
__global__ __launch_bounds__(kPrefixThreads) void ctcx_prefix_reduce(CtcxPrefixParams pp) {
  const CtcxTargetsParams& p = pp.t;
  constexpr int S = kPrefixThreads / CP;   // time slices
  constexpr int TL = kPrefixTile;
  static_assert(TL % S == 0, "a slice's frames keep their phase across tiles");
  // phi: (bl, LSE(bl, nb)) of frame f - 1, by (prefix, frame of the tile), two buffers; the slices' merge takes
  // the same memory once the last tile is read
  constexpr int kPhi = G * TL * 2, kRed = (S - 1) * G * CP * 2;
  __shared__ T lds[2 * kPhi > kRed ? 2 * kPhi : kRed];
  const int tid = threadIdx.x;
  const int cl = tid % CP, sl = tid / CP;
  const int64_t ctiles = (p.C + CP - 1) / CP, ngrp = (p.N + G - 1) / G;
  const int64_t ct = blockIdx.x % ctiles, bg = blockIdx.x / ctiles;
  const int64_t b = bg / ngrp, n0 = (bg - b * ngrp) * G;   // (uniform)
  const int64_t c = ct * CP + cl;
  const bool cvalid = c < p.C;
  const T NINF = ninf<T>();
  const int Tmax = (int)p.Tmax;
  int frames = p.frames[b];
  frames = frames < 0 ? 0 : frames > Tmax ? Tmax : frames;   // (uniform)
  const T* const tails = (const T*)pp.tails;
  const int32_t* const info = pp.info + b * p.N;

  // the bit of prefix g: this thread's class is its last label
  uint32_t same = 0;
#pragma unroll
  for (int g = 0; g < G; ++g)
    if (n0 + g < p.N && (int64_t)info[n0 + g] == c) same |= 1u << g;

  // element e of a tile's fill: prefix e / TL, frame f0 + e % TL
  auto fill = [&](int f0, int buf) {
    for (int e = tid; e < G * TL; e += kPrefixThreads) {
      const int g = e / TL, f = f0 + e % TL;
      T bl = NINF, both = NINF;
      if (n0 + g < p.N && f < frames) {
        const int32_t w = info[n0 + g];
        if (f == 0) {
          bl = both = w == -1 ? (T)0 : NINF;
        } else if (w >= -1) {   // (a NaN row's tails were not written)
          const T* const tl = tails + ((b * p.N + n0 + g) * (int64_t)Tmax + (f - 1)) * 2;
          bl = tl[0];
          both = lse2(bl, tl[1]);
        }
      }
      lds[buf * kPhi + 2 * e] = bl;
      lds[buf * kPhi + 2 * e + 1] = both;
    }
  };

  T mx[G], sum[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    mx[g] = NINF;
    sum[g] = (T)0;
  }
  const T* const nb = (const T*)p.norm + b;
  auto lp_at = [&](int f) {   // (f < frames, c < C)
    const void* const row = row_ptr<Fmt, T>(p.x, (int64_t)f * p.xst_t + b * p.xst_b);
    return row_at<T, Fmt>(row, (uint32_t)c) - nb[(int64_t)f * p.B];
  };

  if (frames > 0) fill(0, 0);
  __syncthreads();
  T nxt = cvalid && sl < frames ? lp_at(sl) : NINF;
  for (int f0 = 0, buf = 0; f0 < frames; f0 += TL, buf ^= 1) {
    if (f0 + TL < frames) fill(f0 + TL, buf ^ 1);
    const int nf = frames - f0 < TL ? frames - f0 : TL;
    const T* const ph = lds + buf * kPhi;
    for (int i = sl; i < nf; i += S) {
      const T lp = nxt;
      const int fn = f0 + i + S;   // this slice's next frame (TL % S == 0: in the next tile too)
      if (cvalid && fn < frames) nxt = lp_at(fn);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const T bl = ph[2 * (g * TL + i)], both = ph[2 * (g * TL + i) + 1];
        lse_push(mx[g], sum[g], ((same >> g) & 1 ? bl : both) + lp);
      }
    }
    __syncthreads();   // tile k is read, tile k + 1 is whole
  }

  if constexpr (S > 1) {   // the slices' pairs, merged in slice order by slice 0
    auto red = [&](int s, int g) { return lds + ((s * G + g) * CP + cl) * 2; };   // (s < S - 1)
    if (sl > 0) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        red(sl - 1, g)[0] = mx[g];
        red(sl - 1, g)[1] = sum[g];
      }
    }
    __syncthreads();
    if (sl > 0) return;
    for (int s = 0; s < S - 1; ++s) {
#pragma unroll
      for (int g = 0; g < G; ++g) lse_merge(mx[g], sum[g], red(s, g)[0], red(s, g)[1]);
    }
  }
  if (!cvalid) return;

  T* const out = (T*)pp.ext;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int64_t n = n0 + g;
    if (n >= p.N) break;
    const int32_t w = info[n];
    T v = mx[g] + lg(sum[g]);   // (no term: -inf + log 0)
    if (c == p.blank_index) {   // the end score: the path score of g itself
      if (frames == 0) {
        v = w == -1 ? (T)0 : NINF;
      } else if (w >= -1) {
        const T* const tl = tails + ((b * p.N + n) * (int64_t)Tmax + (frames - 1)) * 2;
        v = lse2(tl[0], tl[1]);
      }
    }
    if (w < -1) v = (T)__builtin_nanf("");
    out[(b * p.N + n) * p.C + c] = v;
  }
}

template <typename T, int Fmt>
hipError_t reduce_all(const CtcxPrefixParams& p, hipStream_t s) {
  const int cp = p.layout ? kPrefixWideClasses : kPrefixNarrowClasses, g = p.layout ? kPrefixGroupWide : kPrefixGroupNarrow;
  const int64_t blocks = p.t.B * ((p.t.N + g - 1) / g) * ((p.t.C + cp - 1) / cp);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kPrefixThreads);
  if (p.layout) hipLaunchKernelGGL((ctcx_prefix_reduce<T, Fmt, kPrefixGroupWide, kPrefixWideClasses>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((ctcx_prefix_reduce<T, Fmt, kPrefixGroupNarrow, kPrefixNarrowClasses>), grid, block, 0, s, p);
  return hipGetLastError();
}

bool params_ok(const CtcxPrefixParams& pp) {
  const CtcxTargetsParams& p = pp.t;
  return !(p.Tmax < 0 || p.Tmax > 0x7fffffffLL || p.C <= 0 || p.C > 0x7fffffffLL || p.blank_index < 0 ||
           p.blank_index >= p.C || !p.target_length || (p.L > 0 && !p.targets) || !p.frames || !pp.tails || !pp.info ||
           (p.Tmax > 0 && (!p.x || !p.norm)) ||
           (p.xfmt != kPathsInNative && (p.f64 || (p.xfmt != kPathsInF16 && p.xfmt != kPathsInBF16))));
}

}  // namespace

bool ctcx_prefix_rows_fit(int64_t L, int64_t Tmax, int32_t f64) {
  return (L < Tmax ? L : Tmax) <= (f64 ? kPathsMaxLdsT64 : kPathsMaxLdsT32);
}

hipError_t ctcx_launch_prefix_tails(const CtcxPrefixParams& p, hipStream_t s) {
  if (p.t.B <= 0 || p.t.N <= 0) return hipSuccess;
  if (!params_ok(p) || p.t.L < 0) return hipErrorInvalidValue;
  if (p.rows) {
    if (!ctcx_prefix_rows_fit(p.t.L, p.t.Tmax, p.t.f64)) return hipErrorInvalidValue;
    if (p.t.f64) return tails_rows<double, kPathsInNative>(p, s);
    if (p.t.xfmt == kPathsInF16) return tails_rows<float, kPathsInF16>(p, s);
    if (p.t.xfmt == kPathsInBF16) return tails_rows<float, kPathsInBF16>(p, s);
    return tails_rows<float, kPathsInNative>(p, s);
  }
  if (!ctcx_targets_segment(p.t.L) || (p.t.staged && !ctcx_targets_tile(p.t.C, p.t.f64))) return hipErrorInvalidValue;
  if (p.t.f64) return tails_all<double, kPathsInNative>(p, s);
  if (p.t.xfmt == kPathsInF16) return tails_all<float, kPathsInF16>(p, s);
  if (p.t.xfmt == kPathsInBF16) return tails_all<float, kPathsInBF16>(p, s);
  return tails_all<float, kPathsInNative>(p, s);
}

hipError_t ctcx_launch_prefix_reduce(const CtcxPrefixParams& p, hipStream_t s) {
  if (p.t.B <= 0 || p.t.N <= 0) return hipSuccess;
  if (!params_ok(p) || !p.ext) return hipErrorInvalidValue;
  if (p.t.f64) return reduce_all<double, kPathsInNative>(p, s);
  if (p.t.xfmt == kPathsInF16) return reduce_all<float, kPathsInF16>(p, s);
  if (p.t.xfmt == kPathsInBF16) return reduce_all<float, kPathsInBF16>(p, s);
  return reduce_all<float, kPathsInNative>(p, s);
}
