// ctcx_scores.hip — the sum and the minimum of the per-frame log-posteriors over
// every timed token's span of each path's best alignment (include/ctcext.h,
// "Token scores"), from the rows the traceback leaves in the workspace, the
// spans the token-times kernel wrote, the decoder's normaliser and the logits
// where the decode read them.  A translation unit of its own: the decode
// objects neither see nor depend on it.
//
// One 256-thread workgroup per (item, path) row.  The row's tokens are taken in
// groups of kScoresTile, one token per thread.  A group's frames -- from its
// lowest valid start to its highest valid end -- are covered in tiles of
// kScoresTile frames aligned to multiples of kScoresTile, one frame per thread:
// the thread reads the frame's alignment element (the walks are reversed:
// frame f is element frames - 1 - f), the normaliser of the row, gathers the
// one logit, subtracts, and leaves the value in LDS.  The token's thread then
// adds its frames of the tile in ascending order and carries the sum and the
// minimum to the next tile, so every sum is the definition's chain of rounded
// additions whatever the tile boundaries are.
//
// start / end are not trusted: a token is scored only when
// 0 <= frames - L <= start <= end < frames, its index is below the clamped
// decoded length, and every alignment value of the span maps to a class in
// [0, C); the frames a tile reads lie inside such spans' hull, which lies inside
// the walk.  Every other cell of the row is a NaN, and each cell is written
// once, by the thread of its token index.
#include "ctcx_scores.h"

namespace {

constexpr int kNT = kScoresTile;
constexpr int kNone = 0x7fffffff;

// element off of x as T: the element itself, or a half widened as the decode
// kernels' row stage widens it (fp16: the hardware convert; bf16: the bits, 16
// to the left) -- exact for both
template <typename T>
__device__ __forceinline__ T load_as(const void* x, int xfmt, int64_t off) {
  if (xfmt == kScoresInF16) return (T)(float)__builtin_bit_cast(_Float16, ((const uint16_t*)x)[off]);
  if (xfmt == kScoresInBF16) return (T)__uint_as_float((unsigned)((const uint16_t*)x)[off] << 16);
  return ((const T*)x)[off];
}

template <typename T>
__global__ __launch_bounds__(kNT) void ctcx_token_scores(CtcxScoresParams p) {
  __shared__ T s_lp[kNT];
  __shared__ int s_ok[kNT];
  __shared__ int s_lo, s_hi;
  const int64_t bp = blockIdx.x;
  const int64_t b = bp / p.P;
  const int pth = (int)(bp - b * p.P);
  const int tid = threadIdx.x;
  const int Tmax = (int)p.Tmax;
  auto clampT = [&](int v) { return v < 0 ? 0 : v > Tmax ? Tmax : v; };
  const bool empty = p.status && p.status[b] != 0;
  const int frames = clampT(p.frames[b]);
  const int m = empty ? 0 : clampT(p.len[((int64_t)pth * 2 + 0) * p.B + b]);
  int L = empty ? 0 : clampT(p.len[((int64_t)pth * 2 + 1) * p.B + b]);
  if (L > frames) L = frames;   // (a walk is never longer than its item: frame numbers stay >= 0)
  const int base = frames - L;  // the walk's first frame
  const int32_t* const a_rev = p.seq + (bp * 2 + 1) * p.Tmax;
  const int32_t* const start = p.start + bp * p.Tmax;
  const int32_t* const end = p.end + bp * p.Tmax;
  const T* const norm = (const T*)p.norm;
  T* const out_sum = p.logp_sum ? (T*)p.logp_sum + bp * p.Tmax : nullptr;
  T* const out_min = p.logp_min ? (T*)p.logp_min + bp * p.Tmax : nullptr;
  const int C = (int)p.C;
  const T nan = (T)__builtin_nanf("");

  for (int q0 = 0; q0 < Tmax; q0 += kNT) {
    const int q = q0 + tid;
    T acc = nan, mn = nan;
    bool valid = false;
    if (q0 < m) {   // (uniform: a group past the decoded length only fills)
      int s = -1, e = -1;
      if (q < m) {
        s = start[q];
        e = end[q];
        valid = s >= base && s <= e && e < frames;   // (base >= 0)
      }
      if (tid == 0) {
        s_lo = kNone;
        s_hi = -1;
      }
      __syncthreads();
      if (valid) {
        atomicMin(&s_lo, s);
        atomicMax(&s_hi, e);
      }
      __syncthreads();
      const int lo = s_lo, hi = s_hi;   // the hull of the group's valid spans: inside [base, frames)
      __syncthreads();
      bool bad = false;
      if (hi >= 0) {
        for (int f0 = lo / kNT * kNT; f0 <= hi; f0 += kNT) {
          const int f = f0 + tid;
          T lp = nan;
          int ok = 0;
          if (f >= lo && f <= hi) {
            const int v = a_rev[frames - 1 - f];   // element in [0, L)
            const int c = v == p.blank_label ? p.blank_index : v;
            if (c >= 0 && c < C) {
              lp = load_as<T>(p.x, p.xfmt, (int64_t)f * p.xst_t + b * p.xst_b + c) - norm[(int64_t)f * p.B + b];
              ok = 1;
            }
          }
          s_lp[tid] = lp;
          s_ok[tid] = ok;
          __syncthreads();
          if (valid) {
            const int fa = s > f0 ? s : f0;
            const int fb = e < f0 + kNT - 1 ? e : f0 + kNT - 1;
            for (int g = fa; g <= fb; ++g) {   // ascending frames
              const T v = s_lp[g - f0];
              bad |= s_ok[g - f0] == 0;
              if (g == s) {
                acc = mn = v;
              } else {
                acc = acc + v;
                if (v < mn) mn = v;   // (a NaN never replaces, a leading NaN stays)
              }
            }
          }
          __syncthreads();
        }
      }
      if (!valid || bad) acc = mn = nan;
    }
    if (q < Tmax) {
      if (out_sum) out_sum[q] = acc;
      if (out_min) out_min[q] = mn;
    }
  }
}

}  // namespace

hipError_t ctcx_launch_token_scores(const CtcxScoresParams& p, hipStream_t s) {
  if (p.B <= 0 || p.P <= 0) return hipSuccess;
  if (p.B * p.P > 0x7fffffffLL || p.Tmax < 0 || p.Tmax > 0x7fffffffLL - kNT || p.C <= 0 || p.C > 0x7fffffffLL ||
      p.blank_index < 0 || p.blank_index >= p.C || !p.seq || !p.len || !p.frames || !p.start || !p.end ||
      (p.Tmax > 0 && (!p.x || !p.norm)) || (!p.logp_sum && !p.logp_min) ||
      (p.xfmt != kScoresInNative && (p.f64 || (p.xfmt != kScoresInF16 && p.xfmt != kScoresInBF16))))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(p.B * p.P));
  if (p.f64)
    hipLaunchKernelGGL(ctcx_token_scores<double>, grid, dim3(kNT), 0, s, p);
  else
    hipLaunchKernelGGL(ctcx_token_scores<float>, grid, dim3(kNT), 0, s, p);
  return hipGetLastError();
}
