// ctcx_skip.hip — blank-frame skipping (include/ctcext.h, "Blank-frame
// skipping") around the unchanged decode pipeline: the plan and the gather run
// in front of it, the expansion between its traceback and the scan / pack.  A
// translation unit of its own: the decode objects neither see nor depend on it.
//
//   ctcx_skip_plan     one 256-thread workgroup per item, frames in tiles of
//                      kSkipTile, one per thread.  A frame's flag is
//                      x[t, b, blank] - norm[t, b] > thr in the compute dtype
//                      (one load of each); the predecessor's flag crosses
//                      lanes by __shfl_up and waves and tiles through LDS; the
//                      kept frames are counted by the wave-scan / LDS-totals /
//                      carry shape of the token-times kernel.
//   ctcx_skip_gather   row (kmap[b][j], b) of the caller's tensor to row (j, b)
//                      of a dense time-major tensor of the same element type:
//                      one thread per 16-byte piece where pointer, strides and
//                      row size allow, per element otherwise.  The grid covers
//                      every (j, b) of the shape; rows j >= kept[b] are left
//                      alone (nothing downstream reads past the lengths).
//   ctcx_skip_expand   one workgroup per (item, path): the reversed alignment
//                      walk of the compacted decode, in place, to the walk on
//                      the original time axis.
//   ctcx_skip_chunk    the plan of one chunk of a skipping stream: one wave
//                      (chunks up to kSkipChunkSmall frames) or one workgroup
//                      per item, started from what the item carries, appending
//                      to the stream's kmap / cidx.
//   ctcx_skip_finish   one thread per item behind a stream push's commit: n and
//                      the carried flag follow it, the frame counts and the
//                      stable frames go out on the original time axis.
#include "ctcx_skip.h"

namespace {

constexpr int kNT = kSkipTile;
constexpr int kWaves = kNT / 64;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int clamp_len(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// element off of x as T: the element itself, or a half widened as the decode
// kernels' row stage widens it (fp16: the hardware convert; bf16: the bits, 16
// to the left) -- exact for both
template <typename T>
__device__ __forceinline__ T load_as(const void* x, int xfmt, int64_t off) {
  if (xfmt == kSkipInF16) return (T)(float)__builtin_bit_cast(_Float16, ((const uint16_t*)x)[off]);
  if (xfmt == kSkipInBF16) return (T)__uint_as_float((unsigned)((const uint16_t*)x)[off] << 16);
  return ((const T*)x)[off];
}

template <typename T>
__global__ __launch_bounds__(kNT) void ctcx_skip_plan(CtcxSkipPlanParams p) {
  __shared__ int s_dom[2][kWaves], s_cnt[2][kWaves];   // per wave: its last frame's flag, its kept frames; by tile parity
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Tmax = (int)p.Tmax;
  const int n = (p.pre && p.pre[b] != 0) ? 0 : clamp_len(p.seq_len[b], Tmax);
  const T thr = (T)p.thr;
  const T* const norm = (const T*)p.norm;
  int32_t* const kmap = p.kmap + b * p.Tmax;
  int32_t* const cidx = p.cidx + b * (p.Tmax + 1);
  int c_dom = 0;   // carries (uniform): the flag of the frame before this tile, the frames kept so far
  int c_cnt = 0;
  for (int base = 0; base < n; base += kNT) {
    const int par = (base / kNT) & 1;
    const int t = base + tid;
    const bool in = t < n;
    int dom = 0;
    if (in) {
      const T lp = load_as<T>(p.x, p.xfmt, (int64_t)t * p.xst_t + b * p.xst_b + p.blank) - norm[(int64_t)t * p.B + b];
      dom = lp > thr ? 1 : 0;   // (false for NaN)
    }
    int prev = __shfl_up(dom, 1, 64);
    if (lane == 63) s_dom[par][wave] = dom;
    __syncthreads();
    if (lane == 0) prev = wave == 0 ? c_dom : s_dom[par][wave - 1];
    const int keep = (in && !(t > 0 && dom && prev)) ? 1 : 0;
    int c = keep;   // inclusive count within the wave, then across waves
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(c, d, 64);
      if (lane >= d) c += y;
    }
    if (lane == 63) s_cnt[par][wave] = c;
    __syncthreads();
    int ex = c_cnt + c - keep, t_cnt = c_cnt;
    for (int w = 0; w < kWaves; ++w) {
      const int y = s_cnt[par][w];
      if (w < wave) ex += y;
      t_cnt += y;
    }
    if (in) cidx[t] = ex;
    if (keep) kmap[ex] = t;
    c_dom = s_dom[par][kWaves - 1];
    c_cnt = t_cnt;
  }
  if (tid == 0) {
    cidx[n] = c_cnt;
    p.kept[b] = c_cnt;
    if (p.kept_out) p.kept_out[b] = c_cnt;
  }
}

// V: the piece a thread moves (16 bytes, or one element); upr pieces per row,
// st_t / st_b the source strides in pieces
template <typename V>
__global__ __launch_bounds__(256) void ctcx_skip_gather(const V* __restrict__ x, V* __restrict__ xc,
                                                        const int32_t* __restrict__ kmap,
                                                        const int32_t* __restrict__ kept, int64_t Tmax, int64_t B,
                                                        int64_t upr, int64_t st_t, int64_t st_b, int64_t total) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int64_t row = g / upr, u = g - row * upr;
  const int64_t j = row / B, b = row - j * B;
  if (j >= kept[b]) return;
  const int64_t t = kmap[b * Tmax + j];
  xc[g] = x[t * st_t + b * st_b + u];
}

// Output element jo of the rewritten walk is original frame f = n - 1 - jo:
// blank_label where f was dropped (cidx[f + 1] == cidx[f]), else element
// kept - 1 - cidx[f] of the compacted walk.  That input index is never above
// jo (the kept frames from f on are no more than the frames from f on), so in
// place it is safe tile by tile from the far end: a tile reads only at or
// below its own elements, which no earlier (higher) tile wrote, and the
// barrier between a tile's reads and its writes keeps its own elements whole
// until every thread has read them.
__global__ __launch_bounds__(kNT) void ctcx_skip_expand(CtcxSkipExpandParams p) {
  const int64_t bp = blockIdx.x;
  const int64_t b = bp / p.P;
  const int pth = (int)(bp - b * p.P);
  const int tid = threadIdx.x;
  const int Tmax = (int)p.Tmax;
  const int n = clamp_len(p.frames[b], Tmax);
  const int kept = clamp_len(p.kept[b], n);
  int32_t* const lenp = p.len + ((int64_t)pth * 2 + 1) * p.B + b;
  const int L = clamp_len(*lenp, kept);
  if (L == 0) return;   // (uniform) an empty walk stays empty
  int32_t* const row = p.seq + (bp * 2 + 1) * p.Tmax;
  const int32_t* const cidx = p.cidx + b * (p.Tmax + 1);
  const int Lnew = n - clamp_len(p.kmap[b * p.Tmax + (kept - L)], n - 1);
  for (int base = (Lnew - 1) / kNT * kNT; base >= 0; base -= kNT) {
    const int jo = base + tid;
    const bool in = jo < Lnew;
    int v = p.blank_label;
    if (in) {
      const int f = n - 1 - jo;
      const int c0 = cidx[f], c1 = cidx[f + 1];
      const int ji = kept - 1 - c0;
      if (c1 != c0 && ji >= 0 && ji < L) v = row[ji];
    }
    __syncthreads();
    if (in) row[jo] = v;
  }
  __syncthreads();   // (every thread has read the old length)
  if (tid == 0) *lenp = Lnew;
}

// The plan of one chunk of a stream: ctcx_skip_plan's carry / scan shape with
// NT threads per item (one wave for the usual short chunk, kSkipTile for a long
// one), started from the item's carried flag, its frames n and its committed
// kept count, and appending.  Frame t of the chunk is original frame n + t; the
// t > 0 rule reads that number.  What the push may still undo (n, the flag) is
// left in n_next / dom_next; kmap and cidx entries past the committed counts are
// rewritten by the item's next chunk if this one is not committed.
template <typename T, int NT>
__global__ __launch_bounds__(NT) void ctcx_skip_chunk(CtcxSkipChunkParams p) {
  constexpr int NW = NT / 64;
  __shared__ int s_dom[2][NW], s_cnt[2][NW];
  __shared__ int s_last;   // the flag of the chunk's last frame (written once, before its tile's first barrier)
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int F = (int)p.max_frames;
  const CtcxSkipItem it = p.item[b];
  const int n0 = clamp_len(it.n, F);
  const int k0 = clamp_len(*(const int32_t*)(p.state + b * p.stride), n0);
  int n = clamp_len(p.len[b], (int)p.chunk_time);
  if (n > F - n0) n = 0;   // (the prologue's capacity rule has already said so)
  const T thr = (T)p.thr;
  const T* const norm = (const T*)p.norm;
  int32_t* const kmap = p.kmap + b * p.max_frames;
  int32_t* const cidx = p.cidx + b * (p.max_frames + 1);
  int32_t* const ckmap = p.ckmap + b * p.chunk_time;
  int c_dom = it.dom ? 1 : 0;   // carries (uniform): the flag of the frame before this tile, the frames kept so far
  int c_cnt = 0;
  for (int base = 0; base < n; base += NT) {
    const int par = (base / NT) & 1;
    const int t = base + tid;
    const bool in = t < n;
    int dom = 0;
    if (in) {
      const T lp = load_as<T>(p.x, p.xfmt, (int64_t)t * p.xst_t + b * p.xst_b + p.blank) - norm[(int64_t)t * p.B + b];
      dom = lp > thr ? 1 : 0;   // (false for NaN)
    }
    int prev = __shfl_up(dom, 1, 64);
    if (lane == 63) s_dom[par][wave] = dom;
    if (t == n - 1) s_last = dom;
    __syncthreads();
    if (lane == 0) prev = wave == 0 ? c_dom : s_dom[par][wave - 1];
    const int keep = (in && !(n0 + t > 0 && dom && prev)) ? 1 : 0;
    int c = keep;
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(c, d, 64);
      if (lane >= d) c += y;
    }
    if (lane == 63) s_cnt[par][wave] = c;
    __syncthreads();
    int ex = c_cnt + c - keep, t_cnt = c_cnt;
    for (int w = 0; w < NW; ++w) {
      const int y = s_cnt[par][w];
      if (w < wave) ex += y;
      t_cnt += y;
    }
    if (in) cidx[n0 + t] = k0 + ex;
    if (keep) {
      kmap[k0 + ex] = n0 + t;
      ckmap[ex] = t;
    }
    c_dom = s_dom[par][NW - 1];
    c_cnt = t_cnt;
  }
  if (tid == 0) {
    cidx[n0 + n] = k0 + c_cnt;
    p.klen[b] = c_cnt;
    p.cum[b] = k0 + c_cnt;
    p.item[b].n_next = n0 + n;
    p.item[b].dom_next = n > 0 ? s_last : c_dom;   // (no frame: the carried flag stays)
  }
}

// One thread per item, behind the commit (and the stable query) of a push.
__global__ __launch_bounds__(256) void ctcx_skip_finish(CtcxSkipFinishParams p) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= p.B) return;
  CtcxSkipItem it = p.item[b];
  if (!(p.status[b] & p.dead_mask)) {
    it.n = it.n_next;
    it.dom = it.dom_next;
    p.item[b] = it;
  }
  p.n_ws[b] = it.n;
  if (p.frames) p.frames[b] = it.n;
  if (p.kept) p.kept[b] = p.cum[b];
  if (p.stable_frames) {
    int64_t r = p.stable_frames[b];
    if (r > p.cum[b]) r = p.cum[b];
    p.stable_frames[b] = r <= 0 ? 0 : (int64_t)p.kmap[b * p.max_frames + (r - 1)] + 1;
  }
}

}  // namespace

hipError_t ctcx_launch_skip_chunk(const CtcxSkipChunkParams& p, hipStream_t s) {
  if (p.B <= 0) return hipSuccess;
  if (p.B > 0x7fffffffLL || p.chunk_time < 0 || p.chunk_time >= 0x7fffffffLL || p.max_frames < 0 ||
      p.max_frames >= 0x7fffffffLL || (p.chunk_time > 0 && (!p.x || !p.norm || !p.ckmap)) || !p.len || !p.state ||
      !p.item || !p.kmap || !p.cidx || !p.klen || !p.cum ||
      (p.xfmt != kSkipInNative && (p.f64 || (p.xfmt != kSkipInF16 && p.xfmt != kSkipInBF16))))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)p.B);
  if (p.chunk_time <= kSkipChunkSmall) {
    if (p.f64) hipLaunchKernelGGL((ctcx_skip_chunk<double, 64>), grid, dim3(64), 0, s, p);
    else hipLaunchKernelGGL((ctcx_skip_chunk<float, 64>), grid, dim3(64), 0, s, p);
  } else {
    if (p.f64) hipLaunchKernelGGL((ctcx_skip_chunk<double, kNT>), grid, dim3(kNT), 0, s, p);
    else hipLaunchKernelGGL((ctcx_skip_chunk<float, kNT>), grid, dim3(kNT), 0, s, p);
  }
  return hipGetLastError();
}

hipError_t ctcx_launch_skip_finish(const CtcxSkipFinishParams& p, hipStream_t s) {
  if (p.B <= 0) return hipSuccess;
  if (p.B > 0x7fffffffLL || !p.item || !p.status || !p.cum || !p.kmap || !p.n_ws) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctcx_skip_finish, dim3((unsigned)((p.B + 255) / 256)), dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t ctcx_launch_skip_plan(const CtcxSkipPlanParams& p, hipStream_t s) {
  if (p.B <= 0) return hipSuccess;
  if (p.B > 0x7fffffffLL || p.Tmax < 0 || p.Tmax >= 0x7fffffffLL || !p.x || !p.norm || !p.seq_len || !p.kmap ||
      !p.cidx || !p.kept || (p.xfmt != kSkipInNative && (p.f64 || (p.xfmt != kSkipInF16 && p.xfmt != kSkipInBF16))))
    return hipErrorInvalidValue;
  if (p.f64)
    hipLaunchKernelGGL(ctcx_skip_plan<double>, dim3((unsigned)p.B), dim3(kNT), 0, s, p);
  else
    hipLaunchKernelGGL(ctcx_skip_plan<float>, dim3((unsigned)p.B), dim3(kNT), 0, s, p);
  return hipGetLastError();
}

template <typename V>
static hipError_t gather_as(const CtcxSkipGatherParams& p, hipStream_t s) {
  const int64_t per = (int64_t)sizeof(V) / p.esize;   // elements per piece
  const int64_t upr = p.C / per;
  const int64_t total = p.Tmax * p.B * upr;
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctcx_skip_gather<V>, dim3((unsigned)blocks), dim3(256), 0, s, (const V*)p.x, (V*)p.xc, p.kmap,
                     p.kept, p.Tmax, p.B, upr, p.xst_t / per, p.xst_b / per, total);
  return hipGetLastError();
}

hipError_t ctcx_launch_skip_gather(const CtcxSkipGatherParams& p, hipStream_t s) {
  if (p.B <= 0 || p.Tmax <= 0 || p.C <= 0) return hipSuccess;
  if (!p.x || !p.xc || !p.kmap || !p.kept || (p.esize != 2 && p.esize != 4 && p.esize != 8))
    return hipErrorInvalidValue;
  // 16-byte pieces: every row of both tensors starts on a 16-byte boundary and is whole pieces
  const int64_t per = 16 / p.esize;
  if (((uintptr_t)p.x & 15) == 0 && ((uintptr_t)p.xc & 15) == 0 && p.C % per == 0 && p.xst_t % per == 0 &&
      p.xst_b % per == 0)
    return gather_as<u32x4>(p, s);
  return p.esize == 2 ? gather_as<uint16_t>(p, s) : p.esize == 4 ? gather_as<uint32_t>(p, s) : gather_as<uint64_t>(p, s);
}

hipError_t ctcx_launch_skip_expand(const CtcxSkipExpandParams& p, hipStream_t s) {
  if (p.B <= 0 || p.P <= 0) return hipSuccess;
  if (p.B * p.P > 0x7fffffffLL || p.Tmax < 0 || p.Tmax >= 0x7fffffffLL || !p.seq || !p.len || !p.frames || !p.kmap ||
      !p.cidx || !p.kept)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctcx_skip_expand, dim3((unsigned)(p.B * p.P)), dim3(kNT), 0, s, p);
  return hipGetLastError();
}
