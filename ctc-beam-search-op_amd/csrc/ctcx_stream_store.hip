// ctcx_stream_store.hip — the append kernel of a stream's score store
// (include/ctcext.h, "Streaming: token scores"): the rows of the caller's chunk
// that the push takes, and their normaliser, copied behind what the item holds,
// so that the token-scores kernel can read every committed frame of every item
// as one [B][max_frames][C] tensor.  A translation unit of its own: the decode
// objects neither see nor depend on it.
//
// For item b the destination of a push is one contiguous span of len * C
// elements, sx[b][base .. base + len)[:].  The threads of the item's workgroups
// are indexed over that flat span, element e at frame t = e / C, class
// c = e % C: every store is coalesced, the loads within a source row.  Where C,
// the chunk's pointer and its strides are multiples of four elements a thread
// moves four elements of one row at once (8 to 32 bytes a load and a store);
// otherwise one.  The first len threads of the item also copy the row's
// normaliser.  The grid is sized on the static chunk_time * C and B, so a
// captured push replays; threads past len * C exit.  No LDS, no atomics.
//
// base is read from committed state and the commit runs behind this kernel, so
// an item whose push does not commit keeps its base and the next push writes
// the same rows again: roll-back by position.  The prologue's capacity check
// gives base + len <= max_frames; an item for which that does not hold is not
// written at all.
#include "ctcx_stream_store.h"

namespace {

constexpr int kNT = 256;

// how a source element becomes a store element: the bits, or a half widened as
// the decode kernels' row stage widens it (fp16: the hardware convert; bf16:
// the bits, 16 to the left) -- exact for both
struct Bits {
  template <typename D, typename S>
  static __device__ __forceinline__ D cv(S v) { return v; }
};
struct FromF16 {
  template <typename D, typename S>
  static __device__ __forceinline__ D cv(S v) { return (D)(float)__builtin_bit_cast(_Float16, v); }
};
struct FromBF16 {
  template <typename D, typename S>
  static __device__ __forceinline__ D cv(S v) { return (D)__uint_as_float((unsigned)v << 16); }
};

template <typename S, typename D, typename Cv, int V>
__global__ __launch_bounds__(kNT) void ctcx_stream_store(CtcxStreamStoreParams p, uint32_t gx) {
  typedef S SV __attribute__((ext_vector_type(V)));
  typedef D DV __attribute__((ext_vector_type(V)));
  const uint32_t b32 = blockIdx.x / gx;   // gx workgroups per item
  const int64_t b = b32;
  int64_t len = p.len[b];
  if (len > p.chunk_time) len = p.chunk_time;
  const int64_t base = p.base[b * p.base_stride];
  if (len <= 0 || base < 0 || base > p.max_frames - len) return;
  const int64_t i = (int64_t)(blockIdx.x - b32 * gx) * kNT + threadIdx.x;
  // (launch() gives every item at least chunk_time threads, which this copy relies on: chunk_time * C of them on
  //  the one-element path, C >= 1, and chunk_time * (C / 4) on the four-element one, taken only with C % 4 == 0)
  if (i < len) {
    const int64_t src = i * p.B + b, dst = ctcx_store_norm_elem(b, base + i, p.B);
    if (p.f64) ((double*)p.snorm)[dst] = ((const double*)p.norm)[src];
    else ((float*)p.snorm)[dst] = ((const float*)p.norm)[src];
  }
  const int64_t e = i * V;
  if (e >= len * p.C) return;
  int64_t t, c;
  if (p.chunk_time * p.C <= 0x7fffffffLL) {   // (uniform; the 32-bit division is a fraction of the 64-bit one)
    const uint32_t t32 = (uint32_t)e / (uint32_t)p.C;
    t = t32;
    c = (int64_t)((uint32_t)e - t32 * (uint32_t)p.C);
  } else {
    t = e / p.C;
    c = e - t * p.C;
  }
  const S* const src = (const S*)p.x + t * p.xst_t + b * p.xst_b + c;
  D* const dst = (D*)p.sx + ctcx_store_elem(b, base, 0, p.max_frames, p.C) + e;
  if (V == 1) {
    *dst = Cv::template cv<D, S>(*src);
  } else {   // (C % V == 0: the V elements are of one row)
    const SV v = *(const SV*)src;
    DV w;
    for (int q = 0; q < V; ++q) w[q] = Cv::template cv<D, S>(v[q]);
    *(DV*)dst = w;
  }
}

template <typename S, typename D, typename Cv>
hipError_t launch(const CtcxStreamStoreParams& p, hipStream_t s) {
  constexpr int64_t kV = 4;
  const bool wide = p.C % kV == 0 && p.xst_t % kV == 0 && p.xst_b % kV == 0 &&
                    (uintptr_t)p.x % (kV * sizeof(S)) == 0 && (uintptr_t)p.sx % (kV * sizeof(D)) == 0;
  const int64_t threads = wide ? p.chunk_time * (p.C / kV) : p.chunk_time * p.C;
  const int64_t gx = (threads + kNT - 1) / kNT;
  if (gx > 0x7fffffffLL / p.B) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(gx * p.B));
  if (wide) hipLaunchKernelGGL((ctcx_stream_store<S, D, Cv, (int)kV>), grid, dim3(kNT), 0, s, p, (uint32_t)gx);
  else hipLaunchKernelGGL((ctcx_stream_store<S, D, Cv, 1>), grid, dim3(kNT), 0, s, p, (uint32_t)gx);
  return hipGetLastError();
}

}  // namespace

hipError_t ctcx_launch_stream_store(const CtcxStreamStoreParams& p, hipStream_t s) {
  if (p.B <= 0 || p.chunk_time <= 0) return hipSuccess;
  const int es = ctcx_store_esize(p.sfmt, p.f64);
  if (p.B > 0x7fffffffLL || p.C <= 0 || p.C > 0x7fffffffLL || p.max_frames < 0 || p.base_stride <= 0 || es == 0 ||
      p.chunk_time > 0x7fffffffLL || !p.x || !p.norm || !p.len || !p.base || !p.sx || !p.snorm ||
      (p.xfmt != kStoreNative && (p.f64 || (p.xfmt != kStoreF16 && p.xfmt != kStoreBF16))) ||
      (p.sfmt != kStoreNative && p.xfmt != p.sfmt))
    return hipErrorInvalidValue;
  if (p.sfmt != kStoreNative) return launch<uint16_t, uint16_t, Bits>(p, s);
  if (p.f64) return launch<double, double, Bits>(p, s);
  if (p.xfmt == kStoreF16) return launch<uint16_t, float, FromF16>(p, s);
  if (p.xfmt == kStoreBF16) return launch<uint16_t, float, FromBF16>(p, s);
  return launch<float, float, Bits>(p, s);
}
