// ctcx_stream_store.h — shared declarations between the append kernel of a
// stream's score store (ctcx_stream_store.hip) and the C-ABI host layer
// (ctcext_capi.hip): include/ctcext.h, "Streaming: token scores".  The decode
// objects do not depend on this header, and it includes none of theirs: the
// kernel reads the chunk, its normaliser, the prologue's lengths and the items'
// committed frame counts as plain arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// element formats of the chunk and of the store (= CTCEXT_IN_*, ctcx::kIn*)
constexpr int32_t kStoreNative = 0, kStoreF16 = 1, kStoreBF16 = 2;

// ---------------------------------------------------------------------------
// The store's arithmetic, host and device: sx is [B][max_frames][C] of the store's
// element type, snorm [max_frames][B] of the compute dtype -- the x / norm /
// xst_t = C / xst_b = max_frames * C of CtcxScoresParams.

// Bytes per element of sx; 0 for a combination that does not exist (an unknown
// format, or a half store of a float64 stream).
__host__ __device__ inline int ctcx_store_esize(int32_t store_format, int f64) {
  if (store_format == kStoreNative) return f64 ? 8 : 4;
  if ((store_format == kStoreF16 || store_format == kStoreBF16) && !f64) return 2;
  return 0;
}

// Element (frame f, class c) of item b in sx, and its row's normaliser in snorm.
__host__ __device__ inline int64_t ctcx_store_elem(int64_t b, int64_t f, int64_t c, int64_t max_frames, int64_t C) {
  return (b * max_frames + f) * C + c;
}
__host__ __device__ inline int64_t ctcx_store_norm_elem(int64_t b, int64_t f, int64_t B) { return f * B + b; }

// The two buffers' sizes in bytes: false where an argument is negative, the
// format does not exist or a product leaves int64.
inline bool ctcx_store_bytes(int64_t B, int64_t max_frames, int64_t C, int32_t store_format, int f64, int64_t* sx_bytes,
                             int64_t* snorm_bytes) {
  const int es = ctcx_store_esize(store_format, f64);
  if (B < 0 || max_frames < 0 || C < 0 || es == 0) return false;
  int64_t rows, cells;
  if (__builtin_mul_overflow(B, max_frames, &rows) || __builtin_mul_overflow(rows, C, &cells) ||
      __builtin_mul_overflow(cells, (int64_t)es, sx_bytes) ||
      __builtin_mul_overflow(rows, (int64_t)(f64 ? 8 : 4), snorm_bytes))
    return false;
  int64_t total;
  return !__builtin_add_overflow(*sx_bytes, *snorm_bytes, &total);
}

struct CtcxStreamStoreParams {
  const void* x;            // the caller's chunk: (t, b) at x + xst_t * t + xst_b * b elements of xfmt
  const void* norm;         // [chunk_time][B] of the compute dtype: the normaliser of those rows
  const int32_t* len;       // [B] the stream prologue's sanitised chunk lengths (0 for an item with a status bit)
  const int32_t* base;      // item b's frames on the original time axis before this push, as the prologue left
  int64_t base_stride;      // them, at base[b * base_stride]: the committed header's first word, or CtcxSkipItem.n
  void* sx;                 // [B][max_frames][C] of sfmt
  void* snorm;              // [max_frames][B] of the compute dtype
  int64_t chunk_time, max_frames, B, C, xst_t, xst_b;
  int32_t xfmt, sfmt, f64, pad;
};

hipError_t ctcx_launch_stream_store(const CtcxStreamStoreParams& p, hipStream_t s);
