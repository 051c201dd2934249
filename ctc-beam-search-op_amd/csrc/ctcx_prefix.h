// ctcx_prefix.h — shared declarations between the prefix-scores kernels
// (ctcx_prefix.hip) and the C-ABI host layer (ctcext_capi.hip):
// include/ctcext.h, "Prefix scores".  The decode objects do not depend on this
// header, and it includes none of theirs: the kernels read the caller's
// prefixes, the normaliser and the logits as plain arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctcx_targets.h"   // the segments and the staged tile of the packed trellis

constexpr int kPrefixThreads = 256;
// Kernel B, the extension reduce.  A workgroup owns kPrefixWideClasses
// consecutive classes, one per thread (wide), or kPrefixNarrowClasses classes
// times kPrefixNarrowSlices interleaved time slices (narrow); a group of G
// prefixes runs as G (maximum, sum) pairs a thread; the group's tails pass
// through LDS in tiles of kPrefixTile frames, two buffers.
constexpr int kPrefixWideClasses = 256, kPrefixNarrowClasses = 32;
constexpr int kPrefixNarrowSlices = kPrefixThreads / kPrefixNarrowClasses;
constexpr int kPrefixTile = 64;
// Measured ("Prefix scores"): the narrow layout is the faster one up
// to 512 classes and level with the wide one at 5000; G = 4 was the fastest
// narrow group of 4, 8 and 16 (more workgroups for a small alphabet), G = 8 the
// fastest wide one.
constexpr int kPrefixGroupNarrow = 4, kPrefixGroupWide = 8;   // the G of a layout
constexpr int64_t kPrefixWideFrom = 512;                       // class counts above it run wide

// 0 narrow, 1 wide.  Host and device.
__host__ __device__ inline int32_t ctcx_prefix_layout(int64_t C, int32_t /*f64*/) { return C > kPrefixWideFrom ? 1 : 0; }

// The tails workspace of a call: [B][N][Tmax][2] of the compute dtype (bl_f,
// nb_f), then one int32 a prefix: its last label, -1 for the empty prefix, -2
// for a row that is NaN.
inline int64_t ctcx_prefix_tails_bytes(int64_t B, int64_t N, int64_t Tmax, int32_t f64) {
  return B * N * Tmax * 2 * (f64 ? 8 : 4);
}
inline int64_t ctcx_prefix_bytes(int64_t B, int64_t N, int64_t Tmax, int32_t f64) {
  return ctcx_prefix_tails_bytes(B, N, Tmax, f64) + B * N * 4;
}

struct CtcxPrefixParams {
  CtcxTargetsParams t;   // the prefixes and the sources, as the target scores read them; t.out is not used
  void* tails;           // [B][N][Tmax][2] of the compute dtype
  int32_t* info;         // [B][N]
  int32_t rows;          // Kernel A: 1 one wave per prefix (L > kTargetsMaxPacked, or forced); 0 the packed trellis
  int32_t layout;        // Kernel B: 0 narrow, 1 wide
  void* ext;             // [B][N][C] of the compute dtype
};

// Whether the per-row forward holds prefixes of L labels: min(L, Tmax) within the path scores' LDS limits; host only.
bool ctcx_prefix_rows_fit(int64_t L, int64_t Tmax, int32_t f64);
// Kernel A: the forward of every prefix, its two tail states of every frame into p.tails, its word into p.info.
hipError_t ctcx_launch_prefix_tails(const CtcxPrefixParams& p, hipStream_t s);
// Kernel B: p.ext from p.tails, p.info and the logits.
hipError_t ctcx_launch_prefix_reduce(const CtcxPrefixParams& p, hipStream_t s);
