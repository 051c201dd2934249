// ctcx_targets.h — shared declarations between the target-scores kernel
// (ctcx_targets.hip) and the C-ABI host layer (ctcext_capi.hip):
// include/ctcext.h, "Target scores".  The decode objects do not depend on this
// header, and it includes none of theirs: the kernel reads the caller's
// targets, the normaliser and the logits as plain arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// The packed kernel holds targets of at most kTargetsMaxPacked labels (a
// segment of 64 lanes: 63 pairs and the final blank); longer lists take the
// per-row kernels of ctcx_paths.hip.
constexpr int64_t kTargetsMaxPacked = 63;
constexpr int kTargetsThreads = 256;
// The staged route: one buffer of the LDS tile holds kTargetsTileBytes, which
// is kTargetsThreads * 32 bytes, so a thread moves eight floats or four doubles
// a tile.  A tile is F = min(kTargetsMaxTile, kTargetsTileBytes / (C * size))
// whole rows of lp.
//
// The bound between the routes: a class count is staged while F >= 4, that is
// C <= 512 (float32) or C <= 256 (float64).  Staging moves C elements a frame
// for the workgroup's 256 lanes; above that bound it would move more than the
// lanes gather by themselves, a tile would amortise its barrier over fewer than
// four frames, and two buffers per workgroup are what keeps eight workgroups
// on a compute unit.
constexpr int kTargetsTileBytes = 8192, kTargetsMaxTile = 32, kTargetsMinTile = 4;

// Frames per LDS tile of the staged route, or 0: the gathered route.  Host and device.
__host__ __device__ inline int ctcx_targets_tile(int64_t C, int32_t f64) {
  if (C <= 0) return 0;
  const int64_t f = kTargetsTileBytes / (C * (f64 ? 8 : 4));
  return f < kTargetsMinTile ? 0 : f > kTargetsMaxTile ? kTargetsMaxTile : (int)f;
}
// Lanes of a target's segment: the smallest of 8, 16, 32, 64 with max_target + 1 slots; 0: none holds it.
constexpr int ctcx_targets_segment(int64_t L) {
  return L < 0 || L > kTargetsMaxPacked ? 0 : L < 8 ? 8 : L < 16 ? 16 : L < 32 ? 32 : 64;
}

struct CtcxTargetsParams {
  const void* targets;           // [B][N][L], or [N][L] with shared; int32, or int64 with labels_i64
  const int32_t* target_length;  // [B][N], or [N] with shared
  const int32_t* frames;         // [B] frames per item; clamped to [0, Tmax]
  const int32_t* status;         // [B] the call's final CTCEXT_ITEM_* word, or null: nonzero makes the item's rows NaN
  const void* x;                 // the logits: (t, b) at x + xst_t * t + xst_b * b elements of xfmt
  const void* norm;              // [Tmax][B] of the compute dtype
  int64_t Tmax, B, C, xst_t, xst_b, N, L;
  int32_t xfmt, f64, blank_index, shared, labels_i64;
  int32_t staged;                // 1: the LDS tile (ctcx_targets_tile(C, f64) > 0); 0: every lane gathers
  void* out;                     // [B][N] of the compute dtype
};

hipError_t ctcx_launch_target_scores(const CtcxTargetsParams& p, hipStream_t s);
