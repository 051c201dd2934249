// ctcx_tgrad.h — shared declarations between the target-gradients kernel
// (ctcx_tgrad.hip) and the C-ABI host layer (ctcext_capi.hip):
// include/ctcext.h, "Target gradients".  The decode objects do not depend on
// this header, and it includes none of theirs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctcx_targets.h"   // the segments and the staged route's bound of the packed trellis

// Frames between two checkpoints of the forward, which is also the tile of the
// backward: the alpha of a tile lives in LDS as two planes of K * 257 values.
// K = 16 for float32 is the renormalisation period (kPathsRenorm), so a tile
// holds one renormalisation, at its last frame, and every alpha of a tile is
// relative to the one shift its checkpoint carries; with K = 32 the two planes
// alone would take the 64 KiB a workgroup may declare.  float64: 8, the same
// bytes.  The staged route shortens K to the largest power of two whose K rows
// of lp fit one buffer of kTargetsTileBytes (4 at 512 classes).
constexpr int kTgradK32 = 16, kTgradK64 = 8;
constexpr int kTgradPlane = kTargetsThreads + 1;   // (padded: a frame's rows fall into different banks)

__host__ __device__ inline int ctcx_tgrad_tile(int64_t C, int32_t f64, int32_t staged) {
  int k = f64 ? kTgradK64 : kTgradK32;
  if (staged) {
    const int f = ctcx_targets_tile(C, f64);   // >= kTargetsMinTile on this route
    while (k > f) k >>= 1;
  }
  return k;
}

// The checkpoints of one launch (one group of 256 / segment targets per item):
// [B][ceil(Tmax / k)] records (k: the launch's tile) of 256 lanes times (blank state, label state) of
// the compute dtype and the double that the renormalisations took out.
inline int64_t ctcx_tgrad_bytes(int64_t B, int64_t Tmax, int64_t k, int32_t f64) {
  return B * ((Tmax + k - 1) / k) * kTargetsThreads * (2 * (f64 ? 8 : 4) + 8);
}

struct CtcxTgradParams {
  CtcxTargetsParams t;     // the targets and the sources, as the target scores read them; t.out: the scores [B][N]
  const void* weights;     // [B][N] of the compute dtype, or null: ones
  void* grad;              // cell (b, f, c) at grad + ost_b * b + ost_t * f + c, of the compute dtype
  int64_t ost_t, ost_b;
  void* ws;                // ctcx_tgrad_bytes
  int32_t tile;            // frames of a tile: ctcx_tgrad_tile, or a smaller power of two (diagnostics)
  int32_t forward_only;    // diagnostics: stop behind the forward (scores and checkpoints; the slab is not written)
  int64_t group;           // the launch's group of 256 / segment targets (the launcher sets it)
};

// One launch per group of 256 / segment targets, in order on the stream: group 0 stores every cell of the slab,
// the later ones add to it.
hipError_t ctcx_launch_target_grads(const CtcxTgradParams& p, hipStream_t s);
