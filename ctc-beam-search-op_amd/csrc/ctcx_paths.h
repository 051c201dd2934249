// ctcx_paths.h — shared declarations between the path-scores kernels
// (ctcx_paths.hip) and the C-ABI host layer (ctcext_capi.hip): include/ctcext.h,
// "Path scores".  The decode objects do not depend on this header, and it
// includes none of theirs: the kernels read the traceback's walk buffers, the
// normaliser and the logits as plain arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Labels a lane holds in registers (a pair of states each), by instantiation:
// a row of m labels runs in the smallest one with 64 * k >= m.  Rows above
// 64 * kPathsMaxBlock labels run in the LDS instantiation.
constexpr int kPathsBlocks[] = {1, 2, 4, 8, 16, 24};
constexpr int kPathsMaxBlock = 24;
// Frames between two renormalisations of a float32 row's states.
constexpr int kPathsRenorm = 16;
// The widest row the LDS instantiation holds (two states of the compute dtype
// and a label per position, in 160 KiB of LDS)
constexpr int64_t kPathsMaxLdsT32 = 13000, kPathsMaxLdsT64 = 8000;

// element formats of x (= CTCEXT_IN_*, ctcx::kIn*)
constexpr int32_t kPathsInNative = 0, kPathsInF16 = 1, kPathsInBF16 = 2;

struct CtcxPathsParams {
  const int32_t* seq;       // [B][P][2][Tmax] the traceback's reversed walks (0: the decoded row; 1 is not read)
  const int32_t* len;       // [P][2][B] their lengths
  const int32_t* frames;    // [B] frames per item; negative reads as 0
  const int32_t* status;    // [B] the call's final CTCEXT_ITEM_* word, or null: nonzero makes the item's rows NaN
  const void* x;            // the logits: (t, b) at x + xst_t * t + xst_b * b elements of xfmt
  const void* norm;         // [Tmax][B] of the compute dtype: the decoder's normaliser of those rows
  int64_t Tmax, B, C, xst_t, xst_b;
  int32_t P, xfmt, f64, blank_index;
  int32_t force_lds, pad;   // force_lds: every row runs in the LDS instantiation (diagnostics)
  void* path_logp;          // [B][P] of the compute dtype
  // Another source of the rows (ctcx_targets.h, the per-row route of the target
  // scores); all zero: the walk buffers above.  With tgt set, row (b, p) is
  // target p of item b, its labels in reading order; seq and len are not read.
  // A length outside [0, tgt_L] makes the row NaN, one above the item's frames
  // -inf; int64 labels are checked against [0, C) before they are narrowed.
  const void* tgt;          // [B][P][tgt_L], or [P][tgt_L] with tgt_shared; int32, or int64 with tgt_i64
  const int32_t* tgt_len;   // [B][P], or [P] with tgt_shared
  int64_t tgt_L;
  int32_t tgt_shared, tgt_i64;
};

// The widest row of a call: no row has more labels than frames.
__host__ __device__ inline int64_t ctcx_paths_width(const CtcxPathsParams& p) {
  return p.tgt_len && p.tgt_L < p.Tmax ? p.tgt_L : p.Tmax;
}

// Whether rows of Tmax positions (ctcx_paths_width) fit an instantiation (the LDS one holds kPathsMaxLdsT*); host only.
bool ctcx_path_scores_fits(int64_t Tmax, int32_t f64, int32_t force_lds);
hipError_t ctcx_launch_path_scores(const CtcxPathsParams& p, hipStream_t s);
