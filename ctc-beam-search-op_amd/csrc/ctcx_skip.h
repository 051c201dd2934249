// ctcx_skip.h — shared declarations between the blank-frame-skipping kernels
// (ctcx_skip.hip) and the C-ABI host layer (ctcext_capi.hip): include/ctcext.h,
// "Blank-frame skipping".  The decode objects do not depend on this header,
// and it includes none of theirs: the kernels read the inputs, the normaliser
// and the traceback's walk buffers as plain arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Frames of an item one step of the plan and expand kernels covers (one per
// thread); the carries between steps are what the tests' long rows exercise.
constexpr int kSkipTile = 256;

// element formats of x (= CTCEXT_IN_*, ctcx::kIn*)
constexpr int32_t kSkipInNative = 0, kSkipInF16 = 1, kSkipInBF16 = 2;

struct CtcxSkipPlanParams {
  const void* x;            // the caller's rows: (t, b) at x + xst_t * t + xst_b * b elements of xfmt
  const void* norm;         // [Tmax][B] of the compute dtype: the normaliser of those rows (launch_row_norm)
  const int32_t* seq_len;   // [B] lengths; read clamped to [0, Tmax]
  const int32_t* pre;       // [B] the dense prologue's status word, or null: nonzero keeps no frame
  int64_t Tmax, B, xst_t, xst_b;
  int32_t xfmt, f64, blank, pad;
  double thr;               // already rounded to the compute dtype
  int32_t* kmap;            // [B][Tmax]: the frames kept, ascending; entries from kept[b] on are not written
  int32_t* cidx;            // [B][Tmax + 1]: kept frames before t, for t in [0, n]
  int32_t* kept;            // [B]
  int32_t* kept_out;        // [B] the caller's copy, or null
};

struct CtcxSkipGatherParams {
  const void* x;            // as CtcxSkipPlanParams::x
  void* xc;                 // dense [Tmax][B][C] of the same element type: row (j, b) = row (kmap[b][j], b) of x
  const int32_t* kmap;
  const int32_t* kept;
  int64_t Tmax, B, C, xst_t, xst_b;
  int32_t esize;            // bytes per element of x: 2, 4 or 8
};

struct CtcxSkipExpandParams {
  int32_t* seq;             // [B][P][2][Tmax] the traceback's reversed walks; the alignment walks are rewritten
  int32_t* len;             // [P][2][B] their lengths; the alignment walks' are rewritten
  const int32_t* frames;    // [B] the original lengths; read clamped to [0, Tmax]
  const int32_t* kmap;
  const int32_t* cidx;
  const int32_t* kept;
  int64_t Tmax, B;
  int32_t P, blank_label;
};

hipError_t ctcx_launch_skip_plan(const CtcxSkipPlanParams& p, hipStream_t s);
hipError_t ctcx_launch_skip_gather(const CtcxSkipGatherParams& p, hipStream_t s);
hipError_t ctcx_launch_skip_expand(const CtcxSkipExpandParams& p, hipStream_t s);
