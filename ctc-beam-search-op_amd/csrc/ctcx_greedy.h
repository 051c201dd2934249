// ctcx_greedy.h — shared declarations between the greedy (best-path) decode
// kernels (ctcx_greedy.hip) and the C-ABI host layer (ctcext_capi.hip):
// include/ctcext.h, "Greedy decode".  The decode objects do not depend on this
// header, and it includes none of theirs: the kernels read the logits and write
// the normaliser, the walk buffers and the status words as plain arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Classes per LDS tile of the per-row pass (a row of up to this many classes
// stays in LDS between the max pass and the sum pass), and the (t, b) rows a
// wave owns.
constexpr int kGreedyTile = 32;
constexpr int kGreedyRows = 64;
// Frames of an item one step of the collapse covers (one per thread of its four
// compaction waves); a fifth wave adds up the frames' log-probabilities.
constexpr int kGreedyFrames = 256;
constexpr int kGreedyThreads = kGreedyFrames + 64;

// element formats of x (= CTCEXT_IN_*, ctcx::kIn*)
constexpr int32_t kGreedyInNative = 0, kGreedyInF16 = 1, kGreedyInBF16 = 2;
// int32 words of the decode's per-item result (its counters), which the collapse zeroes
constexpr int32_t kGreedyItemWords = 8;

struct CtcxGreedyParams {
  const void* x;            // the logits: (t, b) at x + xst_t * t + xst_b * b elements of xfmt
  const int32_t* sl;        // [B] sanitised lengths (0 for an item with a status bit); negative reads as 0
  const int32_t* pre;       // [B] the status bits known before the decode
  int64_t Tmax, B, C, xst_t, xst_b;
  int32_t xfmt, f64, blank_index, blank_label, merge, pad;
  int64_t pad_value;
  // workspace
  void* norm;               // [Tmax][B] of the compute dtype: the normaliser, where the score kernels read it
  int32_t* k;               // [Tmax][B] the arg-max of row (t, b)
  void* lp;                 // [Tmax][B] of the compute dtype: max - norm
  int32_t* seq;             // [B][1][2][Tmax] the traceback's layout: reversed walks (0: decoded, 1: alignment)
  int32_t* len;             // [1][2][B] their lengths
  int32_t* status_ws;       // [B] the final status word the follow-up kernels and ctcext_dense_check read
  int32_t* item;            // [B][kGreedyItemWords] the decode's per-item counters: zeroed
  int32_t* top_kind;        // [B] the decode's path kinds: 0 (a path with labels or none is not "no label seq")
  // outputs
  int64_t* decoded;         // [B][1][Tmax], padded with pad_value
  int64_t* alignment;       // [B][1][Tmax]
  int32_t* decoded_length;  // [B][1]
  int32_t* alignment_length;   // [B][1]
  void* log_probability;    // [B][1] of the compute dtype
  int32_t* status;          // [B] the caller's
};

// Kernel 1: norm, k and lp of every row below its item's length.
hipError_t ctcx_launch_greedy_frames(const CtcxGreedyParams& p, hipStream_t s);
// Kernel 2: one workgroup per item over the k and lp rows kernel 1 wrote.
hipError_t ctcx_launch_greedy_collapse(const CtcxGreedyParams& p, hipStream_t s);
