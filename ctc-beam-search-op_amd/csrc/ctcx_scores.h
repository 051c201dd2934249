// ctcx_scores.h — shared declarations between the token-scores kernel
// (ctcx_scores.hip) and the C-ABI host layer (ctcext_capi.hip): include/ctcext.h,
// "Token scores".  The decode objects do not depend on this header, and it
// includes none of theirs: the kernel reads the traceback's walk buffers, the
// token spans, the normaliser and the logits as plain arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Frames of a row one step of the kernel covers (one per thread), aligned to
// multiples of it on the item's time axis; a token whose span crosses a
// multiple carries its sum and minimum between steps, which is what the tests'
// tile-straddling cases exercise.
constexpr int kScoresTile = 256;

// element formats of x (= CTCEXT_IN_*, ctcx::kIn*)
constexpr int32_t kScoresInNative = 0, kScoresInF16 = 1, kScoresInBF16 = 2;

struct CtcxScoresParams {
  const int32_t* seq;       // [B][P][2][Tmax] the traceback's reversed walks (1: alignment; 0 is not read)
  const int32_t* len;       // [P][2][B] their lengths
  const int32_t* frames;    // [B] frames per item; negative reads as 0
  const int32_t* status;    // [B] the call's final CTCEXT_ITEM_* word, or null: nonzero empties the item's rows
  const int32_t* start;     // [B][P][Tmax] what the token-times kernel wrote; any value is safe
  const int32_t* end;       // [B][P][Tmax]
  const void* x;            // the logits: (t, b) at x + xst_t * t + xst_b * b elements of xfmt
  const void* norm;         // [Tmax][B] of the compute dtype: the decoder's normaliser of those rows
  int64_t Tmax, B, C, xst_t, xst_b;   // Tmax is also the width of the output rows
  int32_t P, xfmt, f64, blank_index, blank_label, pad;
  void* logp_sum;           // [B][P][Tmax] of the compute dtype, or null
  void* logp_min;           // [B][P][Tmax], or null (not both)
};

hipError_t ctcx_launch_token_scores(const CtcxScoresParams& p, hipStream_t s);
