// ctcx_times.h — shared declarations between the token-times kernel
// (ctcx_times.hip) and the C-ABI host layer (ctcext_capi.hip): include/ctcext.h,
// "Token times".  The decode objects do not depend on this header, and it
// includes none of theirs: the kernel reads the traceback's walk buffers as
// plain int32 arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Elements of a row one step of the kernel covers (one per thread); the carry
// between steps is what the tests' tile-straddling cases exercise.
constexpr int kTimesTile = 256;

struct CtcxTimesParams {
  const int32_t* seq;       // [B][P][2][Tmax] the traceback's reversed walks (0: decoded, 1: alignment)
  const int32_t* len;       // [P][2][B] their lengths
  const int32_t* frames;    // [B] frames per item (sanitised lengths, or a stream's cum); negative reads as 0
  const int32_t* status;    // [B] the call's final CTCEXT_ITEM_* word, or null: nonzero empties the item's rows
  int64_t Tmax, B;          // Tmax is also the width of the output rows
  int32_t P, merge, blank_label, pad;
  int32_t* start;           // [B][P][Tmax], or null with end
  int32_t* end;             // [B][P][Tmax]
  int32_t* trailing_blank;  // [B][P], or null
};

hipError_t ctcx_launch_token_times(const CtcxTimesParams& p, hipStream_t s);
