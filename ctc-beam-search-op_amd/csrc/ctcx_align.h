// ctcx_align.h — shared declarations between the path-alignment kernels
// (ctcx_align.hip) and the C-ABI host layer (ctcext_capi.hip): include/ctcext.h,
// "Path alignments".  The decode objects do not depend on this header, and it
// includes none of theirs: the kernels read the traceback's walk buffers, the
// normaliser and the logits as plain arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Labels a lane holds in registers (a pair of states each) are 1, 2, 4, 8, 16 or
// 24 by instantiation: a row of m labels runs in the smallest one with
// 64 * k >= m, in both compute dtypes.  Rows above 64 * kAlignMaxBlock labels
// run in the LDS instantiation.
constexpr int kAlignMaxBlock = 24;
// Chunks of 64 slots whose three decision bits share a word in the LDS layout.
constexpr int kAlignLdsChunksPerWord = 10;
// Frames whose back-pointer words the traceback holds in registers ahead of the walk.
constexpr int kAlignPrefetch = 32;
// The widest row the LDS instantiation holds (as the path scores': two states
// of the compute dtype and a label per position, in 160 KiB of LDS)
constexpr int64_t kAlignMaxLdsT32 = 13000, kAlignMaxLdsT64 = 8000;

// element formats of x (= CTCEXT_IN_*, ctcx::kIn*)
constexpr int32_t kAlignInNative = 0, kAlignInF16 = 1, kAlignInBF16 = 2;

struct CtcxAlignParams {
  const int32_t* seq;       // [B][P][2][Tmax] the traceback's reversed walks (0: the decoded row; 1 is not read)
  const int32_t* len;       // [P][2][B] their lengths
  const int32_t* frames;    // [B] frames per item; negative reads as 0
  const int32_t* status;    // [B] the call's final CTCEXT_ITEM_* word, or null: nonzero makes the item's rows unaligned
  const void* x;            // the logits: (t, b) at x + xst_t * t + xst_b * b elements of xfmt
  const void* norm;         // [Tmax][B] of the compute dtype: the decoder's normaliser of those rows
  int64_t Tmax, B, C, xst_t, xst_b;
  int32_t P, xfmt, f64, blank_index;
  int32_t force_lds, blank_label;   // force_lds: every row runs in the LDS instantiation (diagnostics)
  int64_t pad_value;
  // workspace
  uint32_t* bp;             // [B * P][Tmax][ctcx_align_words(Tmax)][64] decision bits (frame 0's are never written or read)
  void* fin;                // [B * P][2] of the compute dtype: the forward's v[S - 1], v[S - 2]
  int32_t* vseq;            // [B][P][2][Tmax] walk 0: a copy of seq's; walk 1: the re-alignment, element i = frame frames - 1 - i
  int32_t* vlen;            // [P][2][B]
  // outputs
  void* logp;               // [B][P] of the compute dtype
  int64_t* alignment;       // [B][P][Tmax], padded with pad_value
  int32_t* alignment_length;   // [B][P]
};

// Host only.  Whether rows of Tmax positions fit an instantiation (the LDS one holds kAlignMaxLdsT*).
bool ctcx_path_align_fits(int64_t Tmax, int32_t f64, int32_t force_lds);
// Host only.  32-bit words a lane stores per frame: the larger of what the register
// instantiation of a row of Tmax labels and the LDS instantiation need.
int64_t ctcx_align_words(int64_t Tmax);
// Host only.  Bytes of one row of the back-pointer workspace: Tmax * ctcx_align_words(Tmax) * 256.
inline int64_t ctcx_align_row_bytes(int64_t Tmax) { return Tmax * ctcx_align_words(Tmax) * 256; }

// The forward kernels: every instantiation rows of up to Tmax labels can need.
hipError_t ctcx_launch_path_align(const CtcxAlignParams& p, hipStream_t s);
// The walk back through the decisions: a launch of its own, so that it sees them.
hipError_t ctcx_launch_path_align_back(const CtcxAlignParams& p, hipStream_t s);
// Un-reverses walk 1 into alignment / alignment_length.
hipError_t ctcx_launch_path_align_emit(const CtcxAlignParams& p, hipStream_t s);
