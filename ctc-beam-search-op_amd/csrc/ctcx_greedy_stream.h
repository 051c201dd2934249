// ctcx_greedy_stream.h — shared declarations between the push kernel of a
// greedy stream (ctcx_greedy_stream.hip) and the C-ABI host layer
// (ctcext_capi.hip): include/ctcext.h, "Streaming: greedy".  The decode objects
// do not depend on this header, and it includes none of theirs: the kernel reads
// the chunk and appends to the stream's own rows as plain arrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Classes per LDS tile of the per-row pass (a row of up to this many classes
// stays in LDS between the max pass and the sum pass), and the chunk rows of an
// item one step of the push covers (one per lane of the item's wave).
constexpr int kGreedyStreamTile = 32;
constexpr int kGreedyStreamRows = 64;
// Waves of an item's workgroup under the wide-row evaluator, a wave per chunk row.
constexpr int kGreedyStreamWideWaves = 8;

// element formats of the chunk (= CTCEXT_IN_*)
constexpr int32_t kGreedyStreamInNative = 0, kGreedyStreamInF16 = 1, kGreedyStreamInBF16 = 2;
// status bits of a push (= CTCEXT_ITEM_LENGTH, CTCEXT_ITEM_CAPACITY)
constexpr int32_t kGreedyStreamItemLength = 1, kGreedyStreamItemCapacity = 16;
// CtcxGreedyStreamParams.want
constexpr int32_t kGreedyStreamTimes = 1, kGreedyStreamScores = 2;

// What an item carries from push to push; all zero is "no frame yet" (what a
// reset leaves).  The three floats are of the compute dtype, a float32 in the
// low half of its word.
struct CtcxGreedyStreamItem {
  int32_t frames;        // frames taken since the last reset = the alignment row's length
  int32_t dec_len;       // the decoded row's length
  int32_t prev_k1;       // the last frame's class + 1 (0: none)
  int32_t prev_lab1;     // the last candidate's label + 1 (0: none)
  int32_t trailing;      // blank frames the row ends in
  int32_t pad;
  uint64_t logp;         // the running log-probability
  uint64_t ch_sum;       // the open token's score chain over every frame since its start, the blanks behind its
  uint64_t ch_min;       // last run included: committed to the token's cells when a merging run arrives
};
static_assert(sizeof(CtcxGreedyStreamItem) == 48, "CtcxGreedyStreamItem layout");

// Per item, what the pushes since the last ctcext_greedy_stream_check deferred
// (the layout and the meaning of the beam stream's record).  One lane per item
// writes it, in stream order: no atomics.
struct CtcxGreedyStreamAcc {
  int32_t status;        // every CTCEXT_ITEM_* bit the item had
  int32_t cap_total;     // first _CAPACITY: the frames the item would have held
  int64_t len_chunk;     // first _LENGTH: that push's chunk_time
};
static_assert(sizeof(CtcxGreedyStreamAcc) == 16, "CtcxGreedyStreamAcc layout");

struct CtcxGreedyStreamParams {
  const void* x;               // the chunk: (t, b) at x + xst_t * t + xst_b * b elements of xfmt
  const int32_t* chunk_length; // [B] or null: chunk_time for all; negative reads as 0
  const int32_t* reset;        // [B] or null: nonzero starts a new utterance with this chunk
  int64_t chunk_time, max_frames, B, C, xst_t, xst_b;
  int32_t xfmt, f64, blank_index, blank_label, merge, want;
  int32_t wide, pad;           // wide: the wide-row evaluator (a wave per row) instead of lane per row
  int64_t pad_value;
  CtcxGreedyStreamItem* item;  // [B]
  CtcxGreedyStreamAcc* acc;    // [B]
  // the stream's rows, max_frames wide, appended to
  int64_t* decoded;            // [B][max_frames], padded with pad_value
  int64_t* alignment;          // [B][max_frames]
  int32_t* decoded_length;     // [B]
  int32_t* alignment_length;   // [B]
  void* log_probability;       // [B] of the compute dtype
  int32_t* status;             // [B] the bits of this push
  int32_t* frames;             // [B] frames per item after this push
  int32_t* start;              // [B][max_frames], -1 past the decoded length   } want & kGreedyStreamTimes
  int32_t* end;                // [B][max_frames]                               }
  int32_t* trailing_blank;     // [B]                                           }
  void* logp_sum;              // [B][max_frames] of the compute dtype, NaN past the decoded length   } want & kGreedyStreamScores
  void* logp_min;              // [B][max_frames]                                                     }
};

// One launch: a workgroup per item (one wave, or eight with p.wide).
hipError_t ctcx_launch_greedy_push(const CtcxGreedyStreamParams& p, hipStream_t s);
