// ctcx_stream_dense.h — shared declarations between the kernels of the
// enqueue-only push (ctcx_stream_dense.hip) and the C-ABI host layer
// (ctcext_capi.hip): include/ctcext.h, "Streaming: enqueue-only push".
// Include after ctcx_kernels.h with CTCX_STREAM_HOST defined (the kernels read
// and write the committed CtcxStreamHdr), like ctcx_stable.h.  The decode
// objects do not depend on this header.
#pragma once

#include "ctcx_kernels.h"
#include "ctcx_stable.h"
#include "ctcx_skip.h"

constexpr int32_t kCtcxItemCapacity = 16;   // = CTCEXT_ITEM_CAPACITY

// Per item, what the enqueue-only pushes since the last ctcext_stream_check
// deferred.  One thread (the prologue) or one workgroup (the commit) per item
// writes it, in stream order: no atomics.
struct CtcxStreamAcc {
  int32_t status;        // every CTCEXT_ITEM_* bit the item had
  int32_t cap_total;     // first _CAPACITY: the frames the item would have held
  int64_t len_chunk;     // first _LENGTH: that push's chunk_time
};
static_assert(sizeof(CtcxStreamAcc) == 16, "CtcxStreamAcc layout");

struct CtcxStreamPrologueParams {
  const int32_t* chunk_length;  // [B] the caller's, or null: chunk_time for all
  const int32_t* reset;         // [B] nonzero: the item starts a new utterance with this chunk; or null
  char* state;                  // the committed state buffer: item b's CtcxStreamHdr at state + b * stride
  int64_t stride;
  CtcxStableCache* cache;       // [B]
  int32_t* sl;                  // [B] out: the length the pre-pass and the decode kernel read
  int32_t* cum;                 // [B] out: frames including this push (the traceback's lengths)
  int32_t* pre;                 // [B] out: kItemLength / kCtcxItemCapacity of this push
  CtcxStreamAcc* acc;           // [B]
  int64_t chunk_time, max_frames, B;
  CtcxSkipItem* skip;           // [B] a skipping stream's items, or null.  With it reset[b] clears the item's
                                // entry too, and the capacity is judged on its n (the original time axis), not
                                // on the header's record frames
};

struct CtcxStreamCommitParams {
  char* committed;              // the buffer the decode read: overwritten with ...
  const char* written;          // ... the one it wrote, for every item whose hand-over held
  int64_t stride;
  int64_t copy_bytes;           // header + top arrays + image, a multiple of 16, <= stride
  ctcx::ItemOut* item;          // [B] the decode's; rewritten from the committed header where it failed
  int32_t* top_pos;             // [B][P]   likewise
  int32_t* top_kind;            // [B][P]
  void* log_prob;               // [B][P] of T
  const int32_t* pre;           // [B]
  int32_t* cum;                 // [B] put back to the committed frames where the decode failed
  CtcxStreamAcc* acc;           // [B]
  int32_t* status_ws;           // [B] this push's final status (the workspace copy ctcx_pack_dense also writes)
  int32_t* status;              // [B] the caller's, or null
  int32_t* frames;              // [B] the caller's, or null
  int64_t B;
  int32_t P, f64;
  int32_t few_leaves;           // this push returns hypotheses: fewer leaves than P is kItemFewLeaves
  int32_t pad;
};

hipError_t ctcx_launch_stream_prologue(const CtcxStreamPrologueParams& p, hipStream_t s);
hipError_t ctcx_launch_stream_commit(const CtcxStreamCommitParams& p, hipStream_t s);
