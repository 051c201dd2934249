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

// ---------------------------------------------------------------------------
// Streams (include/ctcext.h, "Streaming: blank-frame skipping"): the plan of one
// chunk on top of what the item carries from its earlier pushes, and the kernel
// behind the commit that makes the push's outcome the item's.

// Per item of a skipping stream.  n and dom are committed; the chunk plan leaves
// the values after the running push in n_next / dom_next, and the finish kernel
// commits them where the push let the item advance.
struct CtcxSkipItem {
  int32_t n;        // frames received since the last reset, on the original time axis
  int32_t dom;      // frame n - 1 was blank-dominant (0 with n == 0)
  int32_t n_next, dom_next;
};
static_assert(sizeof(CtcxSkipItem) == 16, "CtcxSkipItem layout");

// Chunks up to this many frames get one wave per item, longer ones a workgroup
// of kSkipTile threads.
constexpr int kSkipChunkSmall = 128;

struct CtcxSkipChunkParams {
  const void* x;            // the chunk's rows, as CtcxSkipPlanParams::x
  const void* norm;         // [chunk_time][B] of the compute dtype
  const int32_t* len;       // [B] the stream prologue's sanitised chunk lengths (0 for an item with a status bit)
  const char* state;        // the committed state buffer: its first int32 per item is the record (kept) frames
  int64_t stride;
  CtcxSkipItem* item;       // [B]
  int64_t chunk_time, max_frames, B, xst_t, xst_b;
  int32_t xfmt, f64, blank, pad;
  double thr;               // already rounded to the compute dtype
  int32_t* kmap;            // [B][max_frames]: appended from the committed kept count, original frame numbers
  int32_t* cidx;            // [B][max_frames + 1]: appended from n, kept frames before each original frame
  int32_t* ckmap;           // [B][chunk_time]: the chunk's kept frames counted from its first (the gather's map)
  int32_t* klen;            // [B] out: frames of this chunk kept (the pre-pass's and the decode's lengths)
  int32_t* cum;             // [B] out: kept frames including this push (the traceback's lengths)
};

struct CtcxSkipFinishParams {
  CtcxSkipItem* item;       // [B]
  const int32_t* status;    // [B] the commit kernel's status of this push
  int32_t dead_mask;        // its bits that kept the item's decode from being committed
  int32_t pad;
  const int32_t* cum;       // [B] kept frames after the commit
  const int32_t* kmap;      // [B][max_frames]
  int64_t max_frames, B;
  int32_t* n_ws;            // [B] out: n after this push (what the expansion and the token times read as frames)
  int32_t* frames;          // [B] out or null: the caller's copy of it
  int32_t* kept;            // [B] out or null
  int64_t* stable_frames;   // [B] or null: record frames in, original frames out
};

hipError_t ctcx_launch_skip_plan(const CtcxSkipPlanParams& p, hipStream_t s);
hipError_t ctcx_launch_skip_chunk(const CtcxSkipChunkParams& p, hipStream_t s);
hipError_t ctcx_launch_skip_finish(const CtcxSkipFinishParams& p, hipStream_t s);
hipError_t ctcx_launch_skip_gather(const CtcxSkipGatherParams& p, hipStream_t s);
hipError_t ctcx_launch_skip_expand(const CtcxSkipExpandParams& p, hipStream_t s);
