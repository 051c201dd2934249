/* ctcext.h — C ABI of the MI355X CTC beam-search decoder with per-beam
 * best-alignment tracking (libctcext.so).
 *
 * This is the drop-in boundary for the reference TensorFlow op
 *   REGISTER_OP("CTCExtBeamSearchDecoder")
 *       cc/ops/ctc_ext_beam_search_decoder_ops.cc:9-63
 *   CTCExtBeamSearchDecoderOp<T>::Compute
 *       cc/kernels/ctc_ext_beam_search_decoder_kernels.cc:20-95
 * (paths relative to /root/reference/tensorflow_ctc_ext_beam_search_decoder/).
 * Plain pointers and sizes only; no framework types cross it.  A TF OpKernel
 *  or the ctypes binding in ctcext_amd/_lib.py calls it.
 *
 * Two phases, like the reference kernel which counts entries before
 * allocating its outputs (kernels.cc:170-213):
 *   1. ctcext_decode: validates, decodes the whole batch on the GPU and
 *      returns, per top path, the SparseTensor entry counts and dense widths.
 *   2. ctcext_fetch: writes the int64 SparseTensor components and the
 *      log-probabilities into caller-allocated buffers (device or host).
 * Status codes are TensorFlow's (error::Code); messages are the reference's
 * verbatim (kernels.cc:111-139, ctc_ext_beam_search_decoder.h:237-243).
 */
#ifndef CTCEXT_H_
#define CTCEXT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  CTCEXT_OK = 0,
  CTCEXT_INVALID_ARGUMENT = 3,   /* errors::InvalidArgument */
  CTCEXT_FAILED_PRECONDITION = 9,/* errors::FailedPrecondition */
  CTCEXT_UNIMPLEMENTED = 12,
  CTCEXT_INTERNAL = 13
};

enum { CTCEXT_F32 = 0, CTCEXT_F64 = 1 };   /* attr T: {float, double} (ops.cc:24) */

/* Element type of the inputs in memory (ctcext_decode_args.inputs_format).
 * dtype stays the compute and output type; a half format needs CTCEXT_F32:
 * the kernels widen each element to float as they read it (exact for both
 * formats), so the outputs are those of decoding the widened float tensor. */
enum { CTCEXT_IN_NATIVE = 0,   /* elements of dtype */
       CTCEXT_IN_F16 = 1,      /* IEEE binary16 */
       CTCEXT_IN_BF16 = 2 };   /* bfloat16 */

/* Beam scorer (util/ctc_beam_scorer.h:31-65).  The reference op always uses
 * BaseBeamScorer (kernels.cc:260), the identity; the decoder exposes the hook
 * (ctc_ext_beam_search_decoder.h:43-45, 103, 114, 171-182, 226).
 *   CTCEXT_SCORER_BIGRAM: ExpandState caches table[from_label + 1][to_label]
 *   (row 0: expansions of the root), GetStateExpansionScore adds it to the
 *   score it extends.  table is [num_classes + 1][num_classes] of dtype, in
 *   the memory inputs_on_device says; entries are log-probabilities (<= 0). */
enum { CTCEXT_SCORER_BASE = 0, CTCEXT_SCORER_BIGRAM = 1 };

enum {
  CTCEXT_FLAG_FORCE_LITERAL = 1,   /* testing: replay every frame through the literal TopN model */
  CTCEXT_FLAG_PROFILE = 2,         /* time the decode kernel with HIP events (ctcext_stats) */
  CTCEXT_FLAG_PHASES = 4,          /* diagnostics: per-item s_memtime phase counters */
  CTCEXT_FLAG_GLOBAL_STATE = 8,    /* testing: decode on the global-state tier whatever the shape */
  CTCEXT_FLAG_RECORD_RING = 16,    /* keep beam records in an LDS ring and write only those the
                                      traceback can reach (fewer HBM writes).  On by default
                                      where the score-table two-wave kernel runs (float,
                                      beam_width <= 128, num_classes <= 64); opt-in elsewhere */
  CTCEXT_FLAG_RING_MIN = 32,       /* testing: the record ring at its smallest (8 frames), so short
                                      items flush; implies CTCEXT_FLAG_RECORD_RING */
  CTCEXT_FLAG_NO_RING = 64,        /* write every beam record to HBM (no record ring) */
  CTCEXT_FLAG_HELPER_STRICT = 128, /* a two-wave kernel's hand-over wait that runs out of time
                                      (~1 s; never in a correct run) fails the call with
                                      CTCEXT_INTERNAL instead of decoding it again with the
                                      one-wave kernels (ctcext_stats.helper_redecodes) */
  CTCEXT_FLAG_TEST_HELPER_DEAD = 256 /* testing: the helper wave starts out as if its first
                                      wait had run out of time (the failure path, no hang) */
};

/* Version of this header's structs and entry points.  ctcext_stats only ever
 * grows at its end: callers built against an older header use
 * ctcext_get_stats_sized with their sizeof.
 *   4: ctcext_stats.record_bytes, .helper     5: .helper_redecodes,
 *      ctcext_get_stats_sized, ctcext_abi_version, the HELPER_STRICT flag
 *   6: ctcext_get_stats fills the ABI-4 prefix only (fields since: _sized);
 *      ctcext_phase_counters' layout is [batch][32]
 *   7: ctcext_decode_args.inputs_format, .inputs_stride_t, .inputs_stride_b
 *      (appended; zero = the dense [max_time, batch, num_classes] tensor of dtype)
 *   8: ctcext_stats.kernel (the former pad_: same size and offsets);
 *      ctcext_stats.early_recursed_frames (appended: ctcext_get_stats_sized) */
#define CTCEXT_ABI_VERSION 8

typedef struct ctcext_decoder ctcext_decoder;

/* Replaces the op's inputs + attrs (ops.cc:10-17).  The two input tensors
 * travel as (pointer, rank, sizes), the way an OpKernel sees them, so that the
 * reference's shape checks (kernels.cc:111-131) run behind this ABI. */
typedef struct {
  int32_t dtype;                   /* CTCEXT_F32 / CTCEXT_F64 */
  int32_t inputs_on_device;        /* 1: inputs/sequence_length are device (HBM) pointers
                                      on the decoder's (root) device */
  const void* inputs;              /* [max_time, batch_size, num_classes] row-major (or as
                                      inputs_format / inputs_stride_* below say) */
  const int32_t* sequence_length;  /* [batch_size] */
  int64_t max_time, batch_size, num_classes;   /* inputs.dim_size(0..2) (0 past the rank) */
  int32_t beam_width;              /* attr beam_width >= 1 */
  int32_t top_paths;               /* attr top_paths >= 1 */
  int32_t merge_repeated;          /* attr merge_repeated (default false) */
  int32_t blank_index;             /* attr blank_index (default 0) */
  int32_t blank_label;             /* attr blank_label (default -1) */
  int32_t flags;                   /* CTCEXT_FLAG_* */
  void* stream;                    /* hipStream_t; NULL = the decoder's own stream */
  int32_t inputs_dims;             /* inputs.dims(): must be 3 (kernels.cc:111-113) */
  int32_t sequence_length_dims;    /* sequence_length.dims(): must be 1 (kernels.cc:122-124) */
  int64_t sequence_length_size;    /* sequence_length.dim_size(0): must equal batch_size
                                      (kernels.cc:126-130); the number of int32 read */
  int32_t scorer;                  /* CTCEXT_SCORER_* (0: the reference op's BaseBeamScorer) */
  int32_t pad_;
  const void* scorer_table;        /* CTCEXT_SCORER_BIGRAM: [num_classes + 1][num_classes] */
  /* ABI 7.  All zero: today's dense tensor of dtype (callers that zero the
   * struct, or were written before these fields, need no change). */
  int32_t inputs_format;           /* CTCEXT_IN_*: the element type inputs points at */
  int32_t pad2_;
  int64_t inputs_stride_t;         /* element strides of the frame and the item dimension */
  int64_t inputs_stride_b;         /*   (the class stride is 1): element (t, b, c) is at
                                      inputs[t * stride_t + b * stride_b + c].  Both 0: the
                                      dense reference layout (batch * num_classes,
                                      num_classes); dense batch-major [B, T, C] is
                                      (num_classes, max_time * num_classes).  Device inputs
                                      are read in place through the strides */
} ctcext_decode_args;

/* Per top path p: sizes of decoded_indices[p] ([num_decoded, 2]),
 * decoded_values[p] ([num_decoded]), decoded_shape[p] = {batch, max_decoded},
 * and the same for the alignment outputs. */
typedef struct {
  int64_t num_decoded, max_decoded;
  int64_t num_alignment, max_alignment;
} ctcext_path_sizes;

/* Replaces the op's 6 * top_paths + 1 outputs (ops.cc:18-24).  Each list is an
 * array of top_paths pointers; shapes as in ctcext_path_sizes. */
typedef struct {
  int32_t outputs_on_device;       /* 1: all pointers below are device pointers */
  int64_t* const* decoded_indices;
  int64_t* const* decoded_values;
  int64_t* const* decoded_shape;
  int64_t* const* alignment_indices;
  int64_t* const* alignment_values;
  int64_t* const* alignment_shape;
  void* log_probability;           /* [batch_size, top_paths] of dtype */
} ctcext_outputs;

typedef struct {
  int64_t literal_frames;          /* frames replayed through the literal TopN model */
  int64_t literal_nonfinite;       /*   ... because a total or logit was not finite */
  int64_t literal_fill;            /*   ... because the beam filled up mid-frame */
  int64_t duplicate_frames;        /* frames whose beam held one entry twice (reachable
                                      with -inf logits: decoder.h:142 + 189-199) */
  int64_t no_label_paths;          /* paths whose alignment is empty: the reference prints
                                      "No label seq available" (ctc_beam_entry.h:148-150) */
  double decode_kernel_ms;         /* with CTCEXT_FLAG_PROFILE: last ctcx_beam_decode time
                                      (the slowest device of a sharded handle) */
  double norm_kernel_ms;
  double traceback_ms;             /* traceback + scan */
  int32_t n_devices;               /* devices of the handle */
  int32_t tier;                    /* last decode: 0 the LDS-resident fast tier, 1 the
                                      global-state tier (shapes past the LDS / record limits) */
  int32_t ring_frames;             /* last decode: frames of the LDS record ring (0: every
                                      record of every frame written to HBM) */
  int64_t records_written;         /* last decode: beam records written to HBM (all devices) */
  int32_t record_bytes;            /* last decode: bytes per record (8; 16 on the global-state
                                      tier; 4 in the two-wave kernel, beam_width <= 128 and
                                      num_classes <= 64) */
  int32_t helper;                  /* last decode: the two-wave kernel that ran (0: the one-wave
                                      kernel; 1: score-table helper; 2: gather-queue helper) */
  int32_t helper_redecodes;        /* last decode: 1 if a two-wave kernel's hand-over wait ran
                                      out of time and the call was decoded again with the
                                      one-wave kernels (helper is then 0) */
  int32_t kernel;                  /* last decode, root device: the kernels its launchers ran
                                      (CTCEXT_KERNEL_* below); after ctcext_row_facts, the
                                      pre-pass field alone */
  int64_t early_recursed_frames;   /* last decode: frames, summed over items, whose recursion
                                      the helper wave computed during the frame before (the
                                      small-C scored two-wave kernel; a stream's count is
                                      cumulative, like its other counters) */
} ctcext_stats;

/* ctcext_stats.kernel.  Each launcher records what it launched, so the value
 * is the dispatcher's own choice, not a second copy of its rules:
 *   bit 0       HW: a two-wave decode kernel (128 threads per item)
 *   bit 1       SQ: ... its scored gather queue
 *   bits 2..4   RN: heap registers per lane (1, 2, 4)
 *   bits 5..6   WC / 128: the compile-time beam capacity (128, 256; 0: the
 *               layout is carved from the run-time beam_width)
 *   bit 7       BIG: the num_classes > 64 build
 *   bit 8       the bigram beam scorer (0: BaseBeamScorer)
 *   bit 9       double (0: float)
 *   bit 10      the global-state tier's kernel (ctcext_stats.tier == 1)
 *   bit 11      a decode kernel was launched
 *   bits 12..14 the pre-pass, CTCEXT_PREPASS_*
 *   bit 15      a stream build of the decode kernel (CTCEXT_KERNEL_STREAM, below)
 *   bits 16..17 the traceback, CTCEXT_TRACEBACK_* */
#define CTCEXT_KERNEL_HW 0x1
#define CTCEXT_KERNEL_SQ 0x2
#define CTCEXT_KERNEL_RN(k) (((k) >> 2) & 7)
#define CTCEXT_KERNEL_WC(k) ((((k) >> 5) & 3) * 128)
#define CTCEXT_KERNEL_BIG 0x80
#define CTCEXT_KERNEL_BIGRAM 0x100
#define CTCEXT_KERNEL_F64 0x200
#define CTCEXT_KERNEL_GSTATE 0x400
#define CTCEXT_KERNEL_LAUNCHED 0x800
#define CTCEXT_KERNEL_DECODE_MASK 0xfff
#define CTCEXT_KERNEL_PREPASS(k) (((k) >> 12) & 7)
#define CTCEXT_KERNEL_TRACEBACK(k) (((k) >> 16) & 3)
enum { CTCEXT_PREPASS_NONE = 0,
       CTCEXT_PREPASS_FACTS_FUSED = 1,    /* ctcx_row_facts with the normaliser (one read) */
       CTCEXT_PREPASS_FACTS_NORM = 2,     /* ctcx_row_facts, then a row-norm kernel */
       CTCEXT_PREPASS_ROW_PREP_LDS = 3,   /* ctcx_row_prep, the row staged in LDS */
       CTCEXT_PREPASS_ROW_PREP_GLOBAL = 4,/* ctcx_row_prep, the row read from global memory */
       CTCEXT_PREPASS_NORM_ONLY = 5 };    /* ctcx_row_norm (num_classes <= 64, global-state tier) */
enum { CTCEXT_TRACEBACK_NONE = 0,
       CTCEXT_TRACEBACK_SEGMENTED = 1,    /* ctcx_traceback_seg: one block per item */
       CTCEXT_TRACEBACK_ONE_THREAD = 2 }; /* ctcx_traceback: one thread per walk */

/* Handle lifetime.  A handle owns a HIP stream and a grow-only device
 * workspace; it is not thread-safe (use one per thread, like an OpKernel).
 * Every entry point restores the calling thread's current HIP device. */
int ctcext_create(int device, ctcext_decoder** out);
void ctcext_destroy(ctcext_decoder* dec);

/* Multi-device handle for one process driving several GPUs: the batch is split
 * into contiguous shards balanced by sum(sequence_length), one per device
 * (devices[0] is the root: inputs_on_device pointers live there, and the
 * outputs are assembled there).  Each device decodes its shard on its own
 * stream; the per-item walks are gathered to the root over peer copies (xGMI)
 * and packed there, so the outputs are identical to a one-device decode.  The
 * same device may be listed twice (its shards then share its CUs).  Use it
 * with ctcext_decode_sharded + ctcext_fetch. */
int ctcext_create_sharded(const int* devices, int n_devices, ctcext_decoder** out);

/* The reference's ValidateInputsGenerateOutputs (kernels.cc:97-139) plus this
 * library's attribute checks, on the host only (no HIP call, no handle): the
 * messages are the reference's verbatim and come in its order.  The
 * sequence_length values (kernels.cc:134-139) are checked here only when they
 * are host memory (inputs_on_device == 0); ctcext_decode checks them always.
 * After all of those, the ABI-7 fields (CTCEXT_INVALID_ARGUMENT each):
 *   "inputs_format must be CTCEXT_IN_NATIVE, CTCEXT_IN_F16 or CTCEXT_IN_BF16"
 *   "half-precision inputs need dtype float32"
 *   "inputs_stride_t and inputs_stride_b must be given together"
 *   "inputs_stride_t is below num_classes"   (max_time > 1 only)
 *   "inputs_stride_b is below num_classes"   (batch_size > 1 only) */
int ctcext_validate(const ctcext_decode_args* args);

/* Phase 1 (Compute up to the allocation of the outputs).  Synchronous. */
int ctcext_decode(ctcext_decoder* dec, const ctcext_decode_args* args, ctcext_path_sizes* sizes);

/* Phase 1 over a ctcext_create_sharded handle (kernels.cc:68-90's batch loop
 * split across devices).  On a one-device handle it is ctcext_decode. */
int ctcext_decode_sharded(ctcext_decoder* dec, const ctcext_decode_args* args, ctcext_path_sizes* sizes);

/* Phase 2 (StoreAllDecodedSequences + log_probability).  Synchronous. */
int ctcext_fetch(ctcext_decoder* dec, const ctcext_outputs* out);

/* Statistics of the last decode.  ctcext_get_stats fills the ABI-4 prefix
 * only (every field before helper_redecodes: callers built against that
 * header pass a struct of that size); ctcext_get_stats_sized fills the first
 * `size` bytes (pass sizeof(ctcext_stats) for every field of this header). */
int ctcext_get_stats(ctcext_decoder* dec, ctcext_stats* stats);
int ctcext_get_stats_sized(ctcext_decoder* dec, ctcext_stats* stats, size_t size);

/* CTCEXT_ABI_VERSION of the library. */
int32_t ctcext_abi_version(void);

/* Diagnostics: copies the [batch][32] phase counters of the last decode run
 * with CTCEXT_FLAG_PHASES, in the diagnostics build (make phases; the product
 * build leaves them 0).  [0, 24) the decoding wave (cycles: row load,
 * recursion, grow, extract, commit, literal frames; counts: grow events,
 * frames; ... see tools/diag_phases.py for every index), [24, 32) the helper
 * wave of the two-wave kernels. */
int ctcext_phase_counters(ctcext_decoder* dec, uint64_t* out, int64_t n);

/* Diagnostics (tests): the pre-pass of a decode alone, on device buffers and
 * the handle's stream, synchronously -- per (t, b) row of inputs
 * [max_time][batch][num_classes] (num_classes > 64) its record into prep
 * (*row_bytes each: RowHdr {max, largest non-blank value outside the top
 * set S, NaN/+inf flag, |S|}, the 64-class block maxima, S as (value bits,
 * label index) pairs in label order) and its softmax normaliser into norm.
 * With prep == NULL only *row_bytes is set.  Rows past seq_len are skipped. */
int ctcext_row_facts(ctcext_decoder* dec, const void* inputs, int32_t dtype, int64_t max_time, int64_t batch,
                     int64_t num_classes, int32_t blank_index, const int32_t* sequence_length, void* prep,
                     void* norm, int64_t* row_bytes);

/* Message of the last failing call on this thread ("" if none). */
const char* ctcext_last_error(void);

/* Widest beam the LDS-resident fast tier decodes for the given class count
 * and dtype (0: num_classes is past that tier).  Wider beams, and num_classes
 * above 65535 or the LDS row, decode on the global-state tier (beam state in
 * HBM, 16-byte records, the literal path every frame): any shape the
 * reference accepts, at a lower rate. */
int32_t ctcext_max_beam_width(int64_t num_classes, int32_t dtype);

/* ---------------------------------------------------------------------------
 * Streaming decode.  A stream keeps the beam of every item of a batch between
 * calls: the caller pushes the logits in chunks of frames, and after each push
 * ctcext_fetch on the owning decoder returns the hypotheses of everything
 * pushed so far -- bit for bit what ctcext_decode returns for that prefix.
 * New entry points and structs only (CTCEXT_ABI_VERSION is unchanged; detect
 * them by CTCEXT_HAS_STREAM at build time or by symbol at run time).
 *
 * One device per stream: a handle of ctcext_create_sharded with more than one
 * device answers CTCEXT_UNIMPLEMENTED.  Several streams may be open on one
 * decoder; they are independent, only the fetch state (the last push with
 * sizes != NULL, or the last ctcext_decode) is the decoder's.  The decode
 * kernel is chosen once at open (dtype, scorer, num_classes, beam_width and
 * the CTCEXT_HELPER environment variable as read then) and runs for the
 * stream's life, without the record ring. */
#define CTCEXT_HAS_STREAM 1
#define CTCEXT_KERNEL_STREAM 0x8000   /* ctcext_stats.kernel bit 15: a stream build of the decode kernel */

typedef struct ctcext_stream ctcext_stream;

typedef struct {            /* fixed for the stream's life */
  int32_t dtype;            /* CTCEXT_F32 / CTCEXT_F64 */
  int32_t on_device;        /* chunks and lengths are device pointers on the decoder's device */
  int64_t batch_size, num_classes;
  int64_t max_frames;       /* capacity per item: records for this many frames are allocated */
  int32_t beam_width, top_paths, merge_repeated, blank_index, blank_label;
  int32_t flags;            /* CTCEXT_FLAG_FORCE_LITERAL, _GLOBAL_STATE, _PROFILE */
  int32_t scorer; int32_t pad_;
  const void* scorer_table; /* CTCEXT_SCORER_BIGRAM: [num_classes + 1][num_classes] of dtype, in HOST
                               memory whatever on_device says (unlike ctcext_decode_args): its entries
                               are checked by ctcext_stream_validate and it is copied at open */
} ctcext_stream_args;

typedef struct {
  const void* inputs;       /* [chunk_time, batch, num_classes], or through format/strides as in ctcext_decode_args */
  const int32_t* chunk_length; /* [batch]: frames of this chunk per item, 0..chunk_time; NULL = chunk_time for all */
  int64_t chunk_time;
  int32_t inputs_format; int32_t flags;   /* flags: CTCEXT_FLAG_TEST_HELPER_DEAD, _PROFILE only */
  int64_t inputs_stride_t, inputs_stride_b;
  void* stream;             /* hipStream_t, NULL = the decoder's own */
} ctcext_chunk;

/* The attribute checks of ctcext_validate for a stream, host only, no HIP
 * call (the bigram table's entries included: it is host memory); plus
 * "max_frames is negative" and "stream flags: CTCEXT_FLAG_FORCE_LITERAL,
 * _GLOBAL_STATE and _PROFILE only". */
int ctcext_stream_validate(const ctcext_stream_args* args);
/* ... and a chunk against those attributes, host only as well (part of the
 * public stream ABI: a front end checks a block before it queues it): the checks
 * ctcext_stream_push runs before any device work, except the stream's
 * capacity -- the ABI-7 layout messages of ctcext_validate with chunk_time as
 * max_time, and "sequence_length(b) <= chunk_time" when the lengths are host
 * memory (on_device == 0). */
int ctcext_stream_validate_chunk(const ctcext_stream_args* args, const ctcext_chunk* chunk);
int ctcext_stream_open(ctcext_decoder* dec, const ctcext_stream_args* args, ctcext_stream** out);
/* Decodes the chunk on top of what the stream holds.  Synchronous.  With
 * sizes != NULL it also walks the records of all frames so far and sets the
 * decoder's fetch state.  Validation comes before any device work; a rejected
 * push (also: "stream capacity exceeded: item %d would hold %d frames of
 * max_frames %d", CTCEXT_INVALID_ARGUMENT) and a failed one (CTCEXT_INTERNAL:
 * a helper-wave hand-over timeout; a stream cannot re-decode with another
 * kernel) leave the stream as it was.  "Less leaves in the beam search than
 * requested." (CTCEXT_INVALID_ARGUMENT, as ctcext_decode of that prefix) is
 * reported with the chunk pushed.  ctcext_stats after a push: the counters are
 * cumulative over the stream's items. */
int ctcext_stream_push(ctcext_stream* s, const ctcext_chunk* chunk, ctcext_path_sizes* sizes);
/* frames[batch]: frames pushed so far per item. */
int ctcext_stream_frames(ctcext_stream* s, int64_t* frames);
/* Puts the n named items (items == NULL: all) back to no frames, for a
 * continuous-batching slot that starts a new utterance; others are untouched. */
int ctcext_stream_reset(ctcext_stream* s, const int32_t* items, int64_t n);
/* Close every stream before ctcext_destroy of its decoder. */
void ctcext_stream_close(ctcext_stream* s);

/* ---------------------------------------------------------------------------
 * Streaming: the stable prefix.  How much of a stream's decoded output is
 * final: a front end emits those labels once and redraws only the tail.  New
 * entry points only (CTCEXT_ABI_VERSION is unchanged; detect them by
 * CTCEXT_HAS_STREAM_STABLE at build time or by symbol at run time).
 *
 * Definition.  Item b has n = frames[b] frames pushed.  Its live set is the
 * beam records of frame n - 1 at positions 0..m-1, m being the beam size after
 * that frame (the records the last committed push wrote for it).  Every record
 * names its source position in the frame before (link >> 1); follow that from
 * every live position one frame back at a time.
 *   stable_frames[b]  = f + 1, where f is the newest frame at which all chains
 *                       sit on one position k*; 0 when the chains never meet,
 *                       and when n == 0.
 *   decoded_length[b] = the number of labels the decoded walk (the one that
 *                       fills decoded_values) emits on the single chain from
 *                       record (f, k*) down to frame 0, the merge_repeated
 *                       rule applied as it is there.
 * Every hypothesis a later push can return descends from a live entry, so the
 * first decoded_length[b] elements of item b's decoded row are identical in
 * every path of this push and of every later push, until the item is reset;
 * and neither number decreases between resets.
 *
 * The ALIGNMENT outputs get no such guarantee.  An alignment candidate chain
 * can restart at any frame (ctc_beam_entry.h:204-213), and the 4-byte record
 * of the two-wave kernels folds "restarted" and "absent" into one code, so
 * the live alignment states cannot be enumerated from the records; the query
 * leaves them out instead of approximating them.
 *
 * The stream keeps, per item, the frontier of its last answer; a query walks
 * only the frames above it, a push does not touch it, and ctcext_stream_reset
 * clears it for the items it names. */
#define CTCEXT_HAS_STREAM_STABLE 1
/* Host arrays of [batch]; walked may be NULL.  Synchronous, on the decoder's own stream.
 * walked[b]: record frames the convergence walk visited in this call.
 * Null s or a null required pointer: CTCEXT_INVALID_ARGUMENT, "null argument".
 * A stream with no push yet answers zeros. */
int ctcext_stream_stable(ctcext_stream* s, int32_t* decoded_length, int64_t* stable_frames, int64_t* walked);
/* Diagnostics (tests): the same two numbers computed on the host from a copy of the item
 * records, by the naive method -- every live chain walked to frame 0, no cache, no early stop. */
int ctcext_stream_stable_reference(ctcext_stream* s, int32_t* decoded_length, int64_t* stable_frames);

/* ---------------------------------------------------------------------------
 * Dense, enqueue-only decode.  The outputs are padded device tensors of
 * static shape instead of SparseTensor components whose sizes depend on the
 * data, and every check that needs data runs on the device, so the call only
 * enqueues: a caller with the logits on the GPU queues the decode behind the
 * kernels that produce them and carries on, and the call can be captured into
 * a HIP graph.  Errors that depend on data are deferred: they arrive per item
 * in status[], and as a status code and message from ctcext_dense_check.
 * New entry points and structs only (CTCEXT_ABI_VERSION is unchanged; detect
 * them by CTCEXT_HAS_DENSE at build time or by symbol at run time).  One
 * device: a handle of ctcext_create_sharded with more than one device answers
 * CTCEXT_UNIMPLEMENTED. */
#define CTCEXT_HAS_DENSE 1

/* One more ctcext_decode_args.flags bit, read by ctcext_decode_dense and
 * ctcext_dense_reserve only: with stream == NULL the work goes onto the null
 * (legacy default) stream itself instead of the decoder's own stream, so that
 * it is ordered behind work a framework queued there, without a sync. */
enum { CTCEXT_FLAG_DENSE_NULL_STREAM = 512 };

/* status[b] bits; 0 = the item's rows are its hypotheses. */
enum { CTCEXT_ITEM_LENGTH = 1,         /* sequence_length(b) > max_time: item not decoded */
       CTCEXT_ITEM_FEW_LEAVES = 2,     /* fewer leaves than top_paths (decoder.h:240-243) */
       CTCEXT_ITEM_HELPER_TIMEOUT = 4, /* two-wave hand-over wait ran out (never in a correct run) */
       CTCEXT_ITEM_TABLE = 8 };        /* bigram table holds an entry > 0 or NaN (every item) */

/* Device pointers, all of them.  Row [b][p] of decoded / alignment holds path
 * p's label sequence in label order in its first decoded_length[b][p] /
 * alignment_length[b][p] elements and pad_value in the rest.  An item with
 * any status bit has all its top_paths rows empty: lengths 0, rows all
 * pad_value, log_probability -inf; the other items are untouched by it.
 * decoded and alignment need 8-byte alignment only. */
typedef struct {
  int64_t* decoded;           /* [batch][top_paths][max_time], label order, padded */
  int32_t* decoded_length;    /* [batch][top_paths] */
  int64_t* alignment;         /* [batch][top_paths][max_time] */
  int32_t* alignment_length;  /* [batch][top_paths] */
  void*    log_probability;   /* [batch][top_paths] of dtype */
  int32_t* status;            /* [batch] CTCEXT_ITEM_* bits, 0 = good */
  int64_t  pad_value;         /* written past each row's length */
} ctcext_dense_outputs;

/* Host only, no HIP call: every check of ctcext_validate that needs no data,
 * with the same messages in the same order, then (CTCEXT_INVALID_ARGUMENT)
 *   "ctcext_decode_dense needs device inputs"   (inputs_on_device == 0)
 *   "null dense output pointer"                 (batch_size > 0 only) */
int ctcext_dense_validate(const ctcext_decode_args* args, const ctcext_dense_outputs* out);
/* Grows the handle's workspace to what ctcext_decode_dense of these arguments
 * needs (the pointers in args are not read); launches nothing.  May allocate
 * and block. */
int ctcext_dense_reserve(ctcext_decoder* dec, const ctcext_decode_args* args);
/* Validates on the host (ctcext_dense_validate), then enqueues on one stream
 * (args->stream; NULL: the decoder's own, or the null stream with
 * CTCEXT_FLAG_DENSE_NULL_STREAM): a prologue that checks the lengths and the
 * bigram table on the device, the pre-pass, decode and traceback of
 * ctcext_decode, and the padded pack.  A call whose workspace already fits (a
 * ctcext_dense_reserve or an earlier call of the same or a larger shape)
 * makes no allocation, no free, no host-blocking HIP call and no
 * device-to-host copy.  The flags are ctcext_decode's; there is never a
 * re-decode (a helper hand-over timeout is CTCEXT_ITEM_HELPER_TIMEOUT).
 * ctcext_fetch after it answers CTCEXT_FAILED_PRECONDITION.  ctcext_stats
 * after it: tier, kernel, helper, record_bytes, ring_frames; the counters 0. */
int ctcext_decode_dense(ctcext_decoder* dec, const ctcext_decode_args* args, const ctcext_dense_outputs* out);
/* Waits for the stream of the last ctcext_decode_dense, fills every
 * ctcext_stats counter, and returns what ctcext_decode would have returned
 * for the same inputs, message included; the first match wins:
 *   CTCEXT_ITEM_TABLE          CTCEXT_INVALID_ARGUMENT    "beam scorer table entries must be log-probabilities (<= 0)"
 *   lowest b with _LENGTH      CTCEXT_FAILED_PRECONDITION "sequence_length(b) <= max_time" (the numbers)
 *   any _HELPER_TIMEOUT        CTCEXT_INTERNAL            "decode kernel: a helper-wave hand-over wait timed out"
 *   any _FEW_LEAVES            CTCEXT_INVALID_ARGUMENT    "Less leaves in the beam search than requested."
 * Without a preceding ctcext_decode_dense (or after a later ctcext_decode or
 * stream push on the handle): CTCEXT_FAILED_PRECONDITION.  It reads the
 * handle's workspace, not the caller's status[]; after the replay of a graph
 * that captured the call (and the caller's wait for the stream it replayed
 * on) it reports that replay. */
int ctcext_dense_check(ctcext_decoder* dec);
/* Diagnostics: with CTCEXT_FLAG_PROFILE, the time of the pack kernel of the
 * last ctcext_decode_dense in ms, after its ctcext_dense_check (the other
 * kernels' times are in ctcext_stats).  0 for a call replayed from a graph. */
int ctcext_dense_pack_ms(ctcext_decoder* dec, double* ms);

/* ---------------------------------------------------------------------------
 * Streaming: enqueue-only push.  ctcext_stream_push in the manner of
 * ctcext_decode_dense: the push enqueues onto one HIP stream and returns, its
 * outputs are padded device tensors of static shape, and every decision that
 * needs data (the chunk's lengths, the stream's capacity, whether an item's
 * hand-over held, a slot's reset) is taken on the device.  A push is a fixed
 * chain of launches over fixed addresses, so it can be captured into a HIP
 * graph and replayed once per chunk.  The hypotheses after each push are, bit
 * for bit, ctcext_decode's of everything pushed so far for that item.
 * New entry points and structs only (CTCEXT_ABI_VERSION is unchanged; detect
 * them by CTCEXT_HAS_STREAM_DENSE at build time or by symbol at run time).
 *
 * Every buffer such a push touches belongs to the ctcext_stream, none to the
 * decoder: two streams of one decoder may have pushes in flight at once.
 * Successive pushes of one stream object are ordered by the HIP stream they
 * are enqueued on; pushes of one stream object enqueued on different HIP
 * streams are the caller's to order (events).  The synchronous entry points
 * (ctcext_stream_push, _frames, _reset, _stable, _stable_reference) first wait
 * for the enqueue-only pushes of that stream object and refresh the host's
 * frame counts, without clearing the deferred status, so the two forms can be
 * mixed -- except that a captured push must not be replayed after a
 * synchronous push (which swaps the stream's two state buffers). */
#define CTCEXT_HAS_STREAM_DENSE 1

/* One more status[b] bit: the chunk would take the item past max_frames. */
enum { CTCEXT_ITEM_CAPACITY = 16 };

/* Device pointers, all of them.  The five hypothesis pointers as in
 * ctcext_dense_outputs with rows max_frames wide (8-byte alignment only); all
 * five NULL: no traceback and no pack, status / frames / stable_* only. */
typedef struct {
  int64_t* decoded;           /* [batch][top_paths][max_frames], label order, padded */
  int32_t* decoded_length;    /* [batch][top_paths] */
  int64_t* alignment;         /* [batch][top_paths][max_frames] */
  int32_t* alignment_length;  /* [batch][top_paths] */
  void*    log_probability;   /* [batch][top_paths] of dtype */
  int32_t* status;            /* [batch] CTCEXT_ITEM_* bits of THIS push, 0 = good */
  int32_t* frames;            /* [batch] frames per item after this push (may be NULL) */
  int32_t* stable_length;     /* [batch] } both or neither: ctcext_stream_stable's decoded_length */
  int64_t* stable_frames;     /* [batch] } and stable_frames, after this push */
  int64_t  pad_value;         /* written past each row's length */
} ctcext_stream_dense_outputs;

/* Host only, no HIP call: ctcext_stream_validate, then (CTCEXT_INVALID_ARGUMENT)
 *   "ctcext_stream_push_dense needs device chunks"      (on_device == 0)
 *   "chunk flags: CTCEXT_FLAG_TEST_HELPER_DEAD, _PROFILE and _DENSE_NULL_STREAM only"
 * the chunk checks of ctcext_stream_validate_chunk that need no data, and for
 * out != NULL and batch_size > 0
 *   "null dense output pointer"     (status; some but not all of the hypothesis
 *                                    pointers; one of stable_length / stable_frames)
 *   "dense outputs decoded and alignment need 8-byte alignment" */
int ctcext_stream_dense_validate(const ctcext_stream_args* args, const ctcext_chunk* chunk,
                                 const ctcext_stream_dense_outputs* out);
/* Grows the stream's workspace to what ctcext_stream_push_dense of chunks of
 * up to max_chunk_time frames needs; launches nothing.  May allocate and block. */
int ctcext_stream_reserve(ctcext_stream* s, int64_t max_chunk_time);
/* Validates on the host (ctcext_stream_dense_validate; a null s or chunk:
 * "null argument"), then enqueues on one stream (chunk->stream; NULL: the
 * decoder's own, or the null stream with CTCEXT_FLAG_DENSE_NULL_STREAM in
 * chunk->flags): a prologue, the chunk's pre-pass, the stream build of the
 * decode kernel, the commit and, as out asks, the stable-prefix query, the
 * traceback over all frames so far and the padded pack.  A push whose
 * workspace fits (a ctcext_stream_reserve with max_chunk_time >= chunk_time,
 * or an earlier push of at least that size) makes no allocation, no free, no
 * host-blocking HIP call and no device-to-host copy.  out == NULL: decode only.
 *
 * reset (device [batch] or NULL): reset[b] != 0 starts a new utterance in
 * item b with this chunk -- its frames become 0 and its stable-prefix cache
 * entry is cleared before the chunk's frames are decoded.  A status bit of the
 * same push does not undo it.
 * chunk_length NULL: chunk_time for all; a negative length reads as 0.
 *   length > chunk_time                   CTCEXT_ITEM_LENGTH     } the item gets no frame from this push:
 *   frames[b] + length > max_frames       CTCEXT_ITEM_CAPACITY   } its state and frames are as before
 *   a helper-wave hand-over timeout       CTCEXT_ITEM_HELPER_TIMEOUT: likewise, that item only
 *   fewer leaves than top_paths           CTCEXT_ITEM_FEW_LEAVES: the frames count as pushed
 *                                         (pushes with hypothesis outputs only)
 * An item with any bit has all its rows of this push empty (lengths 0, rows
 * pad_value, log_probability -inf); an item without one has the hypotheses of
 * its whole prefix, whether or not this push brought it frames. */
int ctcext_stream_push_dense(ctcext_stream* s, const ctcext_chunk* chunk, const int32_t* reset,
                             const ctcext_stream_dense_outputs* out);
/* Waits for the stream of the last enqueue-only push, refreshes the frame
 * counts ctcext_stream_frames reads, fills ctcext_stats (cumulative counters,
 * as after ctcext_stream_push) and reports over all enqueue-only pushes since
 * the previous check; the first match wins, then the record is cleared:
 *   lowest b that had _LENGTH     CTCEXT_FAILED_PRECONDITION "sequence_length(b) <= chunk_time" (of its first such push)
 *   lowest b that had _CAPACITY   CTCEXT_INVALID_ARGUMENT    "stream capacity exceeded: item b would hold n frames of max_frames m"
 *   any _HELPER_TIMEOUT           CTCEXT_INTERNAL            "decode kernel: a helper-wave hand-over wait timed out"
 *   any _FEW_LEAVES               CTCEXT_INVALID_ARGUMENT    "Less leaves in the beam search than requested."
 * Without an enqueue-only push on the stream: CTCEXT_OK.  After replays of a
 * graph that captured a push it reports those replays. */
int ctcext_stream_check(ctcext_stream* s);
/* Diagnostics: with CTCEXT_FLAG_PROFILE in the chunk's flags, the time of the
 * commit kernel of the last ctcext_stream_push_dense in ms, after its
 * ctcext_stream_check (the other kernels' times are in ctcext_stats). */
int ctcext_stream_commit_ms(ctcext_stream* s, double* ms);

/* ---------------------------------------------------------------------------
 * Token times: the start and end frame of every decoded token, and the blank
 * frames the best path ends in, from each path's alignment, on the device.
 * New entry points and structs only (CTCEXT_ABI_VERSION is unchanged; detect
 * them by CTCEXT_HAS_TOKEN_TIMES at build time or by symbol at run time).
 *
 * Definition.  The inputs are
 *   frames      the item's frame count (its sanitised length),
 *   dec[0..m)   one path's decoded row, merge_repeated already applied,
 *   ali[0..L)   its alignment row; element i is frame frames - L + i, because
 *               an alignment that restarted is a suffix.
 * A run is a maximal stretch of equal alignment values other than blank_label.
 * Runs are matched to tokens from the end:
 *
 *   def token_times(dec, ali, frames, blank_label, merge):
 *       m, L, base = len(dec), len(ali), frames - len(ali)
 *       start, end, runs, i = [-1] * m, [-1] * m, [], 0
 *       while i < L:
 *           j = i
 *           while j + 1 < L and ali[j + 1] == ali[i]: j += 1
 *           if ali[i] != blank_label: runs.append((ali[i], base + i, base + j))
 *           i = j + 1
 *       trailing = 0
 *       while trailing < L and ali[L - 1 - trailing] == blank_label: trailing += 1
 *       j, opened = m - 1, False
 *       for lab, s, e in reversed(runs):
 *           if j < 0: break
 *           if opened and merge and lab == dec[j]:     # an earlier run of the same merged token
 *               start[j] = s; continue
 *           if opened: j -= 1; opened = False
 *           if j < 0 or lab != dec[j]: break           # first mismatch: every earlier token stays -1
 *           start[j] = s; end[j] = e; opened = True
 *       return start, end, trailing
 *
 * So a token's span runs from the first frame of its first run to the last
 * frame of its last run; with merge_repeated a merged token spans the blanks
 * between its runs; tokens the alignment does not reach (the chain restarted,
 * the path has no label sequence, the item has a status bit) are -1 in both
 * arrays; the timed tokens are always a suffix of the row and their start
 * values strictly increase.
 *
 * start and end are int32 [batch][top_paths][width], width being max_time
 * (ctcext_decode_dense, ctcext_decode) or max_frames (a stream); everything
 * past the row's decoded length is -1, whatever pad_value was.
 * trailing_blank is int32 [batch][top_paths].
 *
 * The definition needs a blank_label that is not a label: a request with
 * 0 <= blank_label < num_classes and blank_label != blank_index fails, before
 * any launch, with CTCEXT_INVALID_ARGUMENT
 *   "token times need a blank_label that is no class label".
 *
 * Not covered: handles of more than one device (CTCEXT_UNIMPLEMENTED), and
 * stability -- ctcext_stream_stable says which tokens are final, not that
 * their alignment is, so the times of stable tokens can still move. */
#define CTCEXT_HAS_TOKEN_TIMES 1

/* Device pointers.  trailing_blank may be NULL; start and end come both or
 * neither. */
typedef struct {
  int32_t* start;           /* [batch][top_paths][width] */
  int32_t* end;             /* [batch][top_paths][width] */
  int32_t* trailing_blank;  /* [batch][top_paths] */
} ctcext_token_times;

/* Host only, no HIP call: the blank_label rule above. */
int ctcext_token_times_validate(int64_t num_classes, int32_t blank_index, int32_t blank_label);
/* Elements of a row the kernel covers per step (its carry crosses multiples
 * of this); for tests. */
int32_t ctcext_token_times_tile(void);
/* Enqueues the token-times kernel on the stream of the last
 * ctcext_decode_dense, behind its pack, over that call's rows (width
 * max_time).  No allocation, no host-blocking call, no device-to-host copy;
 * capturable into the same graph as the decode.  Without a preceding
 * ctcext_decode_dense: CTCEXT_FAILED_PRECONDITION.  An item with a status bit
 * has rows of -1 and trailing_blank 0. */
int ctcext_dense_token_times(ctcext_decoder* dec, const ctcext_token_times* out);
/* The same after a ctcext_stream_push_dense that had hypothesis outputs, over
 * the stream's own buffers (never the decoder's); rows are max_frames wide.
 * After a push without hypothesis outputs, or with no enqueue-only push yet:
 * CTCEXT_FAILED_PRECONDITION. */
int ctcext_stream_token_times(ctcext_stream* s, const ctcext_token_times* out);
/* Synchronous; valid whenever ctcext_fetch is (after ctcext_decode, or after a
 * ctcext_stream_push with sizes).  out's pointers are device pointers with
 * outputs_on_device, host pointers without.  One-device handles only:
 * CTCEXT_UNIMPLEMENTED otherwise. */
int ctcext_fetch_token_times(ctcext_decoder* dec, const ctcext_token_times* out, int32_t outputs_on_device);
/* Host only, no HIP call: the definition above for one row.  start and end
 * have m elements (both or neither may be NULL), trailing_blank one (may be
 * NULL).  Shares no code with the kernel. */
int ctcext_token_times_row(const int64_t* decoded, int64_t m, const int64_t* alignment, int64_t L, int64_t frames,
                           int64_t blank_label, int32_t merge_repeated, int32_t* start, int32_t* end,
                           int32_t* trailing_blank);
/* Diagnostics: with CTCEXT_FLAG_PROFILE in the decode's / the chunk's flags,
 * the time of the last token-times kernel in ms.  Waits for it. */
int ctcext_dense_token_times_ms(ctcext_decoder* dec, double* ms);
int ctcext_stream_token_times_ms(ctcext_stream* s, double* ms);

/* ---------------------------------------------------------------------------
 * Blank-frame skipping: runs of blank-dominant frames are dropped in front of
 * the decode, and the alignment is put back on the original time axis behind
 * it.  Opt-in: new entry points and one new struct only (CTCEXT_ABI_VERSION,
 * ctcext_decode_args and ctcext_stats are unchanged; detect the feature by
 * CTCEXT_HAS_BLANK_SKIP at build time or by symbol at run time).  Without
 * these entry points every call does what it did.
 *
 * Definition.  thr is a log-probability (<= 0, not NaN), converted once to
 * the compute dtype.  For item b with n frames (its sanitised length):
 *
 *   def skip_plan(logp_blank, n, thr):   # logp_blank[t] = x[t, b, blank_index] - norm[t, b], in the compute
 *       dom = [logp_blank[t] > thr for t in range(n)]     # dtype; norm is the decoder's own normaliser
 *       return [t for t in range(n) if not (t > 0 and dom[t] and dom[t - 1])]   # kmap: the frames kept
 *
 *   def skip_expand(ali_c, kmap, n, blank_label):   # ali_c: an alignment row of the compacted decode (a
 *       L = len(ali_c)                              # suffix: it covers the last L kept frames)
 *       if L == 0: return []
 *       k = kmap[len(kmap) - L:]
 *       row = [blank_label] * (n - k[0])
 *       for v, f in zip(ali_c, k): row[f - k[0]] = v
 *       return row
 *
 * A frame is dropped when it and the frame before it in the original sequence
 * are both blank-dominant (whether or not that neighbour was kept): the first
 * frame of every blank run stays, so two equal labels either side of a run
 * stay two labels, and frame 0 always stays.  A comparison with NaN is false:
 * a row with NaN or +inf, or with a -inf blank, is kept.  thr = 0 keeps every
 * frame, because x - norm is never above 0 (norm = max + log(sum of
 * exp(x - max)), and the sum holds the term exp(0) = 1, so norm >= max >= x in
 * exact and in rounded arithmetic alike: log of a value >= 1 is >= 0).
 *
 * The outputs.  Decoded rows, log_probability and errors are the plain
 * decode's of the tensor that holds item b's frames kmap_b with length
 * len(kmap_b); "Less leaves in the beam search than requested." is judged on
 * that compacted item.  log_probability is the compacted sequence's: it is
 * NOT corrected for the dropped frames.  Each alignment row is skip_expand of
 * the compacted row: it lies on the original time axis, is at most n long,
 * and dropped frames read blank_label; alignment_shape and max_alignment
 * follow the expanded rows, dense rows stay max_time wide.  Token times after
 * a skipping decode are the definition above applied to the expanded rows,
 * with the original n as frames.
 *
 * Cost: a second logits-sized workspace buffer (the kept rows, in the inputs'
 * own element type) beside the normaliser, the frame map and the kept counts.
 *
 * Not covered: handles of more than one device (CTCEXT_UNIMPLEMENTED).
 * Streams have entry points of their own ("Streaming: blank-frame skipping",
 * below). */
#define CTCEXT_HAS_BLANK_SKIP 1

typedef struct {
  double logp_threshold;    /* thr above */
  int32_t* kept;            /* optional [batch]: frames kept per item (0 for an item with a prologue status bit);
                               a device pointer for the dense form and for device inputs, host memory otherwise */
} ctcext_skip_args;

/* Host only, no HIP call: a threshold above 0 or NaN fails with
 * CTCEXT_INVALID_ARGUMENT "blank skip threshold must be a log-probability (<= 0)". */
int ctcext_skip_validate(const ctcext_skip_args* skip);
/* ctcext_decode with the rule above (synchronous).  ctcext_fetch and
 * ctcext_fetch_token_times then work as after ctcext_decode. */
int ctcext_decode_skip(ctcext_decoder* dec, const ctcext_decode_args* args, const ctcext_skip_args* skip,
                       ctcext_path_sizes* sizes);
/* ctcext_dense_reserve / ctcext_decode_dense with the rule above, under
 * exactly their contract (enqueue-only, capturable after a reserve or a call
 * of the same shape).  ctcext_dense_check and ctcext_dense_token_times work
 * after them; a length error still reports the original max_time. */
int ctcext_dense_reserve_skip(ctcext_decoder* dec, const ctcext_decode_args* args, const ctcext_skip_args* skip);
int ctcext_decode_dense_skip(ctcext_decoder* dec, const ctcext_decode_args* args, const ctcext_skip_args* skip,
                             const ctcext_dense_outputs* out);
/* Diagnostics: with CTCEXT_FLAG_PROFILE in the flags of the last
 * ctcext_decode_dense_skip, the time in ms of what it enqueued in front of the
 * pipeline (normaliser of the caller's rows, plan, gather) and of the
 * expansion.  Waits for them.  The pack time of ctcext_dense_pack_ms includes
 * the expansion after such a call. */
int ctcext_dense_skip_ms(ctcext_decoder* dec, double* front_ms, double* expand_ms);
/* Host only, no HIP call: skip_plan and skip_expand for one row, in plain C++
 * that shares no code with the kernels.  logp_blank holds n values of the
 * compute dtype (f64: doubles, else floats) and thr is converted to it; kmap
 * has room for n entries, *kept receives their count.  ali_c holds L <= kept
 * values, row has room for n, *row_len receives the expanded length. */
int ctcext_skip_plan_row(const void* logp_blank, int32_t f64, int64_t n, double thr, int32_t* kmap, int64_t* kept);
int ctcext_skip_expand_row(const int64_t* ali_c, int64_t L, const int32_t* kmap, int64_t kept, int64_t n,
                           int64_t blank_label, int64_t* row, int64_t* row_len);

/* ---------------------------------------------------------------------------
 * Streaming: blank-frame skipping.  A stream opened with
 * ctcext_stream_open_skip drops runs of blank-dominant frames inside every
 * enqueue-only push, on the device, and carries a run across push boundaries.
 * Opt-in: a stream opened with ctcext_stream_open, and every entry point on
 * it, does exactly what it did (CTCEXT_ABI_VERSION, ctcext_stream_args,
 * ctcext_chunk, ctcext_stream_dense_outputs and ctcext_stats are unchanged;
 * detect the feature by CTCEXT_HAS_STREAM_SKIP or by symbol).
 *
 * Definition.  The plan is causal (frame t is kept or not by frames t and
 * t - 1 alone), so the kept frames of a prefix are a prefix of the kept frames
 * of the whole.  Let item b have received frames 0 .. n - 1 over all its
 * committed pushes since its last reset, and let
 *     kmap_b = skip_plan(logp_blank_b, n, thr)
 * of that whole sequence ("Blank-frame skipping" above).  Its record frames are
 * the kept ones: the state header's frame count and the traceback's lengths
 * count kept frames, and n is kept beside them.  After every push item b's
 * outputs are those of the one-shot skipping decode of everything pushed to b
 * so far:
 *
 *   outputs   Decoded rows, log_probability and CTCEXT_ITEM_FEW_LEAVES are the
 *             plain decode's of the compacted prefix.  Each alignment row is
 *             skip_expand(compacted row, kmap_b, n, blank_label).  A chunk
 *             whose frames are all dropped lengthens the alignment by
 *             blank_labels and adds to trailing_blank; it launches no decode
 *             work for that item (a sanitised length of 0).
 *   frames    frames[b] (the push output, ctcext_stream_frames) is n.
 *             CTCEXT_ITEM_CAPACITY is judged on n + length > max_frames, and
 *             the deferred message's total is on that axis: max_frames still
 *             bounds the output rows, and the records always fit.
 *   stable    stable_length is unchanged.  With r the record-frame answer,
 *             stable_frames[b] is 0 if r == 0, else kmap_b[r - 1] + 1, in the
 *             push output and in ctcext_stream_stable / _stable_reference.  It
 *             never decreases, because kmap ascends.
 *   times     ctcext_stream_token_times applies its definition to the expanded
 *             rows, with n as frames.
 *   no advance  An item that does not advance in a push (CTCEXT_ITEM_LENGTH,
 *             _CAPACITY, _HELPER_TIMEOUT, or a chunk length of 0) keeps n, its
 *             kept count and the carried flag exactly: a zero-length push does
 *             not clear the flag.
 *   reset     reset[b] != 0, or ctcext_stream_reset, puts n, the kept count and
 *             the flag to 0: the item's next frame is frame 0 and is always
 *             kept.  As without skipping, a status bit of the same push does
 *             not undo the reset.
 *   thr = 0   keeps every frame: every output of every push is bit for bit the
 *             non-skipping stream's.
 *
 * ctcext_stream_push (synchronous) on such a stream answers
 * CTCEXT_UNIMPLEMENTED and leaves the stream as it was; _frames, _kept, _reset,
 * _stable, _check, _reserve and _token_times work.
 *
 * Cost: per item 4 * (2 * max_frames + 1) bytes of frame map, and per reserved
 * chunk a second chunk-sized buffer (the kept rows), a normaliser and a map. */
#define CTCEXT_HAS_STREAM_SKIP 1

/* ctcext_stream_open with the rule above.  skip->logp_threshold is checked as
 * by ctcext_skip_validate; skip->kept, where not NULL, is a device int32
 * [batch] that every enqueue-only push of this stream writes (the frames kept
 * per item so far) -- fixed for the stream's life, so a captured push keeps
 * writing it.  Before any allocation: skip == NULL and args->on_device != 1 are
 * CTCEXT_INVALID_ARGUMENT, a handle of more than one device
 * CTCEXT_UNIMPLEMENTED, each with a message of its own. */
int ctcext_stream_open_skip(ctcext_decoder* dec, const ctcext_stream_args* args, const ctcext_skip_args* skip,
                            ctcext_stream** out);
/* Frames kept per item so far, host [batch]; synchronous, like
 * ctcext_stream_frames.  On a stream without skipping: the frame counts. */
int ctcext_stream_kept(ctcext_stream* s, int64_t* kept);
/* Host only, no HIP call, plain C++ that shares no code with the kernels: the
 * plan in chunks.  skip_plan for frames first_frame .. first_frame + n - 1 of
 * an item, whose logp_blank values (of the compute dtype) are the n given,
 * with prev_dom the flag of frame first_frame - 1; the t > 0 rule reads the
 * absolute frame.  kmap (room for n) receives absolute frame numbers, *kept
 * their count, *last_dom the flag of the last frame (prev_dom where n == 0). */
int ctcext_skip_plan_chunk_row(const void* logp_blank, int32_t f64, int64_t n, double thr, int64_t first_frame,
                               int32_t prev_dom, int32_t* kmap, int64_t* kept, int32_t* last_dom);

/* ---------------------------------------------------------------------------
 * Token scores: the sum and the minimum of the per-frame log-posteriors over
 * every timed token's span of the best alignment, on the device -- "how sure"
 * beside the token times' "where".  New entry points and structs only
 * (CTCEXT_ABI_VERSION is unchanged; detect them by CTCEXT_HAS_TOKEN_SCORES at
 * build time or by symbol at run time).
 *
 * Definition.  The inputs, for one path of item b, are
 *   ftype       the compute dtype (float32, or float64 for float64 logits),
 *   frames, dec[0..m), ali[0..L), start[0..m), end[0..m)
 *               exactly as in "Token times",
 *   x[f][c]     the item's logits as the decode read them, widened exactly to
 *               ftype,
 *   norm[f]     the decoder's normaliser of that row, in ftype.
 *
 *   def token_scores(x, norm, ali, frames, start, end, blank_index, blank_label):
 *       base, m = frames - len(ali), len(start)
 *       lsum, lmin = [nan] * m, [nan] * m
 *       for i in range(m):
 *           if start[i] < 0: continue                      # untimed token: NaN
 *           for f in range(start[i], end[i] + 1):          # ascending frames, every frame of the span
 *               v = ali[f - base]
 *               c = blank_index if v == blank_label else v
 *               lp = ftype(x[f][c]) - norm[f]              # one rounded subtraction in ftype
 *               if f == start[i]: acc = mn = lp
 *               else:
 *                   acc = ftype(acc + lp)                  # one rounded add, this order, no fma
 *                   if lp < mn: mn = lp                    # a NaN never replaces, a leading NaN stays
 *           lsum[i], lmin[i] = acc, mn
 *       return lsum, lmin
 *
 * A merged token's span includes the blank frames between its runs; those
 * frames contribute the blank's log-posterior.  The outputs are logp_sum and
 * logp_min, of ftype, [batch][top_paths][width], width being max_time.
 * Everything that is not a timed token is a NaN: untimed tokens, cells past the
 * row's decoded length, and every row of an item with a status bit.  After a
 * skipping decode the definition applies on the original time axis: to the
 * expanded alignment rows, in which dropped frames read blank_label, to the
 * caller's rows, and to the normaliser of the caller's rows that the plan
 * computed.  The blank_label rule of token times applies unchanged, with the
 * same message.  Mean confidence is exp(logp_sum / (end - start + 1)): the
 * caller's one elementwise op, not computed here.
 *
 * The kernel trusts nothing in start / end: it scores a token only when
 * 0 <= start <= end < frames, start >= frames - L, the token index is below
 * the decoded length, and each alignment value of the span is blank_label or
 * in [0, num_classes); otherwise the cell is a NaN and nothing outside the
 * buffers is read.  No cell is written twice.
 *
 * The logits contract: the score calls read the inputs of the decode they
 * follow -- the caller's tensor, through the pointer, format and strides that
 * call was given (for host inputs of a synchronous call: the staged copy in
 * the workspace).  That memory must still be there, unchanged, when the kernel
 * runs; the library keeps no copy.
 *
 * Not covered: handles of more than one device (CTCEXT_UNIMPLEMENTED).  A
 * stream's push keeps neither its chunk nor its normaliser, and an alignment
 * can move to any class at any earlier frame, so these entry points do not
 * follow a push; a stream opened with a score store has its own
 * ("Streaming: token scores", below). */
#define CTCEXT_HAS_TOKEN_SCORES 1

/* Device pointers, [batch][top_paths][max_time] of the compute dtype.  Either
 * may be NULL, not both. */
typedef struct {
  void* logp_sum;
  void* logp_min;
} ctcext_token_scores;

/* Frames of a row the kernel covers per step, aligned to multiples of it on
 * the item's time axis (a token whose span crosses a multiple carries its sum
 * and minimum across steps); for tests. */
int32_t ctcext_token_scores_tile(void);
/* Enqueues the token-scores kernel on the stream of the last
 * ctcext_decode_dense / ctcext_decode_dense_skip, behind whatever that stream
 * holds, over that call's rows.  times->start / times->end are what
 * ctcext_dense_token_times wrote for the same call (both required;
 * trailing_blank is not read).  No allocation, no host-blocking call, no
 * device-to-host copy; capturable into the same graph as the decode.  Without
 * a preceding dense decode: CTCEXT_FAILED_PRECONDITION. */
int ctcext_dense_token_scores(ctcext_decoder* dec, const ctcext_token_times* times, const ctcext_token_scores* out);
/* Synchronous; valid after ctcext_decode / ctcext_decode_skip (not after a
 * stream's push: CTCEXT_FAILED_PRECONDITION).  Computes the times into
 * workspace itself, then the scores.  out's pointers are device pointers with
 * outputs_on_device, host pointers without.  One-device handles only:
 * CTCEXT_UNIMPLEMENTED otherwise. */
int ctcext_fetch_token_scores(ctcext_decoder* dec, const ctcext_token_scores* out, int32_t outputs_on_device);
/* Host only, no HIP call: the definition above for one row, in plain C++ that
 * shares no code with the kernel.  x is one item's rows, dense
 * [frames][num_classes], and norm [frames], both of the compute dtype (f64:
 * doubles, else floats); alignment holds L <= frames values; start / end hold
 * m; logp_sum / logp_min (either may be NULL, not both) receive m values.  A
 * span outside the walk, or a value that maps to no class, gives NaN as in the
 * kernel. */
int ctcext_token_scores_row(const void* x, const void* norm, int32_t f64, int64_t frames, int64_t num_classes,
                            const int64_t* alignment, int64_t L, const int32_t* start, const int32_t* end, int64_t m,
                            int32_t blank_index, int64_t blank_label, void* logp_sum, void* logp_min);
/* Diagnostics: with CTCEXT_FLAG_PROFILE in the decode's flags, the time of the
 * last token-scores kernel of a dense call in ms.  Waits for it. */
int ctcext_dense_token_scores_ms(ctcext_decoder* dec, double* ms);

/* ---------------------------------------------------------------------------
 * Streaming: token scores.  A stream opened with ctcext_stream_open_scores
 * keeps, on the device, the logits and the normaliser of every frame it has
 * committed, and ctcext_stream_token_scores applies the definition of "Token
 * scores" to them after any enqueue-only push.  Opt-in: a stream opened with
 * ctcext_stream_open or ctcext_stream_open_skip allocates nothing more and
 * does exactly what it did (CTCEXT_ABI_VERSION and every existing struct are
 * unchanged; detect the entry points by CTCEXT_HAS_STREAM_SCORES at build
 * time or by symbol at run time).
 *
 * Definition.  After a push, for item b: "Token scores" with
 *   frames      the item's frames since its last reset (the push's frames[b]),
 *   x, norm     the rows of every chunk committed to the item since that reset,
 *               in order, widened exactly to ftype, and the decoder's
 *               normaliser of each row,
 *   ali, start, end   of this push (ctcext_stream_token_times),
 * and width max_frames.  That is what the one-shot calls give for the
 * concatenated logits.  On a skipping stream it applies as after a skipping
 * decode: on the original time axis, to the expanded alignment, the caller's
 * rows -- dropped frames included -- and the normaliser of the caller's rows.
 *
 * The store.  Two buffers for the stream's life, allocated at open:
 *   sx     [batch][max_frames][num_classes], the rows on the original time
 *          axis, frame 0 being the item's first since its last reset;
 *   snorm  [max_frames][batch] of ftype.
 * store_format is sx's element type.  CTCEXT_IN_NATIVE: ftype; a chunk may have
 * any format the stream accepts, another one every push, and is widened
 * exactly on the way in.  CTCEXT_IN_F16 / CTCEXT_IN_BF16 (float32 streams
 * only): two bytes per element, and every chunk must have that inputs_format
 * (checked on the host before anything is enqueued: CTCEXT_INVALID_ARGUMENT
 * "chunk inputs_format differs from the stream's score store format", the
 * stream as it was).  Cost:
 *   batch * max_frames * (num_classes * esize + sizeof(ftype)) bytes
 * (ctcext_stream_scores_bytes) -- at batch 256, max_frames 1500,
 * num_classes 29: 46.1 MB native, 23.8 MB in bf16.
 *
 * A push with chunk_time > 0 enqueues one more kernel, behind the prologue and
 * the normaliser of the caller's rows and in front of the commit: for item b
 * it copies the chunk_length[b] rows the push takes from the caller's chunk
 * (through chunk->inputs, its format and strides) to sx[b][base ..], and their
 * normaliser to snorm[base ..][b], base being the item's frames before the
 * push.  An item with _LENGTH or _CAPACITY copies nothing.
 *
 * Roll-back is by position, not by undo.  The append reads base from committed
 * state and the commit runs behind it, so an item whose push does not commit
 * (a helper hand-over timeout, _LENGTH, _CAPACITY) keeps its base, and its next
 * push writes the same rows again.  Rows at or above an item's frames are
 * never read: the scores kernel reads inside [0, frames) only.  The prologue's
 * capacity check gives base + chunk_length[b] <= max_frames, so nothing is
 * written outside the item's slab.  reset[b] and ctcext_stream_reset put base
 * to 0: the next push appends at frame 0.
 *
 * Such a stream takes device chunks through ctcext_stream_push_dense alone:
 * ctcext_stream_push answers CTCEXT_UNIMPLEMENTED and leaves the stream as it
 * was.  _reserve, _check, _frames, _kept, _reset, _stable and _token_times are
 * unchanged, and a push still allocates nothing after a reserve.
 *
 * Not covered: handles of more than one device (CTCEXT_UNIMPLEMENTED); host
 * chunks and the synchronous push; any mean or exponential of the scores (the
 * caller's one elementwise op); stability -- like the token times, the scores
 * of tokens ctcext_stream_stable calls final can still move, because the best
 * alignment can. */
#define CTCEXT_HAS_STREAM_SCORES 1

typedef struct {
  int32_t store_format;   /* CTCEXT_IN_NATIVE, CTCEXT_IN_F16 or CTCEXT_IN_BF16 */
  int32_t pad_;
} ctcext_stream_scores_args;

/* Host only, no HIP call: ctcext_stream_validate, then (CTCEXT_INVALID_ARGUMENT)
 *   "store_format must be CTCEXT_IN_NATIVE, CTCEXT_IN_F16 or CTCEXT_IN_BF16"
 *   "a half-precision score store needs dtype float32"
 *   "a stream with a score store needs device chunks (on_device == 1): it has the enqueue-only push alone"
 * and the blank_label rule of ctcext_token_times_validate, with its message. */
int ctcext_stream_scores_validate(const ctcext_stream_args* args, const ctcext_stream_scores_args* scores);
/* Host only: the above, ctcext_stream_dense_validate's chunk checks, and the
 * chunk's format against a half store. */
int ctcext_stream_scores_validate_chunk(const ctcext_stream_args* args, const ctcext_stream_scores_args* scores,
                                        const ctcext_chunk* chunk);
/* Host only: the store's size in bytes (the formula above); -1 where
 * ctcext_stream_scores_validate fails or the size leaves int64. */
int64_t ctcext_stream_scores_bytes(const ctcext_stream_args* args, const ctcext_stream_scores_args* scores);
/* ctcext_stream_open with the store.  skip may be NULL (no blank-frame
 * skipping); otherwise as ctcext_stream_open_skip.  A handle of more than one
 * device: CTCEXT_UNIMPLEMENTED. */
int ctcext_stream_open_scores(ctcext_decoder* dec, const ctcext_stream_args* args, const ctcext_skip_args* skip,
                              const ctcext_stream_scores_args* scores, ctcext_stream** out);
/* Enqueues the token-scores kernel on the stream of the last
 * ctcext_stream_push_dense, over the stream's own walks and its store.
 * times->start / times->end are what ctcext_stream_token_times wrote for the
 * same push (both required; nothing in them is trusted).  out's rows are
 * [batch][top_paths][max_frames] of ftype, NaN everywhere but the timed
 * tokens.  No allocation, no host-blocking call, no device-to-host copy;
 * capturable together with the push and the times.
 * CTCEXT_FAILED_PRECONDITION on a stream opened without a store, after a push
 * without hypothesis outputs, and before any enqueue-only push. */
int ctcext_stream_token_scores(ctcext_stream* s, const ctcext_token_times* times, const ctcext_token_scores* out);
/* Diagnostics: with CTCEXT_FLAG_PROFILE in the chunk's flags, the times in ms
 * of the last push's append kernel and of the last token-scores kernel behind
 * it (0 where that push had none).  Waits for them. */
int ctcext_stream_scores_ms(ctcext_stream* s, double* append_ms, double* scores_ms);

#ifdef __cplusplus
}
#endif

#endif /* CTCEXT_H_ */
