// ctcext_capi.hip — host side of libctcext.so: validation, workspace, kernel
// orchestration, multi-device sharding and output transfer behind the C ABI
// in include/ctcext.h.
//
// Mirrors the reference op kernel (cc/kernels/ctc_ext_beam_search_decoder_kernels.cc):
//   ValidateInputsGenerateOutputs  :97-139  -> validate_shapes / check_lengths (ctcext_validate)
//   Compute batch/time loop        :67-90   -> ctcx_row_norm + ctcx_beam_decode per shard
//   TopPaths errors                decoder.h:237-243
//   StoreAllDecodedSequences       :163-257 -> ctcx_traceback + ctcx_scan + ctcx_pack
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ctcext.h"
#define CTCX_STREAM_HOST   // the stream builds' parameter structs (not their DecodeParams member)
#include "ctcx_kernels.h"
#include "ctcx_scores.h"
#include "ctcx_skip.h"
#include "ctcx_stable.h"
#include "ctcx_stream_dense.h"
#include "ctcx_stream_store.h"
#include "ctcx_times.h"

namespace ctcx {
template <typename T>
hipError_t launch_decode(const DecodeParams<T>& p, hipStream_t s);
template <typename T>
int ring_frames(const DecodeParams<T>& p, int cus, int cap, int hk);
template <typename T>
int use_helper_kernel(const DecodeParams<T>& p, int hk);
template <typename T>
int helper_kind(const DecodeParams<T>& p, int mode);
template <typename T>
hipError_t launch_row_norm(const void* x, int xfmt, const int32_t* sl, T* norm, int64_t T_, int64_t B, int64_t C,
                           int64_t xst_t, int64_t xst_b, hipStream_t s);
hipError_t launch_traceback(const TraceParams& tp, hipStream_t s);
template <typename T>
hipError_t launch_row_prep(const void* x, int xfmt, const int32_t* sl, char* prep, T* norm, int64_t T_, int64_t B,
                           int64_t C, int64_t xst_t, int64_t xst_b, int blank, hipStream_t s);
hipError_t launch_widen_rows(const void* x, int xfmt, float* out, int64_t T_, int64_t B, int64_t C, int64_t xst_t,
                             int64_t xst_b, hipStream_t s);
hipError_t launch_scan(const int32_t* len, int64_t* off, int64_t* res, int64_t B, int P, hipStream_t s);
hipError_t launch_pack(const PackParams& pp, hipStream_t s);
hipError_t launch_dense_prologue(DensePrologueParams pp, const void* table, int64_t table_n, int f64, int32_t* bad,
                                 hipStream_t s);
hipError_t launch_pack_dense(const PackDenseParams& pp, hipStream_t s);
}  // namespace ctcx
// the global-state tier (ctcx_decode.hip compiled with CTCX_GSTATE)
hipError_t ctcx_gstate_launch_decode(const void* p, int is_f64, int scored, hipStream_t s);
// the stream builds (CTCX_STREAM, and CTCX_GSTATE with it): p is this file's
// DecodeParams<T>, the stream's own parameters travel beside it
hipError_t ctcx_stream_launch_decode(const void* p, const CtcxStreamParams* sp, int is_f64, hipStream_t s);
hipError_t ctcx_gstate_stream_launch_decode(const void* p, const CtcxStreamParams* sp, int is_f64, int scored,
                                            hipStream_t s);

static_assert(sizeof(ctcx::DecodeParams<float>) == kCtcxDecodeParamsBytes &&
                  sizeof(ctcx::DecodeParams<double>) == kCtcxDecodeParamsBytes,
              "the stream launchers copy exactly this struct (ctcx_kernels.h)");

static thread_local std::string g_err;

// the two-wave kernels a call runs by default (ctcx::helper_kind's mode): the
// scored gather queue for beams <= 128 (cfg3 decode 144.9 -> 126.8 ms, cfg4
// 164.9 -> 162.9 ms, same box: profiles/r5j_ab.txt), the gather queue above
constexpr int kDefaultHelperMode = ctcx::kHelperScored;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// CTCEXT_HELPER (diagnostics; read once per decode call, and once at a
// stream's open): 0 the one-wave kernels, 1 the score table / unscored gather
// queue, 3 the scored gather queue (beams <= 128; the default), 4 the scored
// queue for beams <= 256
static int helper_mode_from_env() {
  const char* hv = getenv("CTCEXT_HELPER");
  return !hv || !hv[0] ? kDefaultHelperMode
         : hv[0] == '0' ? ctcx::kHelperNone
         : hv[0] == '3' ? ctcx::kHelperScored
         : hv[0] == '4' ? ctcx::kHelperScoredWide : ctcx::kHelperLegacy;
}

// CTCEXT_EARLY_RECURSE=0 (diagnostics; read at every launch): the helper wave
// of the small-C scored kernel stages no recursion for the next frame
static int32_t early_recurse_flag_from_env() {
  const char* ev = getenv("CTCEXT_EARLY_RECURSE");
  return (ev && ev[0] == '0') ? ctcx::kTestNoEarlyRecurse : 0;
}

#define HIP_OR_FAIL(expr)                                                             \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fail(CTCEXT_INTERNAL, std::string("HIP error: ") + hipGetErrorString(e_) \
                                       + " at " #expr);                              \
  } while (0)

namespace {

// Restores the calling thread's current HIP device on every exit path: the
// caller (e.g. torch in a per-rank process) reads the same runtime's device.
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

// One device of a handle: its stream, events and the per-shard workspace.
// The root (devs[0]) also holds the whole batch's walks, lengths and outputs.
struct Dev {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t s = nullptr;   // stream of the current call
  hipEvent_t ev[9] = {};     // CTCEXT_FLAG_PROFILE: around the pre-pass, decode, traceback; [4] after the dense pack;
                             // [5], [6] around the token-times kernel of a dense call, [7], [8] the token-scores kernel
  hipEvent_t sk[2] = {};     // ... of a skipping dense call: before the plan's normaliser, after the expansion
  DevBuf x, xw, sl, norm, prep, rec, foff, item, top_pos, top_kind, logp, seq, len, phase, sctab, gstate;
  DevBuf dsl, dstat;         // the dense path: sanitised lengths [B]; status before [B] and after [B] the decode, table flag
  int64_t lo = 0, nb = 0;    // this call's shard [lo, lo + nb)
  int ring = 0;              // this call's record-ring frames (ctcx::ring_frames)
  int rec_bytes = 8;         // this call's record size (8, 16 or 4 bytes)
  int helper = 0;            // this call's two-wave kernel (ctcx::use_helper_kernel)
  int kernel = 0;            // this call's kernels as its launchers noted them (ctcext_stats.kernel)
  int cus = 0;               // compute units of the device
};

}  // namespace

// What the token scores read of the decode they follow (ctcext.h, "Token
// scores"): the logits where the kernels read them, and which normaliser
// applies.  The library keeps no copy of either.
struct ScoreSrc {
  bool have = false;
  const void* x = nullptr;
  int32_t xfmt = 0;
  int64_t st_t = 0, st_b = 0;
  const void* norm = nullptr;   // [T][B] of the compute dtype
  bool f64 = false;
};

struct ctcext_decoder {
  std::vector<Dev> devs;
  // root-side: scan results and output staging
  DevBuf off, res, ptrs, out_idx, out_val;
  HostBuf h_item, h_res, h_kind, h_status;
  // state of the last successful decode (consumed by fetch)
  bool have = false;
  int dtype = 0;
  int64_t T = 0, B = 0, C = 0;
  int32_t W = 0, P = 0;
  std::vector<ctcext_path_sizes> sizes;
  ctcext_stats stats{};
  // the last ctcext_decode_dense (read by ctcext_dense_check)
  struct {
    bool have = false;
    int64_t B = 0, T = 0;
    int32_t P = 0, flags = 0;
    double pack_ms = 0;      // CTCEXT_FLAG_PROFILE: the pack kernel's time (ctcext_dense_pack_ms)
    hipStream_t s = nullptr;
    // what ctcext_dense_token_times reads beside the workspace
    int64_t C = 0;
    int32_t blank_index = 0, blank_label = 0, merge = 0;
    bool times_timed = false;   // events [5], [6] were recorded
    bool skip = false;          // it was a ctcext_decode_dense_skip
    ScoreSrc sc;                // what ctcext_dense_token_scores reads beside that
    bool scores_timed = false;  // events [7], [8] were recorded
  } dense;
  // what ctcext_fetch_token_times needs of the last synchronous decode or
  // push beside the walks: the items' frames (host) and the labels' rule
  struct {
    std::vector<int32_t> frames;
    int64_t C = 0;
    int32_t blank_index = 0, blank_label = 0, merge = 0;
  } tt;
  DevBuf tt_frames, tt_start, tt_end, tt_trail;
  // ... and what ctcext_fetch_token_scores needs of the last ctcext_decode /
  // ctcext_decode_skip (a stream's push leaves nothing to score), with the
  // staging of its outputs
  ScoreSrc ss;
  DevBuf sc_sum, sc_min;
  // blank-frame skipping (ctcext.h, "Blank-frame skipping"): the workspace of
  // the plan, and what the call that is running reads of it
  struct {
    DevBuf norm, kmap, cidx, kept, xc;   // the caller's rows' normaliser [T][B]; kmap [B][T]; cidx [B][T + 1];
                                         // kept [B]; the kept rows, dense [T][B][C] of the inputs' element type
    bool on = false;                     // the running call skips: run_decode / dense_enqueue expand the walks
    const int32_t* frames = nullptr;     // [B] on the device: the original lengths the expansion reads
    int32_t blank_label = 0;
  } skip;
};

static void release_dev(Dev& d) {
  (void)hipSetDevice(d.device);
  if (d.own_stream) (void)hipStreamSynchronize(d.own_stream);
  DevBuf* bufs[] = {&d.x, &d.xw, &d.sl, &d.norm, &d.prep, &d.rec, &d.foff, &d.item, &d.top_pos, &d.top_kind, &d.logp,
                    &d.seq, &d.len, &d.phase, &d.sctab, &d.gstate, &d.dsl, &d.dstat};
  for (DevBuf* b : bufs) b->release();
  for (auto& ev : d.ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : d.sk)
    if (ev) (void)hipEventDestroy(ev);
  if (d.own_stream) (void)hipStreamDestroy(d.own_stream);
  d.own_stream = nullptr;
}

// The LDS-resident fast tier: the 8-byte record's limits and the LDS carve.
static int32_t max_beam_width(int64_t num_classes, int32_t dtype, bool scored) {
  const int ts = dtype == CTCEXT_F64 ? 8 : 4;
  if (num_classes > ctcx::kMaxRecClasses) return 0;
  int lo = 0;
  for (int w = 1; w <= ctcx::kMaxRecBeam; ++w)
    if (ctcx::decode_lds_bytes(w, num_classes, ts, scored) <= ctcx::kLdsBytes) lo = w;
  return lo;
}
static bool use_gstate(const ctcext_decode_args* a) {
  return (a->flags & CTCEXT_FLAG_GLOBAL_STATE) ||
         a->beam_width > max_beam_width(a->num_classes, a->dtype, a->scorer != CTCEXT_SCORER_BASE);
}

extern "C" int32_t ctcext_max_beam_width(int64_t num_classes, int32_t dtype) {
  return max_beam_width(num_classes, dtype, false);
}

extern "C" int ctcext_create_sharded(const int* devices, int n_devices, ctcext_decoder** out) {
  if (!out || !devices || n_devices < 1) return fail(CTCEXT_INVALID_ARGUMENT, "null argument or no devices");
  DeviceGuard guard;
  int n = 0;
  HIP_OR_FAIL(hipGetDeviceCount(&n));
  for (int i = 0; i < n_devices; ++i)
    if (devices[i] < 0 || devices[i] >= n) return fail(CTCEXT_INVALID_ARGUMENT, "invalid device ordinal");
  ctcext_decoder* d = new ctcext_decoder();
  d->devs.resize((size_t)n_devices);
  for (int i = 0; i < n_devices; ++i) {
    Dev& v = d->devs[(size_t)i];
    v.device = devices[i];
    hipError_t e = hipSetDevice(v.device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&v.own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      for (int j = 0; j < i; ++j) release_dev(d->devs[(size_t)j]);
      delete d;
      return fail(CTCEXT_INTERNAL, std::string("HIP error: ") + hipGetErrorString(e));
    }
    for (auto& ev : v.ev) (void)hipEventCreate(&ev);
    for (auto& ev : v.sk) (void)hipEventCreate(&ev);
    // the shard inputs and the gathered walks move between the root and this
    // device by peer copies (xGMI); "already enabled" is fine
    if (v.device != devices[0]) {
      int ok = 0;
      (void)hipDeviceCanAccessPeer(&ok, v.device, devices[0]);
      if (ok) {
        (void)hipDeviceEnablePeerAccess(devices[0], 0);
        (void)hipSetDevice(devices[0]);
        (void)hipDeviceEnablePeerAccess(v.device, 0);
      }
      (void)hipGetLastError();
    }
  }
  *out = d;
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_create(int device, ctcext_decoder** out) { return ctcext_create_sharded(&device, 1, out); }

extern "C" void ctcext_destroy(ctcext_decoder* d) {
  if (!d) return;
  DeviceGuard guard;
  (void)hipSetDevice(d->devs[0].device);
  DevBuf* bufs[] = {&d->off, &d->res, &d->ptrs, &d->out_idx, &d->out_val, &d->tt_frames, &d->tt_start, &d->tt_end,
                    &d->tt_trail, &d->sc_sum, &d->sc_min, &d->skip.norm, &d->skip.kmap, &d->skip.cidx, &d->skip.kept, &d->skip.xc};
  for (DevBuf* b : bufs) b->release();
  d->h_item.release();
  d->h_res.release();
  d->h_kind.release();
  d->h_status.release();
  for (Dev& v : d->devs) release_dev(v);
  delete d;
}

extern "C" const char* ctcext_last_error(void) { return g_err.c_str(); }

extern "C" int ctcext_phase_counters(ctcext_decoder* d, uint64_t* out, int64_t n) {
  if (!d || !out) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  Dev& r = d->devs[0];
  if (!r.phase.p) return fail(CTCEXT_FAILED_PRECONDITION, "no CTCEXT_FLAG_PHASES decode yet");
  if (n < 0 || 8 * (size_t)n > r.phase.cap) return fail(CTCEXT_INVALID_ARGUMENT, "n exceeds the counter buffer");
  DeviceGuard guard;
  HIP_OR_FAIL(hipSetDevice(r.device));
  HIP_OR_FAIL(hipMemcpy(out, r.phase.p, 8 * (size_t)n, hipMemcpyDeviceToHost));
  return CTCEXT_OK;
}

extern "C" int ctcext_row_facts(ctcext_decoder* d, const void* x, int32_t dtype, int64_t max_time, int64_t batch,
                                int64_t num_classes, int32_t blank_index, const int32_t* seq_len, void* prep,
                                void* norm, int64_t* row_bytes) {
  if (!d || !row_bytes) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (dtype != CTCEXT_F32 && dtype != CTCEXT_F64) return fail(CTCEXT_INVALID_ARGUMENT, "dtype");
  if (max_time < 0 || batch < 0 || num_classes <= 64 || blank_index < 0 || blank_index >= num_classes)
    return fail(CTCEXT_INVALID_ARGUMENT, "the pre-pass runs for num_classes > 64 and a blank index inside it");
  const int ts = dtype == CTCEXT_F64 ? 8 : 4;
  *row_bytes = (int64_t)ctcx::prep_row_bytes(num_classes, ts);
  if (!prep) return CTCEXT_OK;   // the size query
  if (!x || !seq_len || !norm) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  Dev& r = d->devs[0];
  DeviceGuard guard;
  HIP_OR_FAIL(hipSetDevice(r.device));
  const hipStream_t st = r.own_stream;
  int* note = ctcx_launch_note();
  note[1] = 0;
  if (dtype == CTCEXT_F64)
    HIP_OR_FAIL(ctcx::launch_row_prep<double>(x, ctcx::kInNative, seq_len, (char*)prep, (double*)norm, max_time,
                                              batch, num_classes, batch * num_classes, num_classes, blank_index,
                                              st));
  else
    HIP_OR_FAIL(ctcx::launch_row_prep<float>(x, ctcx::kInNative, seq_len, (char*)prep, (float*)norm, max_time, batch,
                                             num_classes, batch * num_classes, num_classes, blank_index, st));
  HIP_OR_FAIL(hipStreamSynchronize(st));
  d->stats.kernel = note[1] << 12;
  return CTCEXT_OK;
}

// Frozen at the ABI-4 struct (every field before helper_redecodes): a binary
// built against that header passes a struct of that size, and a copy of the
// grown struct would write past it.  Fields added since are read through
// ctcext_get_stats_sized only.
extern "C" int ctcext_get_stats(ctcext_decoder* d, ctcext_stats* s) {
  return ctcext_get_stats_sized(d, s, offsetof(ctcext_stats, helper_redecodes));
}

// The struct has grown by appending fields (ctcext.h); a caller built against
// an older header passes its own sizeof and receives that prefix only.
extern "C" int ctcext_get_stats_sized(ctcext_decoder* d, ctcext_stats* s, size_t size) {
  if (!d || !s) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  ctcext_stats v = d->stats;
  v.n_devices = (int32_t)d->devs.size();
  memcpy(s, &v, std::min(size, sizeof(ctcext_stats)));
  return CTCEXT_OK;
}

extern "C" int32_t ctcext_abi_version(void) { return CTCEXT_ABI_VERSION; }

// ---------------------------------------------------------------------------
// Validation, in the reference's order (kernels.cc:97-139), host only.

// The op definition's attribute constraints (ops.cc:10-17) and the input
// shapes (kernels.cc:109-130).
static int validate_shapes(const ctcext_decode_args* a) {
  if (!a) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (a->dtype != CTCEXT_F32 && a->dtype != CTCEXT_F64)
    return fail(CTCEXT_INVALID_ARGUMENT, "dtype must be float32 or float64");
  if (a->beam_width < 1)
    return fail(CTCEXT_INVALID_ARGUMENT, "Value for attr 'beam_width' of " + std::to_string(a->beam_width) +
                                             " must be at least minimum 1");
  if (a->top_paths < 1)
    return fail(CTCEXT_INVALID_ARGUMENT, "Value for attr 'top_paths' of " + std::to_string(a->top_paths) +
                                             " must be at least minimum 1");
  if (a->inputs_dims != 3) return fail(CTCEXT_INVALID_ARGUMENT, "inputs is not a 3-Tensor");
  const int64_t T_ = a->max_time, B = a->batch_size, C = a->num_classes;
  if (T_ < 0 || B < 0 || C < 0) return fail(CTCEXT_INVALID_ARGUMENT, "inputs has a negative dimension");
  if (T_ == 0) return fail(CTCEXT_INVALID_ARGUMENT, "max_time is 0");
  if (a->sequence_length_dims != 1) return fail(CTCEXT_INVALID_ARGUMENT, "sequence_length is not a vector");
  if (a->sequence_length_size != B)
    return fail(CTCEXT_FAILED_PRECONDITION, "len(sequence_length) != batch_size.  len(sequence_length):  " +
                                                std::to_string(a->sequence_length_size) +
                                                " batch_size: " + std::to_string(B));
  if (B > 0 && (!a->inputs || !a->sequence_length)) return fail(CTCEXT_INVALID_ARGUMENT, "null input pointer");
  if (a->scorer != CTCEXT_SCORER_BASE && a->scorer != CTCEXT_SCORER_BIGRAM)
    return fail(CTCEXT_INVALID_ARGUMENT, "unknown beam scorer");
  if (a->scorer == CTCEXT_SCORER_BIGRAM && B > 0 && !a->scorer_table)
    return fail(CTCEXT_INVALID_ARGUMENT, "bigram beam scorer without a table");
  return CTCEXT_OK;
}

// The bigram table's entries must be log-probabilities: <= 0 and not NaN
// (exact_step's skipping bounds a child's score by its parent's total).
template <typename T>
static int check_table_t(const T* t, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!(t[i] <= T(0)))
      return fail(CTCEXT_INVALID_ARGUMENT, "beam scorer table entries must be log-probabilities (<= 0)");
  return CTCEXT_OK;
}
static int check_table(const ctcext_decode_args* a, const void* host_table) {
  if (a->scorer != CTCEXT_SCORER_BIGRAM || a->batch_size == 0) return CTCEXT_OK;
  const int64_t n = (a->num_classes + 1) * a->num_classes;
  return a->dtype == CTCEXT_F64 ? check_table_t((const double*)host_table, n)
                                : check_table_t((const float*)host_table, n);
}

// kernels.cc:133-139
static int check_lengths(const int32_t* hsl, int64_t B, int64_t T_) {
  for (int64_t b = 0; b < B; ++b)
    if (!(hsl[b] <= T_))
      return fail(CTCEXT_FAILED_PRECONDITION, "sequence_length(" + std::to_string(b) + ") <= " + std::to_string(T_));
  return CTCEXT_OK;
}

// What the reference leaves unchecked or raises per item, and this library's
// own limits.
static int check_limits(const ctcext_decode_args* a) {
  const int64_t B = a->batch_size, C = a->num_classes;
  if (B == 0) return CTCEXT_OK;
  // the reference reads out of bounds here (no check); this library refuses
  if (a->blank_index < 0 || a->blank_index >= C)
    return fail(CTCEXT_INVALID_ARGUMENT, "blank_index out of range [0, num_classes)");
  // decoder.h:237-239 — raised by the first item's TopPaths
  if (a->top_paths > a->beam_width) return fail(CTCEXT_INVALID_ARGUMENT, "requested more paths than the beam width.");
  // every shape decodes (the global-state tier takes what the LDS tier cannot);
  // this library's int32 positions and labels bound it
  if (C > INT32_MAX / 2 || a->beam_width > (1 << 28))
    return fail(CTCEXT_UNIMPLEMENTED, "num_classes or beam_width beyond this library's 32-bit indices");
  return CTCEXT_OK;
}

// The ABI-7 fields: the element format and the strides of inputs (after every
// check above, so the reference's errors and their order stay as they were).
static int check_layout(const ctcext_decode_args* a) {
  const int f = a->inputs_format;
  if (f != CTCEXT_IN_NATIVE && f != CTCEXT_IN_F16 && f != CTCEXT_IN_BF16)
    return fail(CTCEXT_INVALID_ARGUMENT, "inputs_format must be CTCEXT_IN_NATIVE, CTCEXT_IN_F16 or CTCEXT_IN_BF16");
  if (f != CTCEXT_IN_NATIVE && a->dtype != CTCEXT_F32)
    return fail(CTCEXT_INVALID_ARGUMENT, "half-precision inputs need dtype float32");
  if ((a->inputs_stride_t == 0) != (a->inputs_stride_b == 0))
    return fail(CTCEXT_INVALID_ARGUMENT, "inputs_stride_t and inputs_stride_b must be given together");
  if (a->inputs_stride_t != 0) {
    if (a->max_time > 1 && a->inputs_stride_t < a->num_classes)
      return fail(CTCEXT_INVALID_ARGUMENT, "inputs_stride_t is below num_classes");
    if (a->batch_size > 1 && a->inputs_stride_b < a->num_classes)
      return fail(CTCEXT_INVALID_ARGUMENT, "inputs_stride_b is below num_classes");
  }
  return CTCEXT_OK;
}

extern "C" int ctcext_validate(const ctcext_decode_args* a) {
  int rc = validate_shapes(a);
  if (rc != CTCEXT_OK) return rc;
  if (!a->inputs_on_device) {
    rc = check_lengths(a->sequence_length, a->batch_size, a->max_time);
    if (rc != CTCEXT_OK) return rc;
  }
  rc = check_limits(a);
  if (rc == CTCEXT_OK && !a->inputs_on_device) rc = check_table(a, a->scorer_table);
  if (rc == CTCEXT_OK) rc = check_layout(a);
  if (rc == CTCEXT_OK) g_err.clear();
  return rc;
}

// ---------------------------------------------------------------------------
// Decode.

// Contiguous shards balanced by sum(max(seq_len, 0)): shard i
// ends at the first item whose running sum reaches (i + 1) / n of the total.
static void shard_bounds(const std::vector<int32_t>& hsl, int n, std::vector<int64_t>& lo) {
  const int64_t B = (int64_t)hsl.size();
  lo.assign((size_t)n + 1, B);
  lo[0] = 0;
  int64_t tot = 0;
  for (int32_t v : hsl) tot += v > 0 ? v : 0;
  if (tot == 0) {   // no frames anywhere: split by count
    for (int i = 1; i < n; ++i) lo[(size_t)i] = B * i / n;
    return;
  }
  int64_t run = 0, b = 0;
  for (int i = 1; i < n; ++i) {
    const int64_t goal = (tot * i + n - 1) / n;
    while (b < B && run < goal) {
      const int32_t v = hsl[(size_t)b];
      run += v > 0 ? v : 0;
      ++b;
    }
    lo[(size_t)i] = b;
  }
}

// What the launches of one shard need, decided on the host.
template <typename T>
struct ShardPlan {
  ctcx::DecodeParams<T> p{};
  ctcx::TraceParams tp{};
  bool gs = false, scored = false;
  // a half shard of the global-state tier is widened into workspace first:
  // the caller's rows (p.x then points at the widened copy)
  bool widen = false;
  const void* x_in = nullptr;
  int xfmt_in = 0;
  int64_t xst_t_in = 0, xst_b_in = 0;
};

// Sizes the workspace of one shard (grow-only: nothing is allocated or freed
// when it already fits) and fills the kernels' parameters.  Launches nothing.
// x/sl point at the shard's first item; x holds elements of xfmt
// (CTCEXT_IN_*), row (t, b) of the shard xst_t * t + xst_b * b elements in.
template <typename T>
static int plan_shard(ctcext_decoder* d, Dev& v, bool root, const ctcext_decode_args* a, const void* x, int xfmt,
                      int64_t xst_t, int64_t xst_b, const int32_t* sl, int helper_mode, ShardPlan<T>& pl) {
  const int64_t T_ = a->max_time, C = a->num_classes, B = d->B, Bs = v.nb;
  const int W = a->beam_width, P = a->top_paths;
  const int64_t Bo = root ? B : Bs;   // the root's walk buffers hold the whole batch
  HIP_OR_FAIL(v.norm.ensure(sizeof(T) * (size_t)(T_ * Bs)));
  HIP_OR_FAIL(v.rec.ensure(sizeof(ctcx::Rec) * (size_t)(Bs * T_ * W)));
  HIP_OR_FAIL(v.item.ensure(sizeof(ctcx::ItemOut) * (size_t)Bo));
  HIP_OR_FAIL(v.top_pos.ensure(4 * (size_t)(Bs * P)));
  HIP_OR_FAIL(v.top_kind.ensure(4 * (size_t)(Bo * P)));
  HIP_OR_FAIL(v.logp.ensure(sizeof(T) * (size_t)(Bo * P)));
  HIP_OR_FAIL(v.seq.ensure(4 * (size_t)(Bo * P * 2 * T_)));
  HIP_OR_FAIL(v.len.ensure(4 * (size_t)(Bo * P * 2)));

  const bool gs = pl.gs = use_gstate(a);
  const bool scored = pl.scored = a->scorer != CTCEXT_SCORER_BASE;
  if (gs) {
    // the global-state tier: 16-byte records, the beam state in HBM
    HIP_OR_FAIL(v.rec.ensure(sizeof(ctcx::Rec16) * (size_t)(Bs * T_ * W)));
    HIP_OR_FAIL(v.gstate.ensure(ctcx::gstate_bytes(W, (int)sizeof(T), scored) * (size_t)Bs));
  } else if (C > 64) {
    HIP_OR_FAIL(v.prep.ensure(ctcx::prep_row_bytes(C, (int)sizeof(T)) * (size_t)(T_ * Bs)));
  }
  if (gs && xfmt != CTCEXT_IN_NATIVE && Bs > 0) {
    // the global-state tier reads its rows in place, as T: a half shard is
    // widened into workspace first (the slow catch-all tier; its kernels
    // stay as they are)
    HIP_OR_FAIL(v.xw.ensure(4 * (size_t)(T_ * Bs * C) + 16));
    pl.widen = true;
    pl.x_in = x; pl.xfmt_in = xfmt; pl.xst_t_in = xst_t; pl.xst_b_in = xst_b;
    x = v.xw.p;
    xfmt = CTCEXT_IN_NATIVE;
    xst_t = Bs * C;
    xst_b = C;
  }

  ctcx::DecodeParams<T>& p = pl.p;
  p = ctcx::DecodeParams<T>{};
  p.x = (const T*)x;
  p.xfmt = xfmt;
  p.norm = (const T*)v.norm.p;
  p.seq_len = sl;
  p.Tmax = T_; p.B = Bs; p.C = C; p.xst_t = xst_t; p.xst_b = xst_b;
  p.W = W; p.P = P; p.blank = a->blank_index; p.blank_label = a->blank_label;
  // num_classes == 1 (the blank alone): no label is ever offered, and the
  // fast paths' offer arithmetic divides by C - 1, so every frame takes the
  // literal path (the reference's own loops, decoder.h:146-209, then empty)
  p.force_literal = ((a->flags & CTCEXT_FLAG_FORCE_LITERAL) || C < 2) ? 1 : 0;
  p.rec = (ctcx::Rec*)v.rec.p;
  p.item = (ctcx::ItemOut*)v.item.p;
  p.top_pos = (int32_t*)v.top_pos.p;
  p.top_kind = (int32_t*)v.top_kind.p;
  p.log_prob = (T*)v.logp.p;
  p.prof = nullptr;
  p.scorer_tab = nullptr;
  p.prep = (const char*)v.prep.p;
  if (a->scorer == CTCEXT_SCORER_BIGRAM) {   // each device reads its own copy (enqueue_shard copies it)
    HIP_OR_FAIL(v.sctab.ensure((size_t)((C + 1) * C) * sizeof(T)));
    p.scorer_tab = (const T*)v.sctab.p;
  }
  if (a->flags & CTCEXT_FLAG_PHASES) {
    HIP_OR_FAIL(v.phase.ensure(8 * ctcx::kPhaseN * (size_t)Bs));
    p.prof = (uint64_t*)v.phase.p;
  }
  // the host checked the shapes the kernel's grid and LDS carve assume
  if (Bs > 0x7fffffffLL || (!gs && (W > ctcx::kMaxRecBeam || C > ctcx::kMaxRecClasses)))
    return fail(CTCEXT_INTERNAL, "shard shape outside the kernel's limits");
  v.ring = 0;
  // the two-wave kernel: decided once here (the shape's kind, or none when
  // helper_off), then the ring, the kernel and the traceback's record format
  // all follow p.helper
  const int hk = gs ? 0 : ctcx::helper_kind<T>(p, helper_mode);
  p.test_flags = (a->flags & CTCEXT_FLAG_TEST_HELPER_DEAD) ? ctcx::kTestHelperDead : 0;
  p.test_flags |= early_recurse_flag_from_env();
  // the record ring: asked for, or the default of the score-table two-wave kernel
  const bool ring = (a->flags & (CTCEXT_FLAG_RECORD_RING | CTCEXT_FLAG_RING_MIN)) ||
                    (!(a->flags & CTCEXT_FLAG_NO_RING) && ctcx::helper_rec32(hk, C));
  if (!gs && ring) {
    if (v.cus == 0 && hipDeviceGetAttribute(&v.cus, hipDeviceAttributeMultiprocessorCount, v.device) != hipSuccess)
      v.cus = 1;
    // ring frames: up to 128 (cfg3: 128 frames write 13.96M records per launch
    // instead of 64 frames' 20.86M, for +0.4% decode time, same box:
    // profiles/r5s_ring_frames.txt); CTCEXT_RING_FRAMES (diagnostics) another cap
    const char* rc = getenv("CTCEXT_RING_FRAMES");
    const int cap = (a->flags & CTCEXT_FLAG_RING_MIN) ? 8 : (rc && atoi(rc) >= 8) ? std::min(atoi(rc), 256) : 128;
    p.ring = v.ring = ctcx::ring_frames<T>(p, v.cus, cap, hk);
    if (p.ring > 0) {
      HIP_OR_FAIL(v.foff.ensure(4 * (size_t)(Bs * T_)));
      p.foff = (int32_t*)v.foff.p;
    }
  }
  p.helper = v.helper = ctcx::use_helper_kernel<T>(p, hk);
  if (gs) {
    p.gstate = (char*)v.gstate.p;
    p.gstate_stride = (int64_t)ctcx::gstate_bytes(W, (int)sizeof(T), scored);
  }

  ctcx::TraceParams& tp = pl.tp;
  tp = ctcx::TraceParams{};
  tp.rec = p.rec; tp.item = p.item; tp.seq_len = sl; tp.top_pos = p.top_pos; tp.top_kind = p.top_kind;
  tp.Tmax = T_; tp.B = Bs; tp.W = W; tp.P = P; tp.merge = a->merge_repeated ? 1 : 0;
  tp.blank_label = a->blank_label;
  tp.rec_fmt = gs ? ctcx::kRecFmt128 : ctcx::helper_rec32(v.helper, C) ? ctcx::kRecFmt32 : ctcx::kRecFmt64;
  v.rec_bytes = tp.rec_fmt == ctcx::kRecFmt128 ? 16 : tp.rec_fmt == ctcx::kRecFmt32 ? 4 : 8;
  tp.foff = p.foff;
  tp.seq = (int32_t*)v.seq.p;
  tp.len = (int32_t*)v.len.p;
  tp.len_stride = Bo;
  return CTCEXT_OK;
}

// Enqueues norm + decode + traceback of one shard on its device's stream
// (plan_shard's arguments): the workspace is grown first, then only launches,
// asynchronous copies and event records follow.
template <typename T>
static int enqueue_shard(ctcext_decoder* d, Dev& v, bool root, const ctcext_decode_args* a, const void* x, int xfmt,
                         int64_t xst_t, int64_t xst_b, const int32_t* sl, int helper_mode) {
  const int64_t T_ = a->max_time, C = a->num_classes, Bs = v.nb;
  const bool prof = (a->flags & CTCEXT_FLAG_PROFILE) != 0;
  hipStream_t s = v.s;
  v.kernel = 0;
  ShardPlan<T> pl;
  const int rc = plan_shard<T>(d, v, root, a, x, xfmt, xst_t, xst_b, sl, helper_mode, pl);
  if (rc != CTCEXT_OK) return rc;
  const ctcx::DecodeParams<T>& p = pl.p;
  int* note = ctcx_launch_note();   // (the launchers below run on this thread)
  note[0] = note[1] = note[2] = 0;

  if (prof) HIP_OR_FAIL(hipEventRecord(v.ev[0], s));
  if (pl.widen)
    HIP_OR_FAIL(ctcx::launch_widen_rows(pl.x_in, pl.xfmt_in, (float*)v.xw.p, T_, Bs, C, pl.xst_t_in, pl.xst_b_in, s));
  if (!pl.gs && C > 64) {
    // large C: the normaliser and the row facts the decode kernel reads per
    // frame, one parallel pre-pass
    HIP_OR_FAIL(ctcx::launch_row_prep<T>(p.x, p.xfmt, sl, (char*)v.prep.p, (T*)v.norm.p, T_, Bs, C, p.xst_t, p.xst_b,
                                         a->blank_index, s));
  } else {
    HIP_OR_FAIL(ctcx::launch_row_norm<T>(p.x, p.xfmt, sl, (T*)v.norm.p, T_, Bs, C, p.xst_t, p.xst_b, s));
  }
  if (prof) HIP_OR_FAIL(hipEventRecord(v.ev[1], s));

  if (a->scorer == CTCEXT_SCORER_BIGRAM)
    HIP_OR_FAIL(hipMemcpyAsync(v.sctab.p, a->scorer_table, (size_t)((C + 1) * C) * sizeof(T), hipMemcpyDefault, s));
  if (pl.gs) {
    HIP_OR_FAIL(ctcx_gstate_launch_decode(&p, sizeof(T) == 8, pl.scored, s));
  } else {
    HIP_OR_FAIL(ctcx::launch_decode<T>(p, s));
  }
  if (prof) HIP_OR_FAIL(hipEventRecord(v.ev[2], s));

  HIP_OR_FAIL(ctcx::launch_traceback(pl.tp, s));
  v.kernel = note[0] | (note[1] << 12) | (note[2] << 16);
  if (prof) HIP_OR_FAIL(hipEventRecord(v.ev[3], s));
  return CTCEXT_OK;
}

// The inputs' element strides (both 0 in a: the dense reference layout); the
// stride of a dimension of extent 1 addresses nothing, and takes the value a
// dense tensor would have.
static void input_strides(const ctcext_decode_args* a, int64_t& st_t, int64_t& st_b) {
  const int64_t T_ = a->max_time, B = a->batch_size, C = a->num_classes;
  st_t = a->inputs_stride_t ? a->inputs_stride_t : B * C;
  st_b = a->inputs_stride_b ? a->inputs_stride_b : C;
  if (T_ <= 1 && B <= 1) st_t = st_b = C;
  else if (T_ <= 1) st_t = st_b * B;
  else if (B <= 1) st_b = st_t * T_;
}

// Items [v.lo, v.lo + v.nb) of inputs that v's kernels cannot read in place, as
// a dense tensor in v.x on v's stream, and their lengths in v.sl: in the
// inputs' own element type (halves stay 2 bytes on the way) and their own
// dimension order -- [T][nb][C] from a time-major tensor, [nb][T][C] from a
// batch-major one -- so that the copy is as few pieces as the strides allow.
// st_t / st_b are the inputs' strides, es their element size; xst_t / xst_b
// receive the copy's.
static int stage_shard(Dev& v, const ctcext_decode_args* a, const std::vector<int32_t>& hsl, int64_t st_t,
                       int64_t st_b, size_t es, int64_t& xst_t, int64_t& xst_b) {
  const int64_t T_ = a->max_time, C = a->num_classes;
  const size_t cb = (size_t)C * es;
  HIP_OR_FAIL(v.x.ensure(cb * (size_t)v.nb * (size_t)T_ + 16));
  HIP_OR_FAIL(v.sl.ensure(4 * (size_t)v.nb + 16));
  const char* src = (const char*)a->inputs + (size_t)v.lo * (size_t)st_b * es;
  const bool bmajor = st_t < st_b;
  // outer dimension (extent no, source stride so) over inner (ni, si)
  const int64_t no = bmajor ? v.nb : T_, ni = bmajor ? T_ : v.nb;
  const int64_t so = bmajor ? st_b : st_t, si = bmajor ? st_t : st_b;
  const size_t slab = cb * (size_t)ni;   // one outer index of the shard
  if (si == C && (so == ni * C || no == 1)) {   // wholly contiguous
    HIP_OR_FAIL(hipMemcpyAsync(v.x.p, src, slab * (size_t)no, hipMemcpyDefault, v.s));
  } else if (si == C && so >= ni * C) {
    // contiguous slabs (a [T][nb][C] window of a [T][B][C] tensor; the
    // items of a batch-major tensor with padded frames): one pitched copy
    HIP_OR_FAIL(hipMemcpy2DAsync(v.x.p, slab, src, (size_t)so * es, slab, (size_t)no, hipMemcpyDefault, v.s));
  } else {
    // rows apart in both dimensions (a vocabulary slice): one pitched
    // copy of ni rows per outer index
    for (int64_t o = 0; o < no; ++o)
      HIP_OR_FAIL(hipMemcpy2DAsync((char*)v.x.p + (size_t)o * slab, cb, src + (size_t)o * (size_t)so * es,
                                   (size_t)si * es, cb, (size_t)ni, hipMemcpyDefault, v.s));
  }
  HIP_OR_FAIL(hipMemcpyAsync(v.sl.p, hsl.data() + v.lo, 4 * (size_t)v.nb, hipMemcpyHostToDevice, v.s));
  xst_t = bmajor ? C : v.nb * C;
  xst_b = bmajor ? T_ * C : C;
  return CTCEXT_OK;
}

// ---------------------------------------------------------------------------
// Blank-frame skipping (ctcext.h, "Blank-frame skipping"; kernels in
// ctcx_skip.hip).  In front of the unchanged pipeline: the normaliser of the
// caller's rows, the plan, and the gather of the kept rows into a dense
// tensor that enqueue_shard then decodes with the kept counts as lengths (its
// pre-pass recomputes the normaliser of the kept rows: same rows, same bits).
// Behind its traceback: the expansion of the alignment walks.

extern "C" int ctcext_skip_validate(const ctcext_skip_args* k) {
  if (!k) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!(k->logp_threshold <= 0))   // (NaN too)
    return fail(CTCEXT_INVALID_ARGUMENT, "blank skip threshold must be a log-probability (<= 0)");
  g_err.clear();
  return CTCEXT_OK;
}

// Sizes the plan's workspace (grow-only); launches nothing.
static int skip_reserve(ctcext_decoder* d, const ctcext_decode_args* a) {
  const size_t T_ = (size_t)a->max_time, B = (size_t)a->batch_size, C = (size_t)a->num_classes;
  const size_t ts = a->dtype == CTCEXT_F64 ? 8 : 4;
  const size_t es = a->inputs_format == CTCEXT_IN_NATIVE ? ts : 2;
  HIP_OR_FAIL(d->skip.norm.ensure(ts * T_ * B));
  HIP_OR_FAIL(d->skip.kmap.ensure(4 * T_ * B));
  HIP_OR_FAIL(d->skip.cidx.ensure(4 * (T_ + 1) * B));
  HIP_OR_FAIL(d->skip.kept.ensure(4 * B));
  HIP_OR_FAIL(d->skip.xc.ensure(es * T_ * B * C + 16));
  return CTCEXT_OK;
}

// Enqueues the normaliser, the plan and the gather over the rows at x (of
// a->inputs_format, strides st_t / st_b) with the sanitised lengths sl and the
// dense prologue's status words pre (or null), all on the device.  The
// normaliser is launch_row_norm's for every num_classes: without a pre-pass
// record it takes the row maximum in class order itself, as it does for the
// global-state tier at any num_classes.
template <typename T>
static int skip_front(ctcext_decoder* d, const ctcext_decode_args* a, const ctcext_skip_args* k, const void* x,
                      int64_t st_t, int64_t st_b, const int32_t* sl, const int32_t* pre, hipStream_t s) {
  const int64_t T_ = a->max_time, B = a->batch_size, C = a->num_classes;
  HIP_OR_FAIL(ctcx::launch_row_norm<T>(x, a->inputs_format, sl, (T*)d->skip.norm.p, T_, B, C, st_t, st_b, s));
  CtcxSkipPlanParams pp{};
  pp.x = x;
  pp.norm = d->skip.norm.p;
  pp.seq_len = sl;
  pp.pre = pre;
  pp.Tmax = T_; pp.B = B; pp.xst_t = st_t; pp.xst_b = st_b;
  pp.xfmt = a->inputs_format; pp.f64 = sizeof(T) == 8; pp.blank = a->blank_index;
  pp.thr = (double)(T)k->logp_threshold;
  pp.kmap = (int32_t*)d->skip.kmap.p;
  pp.cidx = (int32_t*)d->skip.cidx.p;
  pp.kept = (int32_t*)d->skip.kept.p;
  pp.kept_out = a->inputs_on_device ? k->kept : nullptr;   // (host memory otherwise: copied down by the caller)
  HIP_OR_FAIL(ctcx_launch_skip_plan(pp, s));
  CtcxSkipGatherParams gp{};
  gp.x = x;
  gp.xc = d->skip.xc.p;
  gp.kmap = pp.kmap;
  gp.kept = pp.kept;
  gp.Tmax = T_; gp.B = B; gp.C = C; gp.xst_t = st_t; gp.xst_b = st_b;
  gp.esize = a->inputs_format == CTCEXT_IN_NATIVE ? (int32_t)sizeof(T) : 2;
  HIP_OR_FAIL(ctcx_launch_skip_gather(gp, s));
  d->skip.frames = sl;
  d->skip.blank_label = a->blank_label;
  return CTCEXT_OK;
}

// The arguments of the decode behind the plan: the kept rows, dense, with the
// kept counts as lengths.
static ctcext_decode_args skip_decode_args(const ctcext_decoder* d, const ctcext_decode_args* a) {
  ctcext_decode_args c = *a;
  c.inputs = d->skip.xc.p;
  c.sequence_length = (const int32_t*)d->skip.kept.p;
  c.inputs_on_device = 1;
  c.inputs_stride_t = c.inputs_stride_b = 0;
  return c;
}

// Between the traceback and scan / pack of a skipping call: the alignment
// walks in the root's buffers, back on the original time axis.
static int skip_expand(ctcext_decoder* d, int64_t T_, int64_t B, int P, hipStream_t s) {
  Dev& root = d->devs[0];
  CtcxSkipExpandParams ep{};
  ep.seq = (int32_t*)root.seq.p;
  ep.len = (int32_t*)root.len.p;
  ep.frames = d->skip.frames;
  ep.kmap = (const int32_t*)d->skip.kmap.p;
  ep.cidx = (const int32_t*)d->skip.cidx.p;
  ep.kept = (const int32_t*)d->skip.kept.p;
  ep.Tmax = T_; ep.B = B; ep.P = P; ep.blank_label = d->skip.blank_label;
  HIP_OR_FAIL(ctcx_launch_skip_expand(ep, s));
  return CTCEXT_OK;
}

template <typename T>
static int run_decode(ctcext_decoder* d, const ctcext_decode_args* a, const std::vector<int32_t>& hsl,
                      hipStream_t root_stream, int helper_mode) {
  const int64_t T_ = a->max_time, B = a->batch_size, C = a->num_classes;
  const int P = a->top_paths;
  const int ts = (int)sizeof(T);
  // the inputs' element size and element strides
  const size_t es = a->inputs_format == CTCEXT_IN_NATIVE ? (size_t)ts : 2;
  int64_t st_t, st_b;
  input_strides(a, st_t, st_b);
  const int nd = (int)d->devs.size();
  Dev& root = d->devs[0];
  std::vector<int64_t> lo;
  shard_bounds(hsl, nd, lo);

  // 1. inputs to every device, then norm + decode + traceback, all async
  for (int i = 0; i < nd; ++i) {
    Dev& v = d->devs[(size_t)i];
    v.lo = lo[(size_t)i];
    v.nb = lo[(size_t)i + 1] - lo[(size_t)i];
    v.s = (i == 0) ? root_stream : v.own_stream;
    if (v.nb == 0 && i > 0) continue;
    HIP_OR_FAIL(hipSetDevice(v.device));
    const void* x;
    const int32_t* sl;
    int64_t xst_t = st_t, xst_b = st_b;
    if (i == 0 && a->inputs_on_device) {   // the root's shard is read in place, through its strides
      x = a->inputs;
      sl = a->sequence_length;
    } else if (v.nb == 0) {
      // an empty root shard (B < n_devices, no frames anywhere): nothing to
      // copy; enqueue_shard only sizes the root's whole-batch buffers and
      // launches no kernel over zero items
      x = nullptr;
      xst_t = xst_b = 0;
      sl = nullptr;
    } else {
      // the shard's items as a dense tensor on its device
      const int rc = stage_shard(v, a, hsl, st_t, st_b, es, xst_t, xst_b);
      if (rc != CTCEXT_OK) return rc;
      x = v.x.p;
      sl = (const int32_t*)v.sl.p;
    }
    int rc = enqueue_shard<T>(d, v, i == 0, a, x, a->inputs_format, xst_t, xst_b, sl, helper_mode);
    if (rc != CTCEXT_OK) return rc;
  }

  // 2. wait for every shard; gather the per-item results to the root
  HIP_OR_FAIL(d->h_item.ensure(sizeof(ctcx::ItemOut) * (size_t)B + 16));
  HIP_OR_FAIL(d->h_res.ensure(8 * (size_t)(P * 4) + 16));
  for (int i = nd - 1; i >= 0; --i) {
    Dev& v = d->devs[(size_t)i];
    if (v.nb == 0 && i > 0) continue;
    HIP_OR_FAIL(hipSetDevice(v.device));
    HIP_OR_FAIL(hipStreamSynchronize(v.s));
  }
  HIP_OR_FAIL(hipSetDevice(root.device));
  hipStream_t s = root.s;
  for (int i = 1; i < nd; ++i) {   // peer copies (xGMI) into the root's whole-batch buffers
    Dev& v = d->devs[(size_t)i];
    if (v.nb == 0) continue;
    const size_t per = (size_t)P * 2 * (size_t)T_ * 4;
    HIP_OR_FAIL(hipMemcpyAsync((char*)root.seq.p + (size_t)v.lo * per, v.seq.p, (size_t)v.nb * per,
                               hipMemcpyDefault, s));
    for (int k = 0; k < 2 * P; ++k)
      HIP_OR_FAIL(hipMemcpyAsync((int32_t*)root.len.p + (size_t)k * B + v.lo, (int32_t*)v.len.p + (size_t)k * v.nb,
                                 4 * (size_t)v.nb, hipMemcpyDefault, s));
    HIP_OR_FAIL(hipMemcpyAsync((int32_t*)root.top_kind.p + (size_t)v.lo * P, v.top_kind.p, 4 * (size_t)(v.nb * P),
                               hipMemcpyDefault, s));
    HIP_OR_FAIL(hipMemcpyAsync((char*)root.logp.p + (size_t)(v.lo * P) * ts, v.logp.p, (size_t)(v.nb * P) * ts,
                               hipMemcpyDefault, s));
    HIP_OR_FAIL(hipMemcpyAsync((ctcx::ItemOut*)root.item.p + v.lo, v.item.p, sizeof(ctcx::ItemOut) * (size_t)v.nb,
                               hipMemcpyDefault, s));
  }
  // 3. SparseTensor sizes over the whole batch
  HIP_OR_FAIL(d->off.ensure(8 * (size_t)(B * P * 2)));
  HIP_OR_FAIL(d->res.ensure(8 * (size_t)(P * 4)));
  HIP_OR_FAIL(d->h_kind.ensure(4 * (size_t)(B * P) + 16));
  if (d->skip.on) {   // (a helper-timeout re-decode comes through here again, over the same plan)
    const int rc = skip_expand(d, T_, B, P, s);
    if (rc != CTCEXT_OK) return rc;
  }
  HIP_OR_FAIL(ctcx::launch_scan((const int32_t*)root.len.p, (int64_t*)d->off.p, (int64_t*)d->res.p, B, P, s));
  HIP_OR_FAIL(hipMemcpyAsync(d->h_item.p, root.item.p, sizeof(ctcx::ItemOut) * (size_t)B, hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipMemcpyAsync(d->h_res.p, d->res.p, 8 * (size_t)(P * 4), hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipMemcpyAsync(d->h_kind.p, root.top_kind.p, 4 * (size_t)(B * P), hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipStreamSynchronize(s));

  d->stats = ctcext_stats{};
  d->stats.tier = use_gstate(a) ? 1 : 0;
  d->stats.ring_frames = root.ring;
  d->stats.record_bytes = root.rec_bytes;
  d->stats.helper = root.helper;
  d->stats.kernel = root.kernel;
  if (a->flags & CTCEXT_FLAG_PROFILE) {
    for (int i = 0; i < nd; ++i) {
      Dev& v = d->devs[(size_t)i];
      if (v.nb == 0) continue;
      float ms = 0;
      (void)hipEventElapsedTime(&ms, v.ev[0], v.ev[1]);
      d->stats.norm_kernel_ms = std::max(d->stats.norm_kernel_ms, (double)ms);
      (void)hipEventElapsedTime(&ms, v.ev[1], v.ev[2]);
      d->stats.decode_kernel_ms = std::max(d->stats.decode_kernel_ms, (double)ms);
      (void)hipEventElapsedTime(&ms, v.ev[2], v.ev[3]);
      d->stats.traceback_ms = std::max(d->stats.traceback_ms, (double)ms);
    }
  }
  const ctcx::ItemOut* io = (const ctcx::ItemOut*)d->h_item.p;
  for (int64_t b = 0; b < B; ++b) {
    d->stats.literal_frames += io[b].literal_steps;
    d->stats.literal_nonfinite += io[b].why_nonfinite;
    d->stats.literal_fill += io[b].why_fill;
    d->stats.duplicate_frames += io[b].dup_frames;
    d->stats.records_written += io[b].records;
    d->stats.early_recursed_frames += ctcx::item_early_frames(io[b]);
  }
  bool dead = false;
  for (int64_t b = 0; b < B; ++b) dead |= (io[b].pad & ctcx::kItemDeadMask) != 0;
  if (dead) {
    // a two-wave kernel's hand-over wait ran out of time (~1 s; never in a
    // correct run): its items' results are incomplete.  The call is decoded
    // again with the one-wave kernels, unless the caller asked to fail
    if (helper_mode == ctcx::kHelperNone || (a->flags & CTCEXT_FLAG_HELPER_STRICT))
      return fail(CTCEXT_INTERNAL, "decode kernel: a helper-wave hand-over wait timed out");
    const int rc = run_decode<T>(d, a, hsl, root_stream, ctcx::kHelperNone);
    d->stats.helper_redecodes += 1;
    return rc;
  }
  // TopPaths (decoder.h:240-243) fails on the first item with too few leaves
  for (int64_t b = 0; b < B; ++b)
    if (io[b].n_leaves < P) return fail(CTCEXT_INVALID_ARGUMENT, "Less leaves in the beam search than requested.");
  const int32_t* kinds = (const int32_t*)d->h_kind.p;
  for (int64_t q = 0; q < B * P; ++q) d->stats.no_label_paths += (kinds[q] < 0) ? 1 : 0;
  (void)C;
  return CTCEXT_OK;
}

// The plan of a synchronous skipping call and the decode behind it.  Host
// inputs are staged on the device first, as a shard is; device inputs are read
// in place.  The kept counts come down to the host afterwards (the call has
// waited by then).
template <typename T>
static int run_decode_skip(ctcext_decoder* d, const ctcext_decode_args* a, const ctcext_skip_args* k,
                           const std::vector<int32_t>& hsl, hipStream_t s, int helper_mode) {
  const int64_t B = a->batch_size;
  Dev& root = d->devs[0];
  int rc = skip_reserve(d, a);
  if (rc != CTCEXT_OK) return rc;
  const void* x = a->inputs;
  const int32_t* sl = a->sequence_length;
  int64_t st_t, st_b;
  input_strides(a, st_t, st_b);
  if (!a->inputs_on_device) {
    root.lo = 0;
    root.nb = B;
    root.s = s;
    const size_t es = a->inputs_format == CTCEXT_IN_NATIVE ? sizeof(T) : 2;
    rc = stage_shard(root, a, hsl, st_t, st_b, es, st_t, st_b);
    if (rc != CTCEXT_OK) return rc;
    x = root.x.p;
    sl = (const int32_t*)root.sl.p;
  }
  rc = skip_front<T>(d, a, k, x, st_t, st_b, sl, nullptr, s);
  if (rc != CTCEXT_OK) return rc;
  const ctcext_decode_args c = skip_decode_args(d, a);
  d->skip.on = true;
  rc = run_decode<T>(d, &c, hsl, s, helper_mode);
  d->skip.on = false;
  if (rc != CTCEXT_OK) return rc;
  if (k->kept && !a->inputs_on_device)   // (with device inputs the plan kernel wrote the caller's copy)
    HIP_OR_FAIL(hipMemcpy(k->kept, d->skip.kept.p, 4 * (size_t)B, hipMemcpyDeviceToHost));
  return CTCEXT_OK;
}

// ctcext_decode_sharded, and with k ctcext_decode_skip.
static int decode_sync(ctcext_decoder* d, const ctcext_decode_args* a, const ctcext_skip_args* k,
                       ctcext_path_sizes* sizes) {
  if (!d || !a) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  d->have = false;
  d->dense.have = false;   // (the workspace ctcext_dense_check reads is this call's now)
  d->ss.have = false;
  int rc = validate_shapes(a);
  if (rc == CTCEXT_OK && k) rc = ctcext_skip_validate(k);
  if (rc != CTCEXT_OK) return rc;
  if (k && d->devs.size() != 1)
    return fail(CTCEXT_UNIMPLEMENTED, "blank-frame skipping needs a one-device decoder handle");
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  const int64_t T_ = a->max_time, B = a->batch_size;
  hipStream_t s = a->stream ? (hipStream_t)a->stream : root.own_stream;

  // sequence_length is read on the host for validation (kernels.cc:134-139)
  // and for the shard split
  std::vector<int32_t> hsl((size_t)B);
  if (B > 0) {
    if (a->inputs_on_device) {
      HIP_OR_FAIL(hipMemcpyAsync(hsl.data(), a->sequence_length, 4 * (size_t)B, hipMemcpyDeviceToHost, s));
      HIP_OR_FAIL(hipStreamSynchronize(s));
    } else {
      memcpy(hsl.data(), a->sequence_length, 4 * (size_t)B);
    }
  }
  rc = check_lengths(hsl.data(), B, T_);
  if (rc == CTCEXT_OK) rc = check_limits(a);
  if (rc == CTCEXT_OK && a->scorer == CTCEXT_SCORER_BIGRAM && B > 0) {
    if (a->inputs_on_device) {
      const size_t tb = (size_t)((a->num_classes + 1) * a->num_classes) * (a->dtype == CTCEXT_F64 ? 8 : 4);
      std::vector<char> ht(tb);
      HIP_OR_FAIL(hipMemcpy(ht.data(), a->scorer_table, tb, hipMemcpyDeviceToHost));
      rc = check_table(a, ht.data());
    } else {
      rc = check_table(a, a->scorer_table);
    }
  }
  if (rc == CTCEXT_OK) rc = check_layout(a);
  if (rc != CTCEXT_OK) return rc;

  const int P = a->top_paths;
  d->B = B;
  d->sizes.assign((size_t)P, ctcext_path_sizes{0, 0, 0, 0});
  d->stats = ctcext_stats{};
  if (B > 0) {
    const int helper_mode = helper_mode_from_env();
    if (k)
      rc = (a->dtype == CTCEXT_F32) ? run_decode_skip<float>(d, a, k, hsl, s, helper_mode)
                                    : run_decode_skip<double>(d, a, k, hsl, s, helper_mode);
    else
      rc = (a->dtype == CTCEXT_F32) ? run_decode<float>(d, a, hsl, s, helper_mode)
                                    : run_decode<double>(d, a, hsl, s, helper_mode);
    if (rc != CTCEXT_OK) return rc;
    const int64_t* r = (const int64_t*)d->h_res.p;
    for (int p = 0; p < P; ++p) {
      d->sizes[p].num_decoded = r[(p * 2 + 0) * 2];
      d->sizes[p].max_decoded = r[(p * 2 + 0) * 2 + 1];
      d->sizes[p].num_alignment = r[(p * 2 + 1) * 2];
      d->sizes[p].max_alignment = r[(p * 2 + 1) * 2 + 1];
    }
  }
  d->have = true;
  d->dtype = a->dtype;
  d->T = T_; d->C = a->num_classes; d->W = a->beam_width; d->P = P;
  d->tt.frames = hsl;
  d->tt.C = a->num_classes; d->tt.blank_index = a->blank_index; d->tt.blank_label = a->blank_label;
  d->tt.merge = a->merge_repeated ? 1 : 0;
  // the rows the kernels read and their normaliser, for ctcext_fetch_token_scores:
  // device inputs in place, host inputs as stage_shard laid them out in root.x
  if (B > 0 && d->devs.size() == 1) {
    ScoreSrc& q = d->ss;
    input_strides(a, q.st_t, q.st_b);
    q.x = a->inputs;
    if (!a->inputs_on_device) {
      const bool bmajor = q.st_t < q.st_b;
      q.x = root.x.p;
      q.st_t = bmajor ? a->num_classes : B * a->num_classes;
      q.st_b = bmajor ? T_ * a->num_classes : a->num_classes;
    }
    q.xfmt = a->inputs_format;
    q.norm = k ? d->skip.norm.p : root.norm.p;
    q.f64 = a->dtype == CTCEXT_F64;
    q.have = true;
  }
  root.s = s;
  if (sizes)
    for (int p = 0; p < P; ++p) sizes[p] = d->sizes[p];
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_decode_sharded(ctcext_decoder* d, const ctcext_decode_args* a, ctcext_path_sizes* sizes) {
  return decode_sync(d, a, nullptr, sizes);
}

extern "C" int ctcext_decode(ctcext_decoder* d, const ctcext_decode_args* a, ctcext_path_sizes* sizes) {
  return decode_sync(d, a, nullptr, sizes);
}

extern "C" int ctcext_decode_skip(ctcext_decoder* d, const ctcext_decode_args* a, const ctcext_skip_args* k,
                                  ctcext_path_sizes* sizes) {
  if (!k) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  return decode_sync(d, a, k, sizes);
}

extern "C" int ctcext_fetch(ctcext_decoder* d, const ctcext_outputs* o) {
  if (!d || !o) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!d->have) return fail(CTCEXT_FAILED_PRECONDITION, "ctcext_fetch without a successful ctcext_decode");
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  hipStream_t s = root.s;
  const int P = d->P;
  const int64_t B = d->B;
  const int ts = d->dtype == CTCEXT_F64 ? 8 : 4;

  // shapes: {batch_size, max length} (kernels.cc:236-237, 253-254)
  std::vector<int64_t> shapes((size_t)P * 4);
  for (int p = 0; p < P; ++p) {
    shapes[p * 4 + 0] = B; shapes[p * 4 + 1] = d->sizes[p].max_decoded;
    shapes[p * 4 + 2] = B; shapes[p * 4 + 3] = d->sizes[p].max_alignment;
  }

  std::vector<int64_t*> idx((size_t)P * 2), val((size_t)P * 2);
  std::vector<size_t> off_in_stage((size_t)P * 2);
  if (o->outputs_on_device) {
    for (int p = 0; p < P; ++p) {
      idx[p * 2] = o->decoded_indices[p]; val[p * 2] = o->decoded_values[p];
      idx[p * 2 + 1] = o->alignment_indices[p]; val[p * 2 + 1] = o->alignment_values[p];
    }
  } else {
    // stage on the device, then copy down
    size_t tot = 0;
    for (int p = 0; p < P; ++p) {
      off_in_stage[p * 2] = tot; tot += (size_t)d->sizes[p].num_decoded;
      off_in_stage[p * 2 + 1] = tot; tot += (size_t)d->sizes[p].num_alignment;
    }
    HIP_OR_FAIL(d->out_idx.ensure(16 * tot + 16));
    HIP_OR_FAIL(d->out_val.ensure(8 * tot + 16));
    for (int k = 0; k < P * 2; ++k) {
      idx[k] = (int64_t*)d->out_idx.p + 2 * off_in_stage[k];
      val[k] = (int64_t*)d->out_val.p + off_in_stage[k];
    }
  }
  std::vector<int64_t*> both((size_t)P * 4);   // must outlive the async copy below
  if (B > 0) {
    HIP_OR_FAIL(d->ptrs.ensure(sizeof(int64_t*) * (size_t)P * 4));
    int64_t** dp = (int64_t**)d->ptrs.p;
    for (int k = 0; k < P * 2; ++k) { both[k] = idx[k]; both[P * 2 + k] = val[k]; }
    HIP_OR_FAIL(hipMemcpyAsync(dp, both.data(), sizeof(int64_t*) * (size_t)P * 4, hipMemcpyHostToDevice, s));
    ctcx::PackParams pp{};
    pp.seq = (const int32_t*)root.seq.p;
    pp.len = (const int32_t*)root.len.p;
    pp.off = (const int64_t*)d->off.p;
    pp.Tmax = d->T; pp.B = B; pp.P = P;
    pp.idx = dp;
    pp.val = dp + P * 2;
    HIP_OR_FAIL(ctcx::launch_pack(pp, s));
  }
  const hipMemcpyKind to_dev = o->outputs_on_device ? hipMemcpyHostToDevice : hipMemcpyHostToHost;
  for (int p = 0; p < P; ++p) {
    HIP_OR_FAIL(hipMemcpyAsync(o->decoded_shape[p], &shapes[p * 4], 16, to_dev, s));
    HIP_OR_FAIL(hipMemcpyAsync(o->alignment_shape[p], &shapes[p * 4 + 2], 16, to_dev, s));
  }
  if (B > 0) {
    HIP_OR_FAIL(hipMemcpyAsync(o->log_probability, root.logp.p, (size_t)(B * P) * ts,
                               o->outputs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (!o->outputs_on_device) {
      for (int p = 0; p < P; ++p) {
        const size_t nd = (size_t)d->sizes[p].num_decoded, na = (size_t)d->sizes[p].num_alignment;
        if (nd) {
          HIP_OR_FAIL(hipMemcpyAsync(o->decoded_indices[p], idx[p * 2], 16 * nd, hipMemcpyDeviceToHost, s));
          HIP_OR_FAIL(hipMemcpyAsync(o->decoded_values[p], val[p * 2], 8 * nd, hipMemcpyDeviceToHost, s));
        }
        if (na) {
          HIP_OR_FAIL(hipMemcpyAsync(o->alignment_indices[p], idx[p * 2 + 1], 16 * na, hipMemcpyDeviceToHost, s));
          HIP_OR_FAIL(hipMemcpyAsync(o->alignment_values[p], val[p * 2 + 1], 8 * na, hipMemcpyDeviceToHost, s));
        }
      }
    }
  }
  HIP_OR_FAIL(hipStreamSynchronize(s));
  g_err.clear();
  return CTCEXT_OK;
}

// ---------------------------------------------------------------------------
// Dense, enqueue-only decode (ctcext.h, "Dense, enqueue-only decode").  The
// checks of ctcext_decode that read data (check_lengths, check_table, the
// per-item results) run on the device: a prologue writes the lengths the
// kernels read and the status known before the decode, enqueue_shard runs on
// those lengths, and ctcx_pack_dense finishes the status and writes the padded
// outputs.  ctcext_dense_check reads the workspace copy of the status later.

extern "C" int ctcext_dense_validate(const ctcext_decode_args* a, const ctcext_dense_outputs* o) {
  int rc = validate_shapes(a);
  if (rc == CTCEXT_OK) rc = check_limits(a);
  if (rc == CTCEXT_OK) rc = check_layout(a);
  if (rc != CTCEXT_OK) return rc;
  if (!a->inputs_on_device) return fail(CTCEXT_INVALID_ARGUMENT, "ctcext_decode_dense needs device inputs");
  if (a->batch_size > 0 && (!o || !o->decoded || !o->decoded_length || !o->alignment || !o->alignment_length ||
                            !o->log_probability || !o->status))
    return fail(CTCEXT_INVALID_ARGUMENT, "null dense output pointer");
  g_err.clear();
  return CTCEXT_OK;
}

// The workspace of a dense call and its plan; launches nothing.  Sized as the
// synchronous path sizes it (plan_shard over the whole batch on the root),
// plus the prologue's words and the pinned buffers ctcext_dense_check fills.
// With skip, the plan's workspace too.
template <typename T>
static int dense_plan(ctcext_decoder* d, const ctcext_decode_args* a, bool skip, int helper_mode, ShardPlan<T>& pl) {
  const int64_t B = a->batch_size;
  if (skip) {
    const int rc = skip_reserve(d, a);
    if (rc != CTCEXT_OK) return rc;
  }
  Dev& root = d->devs[0];
  int64_t st_t, st_b;
  input_strides(a, st_t, st_b);
  d->B = B;
  root.lo = 0;
  root.nb = B;
  HIP_OR_FAIL(root.dsl.ensure(4 * (size_t)B));
  HIP_OR_FAIL(root.dstat.ensure(4 * (2 * (size_t)B + 1)));
  HIP_OR_FAIL(d->h_item.ensure(sizeof(ctcx::ItemOut) * (size_t)B + 16));
  HIP_OR_FAIL(d->h_kind.ensure(4 * (size_t)(B * a->top_paths) + 16));
  HIP_OR_FAIL(d->h_status.ensure(4 * (size_t)B + 16));
  return plan_shard<T>(d, root, true, a, a->inputs, a->inputs_format, st_t, st_b, (const int32_t*)root.dsl.p,
                       helper_mode, pl);
}

// The checks both entry points share; *s is the call's stream.
static int dense_begin(ctcext_decoder* d, const ctcext_decode_args* a, hipStream_t* s) {
  if (d->devs.size() != 1) return fail(CTCEXT_UNIMPLEMENTED, "the dense decode needs a one-device decoder handle");
  // the null stream itself with the flag: torch's legacy default stream has
  // handle 0, and the decoder's own (non-blocking) stream is not ordered behind it
  *s = a->stream ? (hipStream_t)a->stream
       : (a->flags & CTCEXT_FLAG_DENSE_NULL_STREAM) ? (hipStream_t) nullptr : d->devs[0].own_stream;
  return CTCEXT_OK;
}

// ctcext_dense_reserve, and with k ctcext_dense_reserve_skip.
static int dense_reserve(ctcext_decoder* d, const ctcext_decode_args* a, const ctcext_skip_args* k) {
  if (!d || !a) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  int rc = validate_shapes(a);
  if (rc == CTCEXT_OK && k) rc = ctcext_skip_validate(k);
  if (rc == CTCEXT_OK) rc = check_limits(a);
  if (rc == CTCEXT_OK) rc = check_layout(a);
  if (rc != CTCEXT_OK) return rc;
  hipStream_t s;
  rc = dense_begin(d, a, &s);
  if (rc != CTCEXT_OK || a->batch_size == 0) return rc;
  DeviceGuard guard;
  HIP_OR_FAIL(hipSetDevice(d->devs[0].device));
  // (the handle's state of the last call -- fetch, check, stats -- is not touched)
  const int64_t B0 = d->B;
  const int helper_mode = helper_mode_from_env();
  if (a->dtype == CTCEXT_F32) {
    ShardPlan<float> pl;
    rc = dense_plan<float>(d, a, k != nullptr, helper_mode, pl);
  } else {
    ShardPlan<double> pl;
    rc = dense_plan<double>(d, a, k != nullptr, helper_mode, pl);
  }
  d->B = B0;
  if (rc == CTCEXT_OK) g_err.clear();
  return rc;
}

extern "C" int ctcext_dense_reserve(ctcext_decoder* d, const ctcext_decode_args* a) {
  return dense_reserve(d, a, nullptr);
}

extern "C" int ctcext_dense_reserve_skip(ctcext_decoder* d, const ctcext_decode_args* a, const ctcext_skip_args* k) {
  if (!k) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  return dense_reserve(d, a, k);
}

template <typename T>
static int dense_enqueue(ctcext_decoder* d, const ctcext_decode_args* a, const ctcext_skip_args* k,
                         const ctcext_dense_outputs* o, int helper_mode) {
  const int64_t T_ = a->max_time, B = a->batch_size, C = a->num_classes;
  Dev& root = d->devs[0];
  hipStream_t s = root.s;
  ShardPlan<T> pl;
  int rc = dense_plan<T>(d, a, k != nullptr, helper_mode, pl);   // (nothing to grow after a reserve or a call of this shape)
  if (rc != CTCEXT_OK) return rc;
  int32_t* const pre = (int32_t*)root.dstat.p;
  int32_t* const fin = pre + B;
  ctcx::DensePrologueParams pp{};
  pp.seq_len = a->sequence_length;
  pp.sl = (int32_t*)root.dsl.p;
  pp.pre = pre;
  pp.Tmax = T_; pp.B = B;
  const bool bigram = a->scorer == CTCEXT_SCORER_BIGRAM;
  HIP_OR_FAIL(ctcx::launch_dense_prologue(pp, bigram ? a->scorer_table : nullptr, bigram ? (C + 1) * C : 0,
                                          sizeof(T) == 8, fin + B, s));
  int64_t st_t, st_b;
  input_strides(a, st_t, st_b);
  if (k) {
    // the plan over the caller's rows and the prologue's lengths (which stay
    // in dsl for the token times), then the pipeline over the kept rows
    const bool prof = (a->flags & CTCEXT_FLAG_PROFILE) != 0;
    if (prof) HIP_OR_FAIL(hipEventRecord(root.sk[0], s));
    rc = skip_front<T>(d, a, k, a->inputs, st_t, st_b, pp.sl, pre, s);
    if (rc != CTCEXT_OK) return rc;
    const ctcext_decode_args c = skip_decode_args(d, a);
    input_strides(&c, st_t, st_b);
    rc = enqueue_shard<T>(d, root, true, &c, c.inputs, c.inputs_format, st_t, st_b, (const int32_t*)c.sequence_length,
                          helper_mode);
    if (rc == CTCEXT_OK) rc = skip_expand(d, T_, B, a->top_paths, s);
    if (rc == CTCEXT_OK && prof) HIP_OR_FAIL(hipEventRecord(root.sk[1], s));
  } else {
    rc = enqueue_shard<T>(d, root, true, a, a->inputs, a->inputs_format, st_t, st_b, pp.sl, helper_mode);
  }
  if (rc != CTCEXT_OK) return rc;
  ctcx::PackDenseParams pd{};
  pd.seq = (const int32_t*)root.seq.p;
  pd.len = (const int32_t*)root.len.p;
  pd.item = (const ctcx::ItemOut*)root.item.p;
  pd.pre = pre;
  pd.log_prob = root.logp.p;
  pd.Tmax = T_; pd.B = B; pd.P = a->top_paths; pd.f64 = sizeof(T) == 8;
  pd.pad_value = o->pad_value;
  pd.decoded = o->decoded; pd.alignment = o->alignment;
  pd.decoded_length = o->decoded_length; pd.alignment_length = o->alignment_length;
  pd.out_log_prob = o->log_probability;
  pd.status = o->status;
  pd.status_ws = fin;
  HIP_OR_FAIL(ctcx::launch_pack_dense(pd, s));
  if (a->flags & CTCEXT_FLAG_PROFILE) HIP_OR_FAIL(hipEventRecord(root.ev[4], s));
  return CTCEXT_OK;
}

// ctcext_decode_dense, and with k ctcext_decode_dense_skip.
static int decode_dense(ctcext_decoder* d, const ctcext_decode_args* a, const ctcext_skip_args* k,
                        const ctcext_dense_outputs* o) {
  if (!d || !a) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  d->have = false;
  d->dense.have = false;
  d->ss.have = false;
  int rc = ctcext_dense_validate(a, o);
  if (rc == CTCEXT_OK && k) rc = ctcext_skip_validate(k);
  if (rc != CTCEXT_OK) return rc;
  hipStream_t s;
  rc = dense_begin(d, a, &s);
  if (rc != CTCEXT_OK) return rc;
  if (a->batch_size > 0 && (((uintptr_t)o->decoded | (uintptr_t)o->alignment) & 7))
    return fail(CTCEXT_INVALID_ARGUMENT, "dense outputs decoded and alignment need 8-byte alignment");
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  root.s = s;
  d->stats = ctcext_stats{};
  if (a->batch_size > 0) {
    const int helper_mode = helper_mode_from_env();
    rc = a->dtype == CTCEXT_F32 ? dense_enqueue<float>(d, a, k, o, helper_mode)
                                : dense_enqueue<double>(d, a, k, o, helper_mode);
    if (rc != CTCEXT_OK) return rc;
    // what the host knows; ctcext_dense_check fills the counters
    d->stats.tier = use_gstate(a) ? 1 : 0;
    d->stats.ring_frames = root.ring;
    d->stats.record_bytes = root.rec_bytes;
    d->stats.helper = root.helper;
    d->stats.kernel = root.kernel;
  }
  d->B = a->batch_size;
  d->dense.have = true;
  d->dense.B = a->batch_size; d->dense.T = a->max_time; d->dense.P = a->top_paths; d->dense.flags = a->flags;
  d->dense.s = s;
  d->dense.pack_ms = 0;
  d->dense.C = a->num_classes; d->dense.blank_index = a->blank_index; d->dense.blank_label = a->blank_label;
  d->dense.merge = a->merge_repeated ? 1 : 0;
  d->dense.times_timed = false;
  d->dense.skip = k != nullptr;
  // the caller's rows (with skipping the expanded alignment is on their axis)
  // and the normaliser over them: the plan's with skipping, the pre-pass's else
  d->dense.sc = ScoreSrc{};
  d->dense.scores_timed = false;
  if (a->batch_size > 0) {
    ScoreSrc& q = d->dense.sc;
    q.x = a->inputs;
    q.xfmt = a->inputs_format;
    input_strides(a, q.st_t, q.st_b);
    q.norm = k ? d->skip.norm.p : root.norm.p;
    q.f64 = a->dtype == CTCEXT_F64;
    q.have = true;
  }
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_decode_dense(ctcext_decoder* d, const ctcext_decode_args* a, const ctcext_dense_outputs* o) {
  return decode_dense(d, a, nullptr, o);
}

extern "C" int ctcext_decode_dense_skip(ctcext_decoder* d, const ctcext_decode_args* a, const ctcext_skip_args* k,
                                        const ctcext_dense_outputs* o) {
  if (!k) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  return decode_dense(d, a, k, o);
}

extern "C" int ctcext_dense_check(ctcext_decoder* d) {
  if (!d) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!d->dense.have) return fail(CTCEXT_FAILED_PRECONDITION, "ctcext_dense_check without a ctcext_decode_dense");
  const int64_t B = d->dense.B;
  const int P = d->dense.P;
  if (B == 0) {
    g_err.clear();
    return CTCEXT_OK;
  }
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  hipStream_t s = d->dense.s;
  HIP_OR_FAIL(hipMemcpyAsync(d->h_status.p, (const int32_t*)root.dstat.p + B, 4 * (size_t)B, hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipMemcpyAsync(d->h_item.p, root.item.p, sizeof(ctcx::ItemOut) * (size_t)B, hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipMemcpyAsync(d->h_kind.p, root.top_kind.p, 4 * (size_t)(B * P), hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipStreamSynchronize(s));

  ctcext_stats st{};
  st.tier = d->stats.tier; st.ring_frames = d->stats.ring_frames; st.record_bytes = d->stats.record_bytes;
  st.helper = d->stats.helper; st.kernel = d->stats.kernel;
  if (d->dense.flags & CTCEXT_FLAG_PROFILE) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, root.ev[0], root.ev[1]) == hipSuccess) st.norm_kernel_ms = ms;
    if (hipEventElapsedTime(&ms, root.ev[1], root.ev[2]) == hipSuccess) st.decode_kernel_ms = ms;
    if (hipEventElapsedTime(&ms, root.ev[2], root.ev[3]) == hipSuccess) st.traceback_ms = ms;
    if (hipEventElapsedTime(&ms, root.ev[3], root.ev[4]) == hipSuccess) d->dense.pack_ms = ms;
    (void)hipGetLastError();
  }
  const ctcx::ItemOut* io = (const ctcx::ItemOut*)d->h_item.p;
  const int32_t* status = (const int32_t*)d->h_status.p;
  int32_t any = 0;
  int64_t first_len = -1;
  for (int64_t b = 0; b < B; ++b) {
    st.literal_frames += io[b].literal_steps;
    st.literal_nonfinite += io[b].why_nonfinite;
    st.literal_fill += io[b].why_fill;
    st.duplicate_frames += io[b].dup_frames;
    st.records_written += io[b].records;
    st.early_recursed_frames += ctcx::item_early_frames(io[b]);
    any |= status[b];
    if ((status[b] & CTCEXT_ITEM_LENGTH) && first_len < 0) first_len = b;
  }
  d->stats = st;
  // ctcext_decode's own order: the table and the lengths before any device
  // work, the hand-over timeout before TopPaths' leaves
  if (any & CTCEXT_ITEM_TABLE)
    return fail(CTCEXT_INVALID_ARGUMENT, "beam scorer table entries must be log-probabilities (<= 0)");
  if (first_len >= 0)
    return fail(CTCEXT_FAILED_PRECONDITION,
                "sequence_length(" + std::to_string(first_len) + ") <= " + std::to_string(d->dense.T));
  if (any & CTCEXT_ITEM_HELPER_TIMEOUT)
    return fail(CTCEXT_INTERNAL, "decode kernel: a helper-wave hand-over wait timed out");
  if (any & CTCEXT_ITEM_FEW_LEAVES)
    return fail(CTCEXT_INVALID_ARGUMENT, "Less leaves in the beam search than requested.");
  const int32_t* kinds = (const int32_t*)d->h_kind.p;
  for (int64_t q = 0; q < B * P; ++q) d->stats.no_label_paths += (kinds[q] < 0) ? 1 : 0;
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_dense_skip_ms(ctcext_decoder* d, double* front_ms, double* expand_ms) {
  if (!d || !front_ms || !expand_ms) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!d->dense.have || !d->dense.skip || !(d->dense.flags & CTCEXT_FLAG_PROFILE) || d->dense.B == 0)
    return fail(CTCEXT_FAILED_PRECONDITION, "no CTCEXT_FLAG_PROFILE skipping dense decode yet");
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  HIP_OR_FAIL(hipEventSynchronize(root.sk[1]));
  float f = 0;
  HIP_OR_FAIL(hipEventElapsedTime(&f, root.sk[0], root.ev[0]));
  *front_ms = f;
  HIP_OR_FAIL(hipEventElapsedTime(&f, root.ev[3], root.sk[1]));
  *expand_ms = f;
  return CTCEXT_OK;
}

extern "C" int ctcext_dense_pack_ms(ctcext_decoder* d, double* ms) {
  if (!d || !ms) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!d->dense.have || !(d->dense.flags & CTCEXT_FLAG_PROFILE))
    return fail(CTCEXT_FAILED_PRECONDITION, "no CTCEXT_FLAG_PROFILE dense decode checked yet");
  *ms = d->dense.pack_ms;
  return CTCEXT_OK;
}

// ---------------------------------------------------------------------------
// Streaming decode (ctcext.h, "Streaming decode").  A stream owns the records
// of max_frames frames per item, two state buffers (header + LDS image per
// item; the push reads one and writes the other, and they swap when the push
// succeeded) and, on the global-state tier, the state itself.  A push runs
// the chunk's pre-pass, the stream build of the decode kernel the stream chose
// at open, and (sizes != NULL) the traceback over all frames so far into the
// decoder's walk buffers, which ctcext_fetch packs as after ctcext_decode.

struct ctcext_stream {
  ctcext_decoder* dec = nullptr;
  ctcext_stream_args a{};
  bool gs = false, scored = false;
  int helper = 0;            // the two-wave kernel of the stream's life (ctcx::use_helper_kernel at open)
  int rec_fmt = 0, rec_bytes = 8;
  int64_t image_bytes = 0;   // the decode kernel's dynamic LDS bytes (0 on the global-state tier)
  int64_t stride = 0;        // bytes per item in a state buffer
  void* state[2] = {nullptr, nullptr};
  int cur = 0;               // state[cur]: the committed state
  void* rec = nullptr;
  void* gstate = nullptr;
  void* sctab = nullptr;
  void* cum = nullptr;       // [B] int32: frames per item including the running push (the traceback's lengths)
  void* stable_cache = nullptr;   // [B] CtcxStableCache: the frontier of each item's last ctcext_stream_stable answer
  DevBuf x, xw, sl, norm, prep;
  DevBuf stable_out, stable_flags;   // ctcext_stream_stable: its outputs; position flags of beams past its LDS variant
  HostBuf h_stable;                  // ... and the outputs' pinned landing buffer (one copy per query)
  std::vector<int64_t> frames;
  // The enqueue-only push (ctcext_stream_push_dense): every buffer it touches
  // is the stream's own, none the decoder's, so that two streams of one
  // decoder can have pushes in flight at once.  It shares norm, prep, xw and
  // stable_flags above with the synchronous entry points, which wait first.
  struct {
    bool used = false;         // a push has been enqueued: the host's frames may be behind (stream_settle)
    hipStream_t s = nullptr;   // the HIP stream of the last one
    int kernel = 0;            // ctcext_stats.kernel of the last one
    int32_t flags = 0;         // its chunk flags
    bool results = false;      // it had hypothesis outputs
    double commit_ms = 0;
    bool times_timed = false;  // events [5], [6] were recorded since it
    hipEvent_t ev[7] = {};     // CTCEXT_FLAG_PROFILE: around prologue + pre-pass, decode, commit, the rest;
                               // [5], [6] around its token-times kernel
    DevBuf item, top_pos, top_kind, logp, seq, len;
    DevBuf sl, pre, fin, acc, walked;   // [B] each: sanitised lengths, status before / after the decode,
                                        // the deferred record (CtcxStreamAcc), stable's walked
    HostBuf land;              // the check's landing buffer: frames | acc | ItemOut | top_kind
  } dn;
  // Blank-frame skipping (ctcext_stream_open_skip; ctcext.h, "Streaming:
  // blank-frame skipping"): the plan's state per item and the workspace of the
  // chunk in front of the pre-pass, the stream's own like dn.
  struct {
    bool on = false;
    double thr = 0;            // rounded to the compute dtype
    int32_t* kept_out = nullptr;   // the caller's device [B], or null
    DevBuf item;               // [B] CtcxSkipItem
    DevBuf kmap, cidx;         // [B][max_frames], [B][max_frames + 1]
    DevBuf nfr;                // [B] int32: n per item after the last push
    DevBuf norm, ckmap, klen, xc;   // of the chunk: the caller's rows' normaliser, the gather's map, the kept
                                    // lengths, the kept rows [chunk_time][B][C] in the chunk's element type
    HostBuf land;              // stream_settle's: the items
  } sk;
  std::vector<int64_t> kept;   // host mirror of the record frames of a skipping stream (frames holds n there)
  // The score store (ctcext_stream_open_scores; ctcext.h, "Streaming: token
  // scores"): the logits and the normaliser of every committed frame, on the
  // original time axis, allocated at open for the stream's life.
  struct {
    bool on = false;
    int32_t fmt = 0;           // sx's element format (CTCEXT_IN_*)
    void* sx = nullptr;        // [B][max_frames][C]
    void* snorm = nullptr;     // [max_frames][B] of the compute dtype
    bool append_timed = false, scores_timed = false;   // events [0], [1] / [2], [3] were recorded for the last push
    hipEvent_t ev[4] = {};     // CTCEXT_FLAG_PROFILE: around the append kernel, around the token-scores kernel
  } sc;
};

// The stream's attributes as the one-shot argument struct, for the shared
// checks (one frame of a well-formed batch; inputs are not read by them).
static ctcext_decode_args stream_decode_args(const ctcext_stream_args* a) {
  static const int32_t one = 1;
  ctcext_decode_args d{};
  d.dtype = a->dtype;
  d.inputs_on_device = 1;
  d.inputs = &one;
  d.sequence_length = &one;
  d.max_time = 1; d.batch_size = a->batch_size; d.num_classes = a->num_classes;
  d.beam_width = a->beam_width; d.top_paths = a->top_paths; d.merge_repeated = a->merge_repeated;
  d.blank_index = a->blank_index; d.blank_label = a->blank_label; d.flags = a->flags;
  d.inputs_dims = 3; d.sequence_length_dims = 1; d.sequence_length_size = a->batch_size;
  d.scorer = a->scorer; d.scorer_table = a->scorer_table;
  return d;
}

extern "C" int ctcext_stream_validate(const ctcext_stream_args* a) {
  if (!a) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  const ctcext_decode_args d = stream_decode_args(a);
  int rc = validate_shapes(&d);
  if (rc == CTCEXT_OK) rc = check_limits(&d);
  // (the table is host memory whatever on_device says: ctcext.h)
  if (rc == CTCEXT_OK) rc = check_table(&d, a->scorer_table);
  if (rc == CTCEXT_OK && (a->flags & ~(CTCEXT_FLAG_FORCE_LITERAL | CTCEXT_FLAG_GLOBAL_STATE | CTCEXT_FLAG_PROFILE)))
    rc = fail(CTCEXT_INVALID_ARGUMENT, "stream flags: CTCEXT_FLAG_FORCE_LITERAL, _GLOBAL_STATE and _PROFILE only");
  if (rc == CTCEXT_OK && a->max_frames < 0) rc = fail(CTCEXT_INVALID_ARGUMENT, "max_frames is negative");
  if (rc == CTCEXT_OK && a->max_frames > INT32_MAX)
    rc = fail(CTCEXT_UNIMPLEMENTED, "max_frames beyond this library's 32-bit frame indices");
  if (rc == CTCEXT_OK) g_err.clear();
  return rc;
}

// A chunk against its stream's attributes, host only: the layout checks of
// ctcext_validate with chunk_time as max_time, and the lengths when the
// caller holds them on the host (hcl; null: not checked here).
static int check_chunk(const ctcext_stream_args* a, const ctcext_chunk* c, const int32_t* hcl) {
  if (!a || !c) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (c->chunk_time < 0) return fail(CTCEXT_INVALID_ARGUMENT, "inputs has a negative dimension");
  if (a->batch_size > 0 && c->chunk_time > 0 && !c->inputs) return fail(CTCEXT_INVALID_ARGUMENT, "null input pointer");
  if (hcl) {
    const int rc = check_lengths(hcl, a->batch_size, c->chunk_time);
    if (rc != CTCEXT_OK) return rc;
  }
  ctcext_decode_args d = stream_decode_args(a);
  d.max_time = c->chunk_time;
  d.inputs_format = c->inputs_format;
  d.inputs_stride_t = c->inputs_stride_t;
  d.inputs_stride_b = c->inputs_stride_b;
  return check_layout(&d);
}

extern "C" int ctcext_stream_validate_chunk(const ctcext_stream_args* a, const ctcext_chunk* c) {
  int rc = ctcext_stream_validate(a);
  if (rc != CTCEXT_OK) return rc;
  rc = check_chunk(a, c, (c && !a->on_device) ? c->chunk_length : nullptr);
  if (rc == CTCEXT_OK) g_err.clear();
  return rc;
}

static void stream_free(ctcext_stream* st) {
  void* ps[] = {st->state[0], st->state[1], st->rec,   st->gstate, st->sctab, st->cum, st->stable_cache,
                st->sc.sx,    st->sc.snorm};
  for (void* p : ps)
    if (p) (void)hipFree(p);
  DevBuf* bufs[] = {&st->x, &st->xw, &st->sl, &st->norm, &st->prep, &st->stable_out, &st->stable_flags};
  for (DevBuf* b : bufs) b->release();
  st->h_stable.release();
  DevBuf* dbufs[] = {&st->dn.item, &st->dn.top_pos, &st->dn.top_kind, &st->dn.logp, &st->dn.seq, &st->dn.len,
                     &st->dn.sl, &st->dn.pre, &st->dn.fin, &st->dn.acc, &st->dn.walked};
  for (DevBuf* b : dbufs) b->release();
  st->dn.land.release();
  DevBuf* kbufs[] = {&st->sk.item, &st->sk.nfr,   &st->sk.kmap, &st->sk.cidx,
                     &st->sk.norm, &st->sk.ckmap, &st->sk.klen, &st->sk.xc};
  for (DevBuf* b : kbufs) b->release();
  st->sk.land.release();
  for (auto& ev : st->dn.ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : st->sc.ev)
    if (ev) (void)hipEventDestroy(ev);
  delete st;
}

// Landing layout of an enqueue-only stream's check (dn.land): the committed
// frames [B] int32, the deferred record [B], the items' counters [B], and the
// last push's top_kind [B][P].
static size_t land_acc_off(int64_t B) { return (4 * (size_t)B + 15) & ~(size_t)15; }
static size_t land_item_off(int64_t B) { return land_acc_off(B) + sizeof(CtcxStreamAcc) * (size_t)B; }
static size_t land_kind_off(int64_t B) { return land_item_off(B) + sizeof(ctcx::ItemOut) * (size_t)B; }

// Waits for the enqueue-only pushes of st (if it ever had one: a captured push
// may have been replayed since) and brings the committed frames down into the
// host mirror.  The deferred status stays on the device for ctcext_stream_check.
static int stream_settle(ctcext_stream* st) {
  if (!st->dn.used) return CTCEXT_OK;
  const int64_t B = st->a.batch_size;
  if (B == 0) return CTCEXT_OK;
  const int P = st->a.top_paths;
  char* h = (char*)st->dn.land.p;
  hipStream_t s = st->dn.s;
  // (CtcxStreamHdr.frames, the header's first word, of every item: right whichever form of push wrote it last)
  HIP_OR_FAIL(hipMemcpy2DAsync(h, 4, st->state[st->cur], (size_t)st->stride, 4, (size_t)B, hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipMemcpyAsync(h + land_acc_off(B), st->dn.acc.p, sizeof(CtcxStreamAcc) * (size_t)B,
                             hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipMemcpyAsync(h + land_item_off(B), st->dn.item.p, sizeof(ctcx::ItemOut) * (size_t)B,
                             hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipMemcpyAsync(h + land_kind_off(B), st->dn.top_kind.p, 4 * (size_t)(B * P), hipMemcpyDeviceToHost, s));
  if (st->sk.on)
    HIP_OR_FAIL(hipMemcpyAsync(st->sk.land.p, st->sk.item.p, sizeof(CtcxSkipItem) * (size_t)B, hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipStreamSynchronize(s));
  const int32_t* fr = (const int32_t*)h;
  if (st->sk.on) {   // frames are the original axis's n; the header's count is the kept frames
    const CtcxSkipItem* it = (const CtcxSkipItem*)st->sk.land.p;
    for (int64_t b = 0; b < B; ++b) {
      st->frames[(size_t)b] = it[b].n;
      st->kept[(size_t)b] = fr[b];
    }
    return CTCEXT_OK;
  }
  for (int64_t b = 0; b < B; ++b) st->frames[(size_t)b] = fr[b];
  return CTCEXT_OK;
}

// The DecodeParams of a push (or, with no chunk yet, of the kernel query at open).
template <typename T>
static ctcx::DecodeParams<T> stream_decode_params(const ctcext_stream* st) {
  const ctcext_stream_args& a = st->a;
  ctcx::DecodeParams<T> p{};
  p.Tmax = a.max_frames; p.B = a.batch_size; p.C = a.num_classes;
  p.W = a.beam_width; p.P = a.top_paths; p.blank = a.blank_index; p.blank_label = a.blank_label;
  p.force_literal = ((a.flags & CTCEXT_FLAG_FORCE_LITERAL) || a.num_classes < 2) ? 1 : 0;
  p.rec = (ctcx::Rec*)st->rec;
  p.scorer_tab = (const T*)st->sctab;
  p.ring = 0;                 // every record is written: a later chunk may reach what a ring would prune
  p.helper = st->helper;
  if (st->gs) {
    p.gstate = (char*)st->gstate;
    p.gstate_stride = (int64_t)ctcx::gstate_bytes(a.beam_width, (int)sizeof(T), st->scored);
  }
  return p;
}

template <typename T>
static int stream_open_t(ctcext_stream* st) {
  const ctcext_stream_args& a = st->a;
  const int64_t B = a.batch_size, C = a.num_classes, F = a.max_frames;
  const int W = a.beam_width, P = a.top_paths;
  Dev& root = st->dec->devs[0];
  hipStream_t s = root.own_stream;
  if (st->scored) {
    const size_t tb = (size_t)((C + 1) * C) * sizeof(T);
    HIP_OR_FAIL(hipMalloc(&st->sctab, tb));
    // (host memory, checked by ctcext_stream_validate; the copy is done before open returns)
    HIP_OR_FAIL(hipMemcpyAsync(st->sctab, a.scorer_table, tb, hipMemcpyHostToDevice, s));
  }
  if (B > 0x7fffffffLL || (!st->gs && (W > ctcx::kMaxRecBeam || C > ctcx::kMaxRecClasses)))
    return fail(CTCEXT_INTERNAL, "shard shape outside the kernel's limits");
  int* note = ctcx_launch_note();
  note[0] = 0;
  if (st->gs) {
    st->helper = 0;
    st->image_bytes = 0;
    st->rec_fmt = ctcx::kRecFmt128;
    HIP_OR_FAIL(hipMalloc(&st->gstate, ctcx::gstate_bytes(W, (int)sizeof(T), st->scored) * (size_t)B + 256));
  } else {
    // the kernel of the stream's life: launch_decode's rules with the helper
    // kind decided here; its launcher reports the LDS bytes (the image) and
    // launches nothing
    ctcx::DecodeParams<T> p = stream_decode_params<T>(st);
    const int hk = ctcx::helper_kind<T>(p, helper_mode_from_env());
    p.helper = st->helper = ctcx::use_helper_kernel<T>(p, hk);
    int64_t lds = 0;
    CtcxStreamParams sp{};
    sp.query = &lds;
    HIP_OR_FAIL(ctcx_stream_launch_decode(&p, &sp, sizeof(T) == 8, s));
    st->image_bytes = lds;
    st->rec_fmt = ctcx::helper_rec32(st->helper, C) ? ctcx::kRecFmt32 : ctcx::kRecFmt64;
  }
  st->rec_bytes = st->rec_fmt == ctcx::kRecFmt128 ? 16 : st->rec_fmt == ctcx::kRecFmt32 ? 4 : 8;
  st->stride = (int64_t)((ctcx_stream_hdr_bytes(P) + (size_t)st->image_bytes + 255) & ~(size_t)255);
  const size_t sb = (size_t)st->stride * (size_t)B + 256;
  for (int k = 0; k < 2; ++k) {
    HIP_OR_FAIL(hipMalloc(&st->state[k], sb));
    HIP_OR_FAIL(hipMemsetAsync(st->state[k], 0, sb, s));   // frames == 0: every item starts from Reset()
  }
  HIP_OR_FAIL(hipMalloc(&st->rec, (size_t)st->rec_bytes * (size_t)(B * F * W) + 256));
  HIP_OR_FAIL(hipMalloc(&st->cum, 4 * (size_t)B + 256));
  HIP_OR_FAIL(hipMalloc(&st->stable_cache, sizeof(CtcxStableCache) * (size_t)B + 256));
  HIP_OR_FAIL(hipMemsetAsync(st->stable_cache, 0, sizeof(CtcxStableCache) * (size_t)B + 256, s));
  HIP_OR_FAIL(hipStreamSynchronize(s));
  st->frames.assign((size_t)B, 0);
  return CTCEXT_OK;
}

// The per-item state of a skipping stream: sized by the batch and max_frames
// alone, so allocated at open.  Every item starts with no frame and no flag.
static int stream_open_skip_state(ctcext_stream* st) {
  const size_t B = (size_t)st->a.batch_size, F = (size_t)st->a.max_frames;
  hipStream_t s = st->dec->devs[0].own_stream;
  HIP_OR_FAIL(st->sk.item.ensure(sizeof(CtcxSkipItem) * B + 16));
  HIP_OR_FAIL(hipMemsetAsync(st->sk.item.p, 0, sizeof(CtcxSkipItem) * B + 16, s));
  HIP_OR_FAIL(st->sk.kmap.ensure(4 * F * B + 16));
  HIP_OR_FAIL(st->sk.cidx.ensure(4 * (F + 1) * B + 16));
  HIP_OR_FAIL(hipMemsetAsync(st->sk.cidx.p, 0, 4 * (F + 1) * B + 16, s));
  HIP_OR_FAIL(st->sk.land.ensure(sizeof(CtcxSkipItem) * B + 16));
  HIP_OR_FAIL(hipStreamSynchronize(s));
  st->kept.assign(B, 0);
  return CTCEXT_OK;
}

// The score store of a stream: sized by the batch, max_frames and num_classes
// alone, so allocated at open, with the events of its timings (a push
// allocates nothing).  Rows are written before they are read; nothing to clear.
static int stream_open_score_store(ctcext_stream* st, int32_t store_format) {
  const ctcext_stream_args& a = st->a;
  int64_t xb = 0, nb = 0;
  if (!ctcx_store_bytes(a.batch_size, a.max_frames, a.num_classes, store_format, a.dtype == CTCEXT_F64, &xb, &nb))
    return fail(CTCEXT_INVALID_ARGUMENT, "the score store's size leaves 64 bits");
  st->sc.fmt = store_format;
  // (+ 256 like the stream's other buffers: never a zero-byte allocation, with batch_size or max_frames 0; the
  //  kernels stay inside the xb and nb bytes that ctcext_stream_scores_bytes reports)
  HIP_OR_FAIL(hipMalloc(&st->sc.sx, (size_t)xb + 256));
  HIP_OR_FAIL(hipMalloc(&st->sc.snorm, (size_t)nb + 256));
  for (auto& ev : st->sc.ev) HIP_OR_FAIL(hipEventCreate(&ev));
  st->sc.on = true;
  return CTCEXT_OK;
}

// k: the checked skip arguments of ctcext_stream_open_skip, or null; sa: the
// checked arguments of ctcext_stream_open_scores, or null.
static int stream_open_common(ctcext_decoder* d, const ctcext_stream_args* a, const ctcext_skip_args* k,
                              const ctcext_stream_scores_args* sa, ctcext_stream** out) {
  int rc;
  DeviceGuard guard;
  HIP_OR_FAIL(hipSetDevice(d->devs[0].device));
  ctcext_stream* st = new ctcext_stream();
  st->dec = d;
  st->a = *a;
  const ctcext_decode_args da = stream_decode_args(a);
  st->gs = use_gstate(&da);
  st->scored = a->scorer != CTCEXT_SCORER_BASE && a->batch_size > 0;
  rc = a->dtype == CTCEXT_F64 ? stream_open_t<double>(st) : stream_open_t<float>(st);
  if (rc == CTCEXT_OK && k) {
    st->sk.on = true;
    st->sk.thr = a->dtype == CTCEXT_F64 ? k->logp_threshold : (double)(float)k->logp_threshold;
    st->sk.kept_out = k->kept;
    rc = stream_open_skip_state(st);
  }
  if (rc == CTCEXT_OK && sa) rc = stream_open_score_store(st, sa->store_format);
  st->a.scorer_table = nullptr;   // (copied)
  if (rc != CTCEXT_OK) {
    const std::string keep = g_err;
    stream_free(st);
    g_err = keep;
    return rc;
  }
  *out = st;
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_stream_open(ctcext_decoder* d, const ctcext_stream_args* a, ctcext_stream** out) {
  if (!d || !a || !out) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  const int rc = ctcext_stream_validate(a);
  if (rc != CTCEXT_OK) return rc;
  if (d->devs.size() != 1) return fail(CTCEXT_UNIMPLEMENTED, "a stream needs a one-device decoder handle");
  return stream_open_common(d, a, nullptr, nullptr, out);
}

// What a skipping stream asks of its arguments beyond ctcext_stream_validate,
// on the host; the decoder handle is looked at last (it is the one argument
// that needs a device to exist).
extern "C" int ctcext_stream_open_skip(ctcext_decoder* d, const ctcext_stream_args* a, const ctcext_skip_args* k,
                                       ctcext_stream** out) {
  if (!a || !out) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  int rc = ctcext_stream_validate(a);
  if (rc != CTCEXT_OK) return rc;
  if (!k) return fail(CTCEXT_INVALID_ARGUMENT, "ctcext_stream_open_skip needs skip arguments");
  rc = ctcext_skip_validate(k);
  if (rc != CTCEXT_OK) return rc;
  if (a->on_device != 1)
    return fail(CTCEXT_INVALID_ARGUMENT, "a skipping stream needs device chunks (on_device == 1): it has the "
                                         "enqueue-only push alone");
  if (!d) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (d->devs.size() != 1) return fail(CTCEXT_UNIMPLEMENTED, "a skipping stream needs a one-device decoder handle");
  return stream_open_common(d, a, k, nullptr, out);
}

extern "C" int ctcext_stream_kept(ctcext_stream* st, int64_t* kept) {
  if (!st || !kept) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (st->dn.used) {
    DeviceGuard guard;
    HIP_OR_FAIL(hipSetDevice(st->dec->devs[0].device));
    const int rc = stream_settle(st);
    if (rc != CTCEXT_OK) return rc;
  }
  const std::vector<int64_t>& v = st->sk.on ? st->kept : st->frames;   // (without skipping every frame is kept)
  for (size_t b = 0; b < v.size(); ++b) kept[b] = v[b];
  return CTCEXT_OK;
}

extern "C" void ctcext_stream_close(ctcext_stream* st) {
  if (!st) return;
  DeviceGuard guard;
  Dev& root = st->dec->devs[0];
  (void)hipSetDevice(root.device);
  if (root.own_stream) (void)hipStreamSynchronize(root.own_stream);
  if (st->dn.used) (void)hipStreamSynchronize(st->dn.s);   // enqueue-only pushes still in flight
  stream_free(st);
}

extern "C" int ctcext_stream_frames(ctcext_stream* st, int64_t* frames) {
  if (!st || !frames) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (st->dn.used) {   // enqueue-only pushes: the counts live on the device until waited for
    DeviceGuard guard;
    HIP_OR_FAIL(hipSetDevice(st->dec->devs[0].device));
    const int rc = stream_settle(st);
    if (rc != CTCEXT_OK) return rc;
  }
  for (size_t b = 0; b < st->frames.size(); ++b) frames[b] = st->frames[b];
  return CTCEXT_OK;
}

extern "C" int ctcext_stream_reset(ctcext_stream* st, const int32_t* items, int64_t n) {
  if (!st) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  const int64_t B = st->a.batch_size;
  if (items) {
    if (n < 0) return fail(CTCEXT_INVALID_ARGUMENT, "negative item count");
    for (int64_t i = 0; i < n; ++i)
      if (items[i] < 0 || items[i] >= B) return fail(CTCEXT_INVALID_ARGUMENT, "stream item out of range [0, batch_size)");
  }
  DeviceGuard guard;
  Dev& root = st->dec->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  hipStream_t s = root.own_stream;
  {
    const int rc = stream_settle(st);
    if (rc != CTCEXT_OK) return rc;
  }
  // frames = 0 in the committed header: the item's next push runs Reset()
  const int64_t cnt = items ? n : B;
  for (int64_t i = 0; i < cnt; ++i) {
    const int64_t b = items ? items[i] : i;
    HIP_OR_FAIL(hipMemsetAsync((char*)st->state[st->cur] + (size_t)b * (size_t)st->stride, 0, sizeof(CtcxStreamHdr), s));
    // ... and its stable-prefix frontier goes with the utterance
    HIP_OR_FAIL(hipMemsetAsync((CtcxStableCache*)st->stable_cache + b, 0, sizeof(CtcxStableCache), s));
    // ... and so do a skipping stream's n and carried flag: the next frame is frame 0, and kept
    if (st->sk.on) HIP_OR_FAIL(hipMemsetAsync((CtcxSkipItem*)st->sk.item.p + b, 0, sizeof(CtcxSkipItem), s));
  }
  HIP_OR_FAIL(hipStreamSynchronize(s));
  for (int64_t i = 0; i < cnt; ++i) st->frames[(size_t)(items ? items[i] : i)] = 0;
  if (st->sk.on)
    for (int64_t i = 0; i < cnt; ++i) st->kept[(size_t)(items ? items[i] : i)] = 0;
  g_err.clear();
  return CTCEXT_OK;
}

template <typename T>
static int stream_push_t(ctcext_stream* st, const ctcext_chunk* c, const std::vector<int32_t>& hcl,
                         ctcext_path_sizes* sizes, hipStream_t s) {
  ctcext_decoder* d = st->dec;
  Dev& root = d->devs[0];
  const ctcext_stream_args& a = st->a;
  const int64_t B = a.batch_size, C = a.num_classes, F = a.max_frames, Tc = c->chunk_time;
  const int W = a.beam_width, P = a.top_paths;
  const int ts = (int)sizeof(T);
  const bool prof = ((a.flags | c->flags) & CTCEXT_FLAG_PROFILE) != 0;
  int* note = ctcx_launch_note();
  note[0] = note[1] = note[2] = 0;

  // the chunk's element strides, as run_decode takes a whole tensor's
  int xfmt = c->inputs_format;
  const size_t es = xfmt == CTCEXT_IN_NATIVE ? (size_t)ts : 2;
  int64_t st_t = c->inputs_stride_t ? c->inputs_stride_t : B * C;
  int64_t st_b = c->inputs_stride_b ? c->inputs_stride_b : C;
  if (Tc <= 1 && B <= 1) st_t = st_b = C;
  else if (Tc <= 1) st_t = st_b * B;
  else if (B <= 1) st_b = st_t * Tc;
  const void* x = c->inputs;
  const int32_t* sl = nullptr;
  std::vector<int32_t> hcum((size_t)B);
  for (int64_t b = 0; b < B; ++b) hcum[(size_t)b] = (int32_t)(st->frames[(size_t)b] + hcl[(size_t)b]);
  HIP_OR_FAIL(hipMemcpyAsync(st->cum, hcum.data(), 4 * (size_t)B, hipMemcpyHostToDevice, s));
  if (a.on_device && c->chunk_length) {
    sl = c->chunk_length;
  } else {
    HIP_OR_FAIL(st->sl.ensure(4 * (size_t)B + 16));
    HIP_OR_FAIL(hipMemcpyAsync(st->sl.p, hcl.data(), 4 * (size_t)B, hipMemcpyHostToDevice, s));
    sl = (const int32_t*)st->sl.p;
  }
  if (!a.on_device && Tc > 0) {
    // host chunks: the rows as a dense tensor on the device, in their own
    // element type and dimension order (run_decode's shard copy, whole batch)
    const size_t cb = (size_t)C * es;
    HIP_OR_FAIL(st->x.ensure(cb * (size_t)B * (size_t)Tc + 16));
    const char* src = (const char*)c->inputs;
    const bool bmajor = st_t < st_b;
    const int64_t no = bmajor ? B : Tc, ni = bmajor ? Tc : B;
    const int64_t so = bmajor ? st_b : st_t, si = bmajor ? st_t : st_b;
    const size_t slab = cb * (size_t)ni;
    if (si == C && (so == ni * C || no == 1)) {
      HIP_OR_FAIL(hipMemcpyAsync(st->x.p, src, slab * (size_t)no, hipMemcpyDefault, s));
    } else if (si == C && so >= ni * C) {
      HIP_OR_FAIL(hipMemcpy2DAsync(st->x.p, slab, src, (size_t)so * es, slab, (size_t)no, hipMemcpyDefault, s));
    } else {
      for (int64_t o = 0; o < no; ++o)
        HIP_OR_FAIL(hipMemcpy2DAsync((char*)st->x.p + (size_t)o * slab, cb, src + (size_t)o * (size_t)so * es,
                                     (size_t)si * es, cb, (size_t)ni, hipMemcpyDefault, s));
    }
    x = st->x.p;
    st_t = bmajor ? C : B * C;
    st_b = bmajor ? Tc * C : C;
  }

  HIP_OR_FAIL(root.item.ensure(sizeof(ctcx::ItemOut) * (size_t)B));
  HIP_OR_FAIL(root.top_pos.ensure(4 * (size_t)(B * P)));
  HIP_OR_FAIL(root.top_kind.ensure(4 * (size_t)(B * P)));
  HIP_OR_FAIL(root.logp.ensure(sizeof(T) * (size_t)(B * P)));
  if (prof) HIP_OR_FAIL(hipEventRecord(root.ev[0], s));
  if (Tc > 0) {   // the pre-pass over the chunk's rows (chunk-local indices)
    HIP_OR_FAIL(st->norm.ensure(sizeof(T) * (size_t)(Tc * B)));
    if (st->gs && xfmt != CTCEXT_IN_NATIVE) {
      HIP_OR_FAIL(st->xw.ensure(4 * (size_t)(Tc * B * C) + 16));
      HIP_OR_FAIL(ctcx::launch_widen_rows(x, xfmt, (float*)st->xw.p, Tc, B, C, st_t, st_b, s));
      x = st->xw.p;
      xfmt = CTCEXT_IN_NATIVE;
      st_t = B * C;
      st_b = C;
    }
    if (!st->gs && C > 64) {
      HIP_OR_FAIL(st->prep.ensure(ctcx::prep_row_bytes(C, ts) * (size_t)(Tc * B)));
      HIP_OR_FAIL(ctcx::launch_row_prep<T>(x, xfmt, sl, (char*)st->prep.p, (T*)st->norm.p, Tc, B, C, st_t, st_b,
                                           a.blank_index, s));
    } else {
      HIP_OR_FAIL(ctcx::launch_row_norm<T>(x, xfmt, sl, (T*)st->norm.p, Tc, B, C, st_t, st_b, s));
    }
  }
  if (prof) HIP_OR_FAIL(hipEventRecord(root.ev[1], s));

  ctcx::DecodeParams<T> p = stream_decode_params<T>(st);
  p.x = (const T*)x;
  p.xfmt = xfmt;
  p.norm = (const T*)st->norm.p;
  p.seq_len = sl;
  p.xst_t = st_t; p.xst_b = st_b;
  p.item = (ctcx::ItemOut*)root.item.p;
  p.top_pos = (int32_t*)root.top_pos.p;
  p.top_kind = (int32_t*)root.top_kind.p;
  p.log_prob = (T*)root.logp.p;
  p.prep = (const char*)st->prep.p;
  p.test_flags = (c->flags & CTCEXT_FLAG_TEST_HELPER_DEAD) ? ctcx::kTestHelperDead : 0;
  p.test_flags |= early_recurse_flag_from_env();
  CtcxStreamParams sp{};
  sp.in = (const char*)st->state[st->cur];
  sp.out = (char*)st->state[st->cur ^ 1];
  sp.stride = st->stride;
  sp.image_bytes = st->image_bytes;
  if (st->gs) HIP_OR_FAIL(ctcx_gstate_stream_launch_decode(&p, &sp, ts == 8, st->scored, s));
  else HIP_OR_FAIL(ctcx_stream_launch_decode(&p, &sp, ts == 8, s));
  if (prof) HIP_OR_FAIL(hipEventRecord(root.ev[2], s));

  HIP_OR_FAIL(d->h_item.ensure(sizeof(ctcx::ItemOut) * (size_t)B + 16));
  if (sizes) {
    // the walks of every frame so far, from the records the stream keeps
    HIP_OR_FAIL(root.seq.ensure(4 * (size_t)(B * P * 2 * F) + 16));
    HIP_OR_FAIL(root.len.ensure(4 * (size_t)(B * P * 2)));
    ctcx::TraceParams tp{};
    tp.rec = p.rec; tp.item = p.item; tp.seq_len = (const int32_t*)st->cum; tp.top_pos = p.top_pos;
    tp.top_kind = p.top_kind;
    tp.Tmax = F; tp.B = B; tp.W = W; tp.P = P; tp.merge = a.merge_repeated ? 1 : 0;
    tp.blank_label = a.blank_label;
    tp.rec_fmt = st->rec_fmt;
    tp.foff = nullptr;
    tp.seq = (int32_t*)root.seq.p;
    tp.len = (int32_t*)root.len.p;
    tp.len_stride = B;
    HIP_OR_FAIL(ctcx::launch_traceback(tp, s));
    HIP_OR_FAIL(d->h_res.ensure(8 * (size_t)(P * 4) + 16));
    HIP_OR_FAIL(d->off.ensure(8 * (size_t)(B * P * 2)));
    HIP_OR_FAIL(d->res.ensure(8 * (size_t)(P * 4)));
    HIP_OR_FAIL(d->h_kind.ensure(4 * (size_t)(B * P) + 16));
    HIP_OR_FAIL(ctcx::launch_scan((const int32_t*)root.len.p, (int64_t*)d->off.p, (int64_t*)d->res.p, B, P, s));
    HIP_OR_FAIL(hipMemcpyAsync(d->h_res.p, d->res.p, 8 * (size_t)(P * 4), hipMemcpyDeviceToHost, s));
    HIP_OR_FAIL(hipMemcpyAsync(d->h_kind.p, root.top_kind.p, 4 * (size_t)(B * P), hipMemcpyDeviceToHost, s));
  }
  if (prof) HIP_OR_FAIL(hipEventRecord(root.ev[3], s));
  HIP_OR_FAIL(hipMemcpyAsync(d->h_item.p, root.item.p, sizeof(ctcx::ItemOut) * (size_t)B, hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipStreamSynchronize(s));

  const ctcx::ItemOut* io = (const ctcx::ItemOut*)d->h_item.p;
  for (int64_t b = 0; b < B; ++b)
    if ((io[b].pad & ctcx::kItemDeadMask) != 0)   // (the state buffers are not swapped: the stream stays at its pre-push state)
      return fail(CTCEXT_INTERNAL, "decode kernel: a helper-wave hand-over wait timed out");
  // the push is committed
  st->cur ^= 1;
  for (int64_t b = 0; b < B; ++b) st->frames[(size_t)b] = hcum[(size_t)b];
  d->stats = ctcext_stats{};
  d->stats.tier = st->gs ? 1 : 0;
  d->stats.record_bytes = st->rec_bytes;
  d->stats.helper = st->helper;
  d->stats.kernel = note[0] | (note[1] << 12) | (note[2] << 16);
  if (prof) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, root.ev[0], root.ev[1]);
    d->stats.norm_kernel_ms = ms;
    (void)hipEventElapsedTime(&ms, root.ev[1], root.ev[2]);
    d->stats.decode_kernel_ms = ms;
    (void)hipEventElapsedTime(&ms, root.ev[2], root.ev[3]);
    d->stats.traceback_ms = ms;
  }
  for (int64_t b = 0; b < B; ++b) {   // (the kernel carries the counters in the item's header: cumulative)
    d->stats.literal_frames += io[b].literal_steps;
    d->stats.literal_nonfinite += io[b].why_nonfinite;
    d->stats.literal_fill += io[b].why_fill;
    d->stats.duplicate_frames += io[b].dup_frames;
    d->stats.records_written += io[b].records;
    d->stats.early_recursed_frames += ctcx::item_early_frames(io[b]);
  }
  if (!sizes) return CTCEXT_OK;
  for (int64_t b = 0; b < B; ++b)
    if (io[b].n_leaves < P) return fail(CTCEXT_INVALID_ARGUMENT, "Less leaves in the beam search than requested.");
  const int32_t* kinds = (const int32_t*)d->h_kind.p;
  for (int64_t q = 0; q < B * P; ++q) d->stats.no_label_paths += (kinds[q] < 0) ? 1 : 0;
  return CTCEXT_OK;
}

extern "C" int ctcext_stream_push(ctcext_stream* st, const ctcext_chunk* c, ctcext_path_sizes* sizes) {
  if (!st || !c) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (st->sk.on)
    return fail(CTCEXT_UNIMPLEMENTED, "a skipping stream has no synchronous push: use ctcext_stream_push_dense");
  if (st->sc.on)
    return fail(CTCEXT_UNIMPLEMENTED,
                "a stream with a score store has no synchronous push: use ctcext_stream_push_dense");
  ctcext_decoder* d = st->dec;
  const ctcext_stream_args& a = st->a;
  const int64_t B = a.batch_size;
  const int P = a.top_paths;
  if (c->flags & ~(CTCEXT_FLAG_TEST_HELPER_DEAD | CTCEXT_FLAG_PROFILE))
    return fail(CTCEXT_INVALID_ARGUMENT, "chunk flags: CTCEXT_FLAG_TEST_HELPER_DEAD and _PROFILE only");
  int rc = check_chunk(&a, c, nullptr);
  if (rc != CTCEXT_OK) return rc;
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  hipStream_t s = c->stream ? (hipStream_t)c->stream : root.own_stream;
  rc = stream_settle(st);
  if (rc != CTCEXT_OK) return rc;
  // the chunk's lengths are read on the host, as ctcext_decode reads sequence_length
  std::vector<int32_t> hcl((size_t)B, (int32_t)c->chunk_time);
  if (B > 0 && c->chunk_length) {
    if (a.on_device) {
      HIP_OR_FAIL(hipMemcpyAsync(hcl.data(), c->chunk_length, 4 * (size_t)B, hipMemcpyDeviceToHost, s));
      HIP_OR_FAIL(hipStreamSynchronize(s));
    } else {
      memcpy(hcl.data(), c->chunk_length, 4 * (size_t)B);
    }
  }
  rc = check_lengths(hcl.data(), B, c->chunk_time);
  if (rc != CTCEXT_OK) return rc;
  for (int64_t b = 0; b < B; ++b) {
    if (hcl[(size_t)b] < 0) hcl[(size_t)b] = 0;   // (the kernels read a negative length as 0)
    const int64_t tot = st->frames[(size_t)b] + hcl[(size_t)b];
    if (tot > a.max_frames)
      return fail(CTCEXT_INVALID_ARGUMENT, "stream capacity exceeded: item " + std::to_string(b) + " would hold " +
                                               std::to_string(tot) + " frames of max_frames " +
                                               std::to_string(a.max_frames));
  }
  d->have = false;
  d->dense.have = false;   // (the workspace ctcext_dense_check reads is this call's now)
  d->ss.have = false;      // (this push keeps neither its chunk nor its normaliser: nothing to score)
  if (B > 0) {
    rc = a.dtype == CTCEXT_F32 ? stream_push_t<float>(st, c, hcl, sizes, s) : stream_push_t<double>(st, c, hcl, sizes, s);
    if (rc != CTCEXT_OK) return rc;
  }
  if (!sizes) {
    g_err.clear();
    return CTCEXT_OK;
  }
  d->B = B;
  d->sizes.assign((size_t)P, ctcext_path_sizes{0, 0, 0, 0});
  if (B > 0) {
    const int64_t* r = (const int64_t*)d->h_res.p;
    for (int p = 0; p < P; ++p) {
      d->sizes[p].num_decoded = r[(p * 2 + 0) * 2];
      d->sizes[p].max_decoded = r[(p * 2 + 0) * 2 + 1];
      d->sizes[p].num_alignment = r[(p * 2 + 1) * 2];
      d->sizes[p].max_alignment = r[(p * 2 + 1) * 2 + 1];
    }
  }
  d->have = true;
  d->dtype = a.dtype;
  d->T = a.max_frames; d->C = a.num_classes; d->W = a.beam_width; d->P = P;
  d->tt.frames.assign((size_t)B, 0);
  for (int64_t b = 0; b < B; ++b) d->tt.frames[(size_t)b] = (int32_t)st->frames[(size_t)b];
  d->tt.C = a.num_classes; d->tt.blank_index = a.blank_index; d->tt.blank_label = a.blank_label;
  d->tt.merge = a.merge_repeated ? 1 : 0;
  root.s = s;
  for (int p = 0; p < P; ++p) sizes[p] = d->sizes[p];
  g_err.clear();
  return CTCEXT_OK;
}

// ---------------------------------------------------------------------------
// The stable prefix of a stream (ctcext.h, "Streaming: the stable prefix"):
// ctcx_stable.hip's kernel over the committed state headers, the records and
// the per-item frontier cache; and the naive host walk the tests hold it to.

// A skipping stream's answers are record (kept) frames r: on the original time
// axis that is the frame behind the r-th kept one, kmap[r - 1] + 1 (0 for 0).
static int stream_map_stable(ctcext_stream* st, int64_t* stable_frames, hipStream_t s) {
  if (!st->sk.on) return CTCEXT_OK;
  const int64_t B = st->a.batch_size, F = st->a.max_frames;
  std::vector<int32_t> last((size_t)B, -1);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t r = stable_frames[b];
    if (r <= 0) continue;
    if (r > F) return fail(CTCEXT_INTERNAL, "stable frames outside the stream's shape");
    HIP_OR_FAIL(hipMemcpyAsync(&last[(size_t)b], (const int32_t*)st->sk.kmap.p + b * F + (r - 1), 4,
                               hipMemcpyDeviceToHost, s));
  }
  HIP_OR_FAIL(hipStreamSynchronize(s));
  for (int64_t b = 0; b < B; ++b) stable_frames[b] = (int64_t)last[(size_t)b] + 1;
  return CTCEXT_OK;
}

extern "C" int ctcext_stream_stable(ctcext_stream* st, int32_t* decoded_length, int64_t* stable_frames,
                                    int64_t* walked) {
  if (!st || !decoded_length || !stable_frames) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  const ctcext_stream_args& a = st->a;
  const int64_t B = a.batch_size;
  if (B == 0) {
    g_err.clear();
    return CTCEXT_OK;
  }
  DeviceGuard guard;
  Dev& root = st->dec->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  hipStream_t s = root.own_stream;
  {
    const int rc = stream_settle(st);
    if (rc != CTCEXT_OK) return rc;
  }
  // outputs: stable_frames [B] int64 | walked [B] int64 | decoded_length [B] int32
  HIP_OR_FAIL(st->stable_out.ensure(20 * (size_t)B + 16));
  HIP_OR_FAIL(st->h_stable.ensure(20 * (size_t)B + 16));
  CtcxStableParams p{};
  p.state = (const char*)st->state[st->cur];
  p.stride = st->stride;
  p.rec = st->rec;
  p.Tmax = a.max_frames; p.B = B;
  p.W = a.beam_width; p.rec_fmt = st->rec_fmt; p.merge = a.merge_repeated ? 1 : 0;
  p.cache = (CtcxStableCache*)st->stable_cache;
  p.stable_frames = (int64_t*)st->stable_out.p;
  p.walked = p.stable_frames + B;
  p.decoded_length = (int32_t*)(p.walked + B);
  if (!ctcx_stable_in_lds(p.W, p.rec_fmt)) {
    HIP_OR_FAIL(st->stable_flags.ensure(2 * (size_t)B * (size_t)p.W + 16));
    p.flags = (uint8_t*)st->stable_flags.p;
  }
  HIP_OR_FAIL(ctcx_launch_stable(p, s));
  HIP_OR_FAIL(hipMemcpyAsync(st->h_stable.p, st->stable_out.p, 20 * (size_t)B, hipMemcpyDeviceToHost, s));
  HIP_OR_FAIL(hipStreamSynchronize(s));
  const int64_t* h = (const int64_t*)st->h_stable.p;
  memcpy(stable_frames, h, 8 * (size_t)B);
  if (walked) memcpy(walked, h + B, 8 * (size_t)B);
  memcpy(decoded_length, h + 2 * B, 4 * (size_t)B);
  {
    const int rc = stream_map_stable(st, stable_frames, s);
    if (rc != CTCEXT_OK) return rc;
  }
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_stream_stable_reference(ctcext_stream* st, int32_t* decoded_length, int64_t* stable_frames) {
  if (!st || !decoded_length || !stable_frames) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  const ctcext_stream_args& a = st->a;
  const int64_t B = a.batch_size, F = a.max_frames;
  const int W = a.beam_width;
  if (B == 0) {
    g_err.clear();
    return CTCEXT_OK;
  }
  DeviceGuard guard;
  Dev& root = st->dec->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  hipStream_t s = root.own_stream;
  {
    const int rc = stream_settle(st);
    if (rc != CTCEXT_OK) return rc;
  }
  const int fmt = st->rec_fmt;
  const size_t rw = (size_t)st->rec_bytes / 4;
  std::vector<uint32_t> rec;
  std::vector<int> pos;
  for (int64_t b = 0; b < B; ++b) {
    CtcxStreamHdr hdr;
    HIP_OR_FAIL(hipMemcpyAsync(&hdr, (const char*)st->state[st->cur] + (size_t)b * (size_t)st->stride, sizeof(hdr),
                               hipMemcpyDeviceToHost, s));
    HIP_OR_FAIL(hipStreamSynchronize(s));
    decoded_length[b] = 0;
    stable_frames[b] = 0;
    const int64_t n = hdr.frames, m = hdr.nb;
    if (n <= 0 || m <= 0) continue;
    if (n > F || m > W) return fail(CTCEXT_INTERNAL, "stream header outside the stream's shape");
    rec.resize((size_t)n * (size_t)W * rw);
    HIP_OR_FAIL(hipMemcpyAsync(rec.data(), (const char*)st->rec + (size_t)b * (size_t)F * (size_t)W * rw * 4,
                               rec.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OR_FAIL(hipStreamSynchronize(s));
    auto at = [&](int64_t t, int k, uint32_t& link, int& lab) {
      ctcx::rec_link_label(rec.data() + ((size_t)t * (size_t)W + (size_t)k) * rw, fmt, link, lab);
    };
    // every live chain to frame 0; the newest frame that holds them all on one position
    pos.resize((size_t)m);
    for (int64_t i = 0; i < m; ++i) pos[(size_t)i] = (int)i;
    int64_t f = -1;
    int ks = 0;
    for (int64_t t = n - 1; t >= 0; --t) {
      bool one = true;
      for (int64_t i = 1; i < m; ++i) one = one && pos[(size_t)i] == pos[0];
      if (one && f < 0) {
        f = t;
        ks = pos[0];
      }
      for (int64_t i = 0; i < m; ++i) {
        uint32_t link;
        int lab;
        at(t, pos[(size_t)i], link, lab);
        if ((link >> 1) >= (uint32_t)W) return fail(CTCEXT_INTERNAL, "record link outside the beam");
        pos[(size_t)i] = (int)(link >> 1);
      }
    }
    if (f < 0) continue;
    // the decoded walk from (f, ks) to frame 0
    int len = 0, prev = -1, k = ks;
    for (int64_t t = f; t >= 0; --t) {
      uint32_t link;
      int lab;
      at(t, k, link, lab);
      if (link & 1u) {
        if (!a.merge_repeated || lab != prev) ++len;
        prev = lab;
      }
      k = (int)(link >> 1);
    }
    decoded_length[b] = len;
    stable_frames[b] = f + 1;
  }
  {
    const int rc = stream_map_stable(st, stable_frames, s);
    if (rc != CTCEXT_OK) return rc;
  }
  g_err.clear();
  return CTCEXT_OK;
}

// ---------------------------------------------------------------------------
// Streaming: enqueue-only push (ctcext.h, "Streaming: enqueue-only push").
// ctcx_stream_dense.hip's prologue takes the decisions ctcext_stream_push takes
// on the host from the chunk's lengths; the decode reads state[cur] and writes
// state[cur ^ 1] as there; ctcx_stream_commit copies every item whose
// hand-over held back over state[cur], so cur never changes in this path and
// a push is the same chain of launches over the same addresses every time.

// A chunk against a score store's element format: a half store holds the bits it is given.
static int check_store_chunk(int32_t store_format, const ctcext_chunk* c) {
  if (store_format != CTCEXT_IN_NATIVE && c->inputs_format != store_format)
    return fail(CTCEXT_INVALID_ARGUMENT, "chunk inputs_format differs from the stream's score store format");
  return CTCEXT_OK;
}

// What needs no data, on the host: a is a validated stream's attributes.
static int check_push_dense(const ctcext_stream_args* a, const ctcext_chunk* c, const ctcext_stream_dense_outputs* o) {
  if (!a || !c) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!a->on_device) return fail(CTCEXT_INVALID_ARGUMENT, "ctcext_stream_push_dense needs device chunks");
  if (c->flags & ~(CTCEXT_FLAG_TEST_HELPER_DEAD | CTCEXT_FLAG_PROFILE | CTCEXT_FLAG_DENSE_NULL_STREAM))
    return fail(CTCEXT_INVALID_ARGUMENT,
                "chunk flags: CTCEXT_FLAG_TEST_HELPER_DEAD, _PROFILE and _DENSE_NULL_STREAM only");
  const int rc = check_chunk(a, c, nullptr);
  if (rc != CTCEXT_OK) return rc;
  if (o && a->batch_size > 0) {
    const void* hyp[] = {o->decoded, o->decoded_length, o->alignment, o->alignment_length, o->log_probability};
    int nh = 0;
    for (const void* q : hyp) nh += q ? 1 : 0;
    if (!o->status || (nh != 0 && nh != 5) || (!o->stable_length) != (!o->stable_frames))
      return fail(CTCEXT_INVALID_ARGUMENT, "null dense output pointer");
    if (nh == 5 && (((uintptr_t)o->decoded | (uintptr_t)o->alignment) & 7))
      return fail(CTCEXT_INVALID_ARGUMENT, "dense outputs decoded and alignment need 8-byte alignment");
  }
  return CTCEXT_OK;
}

extern "C" int ctcext_stream_dense_validate(const ctcext_stream_args* a, const ctcext_chunk* c,
                                            const ctcext_stream_dense_outputs* o) {
  int rc = ctcext_stream_validate(a);
  if (rc == CTCEXT_OK) rc = check_push_dense(a, c, o);
  if (rc == CTCEXT_OK) g_err.clear();
  return rc;
}

// Grows the stream's own workspace to what a push of Tc frames touches
// (grow-only: nothing is allocated or freed when it already fits).
static int stream_dense_ensure(ctcext_stream* st, int64_t Tc) {
  const ctcext_stream_args& a = st->a;
  const int64_t B = a.batch_size, C = a.num_classes, F = a.max_frames;
  const int W = a.beam_width, P = a.top_paths;
  const size_t ts = a.dtype == CTCEXT_F64 ? 8 : 4;
  auto& n = st->dn;
  HIP_OR_FAIL(n.item.ensure(sizeof(ctcx::ItemOut) * (size_t)B));
  HIP_OR_FAIL(n.top_pos.ensure(4 * (size_t)(B * P)));
  HIP_OR_FAIL(n.top_kind.ensure(4 * (size_t)(B * P)));
  HIP_OR_FAIL(n.logp.ensure(ts * (size_t)(B * P)));
  HIP_OR_FAIL(n.seq.ensure(4 * (size_t)(B * P * 2 * F) + 16));
  HIP_OR_FAIL(n.len.ensure(4 * (size_t)(B * P * 2)));
  HIP_OR_FAIL(n.sl.ensure(4 * (size_t)B));
  HIP_OR_FAIL(n.pre.ensure(4 * (size_t)B));
  HIP_OR_FAIL(n.fin.ensure(4 * (size_t)B));
  HIP_OR_FAIL(n.walked.ensure(8 * (size_t)B));
  HIP_OR_FAIL(n.land.ensure(land_kind_off(B) + 4 * (size_t)(B * P) + 16));
  if (!n.acc.p) {   // (sized by the batch alone: allocated once, and empty from then on until a push writes it)
    HIP_OR_FAIL(n.acc.ensure(sizeof(CtcxStreamAcc) * (size_t)B));
    HIP_OR_FAIL(hipMemset(n.acc.p, 0, sizeof(CtcxStreamAcc) * (size_t)B));
  }
  if (!ctcx_stable_in_lds(W, st->rec_fmt)) HIP_OR_FAIL(st->stable_flags.ensure(2 * (size_t)B * (size_t)W + 16));
  if (!n.ev[0])
    for (auto& ev : n.ev) HIP_OR_FAIL(hipEventCreate(&ev));
  if (Tc > 0) {
    HIP_OR_FAIL(st->norm.ensure(ts * (size_t)(Tc * B)));
    // (half chunks of a float stream on the global-state tier are widened into workspace first)
    if (st->gs && ts == 4) HIP_OR_FAIL(st->xw.ensure(4 * (size_t)(Tc * B * C) + 16));
    if (!st->gs && C > 64) HIP_OR_FAIL(st->prep.ensure(ctcx::prep_row_bytes(C, (int)ts) * (size_t)(Tc * B)));
  }
  if (st->sk.on) {
    HIP_OR_FAIL(st->sk.klen.ensure(4 * (size_t)B));
    HIP_OR_FAIL(st->sk.nfr.ensure(4 * (size_t)B));
    if (Tc > 0) {
      HIP_OR_FAIL(st->sk.norm.ensure(ts * (size_t)(Tc * B)));
      HIP_OR_FAIL(st->sk.ckmap.ensure(4 * (size_t)(Tc * B)));
      HIP_OR_FAIL(st->sk.xc.ensure(ts * (size_t)(Tc * B * C) + 16));   // (room for the widest element type)
    }
  }
  return CTCEXT_OK;
}

extern "C" int ctcext_stream_reserve(ctcext_stream* st, int64_t max_chunk_time) {
  if (!st) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!st->a.on_device) return fail(CTCEXT_INVALID_ARGUMENT, "ctcext_stream_push_dense needs device chunks");
  if (max_chunk_time < 0) return fail(CTCEXT_INVALID_ARGUMENT, "inputs has a negative dimension");
  if (st->a.batch_size == 0) {
    g_err.clear();
    return CTCEXT_OK;
  }
  DeviceGuard guard;
  HIP_OR_FAIL(hipSetDevice(st->dec->devs[0].device));
  const int rc = stream_dense_ensure(st, max_chunk_time);
  if (rc == CTCEXT_OK) g_err.clear();
  return rc;
}

template <typename T>
static int stream_push_dense_t(ctcext_stream* st, const ctcext_chunk* c, const int32_t* reset,
                               const ctcext_stream_dense_outputs* o, hipStream_t s) {
  const ctcext_stream_args& a = st->a;
  const int64_t B = a.batch_size, C = a.num_classes, F = a.max_frames, Tc = c->chunk_time;
  const int W = a.beam_width, P = a.top_paths;
  const int ts = (int)sizeof(T);
  const bool prof = (c->flags & CTCEXT_FLAG_PROFILE) != 0;
  const bool results = o && o->decoded;
  auto& n = st->dn;
  int* note = ctcx_launch_note();
  note[0] = note[1] = note[2] = 0;

  // the chunk's element strides, as stream_push_t takes them
  int xfmt = c->inputs_format;
  int64_t st_t = c->inputs_stride_t ? c->inputs_stride_t : B * C;
  int64_t st_b = c->inputs_stride_b ? c->inputs_stride_b : C;
  if (Tc <= 1 && B <= 1) st_t = st_b = C;
  else if (Tc <= 1) st_t = st_b * B;
  else if (B <= 1) st_b = st_t * Tc;
  const void* x = c->inputs;
  const void* const x_in = x;   // the caller's rows as given: what a score store appends
  const int xfmt_in = xfmt;
  const int64_t st_t_in = st_t, st_b_in = st_b;
  const int32_t* sl = (const int32_t*)n.sl.p;
  auto& k = st->sk;
  char* const committed = (char*)st->state[st->cur];
  char* const other = (char*)st->state[st->cur ^ 1];

  if (prof) HIP_OR_FAIL(hipEventRecord(n.ev[0], s));
  CtcxStreamPrologueParams pp{};
  pp.chunk_length = c->chunk_length;
  pp.reset = reset;
  pp.state = committed;
  pp.stride = st->stride;
  pp.cache = (CtcxStableCache*)st->stable_cache;
  pp.sl = (int32_t*)n.sl.p;
  pp.cum = (int32_t*)st->cum;
  pp.pre = (int32_t*)n.pre.p;
  pp.acc = (CtcxStreamAcc*)n.acc.p;
  pp.chunk_time = Tc; pp.max_frames = F; pp.B = B;
  pp.skip = k.on ? (CtcxSkipItem*)k.item.p : nullptr;
  HIP_OR_FAIL(ctcx_launch_stream_prologue(pp, s));
  if (k.on) {
    // the normaliser of the caller's rows, the chunk's plan on top of what the
    // items carry, and the kept rows, dense: the rest of the push decodes those
    if (Tc > 0) HIP_OR_FAIL(ctcx::launch_row_norm<T>(x, xfmt, sl, (T*)k.norm.p, Tc, B, C, st_t, st_b, s));
    CtcxSkipChunkParams kp{};
    kp.x = x;
    kp.norm = k.norm.p;
    kp.len = sl;
    kp.state = committed;
    kp.stride = st->stride;
    kp.item = (CtcxSkipItem*)k.item.p;
    kp.chunk_time = Tc; kp.max_frames = F; kp.B = B; kp.xst_t = st_t; kp.xst_b = st_b;
    kp.xfmt = xfmt; kp.f64 = ts == 8; kp.blank = a.blank_index;
    kp.thr = k.thr;
    kp.kmap = (int32_t*)k.kmap.p;
    kp.cidx = (int32_t*)k.cidx.p;
    kp.ckmap = (int32_t*)k.ckmap.p;
    kp.klen = (int32_t*)k.klen.p;
    kp.cum = pp.cum;
    HIP_OR_FAIL(ctcx_launch_skip_chunk(kp, s));
    if (Tc > 0) {
      CtcxSkipGatherParams gp{};
      gp.x = x;
      gp.xc = k.xc.p;
      gp.kmap = kp.ckmap;
      gp.kept = kp.klen;
      gp.Tmax = Tc; gp.B = B; gp.C = C; gp.xst_t = st_t; gp.xst_b = st_b;
      gp.esize = xfmt == CTCEXT_IN_NATIVE ? ts : 2;
      HIP_OR_FAIL(ctcx_launch_skip_gather(gp, s));
      x = k.xc.p;
      st_t = B * C;
      st_b = C;
    }
    sl = kp.klen;
  }
  if (Tc > 0) {   // the pre-pass over the chunk's rows, on the sanitised lengths
    if (st->gs && xfmt != CTCEXT_IN_NATIVE) {
      HIP_OR_FAIL(ctcx::launch_widen_rows(x, xfmt, (float*)st->xw.p, Tc, B, C, st_t, st_b, s));
      x = st->xw.p;
      xfmt = CTCEXT_IN_NATIVE;
      st_t = B * C;
      st_b = C;
    }
    if (!st->gs && C > 64)
      HIP_OR_FAIL(ctcx::launch_row_prep<T>(x, xfmt, sl, (char*)st->prep.p, (T*)st->norm.p, Tc, B, C, st_t, st_b,
                                           a.blank_index, s));
    else
      HIP_OR_FAIL(ctcx::launch_row_norm<T>(x, xfmt, sl, (T*)st->norm.p, Tc, B, C, st_t, st_b, s));
  }
  st->sc.append_timed = st->sc.scores_timed = false;
  if (st->sc.on && Tc > 0) {
    // the rows this push takes and their normaliser, behind what each item holds.  The base is committed
    // state (the header's frames; a skipping stream's n) and the commit comes later: an item that does not
    // commit keeps its base, and its next push writes these rows again
    CtcxStreamStoreParams ap{};
    ap.x = x_in;
    ap.norm = k.on ? k.norm.p : st->norm.p;   // (of the caller's rows in both)
    ap.len = (const int32_t*)n.sl.p;
    // (the kernel reads base as the first 32-bit word of the item's record: a reordering of either struct
    //  would break the roll-back without a word)
    static_assert(offsetof(CtcxSkipItem, n) == 0 && sizeof(CtcxSkipItem::n) == 4 && sizeof(CtcxSkipItem) % 4 == 0,
                  "the append reads CtcxSkipItem.n as the item's first word");
    static_assert(offsetof(CtcxStreamHdr, frames) == 0 && sizeof(CtcxStreamHdr::frames) == 4,
                  "the append reads CtcxStreamHdr.frames as the item's first word");
    if (k.on) {
      ap.base = (const int32_t*)k.item.p;   // CtcxSkipItem.n
      ap.base_stride = (int64_t)(sizeof(CtcxSkipItem) / 4);
    } else {
      ap.base = (const int32_t*)committed;  // CtcxStreamHdr.frames
      ap.base_stride = st->stride / 4;
    }
    ap.sx = st->sc.sx;
    ap.snorm = st->sc.snorm;
    ap.chunk_time = Tc; ap.max_frames = F; ap.B = B; ap.C = C; ap.xst_t = st_t_in; ap.xst_b = st_b_in;
    ap.xfmt = xfmt_in; ap.sfmt = st->sc.fmt; ap.f64 = ts == 8;
    if (prof) HIP_OR_FAIL(hipEventRecord(st->sc.ev[0], s));
    HIP_OR_FAIL(ctcx_launch_stream_store(ap, s));
    if (prof) {
      HIP_OR_FAIL(hipEventRecord(st->sc.ev[1], s));
      st->sc.append_timed = true;
    }
  }
  if (prof) HIP_OR_FAIL(hipEventRecord(n.ev[1], s));

  ctcx::DecodeParams<T> p = stream_decode_params<T>(st);
  p.x = (const T*)x;
  p.xfmt = xfmt;
  p.norm = (const T*)st->norm.p;
  p.seq_len = sl;
  p.xst_t = st_t; p.xst_b = st_b;
  p.item = (ctcx::ItemOut*)n.item.p;
  p.top_pos = (int32_t*)n.top_pos.p;
  p.top_kind = (int32_t*)n.top_kind.p;
  p.log_prob = (T*)n.logp.p;
  p.prep = (const char*)st->prep.p;
  p.test_flags = (c->flags & CTCEXT_FLAG_TEST_HELPER_DEAD) ? ctcx::kTestHelperDead : 0;
  p.test_flags |= early_recurse_flag_from_env();
  CtcxStreamParams sp{};
  sp.in = committed;
  sp.out = other;
  sp.stride = st->stride;
  sp.image_bytes = st->image_bytes;
  if (st->gs) HIP_OR_FAIL(ctcx_gstate_stream_launch_decode(&p, &sp, ts == 8, st->scored, s));
  else HIP_OR_FAIL(ctcx_stream_launch_decode(&p, &sp, ts == 8, s));
  if (prof) HIP_OR_FAIL(hipEventRecord(n.ev[2], s));

  CtcxStreamCommitParams cp{};
  cp.committed = committed;
  cp.written = other;
  cp.stride = st->stride;
  cp.copy_bytes = (int64_t)((ctcx_stream_hdr_bytes(P) + (size_t)st->image_bytes + 15) & ~(size_t)15);
  cp.item = p.item; cp.top_pos = p.top_pos; cp.top_kind = p.top_kind; cp.log_prob = n.logp.p;
  cp.pre = pp.pre; cp.cum = pp.cum; cp.acc = pp.acc;
  cp.status_ws = (int32_t*)n.fin.p;
  cp.status = o ? o->status : nullptr;
  cp.frames = (o && !k.on) ? o->frames : nullptr;   // (a skipping stream's are written by its finish kernel)
  cp.B = B; cp.P = P; cp.f64 = ts == 8;
  cp.few_leaves = results ? 1 : 0;
  HIP_OR_FAIL(ctcx_launch_stream_commit(cp, s));
  if (prof) HIP_OR_FAIL(hipEventRecord(n.ev[3], s));

  if (o && o->stable_length) {   // ctcext_stream_stable's launch, over the state just committed, into the caller's buffers
    CtcxStableParams q{};
    q.state = committed;
    q.stride = st->stride;
    q.rec = st->rec;
    q.Tmax = F; q.B = B;
    q.W = W; q.rec_fmt = st->rec_fmt; q.merge = a.merge_repeated ? 1 : 0;
    q.cache = (CtcxStableCache*)st->stable_cache;
    q.stable_frames = o->stable_frames;
    q.walked = (int64_t*)n.walked.p;
    q.decoded_length = o->stable_length;
    if (!ctcx_stable_in_lds(W, q.rec_fmt)) q.flags = (uint8_t*)st->stable_flags.p;
    HIP_OR_FAIL(ctcx_launch_stable(q, s));
  }
  if (k.on) {   // n and the carried flag follow the commit; the outputs that count frames go to the original axis
    CtcxSkipFinishParams fp{};
    fp.item = (CtcxSkipItem*)k.item.p;
    fp.status = (const int32_t*)n.fin.p;
    fp.dead_mask = ctcx::kItemHelperTimeout;
    fp.cum = pp.cum;
    fp.kmap = (const int32_t*)k.kmap.p;
    fp.max_frames = F; fp.B = B;
    fp.n_ws = (int32_t*)k.nfr.p;
    fp.frames = o ? o->frames : nullptr;
    fp.kept = k.kept_out;
    fp.stable_frames = o ? o->stable_frames : nullptr;
    HIP_OR_FAIL(ctcx_launch_skip_finish(fp, s));
  }
  if (results) {
    // the walks of every frame so far, from the records the stream keeps, then ctcx_pack_dense with rows of max_frames
    ctcx::TraceParams tp{};
    tp.rec = p.rec; tp.item = p.item; tp.seq_len = (const int32_t*)st->cum; tp.top_pos = p.top_pos;
    tp.top_kind = p.top_kind;
    tp.Tmax = F; tp.B = B; tp.W = W; tp.P = P; tp.merge = a.merge_repeated ? 1 : 0;
    tp.blank_label = a.blank_label;
    tp.rec_fmt = st->rec_fmt;
    tp.foff = nullptr;
    tp.seq = (int32_t*)n.seq.p;
    tp.len = (int32_t*)n.len.p;
    tp.len_stride = B;
    HIP_OR_FAIL(ctcx::launch_traceback(tp, s));
    if (k.on) {   // the alignment walks of the kept frames, back on the original time axis
      CtcxSkipExpandParams ep{};
      ep.seq = tp.seq;
      ep.len = tp.len;
      ep.frames = (const int32_t*)k.nfr.p;
      ep.kmap = (const int32_t*)k.kmap.p;
      ep.cidx = (const int32_t*)k.cidx.p;
      ep.kept = (const int32_t*)st->cum;
      ep.Tmax = F; ep.B = B; ep.P = P; ep.blank_label = a.blank_label;
      HIP_OR_FAIL(ctcx_launch_skip_expand(ep, s));
    }
    ctcx::PackDenseParams pd{};
    pd.seq = tp.seq;
    pd.len = tp.len;
    pd.item = p.item;
    pd.pre = pp.pre;
    pd.log_prob = n.logp.p;
    pd.Tmax = F; pd.B = B; pd.P = P; pd.f64 = ts == 8;
    pd.pad_value = o->pad_value;
    pd.decoded = o->decoded; pd.alignment = o->alignment;
    pd.decoded_length = o->decoded_length; pd.alignment_length = o->alignment_length;
    pd.out_log_prob = o->log_probability;
    pd.status = o->status;
    pd.status_ws = (int32_t*)n.fin.p;
    HIP_OR_FAIL(ctcx::launch_pack_dense(pd, s));
  }
  if (prof) HIP_OR_FAIL(hipEventRecord(n.ev[4], s));
  n.kernel = note[0] | (note[1] << 12) | (note[2] << 16);
  n.results = results;
  n.times_timed = false;
  return CTCEXT_OK;
}

extern "C" int ctcext_stream_push_dense(ctcext_stream* st, const ctcext_chunk* c, const int32_t* reset,
                                        const ctcext_stream_dense_outputs* o) {
  if (!st || !c) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  const ctcext_stream_args& a = st->a;
  int rc = check_push_dense(&a, c, o);
  if (rc == CTCEXT_OK && st->sc.on) rc = check_store_chunk(st->sc.fmt, c);
  if (rc != CTCEXT_OK) return rc;
  if (a.batch_size == 0) {
    g_err.clear();
    return CTCEXT_OK;
  }
  DeviceGuard guard;
  Dev& root = st->dec->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  // (the null stream itself with the flag: dense_begin)
  hipStream_t s = c->stream ? (hipStream_t)c->stream
                  : (c->flags & CTCEXT_FLAG_DENSE_NULL_STREAM) ? (hipStream_t) nullptr : root.own_stream;
  rc = stream_dense_ensure(st, c->chunk_time);   // (nothing to grow after a reserve or a push of this size)
  if (rc != CTCEXT_OK) return rc;
  rc = a.dtype == CTCEXT_F32 ? stream_push_dense_t<float>(st, c, reset, o, s)
                             : stream_push_dense_t<double>(st, c, reset, o, s);
  // (whatever was enqueued before a failing launch is waited for like a whole push)
  st->dn.used = true;
  st->dn.s = s;
  st->dn.flags = c->flags;
  if (rc == CTCEXT_OK) g_err.clear();
  return rc;
}

extern "C" int ctcext_stream_check(ctcext_stream* st) {
  if (!st) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  auto& n = st->dn;
  const ctcext_stream_args& a = st->a;
  const int64_t B = a.batch_size;
  const int P = a.top_paths;
  if (!n.used || B == 0) {
    g_err.clear();
    return CTCEXT_OK;
  }
  DeviceGuard guard;
  HIP_OR_FAIL(hipSetDevice(st->dec->devs[0].device));
  int rc = stream_settle(st);
  if (rc != CTCEXT_OK) return rc;
  const char* h = (const char*)n.land.p;
  const CtcxStreamAcc* acc = (const CtcxStreamAcc*)(h + land_acc_off(B));
  const ctcx::ItemOut* io = (const ctcx::ItemOut*)(h + land_item_off(B));
  const int32_t* kinds = (const int32_t*)(h + land_kind_off(B));

  ctcext_stats sv{};
  sv.tier = st->gs ? 1 : 0;
  sv.record_bytes = st->rec_bytes;
  sv.helper = st->helper;
  sv.kernel = n.kernel;
  n.commit_ms = 0;
  if (n.flags & CTCEXT_FLAG_PROFILE) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, n.ev[0], n.ev[1]) == hipSuccess) sv.norm_kernel_ms = ms;
    if (hipEventElapsedTime(&ms, n.ev[1], n.ev[2]) == hipSuccess) sv.decode_kernel_ms = ms;
    if (hipEventElapsedTime(&ms, n.ev[2], n.ev[3]) == hipSuccess) n.commit_ms = ms;
    if (hipEventElapsedTime(&ms, n.ev[3], n.ev[4]) == hipSuccess) sv.traceback_ms = ms;
    (void)hipGetLastError();
  }
  int32_t any = 0;
  int64_t first_len = -1, first_cap = -1;
  for (int64_t b = 0; b < B; ++b) {   // (the counters travel in the item's header: cumulative)
    sv.literal_frames += io[b].literal_steps;
    sv.literal_nonfinite += io[b].why_nonfinite;
    sv.literal_fill += io[b].why_fill;
    sv.duplicate_frames += io[b].dup_frames;
    sv.records_written += io[b].records;
    sv.early_recursed_frames += ctcx::item_early_frames(io[b]);
    any |= acc[b].status;
    if ((acc[b].status & CTCEXT_ITEM_LENGTH) && first_len < 0) first_len = b;
    if ((acc[b].status & CTCEXT_ITEM_CAPACITY) && first_cap < 0) first_cap = b;
  }
  st->dec->stats = sv;
  if (!any) {
    if (n.results)
      for (int64_t q = 0; q < B * P; ++q) st->dec->stats.no_label_paths += (kinds[q] < 0) ? 1 : 0;
    g_err.clear();
    return CTCEXT_OK;
  }
  // the messages are built before the record is cleared (its landing copy stays)
  const int64_t len_chunk = first_len >= 0 ? acc[first_len].len_chunk : 0;
  const int32_t cap_total = first_cap >= 0 ? acc[first_cap].cap_total : 0;
  HIP_OR_FAIL(hipMemsetAsync(n.acc.p, 0, sizeof(CtcxStreamAcc) * (size_t)B, n.s));
  HIP_OR_FAIL(hipStreamSynchronize(n.s));
  // the synchronous push's own order: the lengths, the capacity, the hand-over, the leaves
  if (first_len >= 0)
    return fail(CTCEXT_FAILED_PRECONDITION,
                "sequence_length(" + std::to_string(first_len) + ") <= " + std::to_string(len_chunk));
  if (first_cap >= 0)
    return fail(CTCEXT_INVALID_ARGUMENT, "stream capacity exceeded: item " + std::to_string(first_cap) +
                                             " would hold " + std::to_string(cap_total) + " frames of max_frames " +
                                             std::to_string(a.max_frames));
  if (any & CTCEXT_ITEM_HELPER_TIMEOUT)
    return fail(CTCEXT_INTERNAL, "decode kernel: a helper-wave hand-over wait timed out");
  return fail(CTCEXT_INVALID_ARGUMENT, "Less leaves in the beam search than requested.");
}

extern "C" int ctcext_stream_commit_ms(ctcext_stream* st, double* ms) {
  if (!st || !ms) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!st->dn.used || !(st->dn.flags & CTCEXT_FLAG_PROFILE))
    return fail(CTCEXT_FAILED_PRECONDITION, "no CTCEXT_FLAG_PROFILE enqueue-only push checked yet");
  *ms = st->dn.commit_ms;
  return CTCEXT_OK;
}

// ---------------------------------------------------------------------------
// Token times (ctcext.h, "Token times"): ctcx_times.hip's kernel over the walks
// the traceback left in the workspace -- the decoder's after a dense or a
// synchronous call, the stream's own after an enqueue-only push.

extern "C" int32_t ctcext_token_times_tile(void) { return kTimesTile; }

extern "C" int ctcext_token_times_validate(int64_t num_classes, int32_t blank_index, int32_t blank_label) {
  if (blank_label >= 0 && blank_label < num_classes && blank_label != blank_index)
    return fail(CTCEXT_INVALID_ARGUMENT, "token times need a blank_label that is no class label");
  g_err.clear();
  return CTCEXT_OK;
}

static int check_times_out(const ctcext_token_times* o) {
  if (!o) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if ((o->start == nullptr) != (o->end == nullptr))
    return fail(CTCEXT_INVALID_ARGUMENT, "token times: start and end come both or neither");
  if (!o->start && !o->trailing_blank) return fail(CTCEXT_INVALID_ARGUMENT, "token times: no output asked for");
  return CTCEXT_OK;
}

extern "C" int ctcext_dense_token_times(ctcext_decoder* d, const ctcext_token_times* o) {
  if (!d) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  int rc = check_times_out(o);
  if (rc != CTCEXT_OK) return rc;
  if (!d->dense.have)
    return fail(CTCEXT_FAILED_PRECONDITION, "ctcext_dense_token_times without a ctcext_decode_dense");
  rc = ctcext_token_times_validate(d->dense.C, d->dense.blank_index, d->dense.blank_label);
  if (rc != CTCEXT_OK) return rc;
  if (d->dense.B == 0) return CTCEXT_OK;
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  hipStream_t s = d->dense.s;
  const int64_t B = d->dense.B;
  CtcxTimesParams p{};
  p.seq = (const int32_t*)root.seq.p;
  p.len = (const int32_t*)root.len.p;
  p.frames = (const int32_t*)root.dsl.p;
  p.status = (const int32_t*)root.dstat.p + B;
  p.Tmax = d->dense.T; p.B = B; p.P = d->dense.P;
  p.merge = d->dense.merge; p.blank_label = d->dense.blank_label;
  p.start = o->start; p.end = o->end; p.trailing_blank = o->trailing_blank;
  const bool prof = (d->dense.flags & CTCEXT_FLAG_PROFILE) != 0;
  if (prof) HIP_OR_FAIL(hipEventRecord(root.ev[5], s));
  HIP_OR_FAIL(ctcx_launch_token_times(p, s));
  if (prof) {
    HIP_OR_FAIL(hipEventRecord(root.ev[6], s));
    d->dense.times_timed = true;
  }
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_stream_token_times(ctcext_stream* st, const ctcext_token_times* o) {
  if (!st) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  int rc = check_times_out(o);
  if (rc != CTCEXT_OK) return rc;
  auto& n = st->dn;
  const ctcext_stream_args& a = st->a;
  if (a.batch_size > 0 && (!n.used || !n.results))
    return fail(CTCEXT_FAILED_PRECONDITION,
                "ctcext_stream_token_times without a ctcext_stream_push_dense that had hypothesis outputs");
  rc = ctcext_token_times_validate(a.num_classes, a.blank_index, a.blank_label);
  if (rc != CTCEXT_OK) return rc;
  if (a.batch_size == 0) return CTCEXT_OK;
  DeviceGuard guard;
  HIP_OR_FAIL(hipSetDevice(st->dec->devs[0].device));
  hipStream_t s = n.s;
  CtcxTimesParams p{};
  p.seq = (const int32_t*)n.seq.p;
  p.len = (const int32_t*)n.len.p;
  p.frames = st->sk.on ? (const int32_t*)st->sk.nfr.p : (const int32_t*)st->cum;
  p.status = (const int32_t*)n.fin.p;
  p.Tmax = a.max_frames; p.B = a.batch_size; p.P = a.top_paths;
  p.merge = a.merge_repeated ? 1 : 0; p.blank_label = a.blank_label;
  p.start = o->start; p.end = o->end; p.trailing_blank = o->trailing_blank;
  const bool prof = (n.flags & CTCEXT_FLAG_PROFILE) != 0;
  if (prof) HIP_OR_FAIL(hipEventRecord(n.ev[5], s));
  HIP_OR_FAIL(ctcx_launch_token_times(p, s));
  if (prof) {
    HIP_OR_FAIL(hipEventRecord(n.ev[6], s));
    n.times_timed = true;
  }
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_fetch_token_times(ctcext_decoder* d, const ctcext_token_times* o, int32_t outputs_on_device) {
  if (!d) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  int rc = check_times_out(o);
  if (rc != CTCEXT_OK) return rc;
  if (!d->have)
    return fail(CTCEXT_FAILED_PRECONDITION, "ctcext_fetch_token_times without a successful ctcext_decode");
  if (d->devs.size() != 1) return fail(CTCEXT_UNIMPLEMENTED, "token times need a one-device decoder handle");
  rc = ctcext_token_times_validate(d->tt.C, d->tt.blank_index, d->tt.blank_label);
  if (rc != CTCEXT_OK) return rc;
  const int64_t B = d->B, T_ = d->T;
  const int P = d->P;
  if (B == 0 || (int64_t)d->tt.frames.size() != B) {
    if (B != 0) return fail(CTCEXT_INTERNAL, "token times: the frame counts of the last call are missing");
    return CTCEXT_OK;
  }
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  hipStream_t s = root.s;
  const size_t rows = (size_t)(B * P), cells = rows * (size_t)T_;
  HIP_OR_FAIL(d->tt_frames.ensure(4 * (size_t)B));
  HIP_OR_FAIL(hipMemcpyAsync(d->tt_frames.p, d->tt.frames.data(), 4 * (size_t)B, hipMemcpyHostToDevice, s));
  CtcxTimesParams p{};
  p.seq = (const int32_t*)root.seq.p;
  p.len = (const int32_t*)root.len.p;
  p.frames = (const int32_t*)d->tt_frames.p;
  p.status = nullptr;   // (a synchronous call with a failing item has failed as a whole)
  p.Tmax = T_; p.B = B; p.P = P;
  p.merge = d->tt.merge; p.blank_label = d->tt.blank_label;
  if (outputs_on_device) {
    p.start = o->start; p.end = o->end; p.trailing_blank = o->trailing_blank;
  } else {
    if (o->start) {
      HIP_OR_FAIL(d->tt_start.ensure(4 * cells + 16));
      HIP_OR_FAIL(d->tt_end.ensure(4 * cells + 16));
      p.start = (int32_t*)d->tt_start.p;
      p.end = (int32_t*)d->tt_end.p;
    }
    if (o->trailing_blank) {
      HIP_OR_FAIL(d->tt_trail.ensure(4 * rows + 16));
      p.trailing_blank = (int32_t*)d->tt_trail.p;
    }
  }
  HIP_OR_FAIL(ctcx_launch_token_times(p, s));
  if (!outputs_on_device) {
    if (o->start && cells) {
      HIP_OR_FAIL(hipMemcpyAsync(o->start, p.start, 4 * cells, hipMemcpyDeviceToHost, s));
      HIP_OR_FAIL(hipMemcpyAsync(o->end, p.end, 4 * cells, hipMemcpyDeviceToHost, s));
    }
    if (o->trailing_blank) HIP_OR_FAIL(hipMemcpyAsync(o->trailing_blank, p.trailing_blank, 4 * rows, hipMemcpyDeviceToHost, s));
  }
  HIP_OR_FAIL(hipStreamSynchronize(s));
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_dense_token_times_ms(ctcext_decoder* d, double* ms) {
  if (!d || !ms) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!d->dense.have || !d->dense.times_timed)
    return fail(CTCEXT_FAILED_PRECONDITION, "no token times of a CTCEXT_FLAG_PROFILE dense decode");
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  HIP_OR_FAIL(hipEventSynchronize(root.ev[6]));
  float f = 0;
  HIP_OR_FAIL(hipEventElapsedTime(&f, root.ev[5], root.ev[6]));
  *ms = f;
  return CTCEXT_OK;
}

extern "C" int ctcext_stream_token_times_ms(ctcext_stream* st, double* ms) {
  if (!st || !ms) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!st->dn.used || !st->dn.times_timed)
    return fail(CTCEXT_FAILED_PRECONDITION, "no token times of a CTCEXT_FLAG_PROFILE enqueue-only push");
  DeviceGuard guard;
  HIP_OR_FAIL(hipSetDevice(st->dec->devs[0].device));
  HIP_OR_FAIL(hipEventSynchronize(st->dn.ev[6]));
  float f = 0;
  HIP_OR_FAIL(hipEventElapsedTime(&f, st->dn.ev[5], st->dn.ev[6]));
  *ms = f;
  return CTCEXT_OK;
}

// ---------------------------------------------------------------------------
// Token scores (ctcext.h, "Token scores"): ctcx_scores.hip's kernel over the
// walks the traceback left in the workspace, the spans of the token times, the
// normaliser and the logits the decode read (ScoreSrc): the decoder's after a
// dense or a synchronous call; a stream's over its own walks and its score
// store (further down).

extern "C" int32_t ctcext_token_scores_tile(void) { return kScoresTile; }

static int check_scores_out(const ctcext_token_scores* o) {
  if (!o) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!o->logp_sum && !o->logp_min) return fail(CTCEXT_INVALID_ARGUMENT, "token scores: no output asked for");
  return CTCEXT_OK;
}

// What both entry points share of the kernel's parameters.
static void scores_params(CtcxScoresParams& p, const Dev& root, const ScoreSrc& q, int64_t T_, int64_t B, int64_t C,
                          int P, int32_t blank_index, int32_t blank_label) {
  p.seq = (const int32_t*)root.seq.p;
  p.len = (const int32_t*)root.len.p;
  p.x = q.x;
  p.norm = q.norm;
  p.Tmax = T_; p.B = B; p.C = C; p.xst_t = q.st_t; p.xst_b = q.st_b;
  p.P = P; p.xfmt = q.xfmt; p.f64 = q.f64 ? 1 : 0;
  p.blank_index = blank_index; p.blank_label = blank_label;
}

extern "C" int ctcext_dense_token_scores(ctcext_decoder* d, const ctcext_token_times* t,
                                         const ctcext_token_scores* o) {
  if (!d) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  int rc = check_scores_out(o);
  if (rc != CTCEXT_OK) return rc;
  if (!t || !t->start || !t->end)
    return fail(CTCEXT_INVALID_ARGUMENT, "token scores need the start and end of ctcext_dense_token_times");
  if (!d->dense.have)
    return fail(CTCEXT_FAILED_PRECONDITION, "ctcext_dense_token_scores without a ctcext_decode_dense");
  rc = ctcext_token_times_validate(d->dense.C, d->dense.blank_index, d->dense.blank_label);
  if (rc != CTCEXT_OK) return rc;
  if (d->dense.B == 0) return CTCEXT_OK;
  if (!d->dense.sc.have) return fail(CTCEXT_INTERNAL, "token scores: the inputs of the last call are missing");
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  hipStream_t s = d->dense.s;
  const int64_t B = d->dense.B;
  CtcxScoresParams p{};
  scores_params(p, root, d->dense.sc, d->dense.T, B, d->dense.C, d->dense.P, d->dense.blank_index,
                d->dense.blank_label);
  p.frames = (const int32_t*)root.dsl.p;
  p.status = (const int32_t*)root.dstat.p + B;
  p.start = t->start; p.end = t->end;
  p.logp_sum = o->logp_sum; p.logp_min = o->logp_min;
  const bool prof = (d->dense.flags & CTCEXT_FLAG_PROFILE) != 0;
  if (prof) HIP_OR_FAIL(hipEventRecord(root.ev[7], s));
  HIP_OR_FAIL(ctcx_launch_token_scores(p, s));
  if (prof) {
    HIP_OR_FAIL(hipEventRecord(root.ev[8], s));
    d->dense.scores_timed = true;
  }
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_fetch_token_scores(ctcext_decoder* d, const ctcext_token_scores* o, int32_t outputs_on_device) {
  if (!d) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  int rc = check_scores_out(o);
  if (rc != CTCEXT_OK) return rc;
  if (!d->have)
    return fail(CTCEXT_FAILED_PRECONDITION, "ctcext_fetch_token_scores without a successful ctcext_decode");
  if (d->devs.size() != 1) return fail(CTCEXT_UNIMPLEMENTED, "token scores need a one-device decoder handle");
  rc = ctcext_token_times_validate(d->tt.C, d->tt.blank_index, d->tt.blank_label);
  if (rc != CTCEXT_OK) return rc;
  const int64_t B = d->B, T_ = d->T;
  const int P = d->P;
  if (B == 0) return CTCEXT_OK;
  if (!d->ss.have)
    return fail(CTCEXT_FAILED_PRECONDITION,
                "ctcext_fetch_token_scores after a stream's push: a stream keeps no logits to score");
  if ((int64_t)d->tt.frames.size() != B)
    return fail(CTCEXT_INTERNAL, "token scores: the frame counts of the last call are missing");
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  hipStream_t s = root.s;
  const size_t cells = (size_t)(B * P) * (size_t)T_;
  const size_t ts = d->ss.f64 ? 8 : 4;
  // the times into workspace, as ctcext_fetch_token_times computes them
  HIP_OR_FAIL(d->tt_frames.ensure(4 * (size_t)B));
  HIP_OR_FAIL(d->tt_start.ensure(4 * cells + 16));
  HIP_OR_FAIL(d->tt_end.ensure(4 * cells + 16));
  HIP_OR_FAIL(hipMemcpyAsync(d->tt_frames.p, d->tt.frames.data(), 4 * (size_t)B, hipMemcpyHostToDevice, s));
  CtcxTimesParams tp{};
  tp.seq = (const int32_t*)root.seq.p;
  tp.len = (const int32_t*)root.len.p;
  tp.frames = (const int32_t*)d->tt_frames.p;
  tp.status = nullptr;   // (a synchronous call with a failing item has failed as a whole)
  tp.Tmax = T_; tp.B = B; tp.P = P;
  tp.merge = d->tt.merge; tp.blank_label = d->tt.blank_label;
  tp.start = (int32_t*)d->tt_start.p;
  tp.end = (int32_t*)d->tt_end.p;
  HIP_OR_FAIL(ctcx_launch_token_times(tp, s));
  CtcxScoresParams p{};
  scores_params(p, root, d->ss, T_, B, d->tt.C, P, d->tt.blank_index, d->tt.blank_label);
  p.frames = tp.frames;
  p.status = nullptr;
  p.start = tp.start; p.end = tp.end;
  if (outputs_on_device) {
    p.logp_sum = o->logp_sum; p.logp_min = o->logp_min;
  } else {
    if (o->logp_sum) {
      HIP_OR_FAIL(d->sc_sum.ensure(ts * cells + 16));
      p.logp_sum = d->sc_sum.p;
    }
    if (o->logp_min) {
      HIP_OR_FAIL(d->sc_min.ensure(ts * cells + 16));
      p.logp_min = d->sc_min.p;
    }
  }
  HIP_OR_FAIL(ctcx_launch_token_scores(p, s));
  if (!outputs_on_device && cells) {
    if (o->logp_sum) HIP_OR_FAIL(hipMemcpyAsync(o->logp_sum, p.logp_sum, ts * cells, hipMemcpyDeviceToHost, s));
    if (o->logp_min) HIP_OR_FAIL(hipMemcpyAsync(o->logp_min, p.logp_min, ts * cells, hipMemcpyDeviceToHost, s));
  }
  HIP_OR_FAIL(hipStreamSynchronize(s));
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_dense_token_scores_ms(ctcext_decoder* d, double* ms) {
  if (!d || !ms) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!d->dense.have || !d->dense.scores_timed)
    return fail(CTCEXT_FAILED_PRECONDITION, "no token scores of a CTCEXT_FLAG_PROFILE dense decode");
  DeviceGuard guard;
  Dev& root = d->devs[0];
  HIP_OR_FAIL(hipSetDevice(root.device));
  HIP_OR_FAIL(hipEventSynchronize(root.ev[8]));
  float f = 0;
  HIP_OR_FAIL(hipEventElapsedTime(&f, root.ev[7], root.ev[8]));
  *ms = f;
  return CTCEXT_OK;
}

// ---------------------------------------------------------------------------
// Streaming: token scores (ctcext.h).  The store is a stream's own x / norm in
// the layout CtcxScoresParams takes, so the kernel above runs unchanged.

extern "C" int ctcext_stream_scores_validate(const ctcext_stream_args* a, const ctcext_stream_scores_args* sa) {
  if (!a || !sa) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  int rc = ctcext_stream_validate(a);
  if (rc != CTCEXT_OK) return rc;
  const int32_t f = sa->store_format;
  if (f != CTCEXT_IN_NATIVE && f != CTCEXT_IN_F16 && f != CTCEXT_IN_BF16)
    return fail(CTCEXT_INVALID_ARGUMENT, "store_format must be CTCEXT_IN_NATIVE, CTCEXT_IN_F16 or CTCEXT_IN_BF16");
  if (f != CTCEXT_IN_NATIVE && a->dtype != CTCEXT_F32)
    return fail(CTCEXT_INVALID_ARGUMENT, "a half-precision score store needs dtype float32");
  if (a->on_device != 1)
    return fail(CTCEXT_INVALID_ARGUMENT, "a stream with a score store needs device chunks (on_device == 1): it has "
                                         "the enqueue-only push alone");
  rc = ctcext_token_times_validate(a->num_classes, a->blank_index, a->blank_label);
  if (rc == CTCEXT_OK) g_err.clear();
  return rc;
}

extern "C" int ctcext_stream_scores_validate_chunk(const ctcext_stream_args* a, const ctcext_stream_scores_args* sa,
                                                   const ctcext_chunk* c) {
  int rc = ctcext_stream_scores_validate(a, sa);
  if (rc == CTCEXT_OK) rc = check_push_dense(a, c, nullptr);
  if (rc == CTCEXT_OK) rc = check_store_chunk(sa->store_format, c);
  if (rc == CTCEXT_OK) g_err.clear();
  return rc;
}

extern "C" int64_t ctcext_stream_scores_bytes(const ctcext_stream_args* a, const ctcext_stream_scores_args* sa) {
  if (ctcext_stream_scores_validate(a, sa) != CTCEXT_OK) return -1;
  int64_t xb = 0, nb = 0;
  if (!ctcx_store_bytes(a->batch_size, a->max_frames, a->num_classes, sa->store_format, a->dtype == CTCEXT_F64, &xb,
                        &nb)) {
    (void)fail(CTCEXT_INVALID_ARGUMENT, "the score store's size leaves 64 bits");
    return -1;
  }
  return xb + nb;
}

// (the order of ctcext_stream_open_skip: everything the host can say first, the handle last)
extern "C" int ctcext_stream_open_scores(ctcext_decoder* d, const ctcext_stream_args* a, const ctcext_skip_args* k,
                                         const ctcext_stream_scores_args* sa, ctcext_stream** out) {
  if (!a || !sa || !out) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  int rc = ctcext_stream_scores_validate(a, sa);
  if (rc != CTCEXT_OK) return rc;
  if (k) {
    rc = ctcext_skip_validate(k);
    if (rc != CTCEXT_OK) return rc;
  }
  if (ctcext_stream_scores_bytes(a, sa) < 0) return CTCEXT_INVALID_ARGUMENT;
  if (!d) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (d->devs.size() != 1)
    return fail(CTCEXT_UNIMPLEMENTED, "a stream with a score store needs a one-device decoder handle");
  return stream_open_common(d, a, k, sa, out);
}

extern "C" int ctcext_stream_token_scores(ctcext_stream* st, const ctcext_token_times* t,
                                          const ctcext_token_scores* o) {
  if (!st) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  int rc = check_scores_out(o);
  if (rc != CTCEXT_OK) return rc;
  if (!t || !t->start || !t->end)
    return fail(CTCEXT_INVALID_ARGUMENT, "token scores need the start and end of ctcext_stream_token_times");
  auto& n = st->dn;
  const ctcext_stream_args& a = st->a;
  if (!st->sc.on)
    return fail(CTCEXT_FAILED_PRECONDITION,
                "ctcext_stream_token_scores on a stream without a score store (ctcext_stream_open_scores)");
  if (a.batch_size > 0 && (!n.used || !n.results))
    return fail(CTCEXT_FAILED_PRECONDITION,
                "ctcext_stream_token_scores without a ctcext_stream_push_dense that had hypothesis outputs");
  rc = ctcext_token_times_validate(a.num_classes, a.blank_index, a.blank_label);
  if (rc != CTCEXT_OK) return rc;
  if (a.batch_size == 0) return CTCEXT_OK;
  DeviceGuard guard;
  HIP_OR_FAIL(hipSetDevice(st->dec->devs[0].device));
  hipStream_t s = n.s;
  CtcxScoresParams p{};
  p.seq = (const int32_t*)n.seq.p;
  p.len = (const int32_t*)n.len.p;
  p.frames = st->sk.on ? (const int32_t*)st->sk.nfr.p : (const int32_t*)st->cum;
  p.status = (const int32_t*)n.fin.p;
  p.start = t->start; p.end = t->end;
  p.x = st->sc.sx;
  p.norm = st->sc.snorm;
  p.Tmax = a.max_frames; p.B = a.batch_size; p.C = a.num_classes;
  p.xst_t = a.num_classes; p.xst_b = a.max_frames * a.num_classes;
  p.P = a.top_paths; p.xfmt = st->sc.fmt; p.f64 = a.dtype == CTCEXT_F64 ? 1 : 0;
  p.blank_index = a.blank_index; p.blank_label = a.blank_label;
  p.logp_sum = o->logp_sum; p.logp_min = o->logp_min;
  const bool prof = (n.flags & CTCEXT_FLAG_PROFILE) != 0;
  if (prof) HIP_OR_FAIL(hipEventRecord(st->sc.ev[2], s));
  HIP_OR_FAIL(ctcx_launch_token_scores(p, s));
  if (prof) {
    HIP_OR_FAIL(hipEventRecord(st->sc.ev[3], s));
    st->sc.scores_timed = true;
  }
  g_err.clear();
  return CTCEXT_OK;
}

extern "C" int ctcext_stream_scores_ms(ctcext_stream* st, double* append_ms, double* scores_ms) {
  if (!st || !append_ms || !scores_ms) return fail(CTCEXT_INVALID_ARGUMENT, "null argument");
  if (!st->sc.on)
    return fail(CTCEXT_FAILED_PRECONDITION,
                "ctcext_stream_scores_ms on a stream without a score store (ctcext_stream_open_scores)");
  if (!st->dn.used || !(st->dn.flags & CTCEXT_FLAG_PROFILE))
    return fail(CTCEXT_FAILED_PRECONDITION, "no CTCEXT_FLAG_PROFILE enqueue-only push on this stream yet");
  DeviceGuard guard;
  HIP_OR_FAIL(hipSetDevice(st->dec->devs[0].device));
  *append_ms = *scores_ms = 0;
  float f = 0;
  if (st->sc.append_timed) {
    HIP_OR_FAIL(hipEventSynchronize(st->sc.ev[1]));
    HIP_OR_FAIL(hipEventElapsedTime(&f, st->sc.ev[0], st->sc.ev[1]));
    *append_ms = f;
  }
  if (st->sc.scores_timed) {
    HIP_OR_FAIL(hipEventSynchronize(st->sc.ev[3]));
    HIP_OR_FAIL(hipEventElapsedTime(&f, st->sc.ev[2], st->sc.ev[3]));
    *scores_ms = f;
  }
  g_err.clear();
  return CTCEXT_OK;
}
