"""ctypes binding of libctcext.so (the C ABI declared in include/ctcext.h).

This is the Python-side FFI a maintainer of the reference would add in place
of ``load_library.load_op_library('_ctc_ext_beam_search_decoder_ops.so')``
(python/ops/ctc_ext_beam_search_decoder_ops.py:10-11).  The library is built
in-tree by ``__graft_entry__.build()`` (or ``make -C ctc-beam-search-op_amd/csrc``);
there is no fallback: if it is missing or cannot run, calls fail loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CTCEXT_LIB_PATH") or os.path.join(_HERE, "lib", "libctcext.so")   # override: diagnostics builds

CTCEXT_OK = 0
CTCEXT_INVALID_ARGUMENT = 3
CTCEXT_FAILED_PRECONDITION = 9
CTCEXT_UNIMPLEMENTED = 12
CTCEXT_INTERNAL = 13
CTCEXT_F32 = 0
CTCEXT_F64 = 1
CTCEXT_FLAG_FORCE_LITERAL = 1
CTCEXT_FLAG_PROFILE = 2
CTCEXT_FLAG_PHASES = 4
CTCEXT_FLAG_GLOBAL_STATE = 8   # testing: the global-state tier whatever the shape
CTCEXT_FLAG_RECORD_RING = 16   # beam records kept in an LDS ring; only the reachable ones written to HBM
CTCEXT_FLAG_RING_MIN = 32      # testing: the record ring at 8 frames (short items flush); implies RECORD_RING
CTCEXT_FLAG_NO_RING = 64       # every beam record to HBM (the ring is the default for the score-table kernel)
CTCEXT_FLAG_HELPER_STRICT = 128     # a helper hand-over timeout fails the call instead of a one-wave re-decode
CTCEXT_FLAG_TEST_HELPER_DEAD = 256  # testing: the helper wave starts out timed out
CTCEXT_ABI_VERSION = 8
CTCEXT_IN_NATIVE = 0   # inputs_format: elements of dtype
CTCEXT_IN_F16 = 1      # float16 in memory, widened to float32 by the kernels (dtype CTCEXT_F32)
CTCEXT_IN_BF16 = 2     # bfloat16, likewise
CTCEXT_SCORER_BASE = 0
CTCEXT_SCORER_BIGRAM = 1

# every symbol include/ctcext.h declares
EXPORTED_SYMBOLS = ("ctcext_create", "ctcext_create_sharded", "ctcext_destroy", "ctcext_validate",
                    "ctcext_decode", "ctcext_decode_sharded", "ctcext_fetch", "ctcext_get_stats",
                    "ctcext_last_error", "ctcext_max_beam_width", "ctcext_phase_counters", "ctcext_row_facts",
                    "ctcext_get_stats_sized", "ctcext_abi_version",
                    "ctcext_stream_validate", "ctcext_stream_validate_chunk", "ctcext_stream_open",
                    "ctcext_stream_push", "ctcext_stream_frames", "ctcext_stream_reset", "ctcext_stream_close")
CTCEXT_KERNEL_STREAM = 0x8000   # ctcext_stats.kernel: a stream build of the decode kernel
# the dense, enqueue-only decode (CTCEXT_HAS_DENSE)
DENSE_SYMBOLS = ("ctcext_dense_validate", "ctcext_dense_reserve", "ctcext_decode_dense", "ctcext_dense_check",
                 "ctcext_dense_pack_ms")
EXPORTED_SYMBOLS = EXPORTED_SYMBOLS + DENSE_SYMBOLS
# the stable prefix of a stream (CTCEXT_HAS_STREAM_STABLE)
STREAM_STABLE_SYMBOLS = ("ctcext_stream_stable", "ctcext_stream_stable_reference")
EXPORTED_SYMBOLS = EXPORTED_SYMBOLS + STREAM_STABLE_SYMBOLS
# the enqueue-only push of a stream (CTCEXT_HAS_STREAM_DENSE)
STREAM_DENSE_SYMBOLS = ("ctcext_stream_dense_validate", "ctcext_stream_reserve", "ctcext_stream_push_dense",
                        "ctcext_stream_check", "ctcext_stream_commit_ms")
EXPORTED_SYMBOLS = EXPORTED_SYMBOLS + STREAM_DENSE_SYMBOLS
# token times (CTCEXT_HAS_TOKEN_TIMES)
TOKEN_TIMES_SYMBOLS = ("ctcext_token_times_validate", "ctcext_token_times_tile", "ctcext_dense_token_times",
                       "ctcext_stream_token_times", "ctcext_fetch_token_times", "ctcext_token_times_row",
                       "ctcext_dense_token_times_ms", "ctcext_stream_token_times_ms")
EXPORTED_SYMBOLS = EXPORTED_SYMBOLS + TOKEN_TIMES_SYMBOLS
# blank-frame skipping (CTCEXT_HAS_BLANK_SKIP)
BLANK_SKIP_SYMBOLS = ("ctcext_skip_validate", "ctcext_decode_skip", "ctcext_dense_reserve_skip",
                      "ctcext_decode_dense_skip", "ctcext_dense_skip_ms", "ctcext_skip_plan_row",
                      "ctcext_skip_expand_row")
EXPORTED_SYMBOLS = EXPORTED_SYMBOLS + BLANK_SKIP_SYMBOLS
# blank-frame skipping for streams (CTCEXT_HAS_STREAM_SKIP)
STREAM_SKIP_SYMBOLS = ("ctcext_stream_open_skip", "ctcext_stream_kept", "ctcext_skip_plan_chunk_row")
EXPORTED_SYMBOLS = EXPORTED_SYMBOLS + STREAM_SKIP_SYMBOLS
# token scores (CTCEXT_HAS_TOKEN_SCORES)
TOKEN_SCORES_SYMBOLS = ("ctcext_token_scores_tile", "ctcext_dense_token_scores", "ctcext_fetch_token_scores",
                        "ctcext_token_scores_row", "ctcext_dense_token_scores_ms")
EXPORTED_SYMBOLS = EXPORTED_SYMBOLS + TOKEN_SCORES_SYMBOLS
# token scores of a stream, from its score store (CTCEXT_HAS_STREAM_SCORES)
STREAM_SCORES_SYMBOLS = ("ctcext_stream_scores_validate", "ctcext_stream_scores_validate_chunk",
                         "ctcext_stream_scores_bytes", "ctcext_stream_open_scores", "ctcext_stream_token_scores",
                         "ctcext_stream_scores_ms")
EXPORTED_SYMBOLS = EXPORTED_SYMBOLS + STREAM_SCORES_SYMBOLS
CTCEXT_ITEM_CAPACITY = 16        # status bit of a push: the chunk would take the item past max_frames
CTCEXT_FLAG_DENSE_NULL_STREAM = 512   # ctcext_decode_dense: stream NULL is the null stream itself
CTCEXT_ITEM_LENGTH = 1           # status bits: sequence_length(b) > max_time
CTCEXT_ITEM_FEW_LEAVES = 2       # fewer leaves than top_paths
CTCEXT_ITEM_HELPER_TIMEOUT = 4   # a two-wave hand-over wait ran out
CTCEXT_ITEM_TABLE = 8            # the bigram table holds an entry > 0 or NaN


class DecodeArgs(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("inputs_on_device", ctypes.c_int32),
                ("inputs", ctypes.c_void_p), ("sequence_length", ctypes.c_void_p),
                ("max_time", ctypes.c_int64), ("batch_size", ctypes.c_int64),
                ("num_classes", ctypes.c_int64),
                ("beam_width", ctypes.c_int32), ("top_paths", ctypes.c_int32),
                ("merge_repeated", ctypes.c_int32), ("blank_index", ctypes.c_int32),
                ("blank_label", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("stream", ctypes.c_void_p),
                ("inputs_dims", ctypes.c_int32), ("sequence_length_dims", ctypes.c_int32),
                ("sequence_length_size", ctypes.c_int64),
                ("scorer", ctypes.c_int32), ("pad_", ctypes.c_int32), ("scorer_table", ctypes.c_void_p),
                # ABI 7 (all zero: the dense [max_time, batch, num_classes] tensor of dtype)
                ("inputs_format", ctypes.c_int32), ("pad2_", ctypes.c_int32),
                ("inputs_stride_t", ctypes.c_int64), ("inputs_stride_b", ctypes.c_int64)]


class StreamArgs(ctypes.Structure):
    """ctcext_stream_args: a stream's attributes, fixed for its life."""
    _fields_ = [("dtype", ctypes.c_int32), ("on_device", ctypes.c_int32),
                ("batch_size", ctypes.c_int64), ("num_classes", ctypes.c_int64),
                ("max_frames", ctypes.c_int64),
                ("beam_width", ctypes.c_int32), ("top_paths", ctypes.c_int32),
                ("merge_repeated", ctypes.c_int32), ("blank_index", ctypes.c_int32),
                ("blank_label", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("scorer", ctypes.c_int32), ("pad_", ctypes.c_int32), ("scorer_table", ctypes.c_void_p)]


class Chunk(ctypes.Structure):
    """ctcext_chunk: one push of a stream."""
    _fields_ = [("inputs", ctypes.c_void_p), ("chunk_length", ctypes.c_void_p),
                ("chunk_time", ctypes.c_int64),
                ("inputs_format", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("inputs_stride_t", ctypes.c_int64), ("inputs_stride_b", ctypes.c_int64),
                ("stream", ctypes.c_void_p)]


class DenseOutputs(ctypes.Structure):
    """ctcext_dense_outputs: the padded device outputs of ctcext_decode_dense."""
    _fields_ = [("decoded", ctypes.c_void_p), ("decoded_length", ctypes.c_void_p),
                ("alignment", ctypes.c_void_p), ("alignment_length", ctypes.c_void_p),
                ("log_probability", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("pad_value", ctypes.c_int64)]


class TokenTimesOut(ctypes.Structure):
    """ctcext_token_times: the outputs of the token-times calls."""
    _fields_ = [("start", ctypes.c_void_p), ("end", ctypes.c_void_p), ("trailing_blank", ctypes.c_void_p)]


class TokenScoresOut(ctypes.Structure):
    """ctcext_token_scores: the outputs of the token-scores calls."""
    _fields_ = [("logp_sum", ctypes.c_void_p), ("logp_min", ctypes.c_void_p)]


class SkipArgs(ctypes.Structure):
    """ctcext_skip_args: the threshold of a skipping decode and where its kept counts go."""
    _fields_ = [("logp_threshold", ctypes.c_double), ("kept", ctypes.c_void_p)]


class StreamScoresArgs(ctypes.Structure):
    """ctcext_stream_scores_args: the element format of a stream's score store."""
    _fields_ = [("store_format", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class StreamDenseOutputs(ctypes.Structure):
    """ctcext_stream_dense_outputs: the padded device outputs of ctcext_stream_push_dense."""
    _fields_ = [("decoded", ctypes.c_void_p), ("decoded_length", ctypes.c_void_p),
                ("alignment", ctypes.c_void_p), ("alignment_length", ctypes.c_void_p),
                ("log_probability", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("frames", ctypes.c_void_p),
                ("stable_length", ctypes.c_void_p), ("stable_frames", ctypes.c_void_p),
                ("pad_value", ctypes.c_int64)]


class PathSizes(ctypes.Structure):
    _fields_ = [("num_decoded", ctypes.c_int64), ("max_decoded", ctypes.c_int64),
                ("num_alignment", ctypes.c_int64), ("max_alignment", ctypes.c_int64)]


class Outputs(ctypes.Structure):
    _fields_ = [("outputs_on_device", ctypes.c_int32),
                ("decoded_indices", ctypes.POINTER(ctypes.c_void_p)),
                ("decoded_values", ctypes.POINTER(ctypes.c_void_p)),
                ("decoded_shape", ctypes.POINTER(ctypes.c_void_p)),
                ("alignment_indices", ctypes.POINTER(ctypes.c_void_p)),
                ("alignment_values", ctypes.POINTER(ctypes.c_void_p)),
                ("alignment_shape", ctypes.POINTER(ctypes.c_void_p)),
                ("log_probability", ctypes.c_void_p)]


class Stats(ctypes.Structure):
    _fields_ = [("literal_frames", ctypes.c_int64), ("literal_nonfinite", ctypes.c_int64),
                ("literal_fill", ctypes.c_int64), ("duplicate_frames", ctypes.c_int64),
                ("no_label_paths", ctypes.c_int64),
                ("decode_kernel_ms", ctypes.c_double), ("norm_kernel_ms", ctypes.c_double),
                ("traceback_ms", ctypes.c_double), ("n_devices", ctypes.c_int32),
                ("tier", ctypes.c_int32), ("ring_frames", ctypes.c_int32),
                ("records_written", ctypes.c_int64), ("record_bytes", ctypes.c_int32),
                ("helper", ctypes.c_int32), ("helper_redecodes", ctypes.c_int32), ("kernel", ctypes.c_int32),
                ("early_recursed_frames", ctypes.c_int64)]


# ctcext_stats.kernel (include/ctcext.h, CTCEXT_KERNEL_*)
PREPASS_NAMES = ("none", "facts_fused", "facts_norm", "row_prep_lds", "row_prep_global", "norm_only")
TRACEBACK_NAMES = ("none", "segmented", "one_thread")


def decode_kernel_stat(k):
    """The named fields of ctcext_stats.kernel: which decode kernel
    instantiation, pre-pass and traceback the library's launchers ran."""
    return {"launched": bool(k & 0x800), "tier": (k >> 10) & 1, "dtype": "f64" if k & 0x200 else "f32",
            "scorer": "bigram" if k & 0x100 else "base", "RN": (k >> 2) & 7, "WC": ((k >> 5) & 3) * 128,
            "BIG": bool(k & 0x80), "helper": "SQ" if k & 2 else "HW" if k & 1 else "none",
            "stream": bool(k & CTCEXT_KERNEL_STREAM),
            "prepass": PREPASS_NAMES[(k >> 12) & 7], "traceback": TRACEBACK_NAMES[(k >> 16) & 3]}


_lib = None


def load():
    """Load libctcext.so (raises OSError if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("libctcext.so not found at %s: run __graft_entry__.build() or "
                      "make -C ctc-beam-search-op_amd/csrc" % LIB_PATH)
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1.
    # Two HIP runtimes in one process cannot share the GPU (whichever opens it
    # first wins).  Importing torch first maps its copies; libctcext.so's
    # NEEDED entries then bind to them by SONAME, so the process has one runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    lib.ctcext_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.ctcext_create.restype = ctypes.c_int
    lib.ctcext_create_sharded.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.ctcext_create_sharded.restype = ctypes.c_int
    lib.ctcext_validate.argtypes = [ctypes.POINTER(DecodeArgs)]
    lib.ctcext_validate.restype = ctypes.c_int
    lib.ctcext_decode_sharded.argtypes = [ctypes.c_void_p, ctypes.POINTER(DecodeArgs), ctypes.POINTER(PathSizes)]
    lib.ctcext_decode_sharded.restype = ctypes.c_int
    lib.ctcext_destroy.argtypes = [ctypes.c_void_p]
    lib.ctcext_destroy.restype = None
    lib.ctcext_decode.argtypes = [ctypes.c_void_p, ctypes.POINTER(DecodeArgs), ctypes.POINTER(PathSizes)]
    lib.ctcext_decode.restype = ctypes.c_int
    lib.ctcext_fetch.argtypes = [ctypes.c_void_p, ctypes.POINTER(Outputs)]
    lib.ctcext_fetch.restype = ctypes.c_int
    lib.ctcext_get_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(Stats)]
    lib.ctcext_get_stats.restype = ctypes.c_int
    if hasattr(lib, "ctcext_get_stats_sized"):   # (ABI 5; older builds stay loadable for A/B runs)
        lib.ctcext_get_stats_sized.argtypes = [ctypes.c_void_p, ctypes.POINTER(Stats), ctypes.c_size_t]
        lib.ctcext_get_stats_sized.restype = ctypes.c_int
        lib.ctcext_abi_version.argtypes = []
        lib.ctcext_abi_version.restype = ctypes.c_int32
    lib.ctcext_last_error.argtypes = []
    lib.ctcext_last_error.restype = ctypes.c_char_p
    lib.ctcext_max_beam_width.argtypes = [ctypes.c_int64, ctypes.c_int32]
    lib.ctcext_max_beam_width.restype = ctypes.c_int32
    lib.ctcext_phase_counters.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    lib.ctcext_phase_counters.restype = ctypes.c_int
    if hasattr(lib, "ctcext_row_facts"):   # (diagnostics; absent from builds before it, kept loadable for A/B)
        lib.ctcext_row_facts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                         ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
        lib.ctcext_row_facts.restype = ctypes.c_int
    if hasattr(lib, "ctcext_stream_open"):   # (CTCEXT_HAS_STREAM; older builds stay loadable for A/B runs)
        lib.ctcext_stream_validate.argtypes = [ctypes.POINTER(StreamArgs)]
        lib.ctcext_stream_validate.restype = ctypes.c_int
        lib.ctcext_stream_validate_chunk.argtypes = [ctypes.POINTER(StreamArgs), ctypes.POINTER(Chunk)]
        lib.ctcext_stream_validate_chunk.restype = ctypes.c_int
        lib.ctcext_stream_open.argtypes = [ctypes.c_void_p, ctypes.POINTER(StreamArgs), ctypes.POINTER(ctypes.c_void_p)]
        lib.ctcext_stream_open.restype = ctypes.c_int
        lib.ctcext_stream_push.argtypes = [ctypes.c_void_p, ctypes.POINTER(Chunk), ctypes.POINTER(PathSizes)]
        lib.ctcext_stream_push.restype = ctypes.c_int
        lib.ctcext_stream_frames.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.ctcext_stream_frames.restype = ctypes.c_int
        lib.ctcext_stream_reset.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        lib.ctcext_stream_reset.restype = ctypes.c_int
        lib.ctcext_stream_close.argtypes = [ctypes.c_void_p]
        lib.ctcext_stream_close.restype = None
    if hasattr(lib, "ctcext_stream_stable"):   # (CTCEXT_HAS_STREAM_STABLE; older builds stay loadable for A/B runs)
        # (stream, int32 decoded_length[B], int64 stable_frames[B], int64 walked[B] or NULL)
        lib.ctcext_stream_stable.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32),
                                             ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        lib.ctcext_stream_stable.restype = ctypes.c_int
        lib.ctcext_stream_stable_reference.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32),
                                                       ctypes.POINTER(ctypes.c_int64)]
        lib.ctcext_stream_stable_reference.restype = ctypes.c_int
    if hasattr(lib, "ctcext_decode_dense"):   # (CTCEXT_HAS_DENSE; older builds stay loadable for A/B runs)
        lib.ctcext_dense_validate.argtypes = [ctypes.POINTER(DecodeArgs), ctypes.POINTER(DenseOutputs)]
        lib.ctcext_dense_validate.restype = ctypes.c_int
        lib.ctcext_dense_reserve.argtypes = [ctypes.c_void_p, ctypes.POINTER(DecodeArgs)]
        lib.ctcext_dense_reserve.restype = ctypes.c_int
        lib.ctcext_decode_dense.argtypes = [ctypes.c_void_p, ctypes.POINTER(DecodeArgs), ctypes.POINTER(DenseOutputs)]
        lib.ctcext_decode_dense.restype = ctypes.c_int
        lib.ctcext_dense_check.argtypes = [ctypes.c_void_p]
        lib.ctcext_dense_check.restype = ctypes.c_int
        lib.ctcext_dense_pack_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        lib.ctcext_dense_pack_ms.restype = ctypes.c_int
    if hasattr(lib, "ctcext_stream_push_dense"):   # (CTCEXT_HAS_STREAM_DENSE; older builds stay loadable for A/B runs)
        lib.ctcext_stream_dense_validate.argtypes = [ctypes.POINTER(StreamArgs), ctypes.POINTER(Chunk),
                                                     ctypes.POINTER(StreamDenseOutputs)]
        lib.ctcext_stream_dense_validate.restype = ctypes.c_int
        lib.ctcext_stream_reserve.argtypes = [ctypes.c_void_p, ctypes.c_int64]
        lib.ctcext_stream_reserve.restype = ctypes.c_int
        # (stream, chunk, int32 reset[B] on the device or NULL, outputs or NULL)
        lib.ctcext_stream_push_dense.argtypes = [ctypes.c_void_p, ctypes.POINTER(Chunk), ctypes.c_void_p,
                                                 ctypes.POINTER(StreamDenseOutputs)]
        lib.ctcext_stream_push_dense.restype = ctypes.c_int
        lib.ctcext_stream_check.argtypes = [ctypes.c_void_p]
        lib.ctcext_stream_check.restype = ctypes.c_int
        lib.ctcext_stream_commit_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        lib.ctcext_stream_commit_ms.restype = ctypes.c_int
    if hasattr(lib, "ctcext_dense_token_times"):   # (CTCEXT_HAS_TOKEN_TIMES; older builds stay loadable for A/B runs)
        lib.ctcext_token_times_validate.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
        lib.ctcext_token_times_validate.restype = ctypes.c_int
        lib.ctcext_token_times_tile.argtypes = []
        lib.ctcext_token_times_tile.restype = ctypes.c_int32
        lib.ctcext_dense_token_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(TokenTimesOut)]
        lib.ctcext_dense_token_times.restype = ctypes.c_int
        lib.ctcext_stream_token_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(TokenTimesOut)]
        lib.ctcext_stream_token_times.restype = ctypes.c_int
        lib.ctcext_fetch_token_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(TokenTimesOut), ctypes.c_int32]
        lib.ctcext_fetch_token_times.restype = ctypes.c_int
        # (int64 decoded[m], m, int64 alignment[L], L, frames, blank_label, merge_repeated,
        #  int32 start[m], int32 end[m], int32* trailing_blank)
        lib.ctcext_token_times_row.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int64,
                                               ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                               ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        lib.ctcext_token_times_row.restype = ctypes.c_int
        lib.ctcext_dense_token_times_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        lib.ctcext_dense_token_times_ms.restype = ctypes.c_int
        lib.ctcext_stream_token_times_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        lib.ctcext_stream_token_times_ms.restype = ctypes.c_int
    if hasattr(lib, "ctcext_decode_skip"):   # (CTCEXT_HAS_BLANK_SKIP; older builds stay loadable for A/B runs)
        lib.ctcext_skip_validate.argtypes = [ctypes.POINTER(SkipArgs)]
        lib.ctcext_skip_validate.restype = ctypes.c_int
        lib.ctcext_decode_skip.argtypes = [ctypes.c_void_p, ctypes.POINTER(DecodeArgs), ctypes.POINTER(SkipArgs),
                                           ctypes.POINTER(PathSizes)]
        lib.ctcext_decode_skip.restype = ctypes.c_int
        lib.ctcext_dense_reserve_skip.argtypes = [ctypes.c_void_p, ctypes.POINTER(DecodeArgs),
                                                  ctypes.POINTER(SkipArgs)]
        lib.ctcext_dense_reserve_skip.restype = ctypes.c_int
        lib.ctcext_decode_dense_skip.argtypes = [ctypes.c_void_p, ctypes.POINTER(DecodeArgs),
                                                 ctypes.POINTER(SkipArgs), ctypes.POINTER(DenseOutputs)]
        lib.ctcext_decode_dense_skip.restype = ctypes.c_int
        lib.ctcext_dense_skip_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(ctypes.c_double)]
        lib.ctcext_dense_skip_ms.restype = ctypes.c_int
        # (logp_blank[n] of the compute dtype, f64, n, thr, int32 kmap[n], int64* kept)
        lib.ctcext_skip_plan_row.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double,
                                             ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)]
        lib.ctcext_skip_plan_row.restype = ctypes.c_int
        # (int64 ali_c[L], L, int32 kmap[kept], kept, n, blank_label, int64 row[n], int64* row_len)
        lib.ctcext_skip_expand_row.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int64,
                                               ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
                                               ctypes.POINTER(ctypes.c_int64)]
        lib.ctcext_skip_expand_row.restype = ctypes.c_int
    if hasattr(lib, "ctcext_stream_open_skip"):   # (CTCEXT_HAS_STREAM_SKIP; older builds stay loadable for A/B runs)
        lib.ctcext_stream_open_skip.argtypes = [ctypes.c_void_p, ctypes.POINTER(StreamArgs),
                                                ctypes.POINTER(SkipArgs), ctypes.POINTER(ctypes.c_void_p)]
        lib.ctcext_stream_open_skip.restype = ctypes.c_int
        lib.ctcext_stream_kept.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.ctcext_stream_kept.restype = ctypes.c_int
        # (logp_blank[n] of the compute dtype, f64, n, thr, first_frame, prev_dom, int32 kmap[n], int64* kept,
        #  int32* last_dom)
        lib.ctcext_skip_plan_chunk_row.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double,
                                                   ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                   ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)]
        lib.ctcext_skip_plan_chunk_row.restype = ctypes.c_int
    if hasattr(lib, "ctcext_dense_token_scores"):   # (CTCEXT_HAS_TOKEN_SCORES; older builds stay loadable for A/B runs)
        lib.ctcext_token_scores_tile.argtypes = []
        lib.ctcext_token_scores_tile.restype = ctypes.c_int32
        lib.ctcext_dense_token_scores.argtypes = [ctypes.c_void_p, ctypes.POINTER(TokenTimesOut),
                                                  ctypes.POINTER(TokenScoresOut)]
        lib.ctcext_dense_token_scores.restype = ctypes.c_int
        lib.ctcext_fetch_token_scores.argtypes = [ctypes.c_void_p, ctypes.POINTER(TokenScoresOut), ctypes.c_int32]
        lib.ctcext_fetch_token_scores.restype = ctypes.c_int
        # (x[frames][num_classes] and norm[frames] of the compute dtype, f64, frames, num_classes,
        #  int64 alignment[L], L, int32 start[m], int32 end[m], m, blank_index, blank_label, logp_sum[m], logp_min[m])
        lib.ctcext_token_scores_row.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64,
                                                ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
                                                ctypes.c_void_p]
        lib.ctcext_token_scores_row.restype = ctypes.c_int
        lib.ctcext_dense_token_scores_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        lib.ctcext_dense_token_scores_ms.restype = ctypes.c_int
    if hasattr(lib, "ctcext_stream_open_scores"):   # (CTCEXT_HAS_STREAM_SCORES; older builds stay loadable for A/B runs)
        lib.ctcext_stream_scores_validate.argtypes = [ctypes.POINTER(StreamArgs), ctypes.POINTER(StreamScoresArgs)]
        lib.ctcext_stream_scores_validate.restype = ctypes.c_int
        lib.ctcext_stream_scores_validate_chunk.argtypes = [ctypes.POINTER(StreamArgs),
                                                            ctypes.POINTER(StreamScoresArgs), ctypes.POINTER(Chunk)]
        lib.ctcext_stream_scores_validate_chunk.restype = ctypes.c_int
        lib.ctcext_stream_scores_bytes.argtypes = [ctypes.POINTER(StreamArgs), ctypes.POINTER(StreamScoresArgs)]
        lib.ctcext_stream_scores_bytes.restype = ctypes.c_int64
        # (decoder, args, skip args or NULL, scores args, ctcext_stream**)
        lib.ctcext_stream_open_scores.argtypes = [ctypes.c_void_p, ctypes.POINTER(StreamArgs),
                                                  ctypes.POINTER(SkipArgs), ctypes.POINTER(StreamScoresArgs),
                                                  ctypes.POINTER(ctypes.c_void_p)]
        lib.ctcext_stream_open_scores.restype = ctypes.c_int
        lib.ctcext_stream_token_scores.argtypes = [ctypes.c_void_p, ctypes.POINTER(TokenTimesOut),
                                                   ctypes.POINTER(TokenScoresOut)]
        lib.ctcext_stream_token_scores.restype = ctypes.c_int
        lib.ctcext_stream_scores_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                                ctypes.POINTER(ctypes.c_double)]
        lib.ctcext_stream_scores_ms.restype = ctypes.c_int
    _lib = lib
    return lib


def get_stats(lib, handle, st):
    """Fill Stats st from the last decode on handle (only the prefix an older build knows)."""
    if hasattr(lib, "ctcext_get_stats_sized"):
        return lib.ctcext_get_stats_sized(handle, ctypes.byref(st), ctypes.sizeof(st))
    return lib.ctcext_get_stats(handle, ctypes.byref(st))
