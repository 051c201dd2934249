"""Stream token scores without a GPU (include/ctcext.h, "Streaming: token
scores"): the host-only entry points -- ctcext_stream_scores_validate,
_validate_chunk and _bytes -- and, on the oracle, the properties the GPU cases
of test_gpu_stream_scores.py rely on, so that none of them passes vacuously."""
import ctypes

import numpy as np
import pytest

import ctcext_amd
import stream_scores_util as ssc
import stream_skip_util as ssu
from ctcext_amd import _lib

OK, INVALID, UNIMPLEMENTED = _lib.CTCEXT_OK, _lib.CTCEXT_INVALID_ARGUMENT, _lib.CTCEXT_UNIMPLEMENTED
NATIVE, F16, BF16 = _lib.CTCEXT_IN_NATIVE, _lib.CTCEXT_IN_F16, _lib.CTCEXT_IN_BF16

M_FORMAT = "store_format must be CTCEXT_IN_NATIVE, CTCEXT_IN_F16 or CTCEXT_IN_BF16"
M_HALF = "a half-precision score store needs dtype float32"
M_DEVICE = "a stream with a score store needs device chunks (on_device == 1): it has the enqueue-only push alone"
M_BLANK = "token times need a blank_label that is no class label"
M_CHUNK = "chunk inputs_format differs from the stream's score store format"


def _args(B=256, C=29, F=1500, W=16, P=1, dtype=_lib.CTCEXT_F32, on_device=1, blank_label=-1, flags=0):
    a = _lib.StreamArgs()
    a.dtype, a.on_device = dtype, on_device
    a.batch_size, a.num_classes, a.max_frames = B, C, F
    a.beam_width, a.top_paths = W, P
    a.blank_index, a.blank_label, a.flags = 0, blank_label, flags
    return a


def _scores(fmt=NATIVE):
    s = _lib.StreamScoresArgs()
    s.store_format = fmt
    return s


def _validate(a, s):
    lib = _lib.load()
    rc = lib.ctcext_stream_scores_validate(None if a is None else ctypes.byref(a), None if s is None else ctypes.byref(s))
    return rc, lib.ctcext_last_error().decode()


def test_has_the_symbols():
    lib = _lib.load()
    for name in _lib.STREAM_SCORES_SYMBOLS:
        assert hasattr(lib, name), name
    assert set(_lib.STREAM_SCORES_SYMBOLS) <= set(_lib.EXPORTED_SYMBOLS)
    assert lib.ctcext_abi_version() == 8


@pytest.mark.parametrize("fmt", [NATIVE, F16, BF16])
def test_validate_accepts_the_three_formats(fmt):
    assert _validate(_args(), _scores(fmt)) == (OK, "")
    assert _validate(_args(dtype=_lib.CTCEXT_F64), _scores(NATIVE)) == (OK, "")
    # (a blank_label at blank_index is no other class's label: the token-times rule)
    assert _validate(_args(blank_label=0), _scores(fmt)) == (OK, "")


def test_validate_messages():
    assert _validate(None, _scores()) == (INVALID, "null argument")
    assert _validate(_args(), None) == (INVALID, "null argument")
    for fmt in (-1, 3, 7):
        assert _validate(_args(), _scores(fmt)) == (INVALID, M_FORMAT)
    for fmt in (F16, BF16):
        assert _validate(_args(dtype=_lib.CTCEXT_F64), _scores(fmt)) == (INVALID, M_HALF)
    for on_device in (0, 2):
        assert _validate(_args(on_device=on_device), _scores()) == (INVALID, M_DEVICE)
    assert _validate(_args(blank_label=3), _scores()) == (INVALID, M_BLANK)
    # the stream's own checks come first, with their messages
    assert _validate(_args(F=-1), _scores()) == (INVALID, "max_frames is negative")
    assert _validate(_args(W=0), _scores())[0] == INVALID
    # ... and the order of this entry point's own: the format, the dtype, the chunks' place, the label
    assert _validate(_args(dtype=_lib.CTCEXT_F64, on_device=0, blank_label=3), _scores(9)) == (INVALID, M_FORMAT)
    assert _validate(_args(dtype=_lib.CTCEXT_F64, on_device=0, blank_label=3), _scores(F16)) == (INVALID, M_HALF)
    assert _validate(_args(on_device=0, blank_label=3), _scores(F16)) == (INVALID, M_DEVICE)


def _chunk(fmt=NATIVE, t=10, flags=0, st=(0, 0)):
    c = _lib.Chunk()
    c.inputs = 4096   # (never read on the host)
    c.chunk_time, c.inputs_format, c.flags = t, fmt, flags
    c.inputs_stride_t, c.inputs_stride_b = st
    return c


def _validate_chunk(a, s, c):
    lib = _lib.load()
    rc = lib.ctcext_stream_scores_validate_chunk(ctypes.byref(a), ctypes.byref(s), None if c is None else ctypes.byref(c))
    return rc, lib.ctcext_last_error().decode()


def test_validate_chunk():
    a = _args()
    for fmt in (NATIVE, F16, BF16):   # a native store takes every format the stream takes
        assert _validate_chunk(a, _scores(NATIVE), _chunk(fmt)) == (OK, "")
    for store in (F16, BF16):         # a half store its own alone
        for fmt in (NATIVE, F16, BF16):
            want = (OK, "") if fmt == store else (INVALID, M_CHUNK)
            assert _validate_chunk(a, _scores(store), _chunk(fmt)) == want, (store, fmt)
        assert _validate_chunk(a, _scores(store), _chunk(NATIVE, t=0)) == (INVALID, M_CHUNK)
    # the stream's and the store's checks first, then the chunk's own, then the format
    assert _validate_chunk(_args(on_device=0), _scores(BF16), _chunk(F16)) == (INVALID, M_DEVICE)
    assert _validate_chunk(a, _scores(BF16), None) == (INVALID, "null argument")
    assert _validate_chunk(a, _scores(BF16), _chunk(F16, t=-1)) == (INVALID, "inputs has a negative dimension")
    assert _validate_chunk(a, _scores(BF16), _chunk(F16, flags=_lib.CTCEXT_FLAG_PHASES))[0] == INVALID
    assert _validate_chunk(a, _scores(BF16), _chunk(F16, st=(29, 0))) == \
        (INVALID, "inputs_stride_t and inputs_stride_b must be given together")
    assert _validate_chunk(_args(dtype=_lib.CTCEXT_F64), _scores(NATIVE), _chunk(BF16)) == \
        (INVALID, "half-precision inputs need dtype float32")
    assert _validate_chunk(a, _scores(BF16), _chunk(BF16, st=(40 * 256, 40))) == (OK, "")


def _bytes(a, s):
    return _lib.load().ctcext_stream_scores_bytes(ctypes.byref(a), ctypes.byref(s))


def test_bytes_is_the_documented_formula():
    # batch * max_frames * (num_classes * esize + sizeof(ftype)); the cfg3 stream shape
    assert _bytes(_args(), _scores(NATIVE)) == 256 * 1500 * (29 * 4 + 4) == 46_080_000
    assert _bytes(_args(), _scores(BF16)) == 256 * 1500 * (29 * 2 + 4) == 23_808_000
    assert _bytes(_args(), _scores(F16)) == 23_808_000
    assert _bytes(_args(B=3, C=80, F=77, dtype=_lib.CTCEXT_F64), _scores(NATIVE)) == 3 * 77 * (80 * 8 + 8)
    assert _bytes(_args(B=0), _scores()) == 0 and _bytes(_args(F=0), _scores()) == 0
    # invalid arguments: -1, with the validation's message
    assert _bytes(_args(dtype=_lib.CTCEXT_F64), _scores(BF16)) == -1
    assert _lib.load().ctcext_last_error().decode() == M_HALF
    assert _bytes(_args(), _scores(5)) == -1
    assert _bytes(_args(on_device=0), _scores()) == -1
    # a size past int64: -1, not a wrapped number
    assert _bytes(_args(B=2 ** 31, C=2 ** 29, F=2 ** 31 - 1, W=16), _scores()) == -1


def test_python_layer_validates_at_construction():
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.StreamDecoder(2, 5, 8, 1, 16, blank_label=3, token_scores=True)
    assert e.value.message == M_BLANK
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.StreamDecoder(2, 5, 8, 1, 16, dtype="float64", token_scores=True, score_store="bfloat16")
    assert e.value.message == M_HALF
    with pytest.raises(TypeError):
        ctcext_amd.StreamDecoder(2, 5, 8, 1, 16, token_scores=True, score_store="float8")
    with pytest.raises(ValueError):
        ctcext_amd.StreamDecoder(2, 5, 8, 1, 16, score_store="bfloat16")
    # nothing opens before the first push: no device is needed for these
    s = ctcext_amd.StreamDecoder(2, 5, 8, 1, 16, token_scores=True, score_store="float16")
    with pytest.raises(ctcext_amd.UnimplementedError) as e:
        s.push(np.zeros((2, 3, 5), np.float32))
    assert e.value.message == "a stream with a score store has no synchronous push: use ctcext_stream_push_dense"
    with pytest.raises(ctcext_amd.FailedPreconditionError):
        s.token_scores_dense()
    with pytest.raises(ctcext_amd.FailedPreconditionError):
        ctcext_amd.StreamDecoder(2, 5, 8, 1, 16).token_scores_dense()
    s.close()


# ---- the properties the GPU cases rely on, on the oracle

@pytest.mark.parametrize("case", ssc.EVERY_PUSH, ids=ssc.case_id)
def test_every_push_schedules_hold_spans_that_cross_pushes(case):
    kind, shape, merge, push = case
    x, sl, kw, pushes = ssc.every_push_case(*case)
    assert len(pushes) >= 3 and pushes[-1][2] == np.maximum(sl, 0).tolist()
    crossing, timed = ssc.crossing_spans(pushes[-1][3], pushes[-1][4], push)
    if kind in ("sticky", "peaky"):
        assert crossing >= 4, (crossing, timed)
        assert (crossing, timed) == ssc.CROSSING[(kind, shape, push)]
    elif kind == "gaussian":
        # merge off, short tokens, none across a push: kept for those, not for this property
        assert crossing == 0 and timed > 0
    else:   # neg_inf: untimed tokens below the decoded length
        start = pushes[-1][3][0]
        assert timed > 0 and np.isnan(pushes[-1][4][0][start >= 0]).sum() == 0
    # what is expected moves between pushes: the first push's answer does not pass for the last
    assert not np.array_equal(pushes[0][4][0], pushes[-1][4][0], equal_nan=True)


@pytest.mark.parametrize("case", ssc.TILED_PUSH, ids=ssc.case_id)
def test_tiled_schedules_hold_spans_that_cross_pushes(case):
    shape, soft, push = case
    T, B, C, W, P = shape
    x, sl, kw, pushes = ssc.tiled_push_case(*case)
    assert T > _lib.load().ctcext_token_scores_tile() and len(pushes) == -(-T // push)
    crossing, timed = ssc.crossing_spans(pushes[-1][3], pushes[-1][4], push)
    assert crossing >= 4 and (crossing, timed) == ssc.CROSSING[("tiled", shape, push)]
    if B == 3:   # item 2 has no frames: NaN rows after every push
        assert sl[2] == 0 and all(np.isnan(p[4][0][2]).all() for p in pushes)


@pytest.mark.parametrize("push,want", [(3, (6, 14, 3, 5)), (4, (7, 14, 1, 3))])
def test_skipping_schedules_drop_whole_pushes_and_begin_inside_runs(push, want):
    x, sl, kw, e, pushes = ssc.skip_push_case(push)
    crossing, timed = ssc.crossing_spans(pushes[-1][3], pushes[-1][4], push)
    whole, straddle = ssu.exercised(e.kmaps, ssu.schedule(sl, push))
    assert whole >= 1 and straddle >= 1 and crossing >= 1
    assert (crossing, timed, whole, straddle) == want
    # after the last push: the one-shot skipping case's own expectations
    np.testing.assert_array_equal(pushes[-1][4][0], ssc.tsu.skip_case()[5][0])


def test_a_store_that_kept_the_decoy_would_fail_the_rollback_case():
    x, decoy, kw, first, both, mixed = ssc.rollback_case()
    T, B, C, W, P = ssc.ROLLBACK_SHAPE
    for b in range(B):
        timed = ~np.isnan(both[1][0][b])
        assert timed.any()
        differ = both[1][0][b][timed] != mixed[0][b][timed]
        assert differ.sum() >= 1, b
    # ... and chunk 2 changes what chunk 1 left
    assert not np.array_equal(first[1][0], both[1][0], equal_nan=True)
