"""Blank-frame skipping without a GPU: ctcext_skip_plan_row and
ctcext_skip_expand_row (the host definition, plain C++) against the Python
restatement of include/ctcext.h, on the input families and on hand-written
rows; the validate messages; the struct against the header; the symbols; and
the conditions that keep the GPU tests from being vacuous, on the restatement."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import ctcext_amd
import skip_util as su
from ctcext_amd import _lib
from token_times_util import family

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctcext.h")
MSG = "blank skip threshold must be a log-probability (<= 0)"

# (T, B, C, W, P): the GPU tests' family shapes
SHAPES = [(12, 6, 5, 8, 3), (40, 4, 29, 16, 3), (60, 3, 29, 128, 3)]
KINDS = ("peaky", "sticky", "gaussian")
# At log 0.9 these cases drop nothing (counted on the restatement: a Gaussian
# row gives the blank p > 0.9 in almost no frame, a sticky one only at C = 5);
# there the skipping decode is the plain one.  Every family also runs at the
# median of its blank log-probabilities ("median"), where each drops frames.
NOTHING_DROPPED = {("gaussian", s) for s in SHAPES} | {("sticky", s) for s in SHAPES[1:]}


def plan_row(lp, n, thr):
    lib = _lib.load()
    lp = np.ascontiguousarray(lp)
    kmap = np.full((max(n, 1),), -5, np.int32)
    kept = ctypes.c_int64(-1)
    rc = lib.ctcext_skip_plan_row(lp.ctypes.data, 1 if lp.dtype == np.float64 else 0, n, float(thr),
                                  kmap.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(kept))
    assert rc == _lib.CTCEXT_OK, rc
    assert (kmap[kept.value:] == -5).all()
    return kmap[:kept.value].tolist()


def expand_row(ali_c, kmap, n, blank_label):
    lib = _lib.load()
    a = np.ascontiguousarray(np.asarray(ali_c, np.int64))
    k = np.ascontiguousarray(np.asarray(kmap, np.int32))
    row = np.full((max(n, 1),), -99, np.int64)
    ln = ctypes.c_int64(-1)
    rc = lib.ctcext_skip_expand_row(a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), a.size,
                                    k.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), k.size, n, blank_label,
                                    row.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.byref(ln))
    assert rc == _lib.CTCEXT_OK, rc
    assert (row[ln.value:] == -99).all()
    return row[:ln.value].tolist()


@functools.lru_cache(maxsize=None)
def _case(kind, shape, thr, dtype="float32"):
    T, B, C, W, P = shape
    x = family(np.random.default_rng(sum(kind.encode()) + T), kind, T, B, C, np.dtype(dtype))
    sl = su.lengths(T, B)
    if thr == "median":
        thr = su.median_threshold(x, sl)
    return x, sl, thr, su.expected(x, sl, W, P, thr, merge_repeated=True)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_row_functions_match_the_restatement(kind, shape, dtype):
    T, B, C, W, P = shape
    for thr in (su.THR, "median"):
        x, sl, thr, e = _case(kind, shape, thr, dtype)
        lp = su.logp_blank(x)
        for b in range(B):
            n = int(sl[b])
            assert plan_row(lp[:n, b], n, thr) == e.kmaps[b], (kind, shape, b)
            kc = len(e.kmaps[b])
            # every suffix length of a compacted row, with its frames as values
            for L in sorted({0, 1, kc // 2, kc}):
                ali_c = [100 + f for f in e.kmaps[b][kc - L:]]
                want = su.skip_expand(ali_c, e.kmaps[b], n, -1)
                assert expand_row(ali_c, e.kmaps[b], n, -1) == want, (kind, shape, b, L)
                # the properties the definition promises
                assert len(want) <= n and [v for v in want if v != -1] == ali_c
                assert all(v == -1 or v == 100 + (n - len(want) + i) for i, v in enumerate(want))


NAN = float("nan")
D, K = -0.01, -3.0   # blank-dominant and not, at thr = log 0.9

# (name, logp_blank, thr, kmap)
HAND_PLAN = [
    ("all frames dominant: one frame is kept", [D] * 7, su.THR, [0]),
    ("alternating frames", [D, K, D, K, D, K], su.THR, [0, 1, 2, 3, 4, 5]),
    ("the first frame of every run stays", [K, D, D, D, K, D, D], su.THR, [0, 1, 4, 5]),
    ("a NaN row is kept, and ends the run", [D, D, NAN, D, D], su.THR, [0, 2, 3]),
    ("a -inf blank is kept", [D, -math.inf, D, D], su.THR, [0, 1, 2]),
    ("thr = 0 keeps everything", [0.0, 0.0, -0.0, 0.0], 0.0, [0, 1, 2, 3]),
    ("a value equal to thr is not dominant", [-1.0, -1.0, -1.0], -1.0, [0, 1, 2]),
    ("n = 0", [], su.THR, []),
    ("n = 1", [D], su.THR, [0]),
]


@pytest.mark.parametrize("row", HAND_PLAN, ids=[r[0] for r in HAND_PLAN])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hand_written_plans(row, dtype):
    name, lp, thr, kmap = row
    lp = np.asarray(lp, dtype)
    # the expectations above are hand-derived; the restatement agrees with them
    assert su.skip_plan(lp, len(lp), dtype(thr)) == kmap, name
    assert plan_row(lp, len(lp), thr) == kmap, name


B_ = 9   # the hand-written rows' blank_label

# (name, ali_c, kmap, n, row)
HAND_EXPAND = [
    ("L = 0", [], [0, 3], 5, []),
    ("nothing dropped", [1, B_, 2], [0, 1, 2], 3, [1, B_, 2]),
    ("dropped frames read blank_label", [1, B_, 2], [0, 1, 4], 6, [1, B_, B_, B_, 2, B_]),
    ("an alignment shorter than the item", [2, 2], [0, 3, 4, 8], 10, [2, B_, B_, B_, 2, B_]),
    ("one frame kept of twelve", [B_], [0], 12, [B_] * 12),
    ("the last kept frame alone", [5], [0, 2, 7], 9, [5, B_]),
]


@pytest.mark.parametrize("row", HAND_EXPAND, ids=[r[0] for r in HAND_EXPAND])
def test_hand_written_expansions(row):
    name, ali_c, kmap, n, want = row
    assert su.skip_expand(ali_c, kmap, n, B_) == want, name
    assert expand_row(ali_c, kmap, n, B_) == want, name


def test_row_functions_refuse_bad_arguments():
    lib = _lib.load()
    kept, ln = ctypes.c_int64(), ctypes.c_int64()
    lp = np.zeros(4, np.float32)
    kmap = np.zeros(4, np.int32)
    kp = kmap.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    for thr in (0.5, NAN):
        assert lib.ctcext_skip_plan_row(lp.ctypes.data, 0, 4, thr, kp, ctypes.byref(kept)) == _lib.CTCEXT_INVALID_ARGUMENT
    assert lib.ctcext_skip_plan_row(lp.ctypes.data, 0, -1, -1.0, kp, ctypes.byref(kept)) == _lib.CTCEXT_INVALID_ARGUMENT
    a = np.zeros(4, np.int64)
    ap = a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    # L above kept, kept above n, a map that does not ascend
    for L, k, n, km in ((3, 2, 4, [0, 1, 0, 0]), (1, 4, 3, [0, 1, 2, 3]), (2, 2, 4, [3, 1, 0, 0])):
        kmap[:] = km
        assert lib.ctcext_skip_expand_row(ap, L, kp, k, n, -1, ap, ctypes.byref(ln)) == _lib.CTCEXT_INVALID_ARGUMENT


def test_validate_messages():
    lib = _lib.load()
    for thr, ok in ((0.0, True), (-0.0, True), (su.THR, True), (-math.inf, True), (1e-9, False), (math.inf, False),
                    (NAN, False)):
        k = _lib.SkipArgs()
        k.logp_threshold = thr
        rc = lib.ctcext_skip_validate(ctypes.byref(k))
        if ok:
            assert rc == _lib.CTCEXT_OK and lib.ctcext_last_error().decode() == "", thr
        else:
            assert rc == _lib.CTCEXT_INVALID_ARGUMENT and lib.ctcext_last_error().decode() == MSG, thr
    assert lib.ctcext_skip_validate(None) == _lib.CTCEXT_INVALID_ARGUMENT


def test_python_refuses_a_bad_threshold_before_any_device_work():
    """No GPU here: the calls raise from the host-only check, before a handle exists."""
    x = np.zeros((4, 1, 3), np.float32)
    for f in (ctcext_amd.ctc_ext_beam_search_decoder, lambda *a, **k: ctcext_amd.decode_logits(*a, batch_first=False, **k)):
        for thr in (0.1, NAN):
            with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
                f(x, [4], 2, 1, skip_blank=thr)
            assert e.value.message == MSG and e.value.error_code == _lib.CTCEXT_INVALID_ARGUMENT


def test_skip_struct_matches_header(tmp_path):
    """The ctypes mirror of ctcext_skip_args has the C header's size and field
    offsets (gcc on include/ctcext.h), the feature macro is set, and the ABI
    version, ctcext_decode_args and ctcext_stats are what they were."""
    src = tmp_path / "abi.c"
    py = _lib.SkipArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ctcext.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(ctcext_skip_args));']
    for f, _ in py._fields_:
        lines.append('printf("%%s %%zu\\n", "%s", offsetof(ctcext_skip_args, %s));' % (f, f))
    lines += ['printf("has %d\\n", (int)CTCEXT_HAS_BLANK_SKIP);', 'printf("abi %d\\n", (int)CTCEXT_ABI_VERSION);',
              'printf("args %zu\\n", sizeof(ctcext_decode_args));', 'printf("stats %zu\\n", sizeof(ctcext_stats));',
              "return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(py) == 16
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset, f
    assert int(got["has"]) == 1 and int(got["abi"]) == 8
    assert int(got["args"]) == ctypes.sizeof(_lib.DecodeArgs) and int(got["stats"]) == ctypes.sizeof(_lib.Stats)


def test_symbols_and_exports():
    lib = _lib.load()
    for s in _lib.BLANK_SKIP_SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.ctcext_abi_version() == 8
    assert callable(ctcext_amd.kept_frames) and "kept_frames" in ctcext_amd.__all__
    # the return tuples are as they were
    assert len(ctcext_amd.CTCExtBeamSearchDecoder._fields) == 7 and len(ctcext_amd.DenseDecode._fields) == 6


def test_kept_frames_without_a_skipping_decode_fails_precondition():
    import threading
    seen = []

    def run():
        try:
            ctcext_amd.kept_frames(0)
        except ctcext_amd.FailedPreconditionError as e:
            seen.append(e.message)
    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert seen == ["kept_frames without a decode with skip_blank"]


# ---- the conditions the GPU tests rest on, on the restatement

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_family_cases_drop_frames(kind, shape):
    T, B, C, W, P = shape
    x, sl, _, e = _case(kind, shape, su.THR)
    dropped = int(sl.sum() - e.kept.sum())
    if (kind, shape) in NOTHING_DROPPED:
        assert dropped == 0, (kind, shape, dropped)
    else:
        assert dropped >= 1, (kind, shape)
    if kind == "peaky":
        assert su.dropped_share(e, sl) >= 0.25, (shape, su.dropped_share(e, sl))
    x, sl, thr, e = _case(kind, shape, "median")
    assert thr < 0 and su.dropped_share(e, sl) >= 0.1, (kind, shape, thr, su.dropped_share(e, sl))


def test_peaky_12_has_an_item_that_keeps_one_frame_of_twelve():
    x, sl, _, e = _case("peaky", SHAPES[0], su.THR)
    assert sl[0] == 12 and e.kept[0] == 1, (sl.tolist(), e.kept.tolist())
    # ... and its alignment is twelve frames again
    assert all(len(e.ali[0][p]) == 12 for p in range(3))


def test_kept_counts_of_the_larger_cases():
    """The figures the long-row and the large-C GPU cases were chosen by."""
    x, sl, _, e = _case("peaky", SHAPES[2], su.THR)
    assert e.kept.tolist() == [36, 31, 28] and sl.tolist() == [60, 57, 55]
    T, B, C = 700, 3, 5
    x = family(np.random.default_rng(sum(b"peaky") + T), "peaky", T, B, C)
    kept = [len(k) for k in su.plan(x, su.lengths(T, B), su.THR)]
    assert kept == [381, 377, 364], kept
    tile = 256   # the kernels' tile: kept rows and items of more than two tiles
    assert min(kept) > tile and T > 2 * tile
    T, B, C = 300, 2, 100
    x = family(np.random.default_rng(sum(b"peaky") + T), "peaky", T, B, C)
    assert [len(k) for k in su.plan(x, su.lengths(T, B), su.THR)] == [207, 211]
