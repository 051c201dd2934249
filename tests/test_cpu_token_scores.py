"""Token scores without a GPU: ctcext_token_scores_row (the host definition
behind ctcext_amd.token_scores_row) against the Python restatement of
include/ctcext.h, on the oracle's rows of every input family and on
hand-written rows; the properties the GPU tests' input cases are asserted to
have; the symbols."""
import numpy as np
import pytest

import ctcext_amd
from ctcext_amd import _lib
from token_scores_util import (FAMILY_CASES, NEG_INF_SEEDS, SKIP_SHAPE, TILED, family_case, item_norm,
                               nan_cells_inside_decoded_length, skip_case, skip_properties, tile_properties,
                               tiled_case, token_scores)

NAN, INF = float("nan"), float("inf")


def _same(got, want, what):
    """NaN mask, then exact equality of the rest."""
    got, want = np.asarray(got), np.asarray(want, got.dtype)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg="%s: NaN mask" % (what,))
    np.testing.assert_array_equal(got[~np.isnan(got)], want[~np.isnan(want)], err_msg=str(what))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kind,shape,merge", [c for c in FAMILY_CASES if c[1][3] <= 16],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_row_function_matches_definition_on_oracle_rows(kind, shape, merge, dtype):
    T, B, C, W, P = shape
    x, sl, kw, (dec, ali, (start, end, _), (lsum, lmin)) = family_case(kind, shape, merge, dtype)
    scored = 0
    for b in range(B):
        n = int(sl[b])
        norm = item_norm(x, b, n)
        for p in range(P):
            m = len(dec[b][p])
            s, mn = ctcext_amd.token_scores_row(x[:n, b], norm, ali[b][p], n, start[b, p, :m], end[b, p, :m], 0, -1)
            assert s.dtype == x.dtype and mn.dtype == x.dtype and s.shape == (m,) and mn.shape == (m,)
            _same(s, lsum[b, p, :m], ("logp_sum", b, p))
            _same(mn, lmin[b, p, :m], ("logp_min", b, p))
            # what the definition promises: NaN exactly at the untimed tokens (these families hold no NaN
            # and no +inf), a minimum no smaller than the sum of non-positive terms allows
            timed = start[b, p, :m] >= 0
            if kind != "neg_inf":
                np.testing.assert_array_equal(np.isnan(s), ~timed)
                assert (mn[timed] <= 0).all() and (s[timed] <= mn[timed]).all()
            scored += int(timed.sum())
            assert np.isnan(lsum[b, p, m:]).all() and np.isnan(lmin[b, p, m:]).all()
    assert scored > 0 or T == 1   # (one frame may decode to no label at all)


# blank_index 0 and blank_label 9 unless the row says otherwise; norm is given,
# not computed: every value below is exact in float32, so the expectations are
# hand-derived numbers
# (name, x [frames][3], norm, alignment, frames, start, end, blank_index, blank_label, logp_sum, logp_min)
HAND = [
    ("three frames of one label", [[0, 1.5, 0], [0, 0.5, 0], [0, -1, 0]], [2, 1, 1], [1, 1, 1], 3, [0], [2], 0, 9,
     [-3.0], [-2.0]),
    ("a leading NaN stays in both", [[0, NAN, 0], [0, 0.5, 0], [0, -1, 0]], [1, 1, 1], [1, 1, 1], 3, [0], [2], 0, 9,
     [NAN], [NAN]),
    ("a later NaN poisons the sum, never the minimum", [[0, 0.5, 0], [0, NAN, 0], [0, -1, 0]], [1, 1, 1], [1, 1, 1], 3,
     [0], [2], 0, 9, [NAN], [-2.0]),
    ("-inf logit", [[0, 0.5, 0], [0, -INF, 0], [0, -1, 0]], [1, 1, 1], [1, 1, 1], 3, [0], [2], 0, 9, [-INF], [-INF]),
    ("+inf logit under a finite normaliser", [[0, 0.5, 0], [0, INF, 0], [0, -1, 0]], [1, 1, 1], [1, 1, 1], 3,
     [0], [2], 0, 9, [INF], [-2.0]),
    ("+inf logit under its own normaliser: inf - inf", [[0, 0.5, 0], [0, INF, 0], [0, -1, 0]], [1, INF, 1], [1, 1, 1], 3,
     [0], [2], 0, 9, [NAN], [-2.0]),
    ("+inf then -inf", [[0, INF, 0], [0, -INF, 0]], [1, 1], [1, 1], 2, [0], [1], 0, 9, [NAN], [-INF]),
    ("one-frame tokens", [[0, 0.5, 0], [0, 0, 0.25], [0, -1, 0]], [1, 1, 1], [1, 2, 1], 3, [0, 1, 2], [0, 1, 2], 0, 9,
     [-0.5, -0.75, -2.0], [-0.5, -0.75, -2.0]),
    ("an untimed token", [[0, 0.5, 0], [0, 0, 0.25], [0, -1, 0]], [1, 1, 1], [2, 1], 3, [-1, 1, 2], [-1, 1, 2], 0, 9,
     [NAN, -0.75, -2.0], [NAN, -0.75, -2.0]),
    ("a merged token reads the blank between its runs", [[7, 0.5, 0], [-0.25, 7, 7], [7, -1, 0]], [1, 1, 1], [1, 9, 1], 3,
     [0], [2], 0, 9, [-3.75], [-2.0]),
    ("blank_label == blank_index", [[7, 0.5, 0], [7, 7, -0.25], [7, -1, 0]], [1, 1, 1], [1, 2, 1], 3,
     [0], [2], 2, 2, [-3.75], [-2.0]),
    ("an alignment shorter than its item", [[7, 7, 7], [7, 7, 7], [0, 0.5, 0], [0.25, 0, 0], [0, 0, -1]], [9, 9, 1, 1, 1],
     [1, 9, 2], 5, [2, 4], [2, 4], 0, 9, [-0.5, -2.0], [-0.5, -2.0]),
    ("m = 0", [[0, 0, 0]], [1], [9], 1, [], [], 0, 9, [], []),
    # what the kernel refuses, the host definition refuses too
    ("a span outside the walk", [[0, 0, 0], [0, 0.5, 0]], [1, 1], [1], 2, [0, 1, 1, -7], [1, 2, 0, 1], 0, 9,
     [NAN, NAN, NAN, NAN], [NAN, NAN, NAN, NAN]),
    ("a value that is no class", [[0, 0, 0], [0, 0.5, 0]], [1, 1], [5, 1], 2, [0, 1], [1, 1], 0, 9,
     [NAN, -0.5], [NAN, -0.5]),
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("row", HAND, ids=[r[0] for r in HAND])
def test_hand_written_rows(row, dtype):
    name, x, norm, ali, frames, start, end, bi, bl, lsum, lmin = row
    x = np.asarray(x, dtype).reshape(frames, 3)
    norm = np.asarray(norm, dtype)
    if not name.startswith(("a span outside", "a value that is no")):
        # the expectations above are hand-derived; the restatement agrees with them
        with np.errstate(invalid="ignore"):
            s, mn = token_scores(x, norm, ali, frames, start, end, bi, bl, dtype)
        _same(np.asarray(s, dtype), lsum, name + ": restatement sum")
        _same(np.asarray(mn, dtype), lmin, name + ": restatement min")
    s, mn = ctcext_amd.token_scores_row(x, norm, ali, frames, start, end, bi, bl)
    assert s.dtype == dtype and mn.dtype == dtype
    _same(s, lsum, name + ": sum")
    _same(mn, lmin, name + ": min")


def test_row_function_refuses_bad_arguments():
    x, norm = np.zeros((2, 3), np.float32), np.ones((2,), np.float32)
    for kw in (dict(blank_index=3), dict(blank_index=-1), dict(alignment=[1, 1, 1])):
        a = dict(alignment=[1, 1], frames=2, start=[0], end=[1], blank_index=0, blank_label=9)
        a.update(kw)
        with pytest.raises(ctcext_amd.InvalidArgumentError):
            ctcext_amd.token_scores_row(x, norm, **a)


# ---- the input cases of tests/test_gpu_token_scores.py have the properties it relies on

def test_neg_inf_cases_hold_nan_cells_inside_a_decoded_row():
    for shape in sorted(NEG_INF_SEEDS):
        x, sl, kw, (dec, ali, times, scores) = family_case("neg_inf", shape, True)
        assert nan_cells_inside_decoded_length(dec, scores) >= 1, shape


def test_tiled_cases_cross_a_tile_and_the_order_of_the_sum_shows():
    """Every tiled case holds scored spans across a multiple of the kernel's
    tile.  On the two sticky cases every float32 sum is exact in any order (see
    tiled_case); on the soft one, sums of tile-crossing tokens differ from their
    terms added in descending order."""
    tile = _lib.load().ctcext_token_scores_tile()
    assert tile == 256   # (the cases were picked for this tile; another needs other seeds)
    for shape in TILED:
        crossing, differ = tile_properties(tiled_case(shape), tile)
        assert crossing >= 1 and differ == 0, (shape, crossing, differ)
    crossing, differ = tile_properties(tiled_case(TILED[0], True), tile)
    assert crossing >= 1 and differ >= 1, (crossing, differ)


def test_skip_case_drops_frames_inside_a_scored_span():
    T, B, C, W, P = SKIP_SHAPE
    spans, fewer, dominant = skip_properties(skip_case())
    assert spans >= 1 and fewer == B and dominant >= 3, (spans, fewer, dominant)


# ---- symbols; calls without a decode

def test_symbols_and_exports():
    lib = _lib.load()
    for s in _lib.TOKEN_SCORES_SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.ctcext_token_scores_tile() >= 64
    assert lib.ctcext_abi_version() == 8
    assert ctcext_amd.TokenScores._fields == ("logp_sum", "logp_min")
    assert not any(s.startswith("ctcext_stream") for s in _lib.TOKEN_SCORES_SYMBOLS)   # streams keep no logits
    # the existing tuples are as they were
    assert ctcext_amd.TokenTimes._fields == ("start", "end", "trailing_blank")
    assert len(ctcext_amd.DenseDecode._fields) == 6 and len(ctcext_amd.StreamDense._fields) == 9


def test_calls_without_a_decode_fail_precondition():
    """No decode on this thread: the Python entry points answer before any HIP call."""
    import threading
    seen = []

    def run():
        for f in (ctcext_amd.dense_token_scores, ctcext_amd.token_scores):
            try:
                f(device=0)
            except ctcext_amd.FailedPreconditionError as e:
                seen.append(e.message)
    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert seen == ["ctcext_dense_token_scores without a ctcext_decode_dense",
                    "ctcext_fetch_token_scores without a successful ctcext_decode"]
