"""Token times without a GPU: ctcext_token_times_row (the host definition
behind ctcext_amd.token_times_row) against the Python restatement of
include/ctcext.h, on the oracle's rows of every input family and on
hand-written rows; the blank_label rule's message; the symbols."""
import functools

import numpy as np
import pytest

import ctcext_amd
from ctcext_amd import _lib
from token_times_util import NEG_INF_SEEDS, expected, family, token_times

# (T, B, C, W, P): the GPU tests' small shapes
SHAPES = [(1, 2, 3, 2, 1), (12, 6, 5, 8, 3), (40, 4, 29, 16, 3), (30, 6, 6, 16, 3)]


@functools.lru_cache(maxsize=None)
def _case(kind, shape, merge):
    T, B, C, W, P = shape
    rng = np.random.default_rng(NEG_INF_SEEDS.get(shape, 11) if kind == "neg_inf" else sum(kind.encode()) + T)
    x = family(rng, kind, T, B, C)
    sl = np.array([T] + [max(T - 1 - 2 * b, 0) for b in range(1, B)], np.int32)
    kw = dict(merge_repeated=merge, blank_index=0, blank_label=-1)
    return sl, kw, expected(x, sl, W, P, T, **kw)


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["gaussian", "peaky", "sticky", "neg_inf"])
def test_row_function_matches_definition_on_oracle_rows(kind, shape, merge):
    T, B, C, W, P = shape
    sl, kw, (dec, ali, (start, end, trail)) = _case(kind, shape, merge)
    for b in range(B):
        for p in range(P):
            s, e, t = ctcext_amd.token_times_row(dec[b][p], ali[b][p], int(sl[b]), -1, merge)
            m = len(dec[b][p])
            assert s.dtype == np.int32 and e.dtype == np.int32 and s.shape == (m,)
            np.testing.assert_array_equal(s, start[b, p, :m], err_msg="start %d %d" % (b, p))
            np.testing.assert_array_equal(e, end[b, p, :m], err_msg="end %d %d" % (b, p))
            assert t == trail[b, p], (b, p)
            # the properties the definition promises
            timed = np.flatnonzero(s >= 0)
            assert (np.flatnonzero(e >= 0) == timed).all()
            if timed.size:
                assert timed[-1] == m - 1 and (np.diff(timed) == 1).all()   # a suffix
                assert (np.diff(s[timed]) > 0).all() and (s[timed] <= e[timed]).all()
                assert e[timed].max() < sl[b] and s[timed].min() >= 0


def test_neg_inf_family_has_short_alignments_and_untimed_tokens():
    """The case the GPU tests rely on, checked on the oracle's own rows."""
    for shape in sorted(NEG_INF_SEEDS):
        T, B, C, W, P = shape
        sl, kw, (dec, ali, (start, end, trail)) = _case("neg_inf", shape, True)
        short = sum(len(ali[b][p]) < sl[b] for b in range(B) for p in range(P))
        tokens = sum(len(dec[b][p]) for b in range(B) for p in range(P))
        untimed = sum(int((start[b, p, :len(dec[b][p])] < 0).sum()) for b in range(B) for p in range(P))
        assert short >= 1 and 1 <= untimed < tokens, (shape, short, untimed, tokens)


B_ = 9   # the hand-written rows' blank_label

# (name, decoded, alignment, frames, merge, start, end, trailing_blank)
HAND = [
    ("empty alignment", [1, 2], [], 5, False, [-1, -1], [-1, -1], 0),
    ("all blank", [1], [B_, B_, B_], 3, False, [-1], [-1], 3),
    ("shorter than frames", [1, 2], [1, B_, 2, 2, B_], 9, False, [4, 6], [4, 7], 1),
    # the restart cut the first run: what is left of it is the token's span
    ("first run cut", [3, 1], [3, B_, 1, 1], 10, False, [6, 8], [6, 9], 0),
    ("mismatch in the middle", [1, 2, 3], [1, 1, 4, B_, 3], 5, False, [-1, -1, 4], [-1, -1, 4], 0),
    ("mismatch at the end", [1, 2], [1, 3], 2, False, [-1, -1], [-1, -1], 0),
    ("m = 0", [], [B_, 1, B_], 3, False, [], [], 1),
    ("merged token of three runs", [2, 1], [2, B_, 1, 1, B_, B_, 1, B_, 1, B_], 10, True, [0, 2], [0, 8], 1),
    ("the same rows unmerged", [2, 1, 1, 1], [2, B_, 1, 1, B_, B_, 1, B_, 1, B_], 10, False,
     [0, 2, 6, 8], [0, 3, 6, 8], 1),
    ("more runs than tokens", [1], [2, 1], 2, False, [1], [1], 0),
    ("more tokens than runs", [5, 1, 2], [1, 2], 2, False, [-1, 0, 1], [-1, 0, 1], 0),
    ("merged repeat that is two tokens", [1, 1], [1, B_, 1], 3, True, [-1, 0], [-1, 2], 0),
    ("blank_label that occurs nowhere", [1, 2], [1, 1, 2], 3, False, [0, 2], [1, 2], 0),
]


@pytest.mark.parametrize("row", HAND, ids=[r[0] for r in HAND])
def test_hand_written_rows(row):
    name, dec, ali, frames, merge, start, end, trail = row
    # the expectations above are hand-derived; the restatement agrees with them
    assert token_times(dec, ali, frames, B_, merge) == (start, end, trail), name
    s, e, t = ctcext_amd.token_times_row(dec, ali, frames, B_, merge)
    assert (s.tolist(), e.tolist(), t) == (start, end, trail), name


def test_blank_label_rule_message():
    lib = _lib.load()
    msg = "token times need a blank_label that is no class label"
    for C, bi, bl, ok in ((5, 0, -1, True), (5, 0, 5, True), (5, 2, 2, True), (5, 0, 9, True),
                          (5, 0, 3, False), (5, 2, 0, False), (5, 4, 3, False)):
        rc = lib.ctcext_token_times_validate(C, bi, bl)
        if ok:
            assert rc == _lib.CTCEXT_OK and lib.ctcext_last_error().decode() == "", (C, bi, bl)
        else:
            assert rc == _lib.CTCEXT_INVALID_ARGUMENT and lib.ctcext_last_error().decode() == msg, (C, bi, bl)


def test_symbols_and_exports():
    lib = _lib.load()
    for s in _lib.TOKEN_TIMES_SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.ctcext_token_times_tile() >= 64
    assert lib.ctcext_abi_version() == 8
    assert ctcext_amd.TokenTimes._fields == ("start", "end", "trailing_blank")
    # the existing tuples are as they were
    assert len(ctcext_amd.DenseDecode._fields) == 6 and len(ctcext_amd.StreamDense._fields) == 9


def test_calls_without_a_decode_fail_precondition():
    """No decode on this thread: the Python entry points answer before any HIP call."""
    import threading
    seen = []

    def run():
        for f in (ctcext_amd.dense_token_times, ctcext_amd.token_times):
            try:
                f(0)
            except ctcext_amd.FailedPreconditionError as e:
                seen.append(e.message)
    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert seen == ["ctcext_dense_token_times without a ctcext_decode_dense",
                    "ctcext_fetch_token_times without a successful ctcext_decode"]
