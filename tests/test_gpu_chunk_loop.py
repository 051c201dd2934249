"""The scored two-wave kernel's chunk loop at small C (ctcx_decode.hip
exact_step, kSqLoop: wave 0 stays in one loop across a frame's scored chunks,
the helper packs each offer's turn-start lane) and its make_heap in the mask
form (wave_make_heap_m, once per frame), bit-exact against the oracle
-- log-probabilities included -- at the smallest shapes that cross every edge
of that loop: many chunks per frame, full chunks with every offer wanted, one
short chunk and grows that end at the helper's stale-bottom stop, ties through
the chunk boundary, re-offers / deactivations / turns closing mid-chunk,
literal frames in between, ragged lengths, and a helper that starts dead.

Every test first checks that the kernel under test ran: helper kind 3 and the
ABI-8 kernel fields saying two-wave, scored, small C, float, base scorer.
"""
import numpy as np
import pytest

import ctcext_amd
import oracle
from ctcext_amd import _lib
from parity_util import compare, oracle_or_error, random_case

pytestmark = pytest.mark.gpu

C = 29


def _stats():
    return ctcext_amd.get_decoder(0).last_stats


def _assert_scored_kernel():
    st = _stats()
    k = st["kernel"]
    assert st["helper"] == 3, st
    assert k["launched"] and k["helper"] == "SQ" and not k["BIG"] and k["RN"] == 1, k
    assert k["dtype"] == "f32" and k["scorer"] == "base" and k["tier"] == 0, k
    assert st["helper_redecodes"] == 0, st


_LOGITS = {}


def _logits(seed, T, B, scale=1.0, halves=False, neg_inf=False):
    key = (seed, T, B, scale, halves, neg_inf)
    if key not in _LOGITS:
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal((T, B, C)) * scale).astype(np.float32)
        if halves:
            x = (np.round(x * 2) / 2).astype(np.float32)
        if neg_inf:
            x[rng.random(x.shape) < 0.15] = -np.inf
        x.setflags(write=False)
        _LOGITS[key] = x
    return _LOGITS[key]


_REFS = {}


def _check(x, sl, W, P, merge, key=None):
    sl = np.asarray(sl, np.int32)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=merge)
    _assert_scored_kernel()
    if key is None or key not in _REFS:
        ref = oracle.decode(x, sl, W, P, merge)
        if key is not None:
            _REFS[key] = ref
    else:
        ref = _REFS[key]
    compare(out, ref, P)


def test_smallest():
    # one item, a beam that fills within a few frames, two or three chunks per frame
    x = _logits(11, 12, 1)
    _check(x, [12], 16, 1, True)


@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("W", [16, 64, 127, 128])
def test_many_chunks_per_frame(W, P, merge):
    x = _logits(20, 48, 3)
    _check(x, [48, 48, 48], W, P, merge)


@pytest.mark.parametrize("P", [1, 3])
def test_full_chunks_every_offer_wanted(P):
    # near-flat logits: every branch's children score alike, the chunks come full
    x = _logits(21, 48, 3, scale=0.05)
    _check(x, [48, 48, 48], 128, P, True)


@pytest.mark.parametrize("P", [1, 3])
def test_short_chunk_and_stale_bottom_stop(P):
    # peaked logits: few offers beat the bottom, one short chunk per frame, and
    # the helper's gather ends the grow at a turn closed by its (stale) bottom
    x = _logits(22, 48, 3, scale=4.0)
    _check(x, [48, 48, 48], 128, P, True)


@pytest.mark.parametrize("merge", [True, False])
def test_ties_through_the_chunk_boundary(merge):
    # logits rounded to halves: evictions among equal minima, twin lines
    x = _logits(23, 60, 3, halves=True)
    _check(x, [60, 60, 60], 128, 3, merge)


def test_every_beam_width():
    # the frame's make_heap runs in the mask form (wave_make_heap_m) over
    # W + 1 elements: every length, odd and even (a last node with one
    # child), with and without tied totals
    for halves in (False, True):
        x = _logits(26, 10, 2, halves=halves)
        for W in range(1, 129):
            _check(x, [10, 9], W, 1, True)


def test_rare_exits():
    # tiny alphabets and beams with ties: branch evictions, re-offers,
    # deactivations and turns closing mid-chunk (test_gpu_helper_modes' 9306 family)
    x0 = _logits(11, 12, 1)
    ctcext_amd.ctc_ext_beam_search_decoder(x0, np.asarray([12], np.int32), 16, 1)
    _assert_scored_kernel()
    rng = np.random.default_rng(9406)
    for it in range(100):
        x, sl, W, P, kw = random_case(rng, T_max=60, B_max=3, C_max=6, W_max=10, ties=True)
        ref, rerr = oracle_or_error(x, sl, W, P, kw)
        try:
            out, gerr = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, **kw), None
        except ctcext_amd.OpError as e:
            out, gerr = None, e.message
        assert rerr == gerr, (it, rerr, gerr)
        if gerr is None:
            assert _stats()["helper"] == 3, (it, _stats())
            if _stats()["kernel"]["launched"]:
                _assert_scored_kernel()
        if ref is not None:
            compare(out, ref, P)


@pytest.mark.parametrize("W", [16, 128])
def test_leaving_and_reentering_the_loop(W):
    # -inf logits: literal frames, and a beam that empties and refills mid-item
    x = _logits(24, 48, 3, neg_inf=True)
    sl = np.asarray([48, 48, 48], np.int32)
    kw = dict(merge_repeated=True)
    ref, rerr = oracle_or_error(x, sl, W, 3, kw)
    try:
        out, gerr = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, 3, **kw), None
    except ctcext_amd.OpError as e:
        out, gerr = None, e.message
    _assert_scored_kernel()
    assert rerr == gerr, (rerr, gerr)
    if ref is not None:
        compare(out, ref, 3)


def test_ragged_seq_len():
    x = _logits(20, 48, 3)
    x4 = np.concatenate([x, x[:, :1]], axis=1)
    _check(x4, [1, 48, 23, 47], 128, 3, True)
    # (an empty item has one leaf: top_paths 1)
    _check(x4, [48, 0, 1, 47], 128, 1, True)
    _check(x4, [0, 48, 1, 2], 64, 1, False)


DEAD = _lib.CTCEXT_FLAG_TEST_HELPER_DEAD


def test_helper_started_dead():
    x = _logits(25, 30, 3)
    sl = np.full(3, 30, np.int32)
    _check(x, sl, 128, 3, True, key="dead")
    with pytest.warns(RuntimeWarning, match="hand-over wait timed out"):
        out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, 128, 3, merge_repeated=True, flags=DEAD)
    assert _stats()["helper_redecodes"] == 1, _stats()
    compare(out, _REFS["dead"], 3)
    with pytest.raises(ctcext_amd.InternalError) as ei:
        ctcext_amd.ctc_ext_beam_search_decoder(x, sl, 128, 3, merge_repeated=True,
                                               flags=DEAD | _lib.CTCEXT_FLAG_HELPER_STRICT)
    assert ei.value.error_code == _lib.CTCEXT_INTERNAL
    assert "hand-over wait timed out" in str(ei.value)
    # the handle stays usable, on the scored kernel
    _check(x, sl, 128, 3, True, key="dead")
