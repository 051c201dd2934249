"""The small-C scored helper's branch-per-lane filter (ctcx_decode.hip
gather_small_branch: pass 1 of the chunks after a frame's first, one branch
per lane, 64 branches per window), bit-exact against the oracle on all seven
outputs.

Shapes: beams of exactly one window (64), one more (65: a second window of one
branch), a partial second window (100) and two full ones (128); C - 1 = 1
(one label per branch), 2, 28 and 63 (the full 64-bit mask).  The blank first,
last and at a middle index (the label index skips it).  Merge on and off.
Logits: N(0, 1) scaled by 0.25 (dense chunks that fill mid-step), by 3.0
(sparse late chunks, a turn closed at the helper's bottom early in the frame)
and rounded to halves (ties, twin lines and re-offers).

Every case first checks that the kernel under test ran: two-wave, scored,
small C, float, base scorer, no re-decode.
"""
import numpy as np
import pytest

import ctcext_amd
import oracle
from ctcext_amd import _lib
from parity_util import compare

pytestmark = pytest.mark.gpu

B, T, P = 4, 48, 2
SHAPES = [(128, 29), (100, 29), (65, 29), (64, 29), (17, 3), (64, 2), (128, 64)]
KINDS = ["dense", "sparse", "halves"]
BLANKS = ["first", "middle", "last"]


def _stats():
    return ctcext_amd.get_decoder(0).last_stats


def _assert_scored_kernel(redecodes=0):
    st = _stats()
    k = st["kernel"]
    assert st["helper"] == 3, st
    assert k["launched"] and k["helper"] == "SQ" and not k["BIG"] and k["RN"] == 1, k
    assert k["dtype"] == "f32" and k["scorer"] == "base" and k["tier"] == 0, k
    assert st["helper_redecodes"] == redecodes, st


_INPUTS = {}
_REFS = {}


def _blank(C, at):
    return {"first": 0, "middle": C // 2, "last": C - 1}[at]


def _case(W, C, kind, blank, merge):
    """(logits, lengths, oracle outputs), computed once per case and shared."""
    ik = (W, C, kind)
    if ik not in _INPUTS:
        rng = np.random.default_rng(1900 + 131 * W + 7 * C + KINDS.index(kind))
        x = rng.standard_normal((T, B, C))
        if kind == "dense":
            x = x * 0.25
        elif kind == "sparse":
            x = x * 3.0
        else:
            x = np.round(x * 2) / 2
        x = x.astype(np.float32)
        x.setflags(write=False)
        _INPUTS[ik] = (x, np.full(B, T, np.int32))
    x, sl = _INPUTS[ik]
    rk = ik + (blank, merge)
    if rk not in _REFS:
        _REFS[rk] = oracle.decode(x, sl, W, P, merge, blank)
    return x, sl, _REFS[rk]


@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("blank_at", BLANKS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,C", SHAPES)
def test_branch_gather(W, C, kind, blank_at, merge):
    blank = _blank(C, blank_at)
    x, sl, ref = _case(W, C, kind, blank, merge)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=merge, blank_index=blank)
    _assert_scored_kernel()
    compare(out, ref, P)


def test_helper_dead_redecodes():
    # the helper starts out timed out: wave 0 ends the grow, the item is decoded again
    W, C = 100, 29
    x, sl, ref = _case(W, C, "sparse", 0, True)
    with pytest.warns(RuntimeWarning, match="hand-over wait timed out"):
        out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=0,
                                                     flags=_lib.CTCEXT_FLAG_TEST_HELPER_DEAD)
    assert _stats()["helper_redecodes"] == 1, _stats()
    compare(out, ref, P)
    # the handle stays usable, on the scored kernel
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=0)
    _assert_scored_kernel()
    compare(out, ref, P)
