"""The small-C scored helper's two-pass gather (ctcx_decode.hip
gather_small_sparse: the chunks after a frame's first are filtered per scan
step and scored once per chunk), bit-exact against the oracle on all seven
outputs.

Shapes: the beam widths and alphabets at which the gather's index arithmetic
and packing differ (C - 1 = 1, 2, 28 and 63: C = 64 is the last small-C size;
beams that are and are not a multiple of the step).  Logits: N(0, 1) scaled by
0.25 (dense chunks: most scanned offers wanted, chunks fill mid-step), by 3.0
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
SHAPES = [(128, 29), (100, 29), (17, 3), (64, 2), (128, 64)]
KINDS = ["dense", "sparse", "halves"]


def _stats():
    return ctcext_amd.get_decoder(0).last_stats


def _assert_scored_kernel(redecodes=0):
    st = _stats()
    k = st["kernel"]
    assert st["helper"] == 3, st
    assert k["launched"] and k["helper"] == "SQ" and not k["BIG"] and k["RN"] == 1, k
    assert k["dtype"] == "f32" and k["scorer"] == "base" and k["tier"] == 0, k
    assert st["helper_redecodes"] == redecodes, st


_CASES = {}


def _case(W, C, kind, blank):
    """(logits, lengths, oracle outputs), computed once per case and shared."""
    key = (W, C, kind, blank)
    if key not in _CASES:
        rng = np.random.default_rng(7000 + 131 * W + 7 * C + KINDS.index(kind))
        x = rng.standard_normal((T, B, C))
        if kind == "dense":
            x = x * 0.25
        elif kind == "sparse":
            x = x * 3.0
        else:
            x = np.round(x * 2) / 2
        x = x.astype(np.float32)
        x.setflags(write=False)
        sl = np.full(B, T, np.int32)
        ref = oracle.decode(x, sl, W, P, True, blank)
        _CASES[key] = (x, sl, ref)
    return _CASES[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,C", SHAPES)
def test_two_pass_gather(W, C, kind):
    x, sl, ref = _case(W, C, kind, 0)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=0)
    _assert_scored_kernel()
    compare(out, ref, P)


@pytest.mark.parametrize("kind", KINDS)
def test_blank_last(kind):
    W, C = 128, 29
    x, sl, ref = _case(W, C, kind, C - 1)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=C - 1)
    _assert_scored_kernel()
    compare(out, ref, P)


def test_helper_dead_redecodes():
    # the helper starts out timed out: wave 0 ends the grow, the item is decoded again
    W, C = 128, 29
    x, sl, ref = _case(W, C, "sparse", 0)
    with pytest.warns(RuntimeWarning, match="hand-over wait timed out"):
        out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=0,
                                                     flags=_lib.CTCEXT_FLAG_TEST_HELPER_DEAD)
    assert _stats()["helper_redecodes"] == 1, _stats()
    compare(out, ref, P)
    # the handle stays usable, on the scored kernel
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=0)
    _assert_scored_kernel()
    compare(out, ref, P)
