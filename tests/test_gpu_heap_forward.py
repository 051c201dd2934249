"""The scored two-wave float kernel's sort_heap with the heap's child pairs
carried in registers from pop to pop (extract_fwd_f32 in ctcx_decode.hip),
bit-exact against the oracle -- log-probabilities included -- at the beam
widths where a heap position changes role in the one-node-per-lane form:
node 31's right child (position 64, the first child that is not a lane), the
first node without lane children (32), the last lane node (63), the last
position a lane reads (128), and the smallest heaps.  N(0,1) logits, and
logits quantised to halves so that equal totals fill the heap and the pops'
order among them is the layout's.  One longer item at W = 128 lets twin lines
form, so the extract pops through ties at the top of the heap.

Every case first checks that the kernel under test ran (two-wave, scored,
small C, float, base scorer) and that no item was decoded again.
"""
import numpy as np
import pytest

import ctcext_amd
import oracle
from parity_util import compare

pytestmark = pytest.mark.gpu

C = 29
WIDTHS = [2, 3, 31, 32, 33, 63, 64, 65, 127, 128]


def _assert_scored_float_kernel():
    st = ctcext_amd.get_decoder(0).last_stats
    k = st["kernel"]
    assert st["helper"] == 3, st
    assert k["launched"] and k["helper"] == "SQ" and not k["BIG"] and k["RN"] == 1, k
    assert k["dtype"] == "f32" and k["scorer"] == "base" and k["tier"] == 0, k
    assert st["helper_redecodes"] == 0, st


_LOGITS = {}


def _logits(seed, T, B, halves):
    key = (seed, T, B, halves)
    if key not in _LOGITS:
        x = np.random.default_rng(seed).standard_normal((T, B, C)).astype(np.float32)
        if halves:
            x = (np.round(x * 2) / 2).astype(np.float32)
        x.setflags(write=False)
        _LOGITS[key] = x
    return _LOGITS[key]


def _check(x, W, P, merge):
    sl = np.full(x.shape[1], x.shape[0], np.int32)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=merge)
    _assert_scored_float_kernel()
    compare(out, oracle.decode(x, sl, W, P, merge), P)


@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("halves", [False, True])
@pytest.mark.parametrize("W", WIDTHS)
def test_role_changing_widths(W, halves, merge):
    # three paths; two at W = 2, where the op rejects more paths than the beam is wide
    _check(_logits(31, 48, 4, halves), W, min(3, W), merge)


@pytest.mark.parametrize("halves", [False, True])
def test_long_item_ties_at_the_top(halves):
    _check(_logits(32, 400, 2, halves), 128, 3, True)
