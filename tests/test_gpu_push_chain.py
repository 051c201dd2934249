"""The TopN push loop of the float kernels for beams of up to 128
(heap_events_f32 in ctcx_decode.hip: the stop found per lane, two push bodies
per loop trip, an evicted-branch stub per body), all seven outputs bit-exact
against the oracle -- log-probabilities included.

Beam widths: the smallest heaps (2, 3), and the widths either side of the
positions that change role in the one-node-per-lane form -- lane 31, whose
right child (position 64) is the first child that is not a lane; lanes 32..63,
which always stop; the last lane node (63) and the last position a lane reads
(128).  With B = 4 and T = 48 the frames' push counts are odd and even alike,
so the loop leaves through either body, and merge_repeated on and off changes
which entries are branch children, so evicted branch entries come up in both
bodies.  Class counts 3, 29 and 64: one chunk that is never full, the
flagship's, and the last small-C count (a full 64-lane chunk per beam).
Logits: N(0, 1); a grid of four values, so that equal totals fill the heap and
the pushes' order among them is the layout's; peaky frames (one class far
above the rest), where few offers beat the front.  One case more runs the
bigram scorer's kernels at W = 128.
"""
import numpy as np
import pytest

import ctcext_amd
import oracle
import scorer_tables
from parity_util import compare

pytestmark = pytest.mark.gpu

T, B = 48, 4
WIDTHS = [2, 3, 31, 32, 33, 63, 64, 65, 127, 128]
CLASSES = [3, 29, 64]
KINDS = ["gaussian", "grid4", "peaky"]

_LOGITS = {}


def _logits(kind, C):
    key = (kind, C)
    if key not in _LOGITS:
        rng = np.random.default_rng(2600 + 100 * KINDS.index(kind) + C)
        if kind == "grid4":
            x = rng.integers(0, 4, size=(T, B, C)).astype(np.float32) * np.float32(0.5)
        else:
            x = rng.standard_normal((T, B, C)).astype(np.float32)
            if kind == "peaky":
                top = rng.integers(0, C, size=(T, B))
                np.put_along_axis(x, top[..., None], np.float32(8.0), axis=2)
        x.setflags(write=False)
        _LOGITS[key] = x
    return _LOGITS[key]


def _check(x, W, P, merge, tab=None):
    sl = np.array([T, T, T - 5, T - 16], np.int32)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=merge, scorer_table=tab)
    st = ctcext_amd.get_decoder(0).last_stats
    k = st["kernel"]
    assert k["launched"] and k["dtype"] == "f32" and k["RN"] == 1 and k["tier"] == 0, k
    assert k["scorer"] == ("base" if tab is None else "bigram"), k
    assert st.get("helper_redecodes", 0) == 0, st
    compare(out, oracle.decode(x, sl, W, P, merge, scorer_table=tab), P, lp_exact=True)


@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("W", WIDTHS)
def test_push_chain_matches_oracle(W, C, kind, merge):
    # three paths; two at W = 2, where the op rejects more paths than the beam is wide
    _check(_logits(kind, C), W, min(3, W), merge)


@pytest.mark.parametrize("tkind,kind", [("continuous", "gaussian"), ("grid", "grid4")])
def test_push_chain_bigram_scorer(tkind, kind):
    tab = scorer_tables.table(np.random.default_rng(26), tkind, 29, np.float32)
    _check(_logits(kind, 29), 128, 3, True, tab)
