"""The two traceback kernels against the oracle, by record size.

launch_traceback runs the segmented walk (ctcx_traceback_seg: one block per
item, the records staged through LDS segment by segment) when an item's 2 * P
walkers fit one block and a segment holds at least one frame, and the
one-thread-per-walk kernel (ctcx_traceback) otherwise, or always with
CTCEXT_TRACEBACK=0 (read every call).  Both read 4-byte records (the two-wave
kernels at C <= 64), 8-byte ones and the global-state tier's 16-byte ones,
direct or through the record ring's frame offsets.  ctcext_stats.kernel says
which walk ran; the decoded and alignment sequences are the walk's output, so
parity with the oracle checks it.
"""
import numpy as np
import pytest

import ctcext_amd
from ctcext_amd import _lib
from parity_util import compare
import oracle

pytestmark = pytest.mark.gpu

GS = _lib.CTCEXT_FLAG_GLOBAL_STATE
RING = _lib.CTCEXT_FLAG_RECORD_RING
RMIN = _lib.CTCEXT_FLAG_RING_MIN
NORING = _lib.CTCEXT_FLAG_NO_RING

_cache = {}


def _case(C, W, P, T, lengths):
    """Inputs and the oracle's outputs of a shape, computed once."""
    key = (C, W, P, T, tuple(lengths))
    if key not in _cache:
        rng = np.random.default_rng(1000 * C + 10 * W + T)
        x = rng.standard_normal((T, len(lengths), C)).astype(np.float32)
        sl = np.asarray(lengths, np.int32)
        kw = dict(merge_repeated=True, blank_index=C - 1)
        _cache[key] = (x, sl, kw, oracle.decode(x, sl, W, P, **kw))
    return _cache[key]


def _check(C, W, P, T, lengths, flags, walk, record_bytes=None):
    x, sl, kw, ref = _case(C, W, P, T, lengths)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, flags=flags, **kw)
    st = ctcext_amd.get_decoder(0).last_stats
    assert st["kernel"]["traceback"] == walk, st
    if record_bytes is not None:
        assert st["record_bytes"] == record_bytes, st
    compare(out, ref, P, lp_exact=True)
    return st


# (records, C, W, P, T, flags): ragged lengths with a 1-frame item
ONE_THREAD = {
    "rec4_default_ring": (4, 29, 128, 3, 200, 0),
    "rec4_ring_min": (4, 29, 128, 3, 200, RMIN),
    "rec4_no_ring": (4, 29, 128, 3, 200, NORING),
    "rec8_ring": (8, 300, 100, 3, 120, RING),
    "rec8_direct": (8, 300, 100, 3, 120, 0),
    "rec16_global_state": (16, 8, 40, 3, 60, GS),
}


@pytest.mark.parametrize("name", sorted(ONE_THREAD))
def test_one_thread_walk_by_record_size(name, monkeypatch):
    rb, C, W, P, T, flags = ONE_THREAD[name]
    lengths = [T, T // 2 + 1, 1]
    monkeypatch.delenv("CTCEXT_TRACEBACK", raising=False)
    st = _check(C, W, P, T, lengths, flags, "segmented", rb)
    ring = st["ring_frames"]
    monkeypatch.setenv("CTCEXT_TRACEBACK", "0")
    st = _check(C, W, P, T, lengths, flags, "one_thread", rb)
    assert st["ring_frames"] == ring
    if flags & (RING | RMIN):
        assert ring >= 8
    if flags & NORING:
        assert ring == 0


@pytest.mark.parametrize("flags", [0, RMIN], ids=["default", "ring_min"])
def test_segment_of_more_frames_than_its_offsets_hold(flags):
    # W = 2: a 24 KB segment would hold thousands of frames; kTbMaxG = 1024 caps it
    _check(3, 2, 2, 1100, [1100, 1030], flags, "segmented")


@pytest.mark.parametrize("W,walk", [(1535, "segmented"), (1536, "one_thread")])
def test_one_frame_per_segment_and_past_it(W, walk):
    # 16-byte records: W * 16 = kTbBufBytes - 16 is the widest frame a segment holds
    st = _check(5, W, 3, 12, [12, 9], 0, walk, 16)
    assert st["tier"] == 1


def test_more_walkers_than_a_block():
    _check(20, 256, 200, 30, [30, 27], 0, "one_thread", 8)      # 2 * P > 256
    st = _check(8, 600, 300, 12, [12, 9], 0, "one_thread", 16)   # ... on the global-state tier
    assert st["tier"] == 1
