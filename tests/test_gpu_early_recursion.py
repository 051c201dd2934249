"""The next frame's recursion on the helper wave (round 17: CTCX_EARLY_RECURSE,
ctcx_decode.hip help_early_recurse) of the small-C scored two-wave float
kernel.  While wave 0 extracts frame t, the helper computes frame t + 1's
recursion from the final beam, in slot space, and the commit moves the staged
words into place; frame t + 1 then skips wave 0's recursion.  All seven
outputs bit-exact against the oracle, in every case.

ctcext_stats.early_recursed_frames counts, over the items, the frames that
stayed exact and whose recursion came from the helper.  A frame can be one
only if the frame before it started with a full beam and stayed exact, so a
bound follows from the shapes alone: the beam after t frames holds at most
sum_{k <= t} (C - 1)^k prefixes, which first reaches W at t = f0(W, C); the
frame that fills the beam is replayed literally or ends with it just full, so
no frame before f0 + 1 is early, and an item of n frames has at most
max(n - f0 - 1, 0) of them (_bound).  The counter must also be large where the
path is meant to run: at least half of the items' frames on the untied input
families (a case that passes with the path mostly idle proves nothing about
it).

CTCEXT_EARLY_RECURSE=0 in the environment (read at launch; diagnostics) turns
the staging off for a call: the counter is 0 and the outputs are the same.
"""
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
import oracle
from ctcext_amd import _lib
from parity_util import compare
from test_gpu_dense import to_dense
from test_gpu_early_chunk import _draw as _ec_draw, _huge_frame

pytestmark = pytest.mark.gpu

B, T, P = 4, 48, 2
SHAPES = [(128, 29), (100, 29), (64, 29), (16, 6)]
KINDS = ["x3", "x8", "peaked_flat", "halves"]
UNTIED = ("x3", "x8", "peaked_flat")
DEV = "cuda:0"


def _stats():
    return ctcext_amd.get_decoder(0).last_stats


def _assert_scored_kernel(redecodes=0, st=None, stream=False):
    st = st or _stats()
    k = st["kernel"]
    assert st["helper"] == 3, st
    assert k["launched"] and k["helper"] == "SQ" and not k["BIG"] and k["RN"] == 1 and k["WC"] == 128, k
    assert k["dtype"] == "f32" and k["scorer"] == "base" and k["tier"] == 0, k
    assert bool(k["stream"]) == stream, k
    assert st["helper_redecodes"] == redecodes, st


def _f0(W, C):
    """The first frame that can start with W leaves (module docstring)."""
    n, t = 1, 0
    while n < W:
        t += 1
        n += (C - 1) ** t
    return t


def _bound(W, C, lengths):
    f0 = _f0(W, C)
    return int(sum(max(int(n) - f0 - 1, 0) for n in lengths))


def _draw(seed, kind, C, shape=(T, B)):
    rng = np.random.default_rng(17000 + seed)
    x = rng.standard_normal(shape + (C,))
    if kind == "halves":
        x = np.round(x * 2) / 2
    elif kind == "peaked_flat":
        x[0::2] *= 8.0
        x[1::2] *= 0.05
    else:
        x = x * {"x3": 3.0, "x8": 8.0, "x0.25": 0.25}[kind]
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(W, C, kind, blank, seed=0):
    """(logits, lengths, oracle outputs), computed once per case and shared."""
    x = _draw(seed, kind, C)
    x.setflags(write=False)
    sl = np.full(B, T, np.int32)
    return x, sl, oracle.decode(x, sl, W, P, True, blank)


def _decode(x, sl, W, blank=0, paths=P, **kw):
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, paths, merge_repeated=True, blank_index=blank, **kw)
    return out, dict(_stats())


def _decode_off(monkeypatch, x, sl, W, blank=0, paths=P):
    """The same call with the staging forced off."""
    with monkeypatch.context() as m:
        m.setenv("CTCEXT_EARLY_RECURSE", "0")
        out, st = _decode(x, sl, W, blank, paths)
    assert st["early_recursed_frames"] == 0, st
    return out, st


# ---------------------------------------------------------------------------
# 1. shapes and inputs

@pytest.mark.parametrize("blank", ["first", "last"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,C", SHAPES)
def test_shapes_and_inputs(W, C, kind, blank, monkeypatch):
    monkeypatch.delenv("CTCEXT_EARLY_RECURSE", raising=False)
    bi = 0 if blank == "first" else C - 1
    x, sl, ref = _case(W, C, kind, bi)
    out, st = _decode(x, sl, W, bi)
    _assert_scored_kernel()
    compare(out, ref, P)
    early, hi = st["early_recursed_frames"], _bound(W, C, sl)
    print("W=%d C=%d %s blank=%d: early-recursed %d of %d frames (bound %d), literal %d"
          % (W, C, kind, bi, early, B * T, hi, st["literal_frames"]))
    assert 0 < early <= hi, (early, hi)
    if kind in UNTIED:
        assert 2 * early >= B * T, (early, B * T)
    off, st0 = _decode_off(monkeypatch, x, sl, W, bi)
    _assert_scored_kernel()
    compare(off, ref, P)
    assert st0["literal_frames"] == st["literal_frames"], (st0, st)


# ---------------------------------------------------------------------------
# 2. a surviving branch whose parent had left the beam and re-enters it as a
# new child, in a frame whose successor is early-recursed

def _beams(x, b, W, blank):
    """The beam after t frames of item b, t = 1..T, as label tuples (the
    oracle's W best prefixes, unmerged); frames with fewer than W leaves are
    left out."""
    out = {}
    for t in range(1, x.shape[0] + 1):
        try:
            dec = oracle.raw_decode(np.ascontiguousarray(x[:t, b:b + 1]), [t], W, W, False, blank)[0][0]
        except oracle.OracleError:
            continue
        out[t] = {tuple(s) for s in dec}
    return out


def _reentered_parents(x, W, blank):
    """Oracle calls only.  Frame t (0-based) starts from the beam after t
    frames and ends with the beam after t + 1.  Counted: prefixes in both,
    whose parent prefix is not in the first (the branch has no parent link)
    and is in the second (it came back, as a new child of its own parent),
    over the full-beam frames t that have a frame after them."""
    n = 0
    for b in range(x.shape[1]):
        bm = _beams(x, b, W, blank)
        for t in sorted(bm):
            if t + 1 not in bm or t + 1 >= x.shape[0]:
                continue
            cur, nxt = bm[t], bm[t + 1]
            n += sum(1 for s in cur & nxt if len(s) >= 1 and s[:-1] not in cur and s[:-1] in nxt)
    return n


# (W, C, family, seed): found by searching seeds with _reentered_parents alone
REENTERED = [(16, 6, "peaked_flat", 0), (64, 29, "peaked_flat", 1), (16, 6, "halves", 0)]


@pytest.mark.parametrize("W,C,kind,seed", REENTERED)
def test_reentered_parent(W, C, kind, seed, monkeypatch):
    monkeypatch.delenv("CTCEXT_EARLY_RECURSE", raising=False)
    x, sl, ref = _case(W, C, kind, 0, seed)
    n = _reentered_parents(x, W, 0)
    print("re-entered parents W=%d C=%d %s seed %d: %d" % (W, C, kind, seed, n))
    assert n > 0
    out, st = _decode(x, sl, W)
    _assert_scored_kernel()
    compare(out, ref, P)
    assert 0 < st["early_recursed_frames"] <= _bound(W, C, sl), st


# ---------------------------------------------------------------------------
# 3. fallbacks

def test_ragged_lengths_nan_past_the_end(monkeypatch):
    """No staging at an item's last frame: the rows past each length are NaN,
    and a recursion staged from one would make the frame count differ from the
    call with the staging off."""
    monkeypatch.delenv("CTCEXT_EARLY_RECURSE", raising=False)
    W, C = 128, 29
    x = _draw(3, "x3", C).copy()
    sl = np.array([0, 1, 7, T], np.int32)
    for b, n in enumerate(sl):
        x[n:, b] = np.nan
    ref = oracle.decode(x, sl, W, 1, True, 0)
    out, st = _decode(x, sl, W, paths=1)
    _assert_scored_kernel()
    compare(out, ref, 1)
    hi = _bound(W, C, sl)
    print("ragged: early-recursed %d (bound %d), literal %d" % (st["early_recursed_frames"], hi, st["literal_frames"]))
    assert 0 < st["early_recursed_frames"] <= hi, (st, hi)
    off, st0 = _decode_off(monkeypatch, x, sl, W, paths=1)
    compare(off, ref, 1)
    assert st0["literal_frames"] == st["literal_frames"], (st0, st)


def test_plus_inf_row_mid_sequence(monkeypatch):
    """A +inf logit in frame 20 of item 1: that frame's recursion is staged
    (frame 19 is exact) and placed, then the row test sends the frame to the
    literal path, which rolls and recurses by itself; every later frame of the
    item is literal too (NaN totals).  None of them counts."""
    monkeypatch.delenv("CTCEXT_EARLY_RECURSE", raising=False)
    W, C, t0 = 128, 29, 20
    x = _draw(4, "x3", C).copy()
    sl = np.full(B, T, np.int32)
    x[t0, 1, C // 2] = np.inf
    ref = oracle.decode(x, sl, W, P, True, 0)
    out, st = _decode(x, sl, W)
    _assert_scored_kernel()
    compare(out, ref, P)
    hi = _bound(W, C, [T, t0, T, T])
    print("+inf: early-recursed %d (bound %d), literal %d" % (st["early_recursed_frames"], hi, st["literal_frames"]))
    assert 0 < st["early_recursed_frames"] <= hi, (st, hi)
    off, st0 = _decode_off(monkeypatch, x, sl, W)
    compare(off, ref, P)
    assert st0["literal_frames"] == st["literal_frames"] >= T - t0, (st0, st)


def test_nonfinite_total_mid_sequence(monkeypatch):
    """Frame 24 holds rows that pass the row test and give totals of -inf
    (test_gpu_early_chunk._huge_frame).  Its recursion is the helper's, staged
    during frame 23; wave 0's own test of the placed totals sends it to the
    literal path.  Frame 25 follows a literal frame and recurses on wave 0.
    Neither counts: two frames per item off the bound."""
    monkeypatch.delenv("CTCEXT_EARLY_RECURSE", raising=False)
    W, C, t0 = 128, 29, 24
    x = _ec_draw(W, C, "x0.25").copy()
    sl = np.full(B, T, np.int32)
    x[t0] = _huge_frame(x, t0, W, 0)
    ref = oracle.decode(x, sl, W, P, True, 0)
    out, st = _decode(x, sl, W)
    _assert_scored_kernel()
    compare(out, ref, P)
    hi = _bound(W, C, sl) - 2 * B
    print("huge: early-recursed %d (bound %d), literal %d nonfinite %d"
          % (st["early_recursed_frames"], hi, st["literal_frames"], st["literal_nonfinite"]))
    assert 0 < st["early_recursed_frames"] <= hi, (st, hi)
    off, st0 = _decode_off(monkeypatch, x, sl, W)
    compare(off, ref, P)
    assert st0["literal_nonfinite"] == st["literal_nonfinite"] >= B, (st0, st)
    assert st0["literal_frames"] == st["literal_frames"], (st0, st)


@pytest.mark.parametrize("half", ["float16", "bfloat16"])
def test_half_inputs_stay_on_wave0(half, monkeypatch):
    monkeypatch.delenv("CTCEXT_EARLY_RECURSE", raising=False)
    W, C = 128, 29
    xh = torch.as_tensor(_draw(5, "x3", C)).to(getattr(torch, half))
    sl = np.array([T, T - 1, 7, T], np.int32)
    ref = oracle.decode(xh.float().numpy(), sl, W, P, True, 0)
    out = ctcext_amd.decode_logits(xh.cuda(), sl, W, P, batch_first=False, merge_repeated=True, blank_index=0)
    _assert_scored_kernel()
    compare(out, ref, P)
    assert _stats()["early_recursed_frames"] == 0, _stats()


@functools.lru_cache(maxsize=None)
def _dup_cases(n_want=3, max_tries=4000):
    """Seeded single-item -inf-heavy inputs at beams of 16..20 (where the
    helper ranks the extract, so the staging runs) that the oracle reports
    reaching the duplicate-entry state."""
    rng = np.random.default_rng(17500)
    got = []
    for _ in range(max_tries):
        Tn = int(rng.integers(8, 30)); C = int(rng.integers(4, 8)); W = int(rng.integers(16, 21))
        x = rng.standard_normal((Tn, 1, C)).astype(np.float32)
        x[rng.random(x.shape) < (0.3 if rng.random() < 0.5 else 0.5)] = -np.inf
        st = {}
        try:
            ref = oracle.decode(x, [Tn], W, 1, True, 0, stats=st)
        except oracle.OracleError:
            continue
        if st["duplicate_frames"]:
            got.append((x, np.array([Tn], np.int32), W, C, ref, st["duplicate_frames"]))
            if len(got) == n_want:
                break
    assert len(got) == n_want
    return got


def test_duplicate_entry_frames(monkeypatch):
    """dup frames run the literal path, and the frame after one recurses on
    wave 0: bit-exact, the device's count of duplicate frames the oracle's."""
    monkeypatch.delenv("CTCEXT_EARLY_RECURSE", raising=False)
    for k, (x, sl, W, C, ref, nd) in enumerate(_dup_cases()):
        out, st = _decode(x, sl, W, paths=1)
        _assert_scored_kernel()
        compare(out, ref, 1)
        print("dup case %d: W=%d C=%d T=%d duplicate frames %d, early-recursed %d"
              % (k, W, C, sl[0], nd, st["early_recursed_frames"]))
        assert st["duplicate_frames"] == nd, (k, st, nd)
        assert st["early_recursed_frames"] <= max(int(sl[0]) - 1 - nd, 0), (k, st)


def test_helper_dead_falls_back(monkeypatch):
    monkeypatch.delenv("CTCEXT_EARLY_RECURSE", raising=False)
    W, C = 128, 29
    x, sl, ref = _case(W, C, "x3", 0)
    with pytest.warns(RuntimeWarning, match="hand-over wait timed out"):
        out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=0,
                                                     flags=_lib.CTCEXT_FLAG_TEST_HELPER_DEAD)
    st = _stats()
    assert st["helper_redecodes"] == 1 and st["early_recursed_frames"] == 0, st
    compare(out, ref, P)
    out, st = _decode(x, sl, W)
    _assert_scored_kernel()
    compare(out, ref, P)
    assert st["early_recursed_frames"] > 0, st


# ---------------------------------------------------------------------------
# 4. streams: a staged recursion never crosses a push

PUSHES = (1, 3, 7, None)


@pytest.mark.parametrize("W,C,kind", [(128, 29, "x3"), (16, 6, "peaked_flat"), (100, 29, "halves")])
def test_stream_pushes(W, C, kind, monkeypatch):
    monkeypatch.delenv("CTCEXT_EARLY_RECURSE", raising=False)
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    x, sl, _ = _case(W, C, kind, 0)
    kw = dict(merge_repeated=True, blank_index=0)
    with ctcext_amd.StreamDecoder(B, C, W, P, T, **kw) as s:
        t0, prev = 0, 0
        for i, n in enumerate(PUSHES):
            t1 = T if n is None else t0 + n
            out = s.push(x[t0:t1], batch_first=False)
            _assert_scored_kernel(st=s.last_stats, stream=True)
            ref = oracle.decode(np.ascontiguousarray(x[:t1]), np.full(B, t1, np.int32), W, P, **kw)
            compare(out, ref, P)
            early = s.last_stats["early_recursed_frames"]   # (cumulative, like the stream's other counters)
            print("stream W=%d %s push %d (frames %d..%d): early-recursed %d" % (W, kind, i, t0, t1, early))
            # a push's first frame is never early; nor is any frame before f0 + 1
            assert prev <= early <= B * min(t1 - (i + 1), max(t1 - _f0(W, C) - 1, 0)), (i, early)
            t0, prev = t1, early
        assert prev > 0


def test_stream_push_dense(monkeypatch):
    monkeypatch.delenv("CTCEXT_EARLY_RECURSE", raising=False)
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    W, C = 128, 29
    x, sl, _ = _case(W, C, "x8", 0)
    kw = dict(merge_repeated=True, blank_index=0)
    outs, ends = [], []
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, **kw) as s:
        t0 = 0
        for n in PUSHES:
            t1 = T if n is None else t0 + n
            outs.append(s.push_dense(torch.as_tensor(np.array(x[t0:t1]), device=DEV), batch_first=False))
            ends.append(t1)
            t0 = t1
        st = s.check()
        _assert_scored_kernel(st=st, stream=True)
        assert 0 < st["early_recursed_frames"] <= B * (T - len(PUSHES)), st
        for t1, out in zip(ends, outs):
            ref = oracle.decode(np.ascontiguousarray(x[:t1]), np.full(B, t1, np.int32), W, P, **kw)
            got = [t.cpu().numpy() for t in out[:5]]
            for name, g, w in zip(ctcext_amd.StreamDense._fields[:5], got, to_dense(ref, B, P, T, -1)):
                np.testing.assert_array_equal(g, w, err_msg="push to %d: %s" % (t1, name))
