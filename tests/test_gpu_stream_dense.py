"""The enqueue-only push of a stream (ctcext_stream_push_dense /
StreamDecoder.push_dense) on the GPU, against the CPU oracle: after every push
the padded outputs are the oracle's decode of everything pushed so far, for
every kernel family's stream build; the call only enqueues; the per-item status
and the deferred errors of check(); reset inside the push; graph capture and
replay; two streams of one decoder in flight; mixing with the synchronous
entry points; the stable-prefix outputs.

Shapes are the stream tests' own smallest ones (tests/test_gpu_stream.py)."""
import functools
import zlib

import numpy as np
import pytest
import torch

import ctcext_amd
import oracle
from ctcext_amd import _lib
from parity_util import compare
from test_gpu_dense import ASYNC_SHAPE, _async_case, to_dense
from test_gpu_stream import (FAMILIES, M_LEAVES, NP, PUSHES, _aligned_chunks, _inputs, _kw, _oracle_prefix, _Ragged,
                             _set_helper, _stat_row, _utts)
import test_gpu_stream_stable as stable_tests

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GS = _lib.CTCEXT_FLAG_GLOBAL_STATE
DEAD = _lib.CTCEXT_FLAG_TEST_HELPER_DEAD
LENGTH, FEW, TIMEOUT, CAPACITY = (_lib.CTCEXT_ITEM_LENGTH, _lib.CTCEXT_ITEM_FEW_LEAVES,
                                  _lib.CTCEXT_ITEM_HELPER_TIMEOUT, _lib.CTCEXT_ITEM_CAPACITY)
TIMEOUT_MSG = "decode kernel: a helper-wave hand-over wait timed out"
HYP = ctcext_amd.StreamDense._fields[:5]


def _i32(v):
    return torch.as_tensor(np.asarray(v, np.int32), device=DEV)


def _dev(chunk_tbc, batch_major=False):
    """A [t, B, C] numpy chunk on the GPU, time-major or batch-major."""
    t = torch.as_tensor(np.array(chunk_tbc), device=DEV)   # (a writable copy: some recipes are read-only arrays)
    return t.transpose(0, 1).contiguous() if batch_major else t


def _host(out):
    return [None if t is None else t.cpu().numpy() for t in out]


def _assert_rows(got, want, items, what):
    """The five hypothesis tensors of one push (host arrays) equal `want`
    (to_dense) bit for bit on `items`."""
    sel = list(items)
    for name, g, w in zip(HYP, got[:5], want):
        assert g.dtype == w.dtype, (what, name, g.dtype, w.dtype)
        np.testing.assert_array_equal(g[sel], w[sel], err_msg="%s %s" % (what, name))


def _assert_empty(got, items, pad, what):
    for b in items:
        assert (got[0][b] == pad).all() and (got[2][b] == pad).all(), (what, b)
        assert (got[1][b] == 0).all() and (got[3][b] == 0).all(), (what, b)
        assert np.isneginf(got[4][b]).all(), (what, b, got[4][b])


# ---- 1. parity per kernel family

PARITY = ["sq_small", "hw_small", "onewave_rn2", "onewave_rn4", "sq_big", "gather_big", "f64", "bigram", "gstate_f32"]
CASES = [(n, k, 0, -1) for n in PARITY for k in ("normal", "ties")] + [("sq_small", "ties", 1, -7)]


@functools.lru_cache(maxsize=None)
def _parity_case(name, kind):
    """Inputs and the oracle's decode of every pushed prefix, once per (family, kind)."""
    (T, C, W, P), dtype, scorer, env, flags, row = FAMILIES[name]
    rng = np.random.default_rng(zlib.crc32(("dense/%s/%s" % (name, kind)).encode()))
    B = 3
    x = _inputs(rng, kind, T, B, C, NP[dtype])
    sl = np.array([T, T - 3, T // 2], np.int32)
    kw = _kw(kind, C)
    tab = (-np.abs(rng.standard_normal((C + 1, C))) * 2).astype(NP[dtype]) if scorer == "bigram" else None
    refs = [_oracle_prefix(x, sl, t1, W, P, kw, tab) for t1, _, _ in _aligned_chunks(x, sl, PUSHES)]
    return x, sl, kw, tab, refs


@pytest.mark.parametrize("name,kind,extra,pad", CASES, ids=["%s-%s-F+%d" % c[:3] for c in CASES])
def test_family_matches_oracle_after_every_push(name, kind, extra, pad, monkeypatch):
    """Pushes of 1, 1, 1, 1, 5 and the rest, every one with results, enqueued
    back to back with nothing waited for; then one check().  Every push's
    outputs are to_dense of the oracle's decode of that prefix, rows max_frames
    wide; frames is min(sl, t1), status 0, and the kernel the family's stream
    build.  (extra: max_frames = T + 1, an odd row width.)"""
    (T, C, W, P), dtype, scorer, env, flags, row = FAMILIES[name]
    _set_helper(monkeypatch, env)
    x, sl, kw, tab, refs = _parity_case(name, kind)
    B, F = 3, T + extra
    batch_major = PARITY.index(name) % 2 == 1
    chunks = [(t1, _dev(c, batch_major), _i32(ln)) for t1, c, ln in _aligned_chunks(x, sl, PUSHES)]
    torch.cuda.synchronize()
    outs = []
    with ctcext_amd.StreamDecoder(B, C, W, P, F, dtype=NP[dtype], scorer_table=tab, flags=flags, device=DEV,
                                  **kw) as s:
        for t1, c, ln in chunks:
            outs.append(s.push_dense(c, ln, batch_first=batch_major, pad_value=pad))
        st = s.check()
        k = st["kernel"]
        assert k["launched"] and k["stream"] and _stat_row(k) == row, (name, kind, k)
        assert k["traceback"] != "none" and st["tier"] == row[0] and st["records_written"] > 0, st
        assert s.frames.tolist() == sl.tolist()
        for i, ((t1, _, _), out, ref) in enumerate(zip(chunks, outs, refs)):
            got = _host(out)
            assert got[0].shape == (B, P, F) and got[7] is None and got[8] is None
            _assert_rows(got, to_dense(ref, B, P, F, pad), range(B), "%s/%s push %d" % (name, kind, i))
            assert got[5].tolist() == [0] * B, (name, kind, i, got[5])
            assert got[6].tolist() == np.minimum(sl, t1).tolist(), (name, kind, i, got[6])


# ---- 2. the call only enqueues

@pytest.mark.parametrize("where", ["default_stream", "side_stream"])
def test_push_only_enqueues(where, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = ASYNC_SHAPE
    x, sl, want = _async_case()
    n = 150
    chunks = [(_dev(x[t0:t0 + n]), _i32(np.minimum(sl, t0 + n) - np.minimum(sl, t0))) for t0 in range(0, T, n)]
    stream = torch.cuda.Stream(device=DEV) if where == "side_stream" else torch.cuda.default_stream(DEV)

    def blocked(*a, **k):
        raise AssertionError("push_dense reached a host synchronisation")

    warm = ctcext_amd.StreamDecoder(B, C, W, P, T, merge_repeated=True, device=DEV)
    s = ctcext_amd.StreamDecoder(B, C, W, P, T, merge_repeated=True, device=DEV)
    with torch.cuda.stream(stream):
        if where == "default_stream":
            assert torch.cuda.current_stream(DEV).cuda_stream == 0   # the null-stream flag's path
        warm.push_dense(chunks[0][0], chunks[0][1], batch_first=False)   # loads the kernels
        s.reserve(n)
        torch.cuda.synchronize()
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "synchronize", blocked)
            m.setattr(torch.cuda.Stream, "synchronize", blocked)
            m.setattr(torch.Tensor, "cpu", blocked)
            m.setattr(torch.Tensor, "item", blocked)
            for c, ln in chunks:
                out = s.push_dense(c, ln, batch_first=False)
        ev = torch.cuda.Event()
        ev.record()
        done_at_return = ev.query()
        ev.synchronize()
    assert not done_at_return, "the pushes had finished when push_dense returned: it did not only enqueue"
    got = _host(out)
    _assert_rows(got, want, range(B), where)
    assert got[5].tolist() == [0, 0] and got[6].tolist() == sl.tolist()
    s.check()
    warm.close()
    s.close()


# ---- 3. status is per item and deferred

ST_SHAPE = (12, 20, 100, 5, 3)   # T, C, W, P, B; max_frames = T
ST_KW = dict(merge_repeated=False, blank_index=0)


@functools.lru_cache(maxsize=None)
def _status_x():
    T, C, W, P, B = ST_SHAPE
    x = _inputs(np.random.default_rng(41), "normal", T, B, C)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _status_ref(lens):
    """The oracle over the first lens[b] frames of each item, as dense rows of max_frames."""
    T, C, W, P, B = ST_SHAPE
    x = _status_x()
    return to_dense(oracle.decode(x[:max(lens)], np.array(lens, np.int32), W, P, **ST_KW), B, P, T, -1)


def _status_stream(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, C, W, P, B = ST_SHAPE
    s = ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, **ST_KW)
    out = s.push_dense(_dev(_status_x()[:4]), batch_first=False)
    return s, out


def test_status_length(monkeypatch):
    s, first = _status_stream(monkeypatch)
    x = _status_x()
    out = s.push_dense(_dev(x[4:7]), _i32([3, 4, 3]), batch_first=False)
    got = _host(out)
    assert got[5].tolist() == [0, LENGTH, 0] and got[6].tolist() == [7, 4, 7]
    _assert_empty(got, [1], -1, "length")
    _assert_rows(got, _status_ref((7, 4, 7)), [0, 2], "length")
    _assert_rows(_host(first), _status_ref((4, 4, 4)), range(3), "first push")
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        s.check()
    assert e.value.message == "sequence_length(1) <= 3"
    s.check()   # the record was cleared
    assert s.frames.tolist() == [7, 4, 7]
    # item 1 takes the frames it missed, the others none
    out = s.push_dense(_dev(x[4:7]), _i32([0, 3, 0]), batch_first=False)
    got = _host(out)
    assert got[5].tolist() == [0, 0, 0] and got[6].tolist() == [7, 7, 7]
    _assert_rows(got, _status_ref((7, 7, 7)), range(3), "after length")
    s.check()
    s.close()


def test_status_capacity(monkeypatch):
    s, _ = _status_stream(monkeypatch)
    T, C, W, P, B = ST_SHAPE
    x = _status_x()
    chunk = np.concatenate([x[4:], np.zeros((1, B, C), np.float32)])   # 9 frames: item 1 would hold 13
    out = s.push_dense(_dev(chunk), _i32([8, 9, 8]), batch_first=False)
    got = _host(out)
    assert got[5].tolist() == [0, CAPACITY, 0] and got[6].tolist() == [12, 4, 12]
    _assert_empty(got, [1], -1, "capacity")
    _assert_rows(got, _status_ref((12, 4, 12)), [0, 2], "capacity")
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        s.check()
    assert e.value.message == "stream capacity exceeded: item 1 would hold 13 frames of max_frames 12"
    s.check()
    out = s.push_dense(_dev(x[4:]), _i32([0, 8, 0]), batch_first=False)
    got = _host(out)
    assert got[5].tolist() == [0, 0, 0] and got[6].tolist() == [12, 12, 12]
    _assert_rows(got, _status_ref((12, 12, 12)), range(3), "after capacity")
    s.check()
    s.close()


def test_negative_length_reads_as_zero(monkeypatch):
    s, _ = _status_stream(monkeypatch)
    out = s.push_dense(_dev(_status_x()[4:7]), _i32([3, -2, 3]), batch_first=False)
    got = _host(out)
    assert got[5].tolist() == [0, 0, 0] and got[6].tolist() == [7, 4, 7]
    _assert_rows(got, _status_ref((7, 4, 7)), range(3), "negative")
    s.check()
    s.close()


def test_status_helper_timeout_leaves_the_stream_intact(monkeypatch):
    """test_failed_push_leaves_the_stream_intact for the enqueue-only push."""
    s, _ = _status_stream(monkeypatch)
    T, C, W, P, B = ST_SHAPE
    x = _status_x()
    sl = np.array([T, T - 3, T // 2], np.int32)
    out = s.push_dense(_dev(x[4:7]), batch_first=False, flags=DEAD)
    got = _host(out)
    assert got[5].tolist() == [TIMEOUT] * B and got[6].tolist() == [4, 4, 4]
    _assert_empty(got, range(B), -1, "timeout")
    with pytest.raises(ctcext_amd.InternalError) as e:
        s.check()
    assert e.value.message == TIMEOUT_MSG and s.last_stats["kernel"]["helper"] == "SQ"
    assert s.frames.tolist() == [4, 4, 4]
    for t0, t1 in ((4, 7), (7, T)):
        ln = np.minimum(sl, t1) - np.minimum(sl, t0)
        out = s.push_dense(_dev(x[t0:t1]), _i32(ln), batch_first=False)
        got = _host(out)
        assert got[5].tolist() == [0] * B
        _assert_rows(got, _status_ref(tuple(np.minimum(sl, t1).tolist())), range(B), "after timeout %d" % t1)
    s.check()
    assert s.frames.tolist() == sl.tolist()
    s.close()


def test_too_few_leaves_counts_as_pushed(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, C, W, P, B = 4, 3, 8, 4, 3
    x = _inputs(np.random.default_rng(5), "normal", T, B, C)
    sl = np.full((B,), T, np.int32)
    kw = dict(merge_repeated=False, blank_index=0)
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, **kw) as s:
        got = _host(s.push_dense(_dev(x[:1]), batch_first=False))
        assert got[5].tolist() == [FEW] * B and got[6].tolist() == [1, 1, 1]
        _assert_empty(got, range(B), -1, "few leaves")
        with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
            s.check()
        assert e.value.message == M_LEAVES
        assert s.frames.tolist() == [1, 1, 1]
        # a push without hypothesis outputs does not look at the leaves
        s2 = ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, **kw)
        q = s2.push_dense(_dev(x[:1]), batch_first=False, results=False)
        assert q.decoded is None and _host(q)[5].tolist() == [0] * B
        s2.check()
        s2.close()
        got = _host(s.push_dense(_dev(x[1:2]), batch_first=False))
        assert got[5].tolist() == [0] * B
        _assert_rows(got, to_dense(_oracle_prefix(x, sl, 2, W, P, kw), B, P, T, -1), range(B), "second frame")
        s.check()


# ---- 4. reset inside the push

def _slots(r, ends, n_max):
    """The continuous-batching schedule over _Ragged r: per push, (frames per
    item, reset flags); item b's utterances end at ends[b] (frames of its
    concatenated array), and the push that brings an utterance's first frames
    resets the item."""
    B = r.B
    nxt = [0] * B   # index of the utterance end ahead of each item
    while any(r.at[b] < ends[b][-1] for b in range(B)):
        n, rs = [], []
        for b in range(B):
            if r.at[b] == ends[b][nxt[b]] and nxt[b] + 1 < len(ends[b]):
                nxt[b] += 1
                rs.append(1)
            else:
                rs.append(0)
            n.append(min(n_max, ends[b][nxt[b]] - r.at[b]))
        yield n, rs


def test_reset_inside_the_push(monkeypatch):
    """Utterances of unequal length, chunks of 4 frames: an item that finishes
    takes its next utterance through reset= on the push that brings its first
    frames; no reset() call.  After every push every item is the oracle's decode
    of its current utterance's prefix, and the stable outputs equal those of a
    synchronous twin that uses reset(): they restart for the reset item."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    C, W, P, F = 20, 100, 3, 16
    kw = dict(merge_repeated=False, blank_index=0)
    ends = [[10, 17], [6, 12, 17], [13]]
    utts = _utts(np.random.default_rng(61), 3, 17, C)
    r = _Ragged(utts, W, P, kw)
    want, outs = [], []
    with ctcext_amd.StreamDecoder(3, C, W, P, F, device=DEV, **kw) as s, \
            ctcext_amd.StreamDecoder(3, C, W, P, F, **kw) as twin:
        for n, rs in _slots(r, ends, 4):
            for b in range(3):
                if rs[b]:
                    r.reset(b)
            c = r.chunk(n, 4)   # [B, 4, C]
            outs.append(s.push_dense(torch.as_tensor(c, device=DEV), _i32(n), reset=_i32(rs), stable=True))
            if any(rs):
                twin.reset([b for b in range(3) if rs[b]])
            twin.push(c, n, results=False)
            want.append((list(n), list(rs), r.frames(), to_dense(r.ref(), 3, P, F, -1), twin.stable()))
        s.check()
        assert any(any(rs) for _, rs, _, _, _ in want) and len(want) >= 5
        prev = None
        for i, (out, (n, rs, fr, rows, stab)) in enumerate(zip(outs, want)):
            got = _host(out)
            assert got[5].tolist() == [0, 0, 0] and got[6].tolist() == fr, (i, n, rs, got[5], got[6])
            _assert_rows(got, rows, range(3), "push %d" % i)
            assert got[7].tolist() == stab.decoded_length.tolist(), (i, got[7], stab)
            assert got[8].tolist() == stab.frames.tolist(), (i, got[8], stab)
            for b in range(3):
                assert got[8][b] <= fr[b]
                if prev is not None and not rs[b]:
                    assert got[8][b] >= prev[b]   # it only restarts with a reset
            prev = got[8]
        assert s.frames.tolist() == r.frames()


# ---- 5. graph capture and replay

@pytest.mark.parametrize("flags", [0, GS], ids=["two_wave", "global_state"])
def test_graph_capture_and_replay(flags, monkeypatch):
    """One push_dense of 4 frames captured on a side stream and replayed 8
    times on new chunks, ragged lengths and reset flags copied into the static
    inputs; item 1 is reset at replay 5.  The workspace comes from reserve(4)
    alone, so a push that allocated, freed or blocked would fail the capture."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    B, C, W, P, F = 3, 20, 100, 3, 40
    kw = dict(merge_repeated=True, blank_index=0)
    r = _Ragged(_utts(np.random.default_rng(505), B, 32, C), W, P, kw)
    side = torch.cuda.Stream(device=DEV)
    warm = ctcext_amd.StreamDecoder(B, C, W, P, F, flags=flags, device=DEV, **kw)
    with torch.cuda.stream(side):
        warm.push_dense(torch.zeros((B, 4, C), device=DEV), reset=_i32([0] * B))
    side.synchronize()
    s = ctcext_amd.StreamDecoder(B, C, W, P, F, flags=flags, device=DEV, **kw)
    s.reserve(4)
    xs = torch.zeros((B, 4, C), device=DEV)
    lens = torch.zeros((B,), dtype=torch.int32, device=DEV)
    rs = torch.zeros((B,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = s.push_dense(xs, lens, reset=rs, pad_value=-7)
    schedule = [[4, 3, 2], [4, 4, 0], [1, 4, 4], [4, 0, 3], [2, 4, 4], [4, 4, 1], [3, 2, 4], [4, 4, 4]]
    for i, n in enumerate(schedule):
        reset = [0, 1 if i == 5 else 0, 0]
        if reset[1]:
            r.reset(1)
        xs.copy_(torch.as_tensor(r.chunk(n, 4)))
        lens.copy_(torch.as_tensor(np.asarray(n, np.int32)))
        rs.copy_(torch.as_tensor(np.asarray(reset, np.int32)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = _host(out)
        assert got[5].tolist() == [0] * B and got[6].tolist() == r.frames(), (i, got[5], got[6], r.frames())
        _assert_rows(got, to_dense(r.ref(), B, P, F, -7), range(B), "replay %d" % i)
    st = s.check()
    assert st["records_written"] > 0 and st["kernel"]["stream"], st
    assert st["tier"] == (1 if flags else 0) and (flags or st["kernel"]["helper"] == "SQ"), st
    assert s.frames.tolist() == r.frames()
    s.close()
    warm.close()


# ---- 6. two streams of one decoder in flight

def test_two_streams_of_one_decoder_in_flight(monkeypatch):
    """Pushes of two StreamDecoders on one decoder handle interleaved on two
    torch streams, nothing waited for until the end: each has a workspace of
    its own, so neither disturbs the other."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    kw = dict(merge_repeated=True, blank_index=0)
    ra = _Ragged(_utts(np.random.default_rng(31), 3, 12, 20), 100, 5, kw)
    rb = _Ragged(_utts(np.random.default_rng(32), 3, 12, 6), 8, 3, kw)
    plan = []
    for na, nb in (([1, 1, 1], [2, 2, 1]), ([4, 3, 2], [1, 0, 3]), ([3, 3, 3], [5, 5, 5]), ([2, 0, 4], [3, 4, 2])):
        ca, cb = torch.as_tensor(ra.chunk(na), device=DEV), torch.as_tensor(rb.chunk(nb), device=DEV)
        plan.append((ca, _i32(na), to_dense(ra.ref(), 3, 5, 12, -1), cb, _i32(nb), to_dense(rb.ref(), 3, 3, 12, -1)))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    outs = []
    with ctcext_amd.StreamDecoder(3, 20, 100, 5, 12, device=DEV, **kw) as sa, \
            ctcext_amd.StreamDecoder(3, 6, 8, 3, 12, device=DEV, **kw) as sb:
        for ca, la, _, cb, lb, _ in plan:
            with torch.cuda.stream(s1):
                oa = sa.push_dense(ca, la)
            with torch.cuda.stream(s2):
                ob = sb.push_dense(cb, lb)
            outs.append((oa, ob))
        assert sa.dec is sb.dec
        sa.check()
        sb.check()
        torch.cuda.synchronize()
        for i, ((oa, ob), (_, _, wa, _, _, wb)) in enumerate(zip(outs, plan)):
            ga, gb = _host(oa), _host(ob)
            assert ga[5].tolist() == [0] * 3 and gb[5].tolist() == [0] * 3
            _assert_rows(ga, wa, range(3), "stream a push %d" % i)
            _assert_rows(gb, wb, range(3), "stream b push %d" % i)
        assert sa.frames.tolist() == ra.frames() and sb.frames.tolist() == rb.frames()


# ---- 7. mixing with the synchronous entry points

def test_mixing_with_the_synchronous_push(monkeypatch):
    """Enqueue-only pushes, then a synchronous push with no check() between,
    then frames and stable(): all as in an all-synchronous run of the same
    schedule, and the oracle's."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    (T, C, W, P) = FAMILIES["sq_small"][0]
    B = 3
    x = _inputs(np.random.default_rng(71), "ties", T, B, C)
    sl = np.array([T, T - 3, T // 2], np.int32)
    kw = _kw("ties", C)
    pushes = list(_aligned_chunks(x, sl, (3, 4, 5, 6, None)))
    form = ("dense", "dense", "sync", "dense", "sync")
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, **kw) as a, \
            ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, **kw) as m:
        for (t1, c, ln), how in zip(pushes, form):
            ref = _oracle_prefix(x, sl, t1, W, P, kw)
            oa = a.push(_dev(c), _i32(ln), batch_first=False)
            compare(oa, ref, P, lp_exact=True)
            if how == "dense":
                om = m.push_dense(_dev(c), _i32(ln), batch_first=False)
            else:
                compare(m.push(_dev(c), _i32(ln), batch_first=False), ref, P, lp_exact=True)
            # (each of these waits for the enqueue-only pushes first)
            assert m.frames.tolist() == a.frames.tolist() == np.minimum(sl, t1).tolist()
            sa, sm = a.stable(), m.stable()
            assert sm.decoded_length.tolist() == sa.decoded_length.tolist(), t1
            assert sm.frames.tolist() == sa.frames.tolist(), t1
            if how == "dense":
                got = _host(om)
                assert got[5].tolist() == [0] * B
                _assert_rows(got, to_dense(ref, B, P, T, -1), range(B), "dense push to %d" % t1)
        m.check()


# ---- 8. the stable-prefix outputs

@pytest.mark.parametrize("name", ["sq_small", "gstate_f32"])
def test_stable_outputs(name, monkeypatch):
    """On the stable tests' two-hot recipe: stable_length / stable_frames of
    push_dense(stable=True) equal stable() on the same stream and the naive
    host reference on a synchronous twin, after every push; not vacuous."""
    (T, C, W), dtype, env, flags, rbytes, row = stable_tests.FAMILIES[name]
    x = stable_tests._recipe(T, C, dtype)
    B = stable_tests.B
    seen = set()
    with stable_tests._open(name, False, 5, monkeypatch) as twin, stable_tests._open(name, False, 5, monkeypatch) as s:
        for t1, chunk in stable_tests._pushes(x, stable_tests._boundaries(T)):
            out = s.push_dense(_dev(chunk), batch_first=False, results=False, stable=True)
            twin.push(chunk, batch_first=False, results=False)
            ref = twin._stable_reference()
            got = _host(out)
            assert out.decoded is None and got[7].dtype == np.int32 and got[8].dtype == np.int64
            assert got[7].tolist() == ref.decoded_length.tolist(), (name, t1, got[7], ref)
            assert got[8].tolist() == ref.frames.tolist(), (name, t1, got[8], ref)
            again = s.stable()
            assert again.decoded_length.tolist() == got[7].tolist() and again.frames.tolist() == got[8].tolist()
            assert got[6].tolist() == [t1] * B
            seen.update(got[7].tolist())
        s.check()
    assert len(seen) >= 5 and max(seen) * 3 >= T, (name, seen)
