"""Token scores of a stream on the GPU (ctcext_stream_open_scores /
_stream_token_scores behind StreamDecoder(token_scores=True) and
token_scores_dense): after a push, NaN mask and then exact equality with the
definition of include/ctcext.h, "Token scores", applied to everything committed
to each item so far (stream_scores_util.expected_held: the CPU oracle's rows,
their token times and the oracle's normaliser), width max_frames.  Shapes are
(T, B, C, W, P); test_cpu_stream_scores.py asserts on the oracle what these
cases rely on."""
import ctypes

import numpy as np
import pytest
import torch

import ctcext_amd
import skip_util
import stream_scores_util as ssc
from ctcext_amd import _lib
from token_scores_util import lengths
from token_times_util import family

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MSG = "token times need a blank_label that is no class label"
KW = dict(merge_repeated=True, blank_index=0, blank_label=-1)
DEAD = _lib.CTCEXT_FLAG_TEST_HELPER_DEAD
LENGTH, FEW, TIMEOUT, CAPACITY = (_lib.CTCEXT_ITEM_LENGTH, _lib.CTCEXT_ITEM_FEW_LEAVES, _lib.CTCEXT_ITEM_HELPER_TIMEOUT,
                                  _lib.CTCEXT_ITEM_CAPACITY)


def _host(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in ts]


def _dev(x):
    return torch.as_tensor(np.asarray(x), device=DEV)


def _i32(v):
    return torch.as_tensor(np.asarray(v, np.int32), device=DEV)


def _assert_scores(sc, want, items=None, what=""):
    got = _host(sc)
    sel = slice(None) if items is None else list(items)
    for name, g, w in zip(ctcext_amd.TokenScores._fields, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        g, w = g[sel], w[sel]
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg="%s %s: NaN mask" % (what, name))
        np.testing.assert_array_equal(g[~np.isnan(g)], w[~np.isnan(w)], err_msg="%s %s" % (what, name))


def _assert_times(tt, want, items=None, what=""):
    sel = slice(None) if items is None else list(items)
    for name, g, w in zip(ctcext_amd.TokenTimes._fields, _host(tt), want):
        np.testing.assert_array_equal(g[sel], w[sel], err_msg="%s %s" % (what, name))


def _assert_nan(sc, items, what=""):
    for g in _host(sc):
        assert np.isnan(g[list(items)]).all(), what


def _stream(B, C, W, P, F, **kw):
    return ctcext_amd.StreamDecoder(B, C, W, P, F, device=DEV, token_scores=True, **kw)


def _push(s, chunk, n=None, **kw):
    """One push_dense of chunk [t, B, C] (numpy or CUDA tensor) and its times and scores."""
    c = chunk if torch.is_tensor(chunk) else _dev(chunk)
    kw.setdefault("batch_first", False)
    out = s.push_dense(c, None if n is None else _i32(n), **kw)
    tt = s.token_times_dense()
    return out, tt, s.token_scores_dense(tt)


def _run(s, pushes, what, status=None):
    """Every push of a stream_scores_util schedule, waited for once at the end."""
    got = [_push(s, chunk, n) for chunk, n, frames, times, scores in pushes]
    for i, ((out, tt, sc), (chunk, n, frames, times, scores)) in enumerate(zip(got, pushes)):
        w = "%s push %d" % (what, i)
        assert _host([out.frames])[0].tolist() == frames, w
        if status is not None:
            assert _host([out.status])[0].tolist() == status, w
        _assert_times(tt, times, what=w)
        _assert_scores(sc, scores, what=w)
    return got


# ---- 1. after every push; 8. the same bits as the one-shot decode on the same GPU

@pytest.mark.parametrize("case", ssc.EVERY_PUSH, ids=ssc.case_id)
def test_after_every_push(case, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    kind, shape, merge, push = case
    T, B, C, W, P = shape
    x, sl, kw, pushes = ssc.every_push_case(*case)
    with _stream(B, C, W, P, T, **kw) as s:
        with pytest.raises(ctcext_amd.FailedPreconditionError):
            s.token_scores_dense()   # no enqueue-only push yet
        got = _run(s, pushes, ssc.case_id(case), status=[0] * B)
        st = s.check()
        assert st["kernel"]["stream"], st
        last = got[-1][2]
        assert tuple(last.logp_sum.shape) == (B, P, T) and last.logp_sum.is_cuda and last.logp_sum.dtype == torch.float32
        # a push without hypothesis outputs leaves nothing to score
        s.reset()
        s.push_dense(_dev(pushes[0][0]), _i32(pushes[0][1]), batch_first=False, results=False)
        with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
            s.token_scores_dense(got[-1][1])
        assert e.value.error_code == _lib.CTCEXT_FAILED_PRECONDITION
        s.check()
    # the one-shot decode of the concatenated logits: the same kernel over the caller's tensor
    ctcext_amd.decode_dense(_dev(np.array(x)), _i32(sl), W, P, batch_first=False, token_scores=True, **kw)
    one = _host(ctcext_amd.dense_token_scores())
    ctcext_amd.dense_check()
    for g, w in zip(_host(last), one):
        assert g.shape == w.shape and (~np.isnan(w)).any()
        np.testing.assert_array_equal(g.view(np.uint32)[~np.isnan(w)], w.view(np.uint32)[~np.isnan(w)])
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w))


# ---- 2. rows longer than the scores kernel's tile

@pytest.mark.parametrize("case", ssc.TILED_PUSH, ids=ssc.case_id)
def test_rows_longer_than_the_scores_tile(case, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape, soft, push = case
    T, B, C, W, P = shape
    x, sl, kw, pushes = ssc.tiled_push_case(*case)
    status = [0 if sl[b] > 0 else FEW for b in range(B)]   # item 2 of the first: no frames, fewer leaves than top_paths
    with _stream(B, C, W, P, T, **kw) as s:
        _run(s, pushes, ssc.case_id(case), status=status)
        if any(status):
            with pytest.raises(ctcext_amd.InvalidArgumentError):
                s.check()
        s.check()


# ---- 3. normaliser paths and types

def _whole(x, sl, push, W, P, kw, what, stream_kw=None, chunks=None):
    """x [T, B, C] in pushes of `push` frames through a new stream, checked
    after every push; chunks(i, chunk) makes the tensor that is pushed."""
    T, B, C = x.shape
    pushes = ssc.run_schedule(x, sl, push, W, P, T, **kw)
    assert (~np.isnan(pushes[-1][4][0])).any()
    with _stream(B, C, W, P, T, dtype=x.dtype.name, **kw, **(stream_kw or {})) as s:
        fed = [(chunk if chunks is None else chunks(i, chunk), n, f, t, sc) for i, (chunk, n, f, t, sc) in enumerate(pushes)]
        got = _run(s, fed, what, status=[0] * B)
        st = s.check()
    return got, st


def test_large_c_normaliser(monkeypatch):
    """C = 80: the row_prep pre-pass writes the normaliser the append copies."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 20, 2, 80, 8, 2
    x = family(np.random.default_rng(80), "peaky", T, B, C)
    got, st = _whole(x, lengths(T, B), 6, W, P, KW, "C = 80")
    assert st["kernel"]["prepass"] not in ("none", "norm_only"), st   # (launch_row_prep's normaliser, not launch_row_norm's)


def test_float64(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (12, 6, 5, 8, 3)
    T, B, C, W, P = shape
    x, sl, kw, _ = ssc.tsu.family_case("gaussian", shape, True, "float64")
    got, st = _whole(np.array(x), sl, 5, W, P, kw, "float64")
    assert got[-1][2].logp_sum.dtype == torch.float64 and got[-1][2].logp_min.dtype == torch.float64


def test_float64_rows_of_four_element_multiples(monkeypatch):
    """C = 8, dense float64 chunks: the append moves four elements a thread."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 14, 3, 8, 8, 2
    x = family(np.random.default_rng(64), "sticky", T, B, C, np.float64)
    _whole(x, np.array([T, T - 3, T // 2], np.int32), 5, W, P, KW, "float64, C = 8")


def _bf16(x):
    """x rounded to bfloat16, as float32."""
    return torch.as_tensor(x).to(torch.bfloat16).float().numpy()


def test_global_state_tier_with_bf16_chunks(monkeypatch):
    """The global-state tier widens a half chunk into workspace for its
    pre-pass; the append reads the caller's rows, through their own strides
    (batch-major here, which the widened copy is not)."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 24, 3, 29, 16, 2
    x = _bf16(family(np.random.default_rng(41), "sticky", T, B, C))
    got, st = _whole(x, np.array([T, T - 3, T // 2], np.int32), 7, W, P, KW, "global state",
                     stream_kw=dict(flags=_lib.CTCEXT_FLAG_GLOBAL_STATE),
                     chunks=lambda i, c: _dev(c).to(torch.bfloat16).transpose(0, 1).contiguous().transpose(0, 1))
    assert st["tier"] == 1, st


# ---- 4. formats

@pytest.mark.parametrize("C,lo", [(29, 5), (28, 8), (28, 5)], ids=["C29", "C28-aligned", "C28-unaligned"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_half_store_fed_vocabulary_slices_in_place(dtype, C, lo, monkeypatch):
    """A two-byte store fed batch-first views with gaps in both dimensions: the
    append gathers from the caller's tensor, and the scores kernel widens the
    store's halves.  Rows of 29 halves go an element a thread; rows of 28 that
    begin on an 8-byte boundary four, and those that do not one again."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, W, P = 24, 3, 16, 2
    push = 7
    full = _dev(family(np.random.default_rng(40), "sticky", T, B, 40).transpose(1, 0, 2).copy()).to(dtype)   # [B, T, 40]
    x = full[:, :, lo:lo + C].float().transpose(0, 1).contiguous().cpu().numpy()   # the widened slice, [T, B, C]
    sl = np.array([T, T - 3, T // 2], np.int32)
    pushes = ssc.run_schedule(x, sl, push, W, P, T, **KW)
    name = str(dtype).replace("torch.", "")
    with _stream(B, C, W, P, T, score_store=name, **KW) as s:
        got, pos = [], [0] * B
        for chunk, n, frames, times, scores in pushes:
            # item b's next frames, each item from its own position: a [B, push, 40] staging tensor, sliced
            stage = torch.zeros((B, push, 40), dtype=dtype, device=DEV)
            for b in range(B):
                stage[b, :n[b]] = full[b, pos[b]:pos[b] + n[b]]
            view = stage[:, :, lo:lo + C]
            assert not view.is_contiguous() and view.stride(-1) == 1
            got.append(_push(s, view, n, batch_first=True))
            pos = frames
        for i, ((out, tt, sc), p) in enumerate(zip(got, pushes)):
            _assert_times(tt, p[3], what="%s push %d" % (name, i))
            _assert_scores(sc, p[4], what="%s push %d" % (name, i))
        assert got[-1][2].logp_sum.dtype == torch.float32
        s.check()


@pytest.mark.parametrize("C", [29, 28])
def test_native_store_fed_bf16_then_f16_then_f32(C, monkeypatch):
    """Each chunk is widened exactly on its way in (C = 28: four elements a thread)."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, W, P = 21, 3, 16, 2
    push = 7
    raw = family(np.random.default_rng(43), "sticky", T, B, C)
    kinds = [torch.bfloat16, torch.float16, torch.float32]
    x = np.concatenate([torch.as_tensor(raw[i * push:(i + 1) * push]).to(k).float().numpy() for i, k in enumerate(kinds)])
    assert (x[:push] != raw[:push]).any() and (x[push:2 * push] != raw[push:2 * push]).any()
    got, st = _whole(x, np.full((B,), T, np.int32), push, W, P, KW, "mixed formats",
                     chunks=lambda i, c: _dev(c).to(kinds[i]))


# ---- 5. roll-back: by position, not by undo

def test_a_push_that_times_out_leaves_no_rows_behind(monkeypatch):
    """Chunk 1, a decoy chunk whose hand-over fails for every item, the real
    chunk 2: the scores are those of chunk 1 + chunk 2 (the CPU file asserts
    that the decoy's rows in place of chunk 2's would change a timed token of
    every item)."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = ssc.ROLLBACK_SHAPE
    n = ssc.ROLLBACK_PUSH
    x, decoy, kw, first, both, mixed = ssc.rollback_case()
    with _stream(B, C, W, P, T, **kw) as s:
        o1, t1, s1 = _push(s, x[:n])
        od, td, sd = _push(s, decoy, flags=DEAD)
        o2, t2, s2 = _push(s, x[n:])
        assert _host([o1.status])[0].tolist() == [0] * B
        assert _host([od.status])[0].tolist() == [TIMEOUT] * B and _host([od.frames])[0].tolist() == [n] * B
        assert _host([o2.status])[0].tolist() == [0] * B and _host([o2.frames])[0].tolist() == [T] * B
        _assert_scores(s1, first[1], what="chunk 1")
        _assert_nan(sd, range(B), "the decoy push")
        _assert_times(t2, both[0], what="chunk 1 + chunk 2")
        _assert_scores(s2, both[1], what="chunk 1 + chunk 2")
        with pytest.raises(ctcext_amd.InternalError):
            s.check()
        assert s.last_stats["kernel"]["helper"] != "none"
        s.check()


def test_length_and_capacity_items_keep_their_rows(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    B, C, W, P, F = 3, 5, 8, 3, 30
    t = 16
    x = family(np.random.default_rng(52), "sticky", 40, B, C)
    decoy = family(np.random.default_rng(53), "gaussian", t, B, C)
    held = ssc.Held(B, C)
    with _stream(B, C, W, P, F, **KW) as s:
        o1, t1, s1 = _push(s, x[:t], [8, t, t])
        held.take_chunk(x[:t], [8, t, t])
        w1 = ssc.expected_held(held, W, P, F, **KW)
        # item 0: a length above chunk_time; item 1: 16 + 16 frames of 30; item 2 advances
        o2, t2, s2 = _push(s, decoy, [t + 1, t, 10])
        held.take_chunk(decoy, [0, 0, 10])
        w2 = ssc.expected_held(held, W, P, F, **KW)
        # the same rows again would have been wrong: every item takes frames of x now
        o3, t3, s3 = _push(s, x[t:2 * t], [10, 10, 4])
        held.take_chunk(x[t:2 * t], [10, 10, 4])
        w3 = ssc.expected_held(held, W, P, F, **KW)
        # a push with lengths all 0 changes nothing
        o4, t4, s4 = _push(s, decoy, [0, 0, 0])
        _assert_scores(s1, w1[1], what="chunk 1")
        assert _host([o2.status])[0].tolist() == [LENGTH, CAPACITY, 0] and _host([o2.frames])[0].tolist() == [8, t, t + 10]
        _assert_nan(s2, [0, 1], "items with a status bit")
        _assert_scores(s2, w2[1], items=[2], what="the item that advanced")
        assert _host([o3.status])[0].tolist() == [0] * B and _host([o3.frames])[0].tolist() == [18, 26, 30]
        _assert_times(t3, w3[0], what="after the refused push")
        _assert_scores(s3, w3[1], what="after the refused push")
        assert _host([o4.status])[0].tolist() == [0] * B and _host([o4.frames])[0].tolist() == [18, 26, 30]
        _assert_scores(s4, w3[1], what="lengths all 0")
        with pytest.raises(ctcext_amd.FailedPreconditionError):
            s.check()
        s.check()


# ---- 6. reset

@pytest.mark.parametrize("how", ["reset_argument", "reset_call"])
def test_reset_starts_the_items_store_at_frame_zero(how, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    B, C, W, P, F = 3, 6, 16, 3, 24
    x = family(np.random.default_rng(61), "sticky", 3 * 8, B, C)
    held = ssc.Held(B, C)
    with _stream(B, C, W, P, F, **KW) as s:
        got, want = [], []
        for i in range(3):
            chunk = x[8 * i:8 * i + 8]
            rs = [0, 1, 0] if i == 1 else [0, 0, 0]
            if rs[1]:
                held.reset(1)
            if rs[1] and how == "reset_call":
                s.reset([1])
                got.append(_push(s, chunk, [8, 5, 8]))
            else:
                got.append(_push(s, chunk, [8, 5, 8], reset=_i32(rs)))
            held.take_chunk(chunk, [8, 5, 8])
            want.append((held.frames(), ssc.expected_held(held, W, P, F, **KW)))
        for i, ((out, tt, sc), (frames, (times, scores))) in enumerate(zip(got, want)):
            assert _host([out.frames])[0].tolist() == frames, i
            _assert_times(tt, times, what="push %d" % i)
            _assert_scores(sc, scores, what="push %d" % i)
        assert want[-1][0] == [24, 10, 24]
        s.check()


# ---- 7. a skipping stream: the original time axis

@pytest.mark.parametrize("push", [3, 4])
def test_skipping_stream(push, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = ssc.tsu.SKIP_SHAPE
    x, sl, kw, e, pushes = ssc.skip_push_case(push)
    with _stream(B, C, W, P, T, skip_blank=skip_util.THR, **kw) as s:
        _run(s, pushes, "skipping / %d" % push, status=[0] * B)
        s.check()
        assert s.kept_frames().tolist() == e.kept.tolist() and (e.kept < sl).all()


def test_skipping_stream_with_threshold_zero_equals_the_plain_stream(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    case = ssc.EVERY_PUSH[1]
    kind, shape, merge, push = case
    T, B, C, W, P = shape
    x, sl, kw, pushes = ssc.every_push_case(*case)
    with _stream(B, C, W, P, T, **kw) as plain, _stream(B, C, W, P, T, skip_blank=0.0, **kw) as skip:
        a = [_push(plain, c, n) for c, n, *_ in pushes]
        b = [_push(skip, c, n) for c, n, *_ in pushes]
        for i, ((_, _, sa), (_, _, sb), p) in enumerate(zip(a, b, pushes)):
            _assert_scores(sb, p[4], what="threshold 0, push %d" % i)
            for g, w in zip(_host(sa), _host(sb)):
                np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32))
        plain.check()
        skip.check()
        assert skip.kept_frames().tolist() == sl.tolist()


# ---- 9. the calls only enqueue

@pytest.mark.parametrize("where", ["default_stream", "side_stream"])
def test_calls_only_enqueue(where, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    case = ssc.EVERY_PUSH[3]
    kind, shape, merge, push = case
    T, B, C, W, P = shape
    x, sl, kw, pushes = ssc.every_push_case(*case)
    chunks = [(_dev(c), _i32(n)) for c, n, *_ in pushes]
    stream = torch.cuda.Stream(device=DEV) if where == "side_stream" else torch.cuda.default_stream(DEV)

    def blocked(*a, **k):
        raise AssertionError("a stream scores call reached a host synchronisation")

    warm = _stream(B, C, W, P, T, **kw)
    s = _stream(B, C, W, P, T, **kw)
    with torch.cuda.stream(stream):
        _push(warm, chunks[0][0], None)   # loads the kernels
        s.reserve(push)
        torch.cuda.synchronize()
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "synchronize", blocked)
            m.setattr(torch.cuda.Stream, "synchronize", blocked)
            m.setattr(torch.Tensor, "cpu", blocked)
            m.setattr(torch.Tensor, "item", blocked)
            for c, n in chunks:
                s.push_dense(c, n, batch_first=False)
                tt = s.token_times_dense()
                sc = s.token_scores_dense(tt)
        ev = torch.cuda.Event()
        ev.record()
        done_at_return = ev.query()
        ev.synchronize()
    assert not done_at_return, "the work had finished when token_scores_dense returned: it did not only enqueue"
    _assert_scores(sc, pushes[-1][4], what=where)
    s.check()
    warm.close()
    s.close()


# ---- 10. graph capture

def test_graph_capture_and_replay(monkeypatch):
    """One push_dense + token_times_dense + token_scores_dense captured on a
    side stream and replayed once per chunk on new data copied into the static
    tensors.  The store is the stream's from its opening and the workspace
    comes from reserve alone, so a call that allocated from HIP, freed or
    blocked would fail the capture."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    case = ssc.EVERY_PUSH[3]
    kind, shape, merge, push = case
    T, B, C, W, P = shape
    x, sl, kw, pushes = ssc.every_push_case(*case)
    side = torch.cuda.Stream(device=DEV)
    warm = _stream(B, C, W, P, T, **kw)
    with torch.cuda.stream(side):
        _push(warm, torch.zeros((push, B, C), device=DEV))
    side.synchronize()
    s = _stream(B, C, W, P, T, **kw)
    s.reserve(push)
    xs = torch.zeros((push, B, C), device=DEV)
    lens = torch.zeros((B,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = s.push_dense(xs, lens, batch_first=False)
        tt = s.token_times_dense()
        sc = s.token_scores_dense(tt)
    for i, (chunk, n, frames, times, scores) in enumerate(pushes):
        xs.copy_(torch.as_tensor(chunk))
        lens.copy_(torch.as_tensor(n))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert _host([out.frames])[0].tolist() == frames, i
        _assert_times(tt, times, what="replay %d" % i)
        _assert_scores(sc, scores, what="replay %d" % i)
    assert s.check()["records_written"] > 0
    s.close()
    warm.close()


# ---- 11. two streams of one decoder

def test_two_streams_of_one_decoder_read_their_own_store(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    ca, cb = ssc.EVERY_PUSH[1], ssc.EVERY_PUSH[2]   # sticky and peaky of one shape and push size
    assert ca[1:] == cb[1:]
    T, B, C, W, P = ca[1]
    pa, pb = ssc.every_push_case(*ca)[3], ssc.every_push_case(*cb)[3]
    kw = ssc.every_push_case(*ca)[2]
    a, b = _stream(B, C, W, P, T, **kw), _stream(B, C, W, P, T, **kw)
    got = []
    for qa, qb in zip(pa, pb):
        a.push_dense(_dev(qa[0]), _i32(qa[1]), batch_first=False)
        b.push_dense(_dev(qb[0]), _i32(qb[1]), batch_first=False)
        got.append((a.token_scores_dense(), b.token_scores_dense()))   # a's after b's push went in
    a.check()
    b.check()
    for i, ((sa, sb), qa, qb) in enumerate(zip(got, pa, pb)):
        _assert_scores(sa, qa[4], what="stream a push %d" % i)
        _assert_scores(sb, qb[4], what="stream b push %d" % i)
    a.close()
    b.close()


# ---- 12. errors

def test_preconditions(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 12, 2, 5, 8, 1
    x = family(np.random.default_rng(6), "gaussian", T, B, C)
    # a stream without the store: the Python layer's answer, and the library's own
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV) as s:
        s.push_dense(_dev(x[:4]), batch_first=False)
        tt = s.token_times_dense()
        with pytest.raises(ctcext_amd.FailedPreconditionError):
            s.token_scores_dense(tt)
        t, o = _lib.TokenTimesOut(), _lib.TokenScoresOut()
        t.start, t.end = tt.start.data_ptr(), tt.end.data_ptr()
        keep = torch.zeros((B, P, T), device=DEV)
        o.logp_sum = keep.data_ptr()
        assert s.lib.ctcext_stream_token_scores(s.handle, ctypes.byref(t), ctypes.byref(o)) == _lib.CTCEXT_FAILED_PRECONDITION
        assert s.lib.ctcext_last_error().decode() == \
            "ctcext_stream_token_scores on a stream without a score store (ctcext_stream_open_scores)"
        ms = ctypes.c_double()
        assert s.lib.ctcext_stream_scores_ms(s.handle, ctypes.byref(ms), ctypes.byref(ms)) == _lib.CTCEXT_FAILED_PRECONDITION
        s.check()
    # before any push, and after a push without hypothesis outputs
    with _stream(B, C, W, P, T) as s:
        with pytest.raises(ctcext_amd.FailedPreconditionError):
            s.token_scores_dense()
        s.reserve(4)   # (opens the stream)
        assert s.lib.ctcext_stream_token_scores(s.handle, ctypes.byref(t), ctypes.byref(o)) == _lib.CTCEXT_FAILED_PRECONDITION
        s.push_dense(_dev(x[:4]), batch_first=False, results=False)
        with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
            s.token_scores_dense(tt)
        assert e.value.message == "ctcext_stream_token_scores without a ctcext_stream_push_dense that had hypothesis outputs"
        # the synchronous push: refused, and the stream as it was
        with pytest.raises(ctcext_amd.UnimplementedError):
            s.push(_dev(x[4:8]), batch_first=False)
        c = _lib.Chunk()
        c.inputs, c.chunk_time = _dev(x[4:8]).data_ptr(), 4
        assert s.lib.ctcext_stream_push(s.handle, ctypes.byref(c), None) == _lib.CTCEXT_UNIMPLEMENTED
        assert s.lib.ctcext_last_error().decode() == \
            "a stream with a score store has no synchronous push: use ctcext_stream_push_dense"
        assert s.frames.tolist() == [4, 4]
        out, t2, sc = _push(s, x[4:8])
        held = ssc.Held(B, C)
        held.take_chunk(x[:8], [8, 8])
        _assert_scores(sc, ssc.expected_held(held, W, P, T)[1], what="after the refused push")
        s.check()
    # a blank_label that is a class label: refused when the stream is made, with the existing message
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        _stream(B, C, W, P, T, blank_label=3)
    assert e.value.message == MSG and e.value.error_code == _lib.CTCEXT_INVALID_ARGUMENT


def test_wrong_chunk_format_is_refused_before_anything_is_enqueued(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 12, 2, 5, 8, 2
    x = _bf16(family(np.random.default_rng(8), "sticky", T, B, C))
    held = ssc.Held(B, C)
    with _stream(B, C, W, P, T, score_store="bfloat16", **KW) as s:
        _push(s, _dev(x[:6]).to(torch.bfloat16))
        held.take_chunk(x[:6], [6, 6])
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        for wrong in (torch.float16, torch.float32):
            with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
                s.push_dense(_dev(x[6:]).to(wrong), batch_first=False)
            assert e.value.message == "chunk inputs_format differs from the stream's score store format"
        assert s.frames.tolist() == [6, 6]
        out, tt, sc = _push(s, _dev(x[6:]).to(torch.bfloat16))
        held.take_chunk(x[6:], [6, 6])
        times, scores = ssc.expected_held(held, W, P, T, **KW)
        assert _host([out.frames])[0].tolist() == [T, T]
        _assert_times(tt, times, what="after the refused chunks")
        _assert_scores(sc, scores, what="after the refused chunks")
        s.check()
    # the first push of a stream, which opens it: refused as well, nothing opened
    with _stream(B, C, W, P, T, score_store="bfloat16", **KW) as s:
        with pytest.raises(ctcext_amd.InvalidArgumentError):
            s.push_dense(_dev(x[:6]).to(torch.float16), batch_first=False)
        assert not s.handle


I32_MAX = 2 ** 31 - 1


def test_out_of_range_spans_are_refused(monkeypatch):
    """Plain out-of-range integers in start / end, through the C ABI: every cell
    is a NaN and the call completes normally."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    case = ssc.EVERY_PUSH[0]
    kind, shape, merge, push = case
    T, B, C, W, P = shape
    x, sl, kw, pushes = ssc.every_push_case(*case)
    with _stream(B, C, W, P, T, **kw) as s:
        for chunk, n, *_ in pushes:
            out, tt, sc = _push(s, chunk, n)

        def call(start, end, lsum, lmin):
            t, o = _lib.TokenTimesOut(), _lib.TokenScoresOut()
            t.start, t.end = start.data_ptr(), end.data_ptr()
            o.logp_sum, o.logp_min = [None if v is None else v.data_ptr() for v in (lsum, lmin)]
            return s.lib.ctcext_stream_token_scores(s.handle, ctypes.byref(t), ctypes.byref(o))

        def filled(v):
            return torch.full((B, P, T), v, dtype=torch.int32, device=DEV)

        for st, en in ((-7, -7), (T, T), (5, 2), (I32_MAX, I32_MAX), (-7, 3), (0, T), (0, I32_MAX), (I32_MAX, 0)):
            lsum, lmin = torch.zeros((B, P, T), device=DEV), torch.zeros((B, P, T), device=DEV)
            assert call(filled(st), filled(en), lsum, lmin) == _lib.CTCEXT_OK, (st, en)
            got = _host([lsum, lmin])
            assert np.isnan(got[0]).all() and np.isnan(got[1]).all(), (st, en)
        # either output alone; neither: refused
        lsum = torch.full((B, P, T), 77.0, device=DEV)
        assert call(tt.start, tt.end, lsum, None) == _lib.CTCEXT_OK
        _assert_scores([lsum], pushes[-1][4][:1], what="logp_sum alone")
        assert call(tt.start, tt.end, None, None) == _lib.CTCEXT_INVALID_ARGUMENT
        _assert_scores(sc, pushes[-1][4], what="the last push")
        s.check()


def test_scores_ms_after_a_profiled_push(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 12, 2, 5, 8, 1
    x = family(np.random.default_rng(6), "gaussian", T, B, C)
    with _stream(B, C, W, P, T) as s:
        _push(s, x[:6])
        with pytest.raises(ctcext_amd.FailedPreconditionError):
            s.scores_ms()   # that push was not profiled
        _push(s, x[6:], flags=_lib.CTCEXT_FLAG_PROFILE)
        append_ms, scores_ms = s.scores_ms()
        assert append_ms > 0 and scores_ms > 0
        s.push_dense(_dev(x[:0]), batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE)   # no frame: no append
        assert s.scores_ms() == (0.0, 0.0)
        s.check()
