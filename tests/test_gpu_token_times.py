"""Token times on the GPU (ctcext_dense_token_times / _stream_token_times /
_fetch_token_times behind dense_token_times, StreamDecoder.token_times_dense
and token_times): exact equality with the definition of include/ctcext.h,
restated in token_times_util.token_times and applied to the CPU oracle's rows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
import oracle
from ctcext_amd import _lib, ops
from test_gpu_dense import ASYNC_SHAPE, _async_case
from token_times_util import NEG_INF_SEEDS, expected, expected_from_rows, family, runs_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MSG = "token times need a blank_label that is no class label"


def _host(tt):
    torch.cuda.synchronize()
    return [t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in tt]


def _assert_times(tt, want, items=None, what=""):
    got = _host(tt)
    sel = slice(None) if items is None else list(items)
    for name, g, w in zip(ctcext_amd.TokenTimes._fields, got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g[sel], w[sel], err_msg="%s %s" % (what, name))


def _lengths(T, B):
    return np.array([T] + [max(T - 1 - 2 * b, 0) for b in range(1, B)], np.int32)


def _dense(x, sl, W, P, **kw):
    out = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), torch.as_tensor(np.asarray(sl, np.int32), device=DEV),
                                  W, P, batch_first=False, **kw)
    return out, ctcext_amd.dense_token_times()


def _rows_from_dense(dense, items):
    """Rows as lists from padded tensors (host): dec[b][p], ali[b][p]."""
    dec, dl, ali, al = dense[:4]
    P = dec.shape[1]
    return ([[dec[b, p, :dl[b, p]].tolist() for p in range(P)] for b in items],
            [[ali[b, p, :al[b, p]].tolist() for p in range(P)] for b in items])


# ---- 1. the dense form over the families

SHAPES = [(1, 2, 3, 2, 1), (12, 6, 5, 8, 3), (40, 4, 29, 16, 3), (60, 3, 29, 128, 3)]
FAMILY_CASES = ([(k, s, m) for k in ("gaussian", "peaky", "sticky") for s in SHAPES for m in (False, True)]
                + [("neg_inf", s, True) for s in sorted(NEG_INF_SEEDS)])


@functools.lru_cache(maxsize=None)
def _family_case(kind, shape, merge, dtype="float32"):
    T, B, C, W, P = shape
    rng = np.random.default_rng(NEG_INF_SEEDS[shape] if kind == "neg_inf" else sum(kind.encode()) + T)
    x = family(rng, kind, T, B, C, np.dtype(dtype))
    x.setflags(write=False)
    sl = _lengths(T, B)
    kw = dict(merge_repeated=merge, blank_index=0, blank_label=-1)
    return x, sl, kw, expected(x, sl, W, P, T, **kw)


@pytest.mark.parametrize("kind,shape,merge", FAMILY_CASES,
                         ids=["%s-%s-%s" % (k, "x".join(map(str, s)), "merge" if m else "plain") for k, s, m in FAMILY_CASES])
def test_dense_matches_definition(kind, shape, merge, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = shape
    x, sl, kw, (dec, ali, want) = _family_case(kind, shape, merge)
    if kind == "neg_inf":
        # on the oracle's own rows: an alignment shorter than its item, an untimed token
        assert any(len(ali[b][p]) < sl[b] for b in range(B) for p in range(P))
        assert any((want[0][b, p, :len(dec[b][p])] < 0).any() for b in range(B) for p in range(P))
    if kind == "peaky" and T >= 12:
        assert (want[2] > 0).any()
    out, tt = _dense(np.array(x), sl, W, P, **kw)
    assert tuple(tt.start.shape) == (B, P, T) and tuple(tt.trailing_blank.shape) == (B, P) and tt.start.is_cuda
    _assert_times(tt, want, what="%s %s" % (kind, shape))
    assert _host([out.status])[0].tolist() == [0] * B
    ctcext_amd.dense_check()


TILED = [(700, 3, 5, 8, 3), (257, 2, 4, 4, 4)]


@functools.lru_cache(maxsize=None)
def _tiled_case(shape):
    T, B, C, W, P = shape
    # (T = 700: a seed, picked on the CPU, at which the straddling cases asserted below exist)
    x = family(np.random.default_rng(17 if T == 700 else T), "sticky", T, B, C)
    sl = np.array([T, T - 177, 0] if B == 3 else [T, T - 1], np.int32)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    live = [b for b in range(B) if sl[b] > 0]   # (an item without frames has fewer leaves than top_paths)
    dec, ali, want_live = expected(x[:, live], sl[live], W, P, T, **kw)
    want = [np.full((B,) + w.shape[1:], -1 if w.ndim == 3 else 0, np.int32) for w in want_live]
    for w, wl in zip(want, want_live):
        w[live] = wl
    return x, sl, kw, live, dec, ali, want


@pytest.mark.parametrize("shape", TILED, ids=lambda s: "x".join(map(str, s)))
def test_rows_longer_than_the_kernel_tile(shape, monkeypatch):
    """Rows of several tiles: the carries between tiles.  At T = 700 the
    expected values themselves show a token span, and a merged token of several
    runs, lying across a tile boundary of the kernel as built (tiles count from
    the last frame)."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = shape
    tile = _lib.load().ctcext_token_times_tile()
    x, sl, kw, live, dec, ali, want = _tiled_case(shape)
    if T >= 2 * tile + 1:
        span = multi = 0
        for i, b in enumerate(live):
            for p in range(P):
                runs = runs_of(ali[i][p], int(sl[b]), -1)
                for k in range(1, int(sl[b]) // tile + 1):
                    fb = int(sl[b]) - k * tile          # the first frame of the tile nearer the end
                    for j in range(len(dec[i][p])):
                        s, e = want[0][b, p, j], want[1][b, p, j]
                        if 0 <= s < fb <= e:
                            span += 1
                            mine = [r for r in runs if s <= r[1] and r[2] <= e]
                            multi += any(r[2] < fb for r in mine) and any(r[1] >= fb for r in mine)
        assert span > 0 and multi > 0, (span, multi)
    out, tt = _dense(x, sl, W, P, **kw)
    _assert_times(tt, want, what=str(shape))
    assert _host([out.status])[0].tolist() == [0 if b in live else _lib.CTCEXT_ITEM_FEW_LEAVES for b in range(B)]


def test_float64(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (12, 6, 5, 8, 3)
    T, B, C, W, P = shape
    x, sl, kw, (dec, ali, want) = _family_case("gaussian", shape, True, "float64")
    out, tt = _dense(np.array(x), sl, W, P, **kw)
    assert out.log_probability.dtype == torch.float64
    _assert_times(tt, want, what="float64")


@pytest.mark.parametrize("blank_index,blank_label", [(2, 2), (0, 29 + 4)])
def test_blank_label_forms(blank_index, blank_label, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 4, 29, 16, 3
    x = family(np.random.default_rng(5), "peaky", T, B, C, blank=blank_index)
    sl = _lengths(T, B)
    kw = dict(merge_repeated=True, blank_index=blank_index, blank_label=blank_label)
    dec, ali, want = expected(x, sl, W, P, T, **kw)
    assert (want[2] > 0).any() and (want[0] >= 0).any()
    out, tt = _dense(x, sl, W, P, **kw)
    _assert_times(tt, want, what="blank %d/%d" % (blank_index, blank_label))


def test_blank_label_that_is_a_class_label_is_refused(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 12, 2, 5, 8, 1
    x = family(np.random.default_rng(6), "gaussian", T, B, C)
    ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), [T, T], W, P, batch_first=False, blank_label=3)
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.dense_token_times()
    assert e.value.message == MSG and e.value.error_code == _lib.CTCEXT_INVALID_ARGUMENT
    ctcext_amd.dense_check()


def test_item_with_a_status_bit_is_empty_and_alone(monkeypatch):
    """sequence_length above max_time: that item's rows are -1, its
    trailing_blank 0, and its neighbours are what they are without it."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (12, 6, 5, 8, 3)
    T, B, C, W, P = shape
    x, sl, kw, (dec, ali, want) = _family_case("peaky", shape, False)
    bad = np.array(sl)
    bad[1] = T + 1
    out, tt = _dense(np.array(x), bad, W, P, **kw)
    got = _host(tt)
    assert (got[0][1] == -1).all() and (got[1][1] == -1).all() and (got[2][1] == 0).all()
    _assert_times(tt, want, items=[0, 2, 3, 4, 5], what="neighbours")
    assert _host([out.status])[0].tolist() == [0, _lib.CTCEXT_ITEM_LENGTH, 0, 0, 0, 0]
    with pytest.raises(ctcext_amd.FailedPreconditionError):
        ctcext_amd.dense_check()


def test_optional_outputs_through_the_c_abi(monkeypatch):
    """trailing_blank may be NULL; start and end come both or neither."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (40, 4, 29, 16, 3)
    T, B, C, W, P = shape
    x, sl, kw, (dec, ali, want) = _family_case("peaky", shape, True)
    _dense(np.array(x), sl, W, P, **kw)
    d = ctcext_amd.get_decoder(0)

    def fresh():
        return (torch.full((B, P, T), 77, dtype=torch.int32, device=DEV), torch.full((B, P, T), 77, dtype=torch.int32, device=DEV),
                torch.full((B, P), 77, dtype=torch.int32, device=DEV))

    def call(start, end, trail):
        o = _lib.TokenTimesOut()
        o.start, o.end, o.trailing_blank = [None if t is None else t.data_ptr() for t in (start, end, trail)]
        return d.lib.ctcext_dense_token_times(d.handle, ctypes.byref(o))

    s, e, t = fresh()
    assert call(s, e, None) == _lib.CTCEXT_OK
    _assert_times((s, e), want[:2], what="no trailing_blank")
    assert (t == 77).all().item()
    s, e, t = fresh()
    assert call(None, None, t) == _lib.CTCEXT_OK
    np.testing.assert_array_equal(_host([t])[0], want[2])
    assert (s == 77).all().item() and (e == 77).all().item()
    for args in ((s, None, t), (None, e, t), (None, None, None)):
        assert call(*args) == _lib.CTCEXT_INVALID_ARGUMENT
    ctcext_amd.dense_check()


def test_without_a_dense_decode_fails_precondition(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    x = family(np.random.default_rng(7), "gaussian", 6, 2, 4)
    ctcext_amd.decode_logits(torch.as_tensor(x, device=DEV), [6, 6], 8, 1, batch_first=False)   # ends any dense call
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.dense_token_times()
    assert e.value.message == "ctcext_dense_token_times without a ctcext_decode_dense"


# ---- 2. the call only enqueues; graph capture

@functools.lru_cache(maxsize=None)
def _async_times():
    T, B, C, W, P = ASYNC_SHAPE
    x, sl, dense = _async_case()
    dec, ali = _rows_from_dense(dense, range(B))
    return expected_from_rows(dec, ali, sl, B, P, T, -1, True)


@pytest.mark.parametrize("where", ["default_stream", "side_stream"])
def test_call_only_enqueues(where, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = ASYNC_SHAPE
    x, sl, _ = _async_case()
    want = _async_times()
    xd, sld = torch.as_tensor(x, device=DEV), torch.as_tensor(sl, device=DEV)
    stream = torch.cuda.Stream(device=DEV) if where == "side_stream" else torch.cuda.default_stream(DEV)

    def blocked(*a, **k):
        raise AssertionError("dense_token_times reached a host synchronisation")

    with torch.cuda.stream(stream):
        ctcext_amd.decode_dense(xd, sld, W, P, batch_first=False, merge_repeated=True)   # warm-up: workspace, kernels
        ctcext_amd.dense_token_times()
        torch.cuda.synchronize()
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "synchronize", blocked)
            m.setattr(torch.cuda.Stream, "synchronize", blocked)
            m.setattr(torch.Tensor, "cpu", blocked)
            m.setattr(torch.Tensor, "item", blocked)
            ctcext_amd.decode_dense(xd, sld, W, P, batch_first=False, merge_repeated=True)
            tt = ctcext_amd.dense_token_times()
        ev = torch.cuda.Event()
        ev.record()
        done_at_return = ev.query()
        ev.synchronize()
    assert not done_at_return, "the work had finished when dense_token_times returned: it did not only enqueue"
    _assert_times(tt, want, what=where)
    ctcext_amd.dense_check()


def test_graph_capture_and_replay(monkeypatch):
    """decode_dense and dense_token_times captured together on a side stream
    and replayed on new logits and lengths; the workspace of the captured shape
    comes from ctcext_dense_reserve alone, so a call that allocated from HIP,
    freed or blocked would fail the capture."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 3, 20, 100, 3
    rng = np.random.default_rng(405)
    side = torch.cuda.Stream(device=DEV)
    kw = dict(batch_first=False, merge_repeated=True, pad_value=-7)
    with torch.cuda.stream(side):
        ctcext_amd.decode_dense(torch.zeros((4, 1, C), device=DEV), torch.full((1,), 4, dtype=torch.int32, device=DEV),
                                W, P, **kw)
        ctcext_amd.dense_token_times()   # loads the kernel
    side.synchronize()
    xs = torch.zeros((T, B, C), device=DEV)
    sls = torch.zeros((B,), dtype=torch.int32, device=DEV)
    dec = ctcext_amd.get_decoder(0)
    a = ops._args(xs.data_ptr(), (T, B, C), _lib.CTCEXT_F32, True, sls.data_ptr(), (B,), W, P, True, 0, -1, 0, None)
    assert dec.lib.ctcext_dense_reserve(dec.handle, ctypes.byref(a)) == _lib.CTCEXT_OK
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctcext_amd.decode_dense(xs, sls, W, P, **kw)
        tt = ctcext_amd.dense_token_times()
    for sl in ([T, T - 7, 3], [5, T, T - 1]):
        x = family(rng, "sticky", T, B, C)
        xs.copy_(torch.as_tensor(x))
        sls.copy_(torch.as_tensor(np.asarray(sl, np.int32)))
        torch.cuda.synchronize()
        g.replay()
        _assert_times(tt, expected(x, sl, W, P, T, merge_repeated=True)[2], what="replay %s" % (sl,))
        assert ctcext_amd.dense_check()["records_written"] > 0


# ---- 3. streams

STREAM_SHAPES = [(40, 3, 6, 16, 3), (40, 3, 29, 128, 3)]
PUSH_FRAMES = (3, 1, 1, 5, 7, 4, 4, 4, 4, 4, 3)   # 40 in all
NO_FRAMES = (2, 1)    # (push, item): the item gets no frame in that push
RESET = (4, 2)        # (push, item): the item starts a new utterance with that push


class _Script:
    """Per push: the chunk [t, B, C], the lengths, the reset flags, and the
    oracle's token times of what each item holds afterwards."""

    def __init__(self, shape, seed, merge=True):
        T, B, C, W, P = shape
        rng = np.random.default_rng(seed)
        utt = family(rng, "sticky", 2 * T, B, C)   # item b's frames, in the order it is given them
        kw = dict(merge_repeated=merge, blank_index=0, blank_label=-1)
        at, begin = [0] * B, [0] * B
        self.pushes = []
        for i, t in enumerate(PUSH_FRAMES):
            n = [0 if (i, b) == NO_FRAMES else t for b in range(B)]
            reset = [1 if (i, b) == RESET else 0 for b in range(B)]
            chunk = np.zeros((t, B, C), np.float32)
            for b in range(B):
                if reset[b]:
                    begin[b] = at[b]
                chunk[:n[b], b] = utt[at[b]:at[b] + n[b], b]
                at[b] += n[b]
            frames = [a - s for a, s in zip(at, begin)]
            held = np.zeros((max(frames), B, C), np.float32)
            for b in range(B):
                held[:frames[b], b] = utt[begin[b]:at[b], b]
            want = expected(held, frames, W, P, T, **kw)[2]
            self.pushes.append((chunk, np.array(n, np.int32), np.array(reset, np.int32), frames, want))
        self.kw = kw


@functools.lru_cache(maxsize=None)
def _script(shape, seed=0):
    return _Script(shape, seed + shape[3])


def _i32(v):
    return torch.as_tensor(np.asarray(v, np.int32), device=DEV)


@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream_times_after_every_push(shape, monkeypatch):
    """Pushes of 3, 1, 1, 5, 7 frames, then fours: after every one the times are
    the definition's on the oracle's decode of what each item holds.  Item 1
    gets no frame in the third push; item 2 is reset with the fifth and its
    frames restart at 0."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = shape
    sc = _script(shape)
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, **sc.kw) as s:
        with pytest.raises(ctcext_amd.FailedPreconditionError):
            s.token_times_dense()   # no enqueue-only push yet
        got = []
        for chunk, n, reset, frames, want in sc.pushes:
            out = s.push_dense(torch.as_tensor(chunk, device=DEV), _i32(n), reset=_i32(reset), batch_first=False)
            got.append((out, s.token_times_dense()))
        s.check()
        for i, ((out, tt), (chunk, n, reset, frames, want)) in enumerate(zip(got, sc.pushes)):
            assert _host([out.frames])[0].tolist() == frames, i
            assert tuple(tt.start.shape) == (B, P, T)
            _assert_times(tt, want, what="push %d" % i)
        assert got[-1][0].frames.cpu().tolist()[0] == T and RESET[0] < len(sc.pushes)
        # a push without hypothesis outputs leaves nothing to time
        s.reset()
        s.push_dense(torch.as_tensor(sc.pushes[0][0], device=DEV), batch_first=False, results=False)
        with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
            s.token_times_dense()
        assert e.value.error_code == _lib.CTCEXT_FAILED_PRECONDITION
        s.check()


def test_two_streams_of_one_decoder_read_their_own_buffers(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = STREAM_SHAPES[0]
    T, B, C, W, P = shape
    sa, sb = _script(shape), _script(shape, 100)
    a = ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, **sa.kw)
    b = ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, **sb.kw)
    got = []
    for pa, pb in zip(sa.pushes, sb.pushes):
        a.push_dense(torch.as_tensor(pa[0], device=DEV), _i32(pa[1]), reset=_i32(pa[2]), batch_first=False)
        b.push_dense(torch.as_tensor(pb[0], device=DEV), _i32(pb[1]), reset=_i32(pb[2]), batch_first=False)
        got.append((a.token_times_dense(), b.token_times_dense()))   # a's after b's push went in
    a.check()
    b.check()
    assert any((pa[4][0] != pb[4][0]).any() for pa, pb in zip(sa.pushes, sb.pushes))
    for i, ((ta, tb), pa, pb) in enumerate(zip(got, sa.pushes, sb.pushes)):
        _assert_times(ta, pa[4], what="stream a push %d" % i)
        _assert_times(tb, pb[4], what="stream b push %d" % i)
    a.close()
    b.close()


# ---- 4. the synchronous form

def test_token_times_after_decode_logits_equals_the_dense_form(monkeypatch):
    """C = 29, W = 128, T = 40: the record ring runs (tests/test_gpu_layouts.py)."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 3, 29, 128, 3
    x = family(np.random.default_rng(9), "sticky", T, B, C)
    sl = _lengths(T, B)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    want = expected(x, sl, W, P, T, **kw)[2]
    ctcext_amd.decode_logits(torch.as_tensor(x, device=DEV), torch.as_tensor(sl, device=DEV), W, P, batch_first=False, **kw)
    assert ctcext_amd.get_decoder(0).last_stats["ring_frames"] > 0
    tt = ctcext_amd.token_times()
    assert tt.start.is_cuda and tuple(tt.start.shape) == (B, P, T)
    _assert_times(tt, want, what="device outputs")
    # host logits: numpy out
    ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, **kw)
    th = ctcext_amd.token_times()
    assert isinstance(th.start, np.ndarray)
    _assert_times(th, want, what="host outputs")
    out, td = _dense(x, sl, W, P, **kw)
    _assert_times(td, [np.asarray(t) for t in th], what="dense form")
    with pytest.raises(ctcext_amd.FailedPreconditionError):
        ctcext_amd.token_times()   # a dense call leaves nothing to fetch


def test_token_times_after_push(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = STREAM_SHAPES[0]
    T, B, C, W, P = shape
    sc = _script(shape)
    chunk, n, reset, frames, want = sc.pushes[0]
    with ctcext_amd.StreamDecoder(B, C, W, P, T, **sc.kw) as s:
        s.push(chunk, n, batch_first=False)
        tt = ctcext_amd.token_times()
        assert isinstance(tt.start, np.ndarray) and tt.start.shape == (B, P, T)
        _assert_times(tt, want, what="after push")
        chunk2, n2, _, frames2, want2 = sc.pushes[1]
        s.push(chunk2, n2, batch_first=False)
        _assert_times(ctcext_amd.token_times(), want2, what="after the second push")
