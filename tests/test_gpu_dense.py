"""The dense, enqueue-only decode (ctcext_decode_dense / decode_dense) on the
GPU, against the CPU oracle: padded outputs over each kernel family, the
per-item status and the deferred errors of dense_check, that the call only
enqueues, graph capture and the shape edges."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
import oracle
import range_inputs
from ctcext_amd import _lib, ops
from test_gpu_kernel_matrix import SMALL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GS = _lib.CTCEXT_FLAG_GLOBAL_STATE
LENGTH, FEW, TIMEOUT, TABLE = (_lib.CTCEXT_ITEM_LENGTH, _lib.CTCEXT_ITEM_FEW_LEAVES,
                               _lib.CTCEXT_ITEM_HELPER_TIMEOUT, _lib.CTCEXT_ITEM_TABLE)
FEW_MSG = "Less leaves in the beam search than requested."
TABLE_MSG = "beam scorer table entries must be log-probabilities (<= 0)"
TIMEOUT_MSG = "decode kernel: a helper-wave hand-over wait timed out"


def to_dense(ref, B, P, T, pad):
    """The oracle's SparseTensor components as the padded tensors of
    DenseDecode: (decoded, decoded_lengths, alignment, alignment_lengths,
    log_probability)."""
    dec = np.full((B, P, T), pad, np.int64)
    ali = np.full((B, P, T), pad, np.int64)
    dl = np.zeros((B, P), np.int32)
    al = np.zeros((B, P), np.int32)
    for p in range(P):
        for idx, val, arr, ln in ((ref.decoded_indices[p], ref.decoded_values[p], dec, dl),
                                  (ref.alignment_indices[p], ref.alignment_values[p], ali, al)):
            for (b, i), v in zip(np.asarray(idx).reshape(-1, 2), np.asarray(val)):
                arr[b, p, i] = v
                ln[b, p] = max(ln[b, p], i + 1)
    return dec, dl, ali, al, np.asarray(ref.log_probability)


def _host(out):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _assert_dense(out, want, items=None, status=0):
    """out (DenseDecode) equals want (to_dense) bit for bit on `items` (all),
    whose status is `status`."""
    got = _host(out)
    sel = slice(None) if items is None else list(items)
    for name, g, w in zip(ctcext_amd.DenseDecode._fields, got[:5], want):
        assert g.dtype == w.dtype, (name, g.dtype, w.dtype)
        np.testing.assert_array_equal(g[sel], w, err_msg=name)
    np.testing.assert_array_equal(got[5][sel], status, err_msg="status")


def _assert_empty(out, items, pad):
    got = _host(out)
    for b in items:
        assert (got[0][b] == pad).all() and (got[2][b] == pad).all(), b
        assert (got[1][b] == 0).all() and (got[3][b] == 0).all(), b
        assert np.isneginf(got[4][b]).all(), (b, got[4][b])


def _inputs(rng, kind, T, B, C, dtype=np.float32):
    if kind in ("logsoftmax", "edges"):   # the whole float range (tests/range_inputs.py)
        return range_inputs.family(rng, kind, T, B, C, dtype)
    x = rng.standard_normal((T, B, C))
    if kind == "ties":
        x = np.round(x * 2) / 2
    elif kind == "neg_inf":
        x[rng.random(x.shape) < 0.15] = -np.inf
    return x.astype(dtype)


def _kw(kind, C):
    # merge_repeated both ways, a non-zero blank, a blank_label that is not the default
    return {"normal": dict(merge_repeated=False, blank_index=0, blank_label=C),
            "ties": dict(merge_repeated=True, blank_index=C // 2, blank_label=C + 3),
            "neg_inf": dict(merge_repeated=True, blank_index=0, blank_label=-2),
            "logsoftmax": dict(merge_repeated=True, blank_index=C // 2, blank_label=C + 3),
            "edges": dict(merge_repeated=False, blank_index=0, blank_label=C)}[kind]


def _table(rng, C, dtype):
    return (-np.abs(rng.standard_normal((C + 1, C))) * 2).astype(dtype)


# ---- 1. parity with the oracle over each kernel family

# id -> ((T, C, W, P), dtype, CTCEXT_HELPER or None, flags, bigram, the kernel the call must have run)
PARITY = {
    "one_wave": (SMALL[(1, 128, False)], np.float32, "0", 0, False, dict(helper="none", RN=1, BIG=False)),
    "two_wave": (SMALL[(1, 128, False)], np.float32, None, 0, False, dict(helper="SQ", BIG=False)),
    "large_c": (SMALL[(1, 128, True)], np.float32, None, 0, False, dict(BIG=True)),
    "beam_400": (SMALL[(4, 0, False)], np.float32, None, 0, False, dict(RN=4, WC=0)),
    "float64": (SMALL[(1, 128, False)], np.float64, None, 0, False, dict(dtype="f64")),
    "global_state": ((10, 8, 40, 3), np.float32, None, GS, False, dict(tier=1)),
    "bigram": (SMALL[(1, 128, False)], np.float32, None, 0, True, dict(scorer="bigram")),
    "odd_max_time": ((7, 6, 16, 3), np.float32, None, 0, False, dict()),
}
PAD = -7


@pytest.mark.parametrize("name", sorted(PARITY))
def test_dense_matches_oracle(name, monkeypatch):
    (T, C, W, P), dtype, helper_env, flags, bigram, kernel = PARITY[name]
    if helper_env is None:
        monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    else:
        monkeypatch.setenv("CTCEXT_HELPER", helper_env)
    rng = np.random.default_rng(sum(name.encode()))
    B = 3
    sl = np.array([T, max(T - 3, 1), T // 2], np.int32)
    tab = _table(rng, C, dtype) if bigram else None
    for kind in ("normal", "ties", "neg_inf"):
        kw = _kw(kind, C)
        x = _inputs(rng, kind, T, B, C, dtype)
        ref = oracle.decode(x, sl, W, P, scorer_table=tab, **kw)
        out = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), torch.as_tensor(sl, device=DEV), W, P,
                                      batch_first=False, pad_value=PAD, flags=flags,
                                      scorer_table=None if tab is None else torch.as_tensor(tab, device=DEV), **kw)
        assert tuple(out.decoded.shape) == (B, P, T) and out.status.dtype == torch.int32
        _assert_dense(out, to_dense(ref, B, P, T, PAD))
        st = ctcext_amd.dense_check()
        k = st["kernel"]
        assert k["launched"], st
        for key, v in kernel.items():
            assert k[key] == v, (name, kind, key, k)
        assert st["records_written"] > 0, st
        # after a dense call there is nothing for ctcext_fetch
        with pytest.raises(ctcext_amd.FailedPreconditionError):
            ctcext_amd.get_decoder(0).fetch([[0], [0], [0], [0], [0], [0]], 0, True)


@pytest.mark.parametrize("kind", ["logsoftmax", "edges"])
@pytest.mark.parametrize("name", ["two_wave", "large_c"])
def test_dense_numeric_range(name, kind, monkeypatch):
    """log_softmax outputs, and terms at expf's underflow bound and in its
    subnormal band, through the enqueue-only call: a small-C and a large-C
    kernel family."""
    (T, C, W, P), dtype, helper_env, flags, bigram, kernel = PARITY[name]
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    rng = range_inputs.rng_for("dense/%s/%s" % (name, kind))
    B = 3
    sl = np.array([T, max(T - 3, 1), T // 2], np.int32)
    kw = _kw(kind, C)
    x = _inputs(rng, kind, T, B, C, dtype)
    range_inputs.assert_census(kind, np.concatenate([x[:n, b] for b, n in enumerate(sl)]))
    ref = oracle.decode(x, sl, W, P, **kw)
    out = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), torch.as_tensor(sl, device=DEV), W, P,
                                  batch_first=False, pad_value=PAD, flags=flags, **kw)
    _assert_dense(out, to_dense(ref, B, P, T, PAD))
    st = ctcext_amd.dense_check()
    assert st["kernel"]["launched"], st
    for key, v in kernel.items():
        assert st["kernel"][key] == v, (name, kind, key, st["kernel"])
    assert st["literal_nonfinite"] == 0, st


def test_dense_bf16_vocabulary_slice_in_place():
    """A batch-major bf16 view with gaps in both dimensions, read in place."""
    T, C, W, P = SMALL[(1, 128, False)]
    B = 3
    rng = np.random.default_rng(2026)
    full = torch.as_tensor(rng.standard_normal((B, T, C + 6)).astype(np.float32), device=DEV).to(torch.bfloat16)
    view = full[:, :, 3:3 + C]
    assert not view.is_contiguous()
    sl = np.array([T, T - 3, T // 2], np.int32)
    x = view.float().transpose(0, 1).contiguous().cpu().numpy()   # the widened slice, [T, B, C]
    ref = oracle.decode(x, sl, W, P, merge_repeated=True)
    out = ctcext_amd.decode_dense(view, torch.as_tensor(sl, device=DEV), W, P, merge_repeated=True)
    assert out.log_probability.dtype == torch.float32
    _assert_dense(out, to_dense(ref, B, P, T, -1))
    ctcext_amd.dense_check()


@pytest.mark.parametrize("T", [8, 7])
def test_dense_output_base_8_bytes_off_16(T):
    """Preallocated outputs whose base is 8 bytes off 16-byte alignment: with
    T = 8 every row starts 8 bytes off (a lone first and last element around
    the 16-byte stores), with T = 7 every other one; nothing is written
    outside the view."""
    C, W, P, B = 6, 16, 3, 3
    rng = np.random.default_rng(88 + T)
    x = _inputs(rng, "normal", T, B, C)
    sl = np.array([T, T - 2, 1], np.int32)
    n = B * P * T
    bufs = [torch.full((n + 2,), 4242, dtype=torch.int64, device=DEV) for _ in range(2)]
    views = [b[1:1 + n].view(B, P, T) for b in bufs]
    for v in views:
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    fresh = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), sl, W, P, batch_first=False, pad_value=PAD)
    outs = ctcext_amd.DenseDecode(views[0], fresh.decoded_lengths, views[1], fresh.alignment_lengths,
                                  fresh.log_probability, fresh.status)
    got = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), torch.as_tensor(sl, device=DEV), W, P,
                                  batch_first=False, pad_value=PAD, out=outs)
    assert got.decoded.data_ptr() == views[0].data_ptr()
    _assert_dense(got, to_dense(oracle.decode(x, sl, W, P), B, P, T, PAD))
    for b in bufs:
        assert b[0].item() == 4242 and b[-1].item() == 4242
    ctcext_amd.dense_check()


# ---- 2. per-item status and the deferred errors

def _status_x():
    return np.random.default_rng(7).standard_normal((6, 3, 2)).astype(np.float32)


def _alone(x, b, W, P, T, pad=-1):
    """Item b decoded by the oracle on its own, as dense rows."""
    return to_dense(oracle.decode(x[:, b:b + 1], [x.shape[0]], W, P), 1, P, T, pad)


def _assert_items_alone(out, x, items, W, P):
    got = _host(out)
    for b in items:
        want = _alone(x, b, W, P, x.shape[0])
        for name, g, w in zip(ctcext_amd.DenseDecode._fields, got[:5], want):
            np.testing.assert_array_equal(g[b:b + 1], w, err_msg="%s item %d" % (name, b))


def test_status_few_leaves_is_per_item():
    x, W, P = _status_x(), 8, 3
    with pytest.raises(oracle.OracleError, match=FEW_MSG):
        oracle.decode(x, [6, 1, 6], W, P)
    out = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), [6, 1, 6], W, P, batch_first=False)
    got = _host(out)
    assert got[5].tolist() == [0, FEW, 0]
    _assert_empty(out, [1], -1)
    _assert_items_alone(out, x, [0, 2], W, P)
    assert got[1][0].tolist() == [2, 3, 1] and got[1][2].tolist() == [1, 2, 3]
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.dense_check()
    assert e.value.message == FEW_MSG and e.value.error_code == _lib.CTCEXT_INVALID_ARGUMENT


def test_status_length_above_max_time_is_per_item():
    x, W, P = _status_x(), 8, 3
    with pytest.raises(oracle.OracleError) as oe:
        oracle.decode(x, [6, 7, 6], W, P)
    assert str(oe.value) == "sequence_length(1) <= 6"
    out = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), [6, 7, 6], W, P, batch_first=False)
    assert _host(out)[5].tolist() == [0, LENGTH, 0]
    _assert_empty(out, [1], -1)
    _assert_items_alone(out, x, [0, 2], W, P)
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.dense_check()
    assert e.value.message == "sequence_length(1) <= 6"


def test_negative_length_reads_as_zero():
    x, W, P = _status_x(), 8, 1
    ref = oracle.decode(x, [6, -2, 6], W, P)
    out = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), [6, -2, 6], W, P, batch_first=False)
    _assert_dense(out, to_dense(ref, 3, P, 6, -1))
    got = _host(out)
    assert got[1][1].tolist() == [0] and got[3][1].tolist() == [0]
    ctcext_amd.dense_check()


def test_status_bad_table_empties_every_item():
    x, W, P = _status_x(), 8, 3
    tab = -np.abs(np.random.default_rng(8).standard_normal((3, 2))).astype(np.float32)
    good = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), [6, 6, 6], W, P, batch_first=False,
                                   scorer_table=torch.as_tensor(tab, device=DEV))
    _assert_dense(good, to_dense(oracle.decode(x, [6, 6, 6], W, P, scorer_table=tab), 3, P, 6, -1))
    ctcext_amd.dense_check()
    tab[2, 1] = 0.5
    out = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), [6, 6, 6], W, P, batch_first=False,
                                  scorer_table=torch.as_tensor(tab, device=DEV))
    assert _host(out)[5].tolist() == [TABLE, TABLE, TABLE]
    _assert_empty(out, [0, 1, 2], -1)
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.dense_check()
    assert e.value.message == TABLE_MSG
    # a NaN entry is refused as well
    tab[2, 1] = np.nan
    out = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), [6, 6, 6], W, P, batch_first=False,
                                  scorer_table=torch.as_tensor(tab, device=DEV))
    assert _host(out)[5].tolist() == [TABLE, TABLE, TABLE]


def test_status_helper_timeout(monkeypatch):
    """CTCEXT_FLAG_TEST_HELPER_DEAD: the two-wave kernel's failure path (no
    hang, no re-decode): every item reports it, and the next call is right."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, C, W, P = SMALL[(1, 128, False)]
    B = 3
    x = _inputs(np.random.default_rng(31), "normal", T, B, C)
    sl = np.full(B, T, np.int32)
    xd, sld = torch.as_tensor(x, device=DEV), torch.as_tensor(sl, device=DEV)
    out = ctcext_amd.decode_dense(xd, sld, W, P, batch_first=False, flags=_lib.CTCEXT_FLAG_TEST_HELPER_DEAD)
    assert _host(out)[5].tolist() == [TIMEOUT] * B
    _assert_empty(out, range(B), -1)
    with pytest.raises(ctcext_amd.InternalError) as e:
        ctcext_amd.dense_check()
    assert e.value.message == TIMEOUT_MSG and e.value.error_code == _lib.CTCEXT_INTERNAL
    assert ctcext_amd.get_decoder(0).last_stats["helper_redecodes"] == 0
    out = ctcext_amd.decode_dense(xd, sld, W, P, batch_first=False)
    _assert_dense(out, to_dense(oracle.decode(x, sl, W, P), B, P, T, -1))
    assert ctcext_amd.dense_check()["kernel"]["helper"] == "SQ"


# ---- 3. the call only enqueues

ASYNC_SHAPE = (600, 2, 29, 128, 3)


@functools.lru_cache(maxsize=None)
def _async_case():
    T, B, C, W, P = ASYNC_SHAPE
    x = np.random.default_rng(600).standard_normal((T, B, C)).astype(np.float32)
    sl = np.array([T, T - 50], np.int32)
    return x, sl, to_dense(oracle.decode(x, sl, W, P, merge_repeated=True), B, P, T, -1)


@pytest.mark.parametrize("where", ["default_stream", "side_stream"])
def test_call_only_enqueues(where, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = ASYNC_SHAPE
    x, sl, want = _async_case()
    xd, sld = torch.as_tensor(x, device=DEV), torch.as_tensor(sl, device=DEV)
    stream = torch.cuda.Stream(device=DEV) if where == "side_stream" else torch.cuda.default_stream(DEV)

    def blocked(*a, **k):
        raise AssertionError("decode_dense reached a host synchronisation")

    with torch.cuda.stream(stream):
        if where == "default_stream":
            assert torch.cuda.current_stream(DEV).cuda_stream == 0   # the null-stream flag's path
        ctcext_amd.decode_dense(xd, sld, W, P, batch_first=False, merge_repeated=True)   # warm-up: workspace, kernels
        torch.cuda.synchronize()
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "synchronize", blocked)
            m.setattr(torch.cuda.Stream, "synchronize", blocked)
            m.setattr(torch.Tensor, "cpu", blocked)
            m.setattr(torch.Tensor, "item", blocked)
            out = ctcext_amd.decode_dense(xd, sld, W, P, batch_first=False, merge_repeated=True)
        ev = torch.cuda.Event()
        ev.record()
        done_at_return = ev.query()
        ev.synchronize()
    assert not done_at_return, "the decode had finished when decode_dense returned: it did not only enqueue"
    _assert_dense(out, want)
    ctcext_amd.dense_check()


# ---- 4. graph capture

def test_graph_capture_and_replay(monkeypatch):
    """One decode_dense captured on a side stream, replayed on new logits and
    lengths copied into the static inputs.  The workspace of the captured
    shape comes from ctcext_dense_reserve alone (the warm-up call that loads
    the kernels is a shorter, smaller batch), so a call that allocated, freed
    or blocked would fail the capture."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 3, 20, 100, 3
    rng = np.random.default_rng(404)
    side = torch.cuda.Stream(device=DEV)
    kw = dict(batch_first=False, merge_repeated=True, pad_value=PAD)
    with torch.cuda.stream(side):
        ctcext_amd.decode_dense(torch.zeros((4, 1, C), device=DEV), torch.full((1,), 4, dtype=torch.int32, device=DEV),
                                W, P, **kw)
    side.synchronize()
    xs = torch.zeros((T, B, C), device=DEV)
    sls = torch.zeros((B,), dtype=torch.int32, device=DEV)
    dec = ctcext_amd.get_decoder(0)
    a = ops._args(xs.data_ptr(), (T, B, C), _lib.CTCEXT_F32, True, sls.data_ptr(), (B,), W, P, True, 0, -1, 0, None)
    assert dec.lib.ctcext_dense_reserve(dec.handle, ctypes.byref(a)) == _lib.CTCEXT_OK
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = ctcext_amd.decode_dense(xs, sls, W, P, **kw)
    for sl in ([T, T - 7, 3], [5, T, T - 1]):
        x = _inputs(rng, "normal", T, B, C)
        xs.copy_(torch.as_tensor(x))
        sls.copy_(torch.as_tensor(np.asarray(sl, np.int32)))
        torch.cuda.synchronize()
        g.replay()
        _assert_dense(out, to_dense(oracle.decode(x, sl, W, P, merge_repeated=True), B, P, T, PAD))
        assert ctcext_amd.dense_check()["records_written"] > 0


# ---- 5. shape edges

def test_empty_batch_launches_nothing():
    out = ctcext_amd.decode_dense(torch.zeros((5, 0, 6), device=DEV), torch.zeros((0,), dtype=torch.int32, device=DEV),
                                  8, 2, batch_first=False)
    assert [tuple(t.shape) for t in out] == [(0, 2, 5), (0, 2), (0, 2, 5), (0, 2), (0, 2), (0,)]
    st = ctcext_amd.dense_check()
    assert not st["kernel"]["launched"] and st["kernel_raw"] == 0 and st["records_written"] == 0


def test_zero_length_item():
    x, W, P = _status_x(), 8, 1
    ref = oracle.decode(x, [6, 0, 3], W, P)
    out = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), torch.as_tensor([6, 0, 3], dtype=torch.int32,
                                                                                  device=DEV), W, P, batch_first=False)
    _assert_dense(out, to_dense(ref, 3, P, 6, -1))
    got = _host(out)
    assert got[1][1].tolist() == [0] and got[3][1].tolist() == [0] and got[4][1].tolist() == [0.0]
    ctcext_amd.dense_check()
