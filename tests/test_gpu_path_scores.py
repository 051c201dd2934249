"""Path scores on the GPU (dense_path_scores, path_scores,
StreamDecoder.path_scores_dense): -inf and NaN cells exactly, finite ones within
path_scores_util.TOL of the definition in longdouble on the CPU oracle's rows."""
import ctypes

import numpy as np
import pytest
import torch

import ctcext_amd
import path_scores_util as u
from ctcext_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KW = dict(blank_index=0, blank_label=-1)


def _check(got, want, what=""):
    torch.cuda.synchronize()
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    for mask in (np.isnan, np.isneginf, np.isposinf):
        np.testing.assert_array_equal(mask(got), mask(want), err_msg="%s: %s cells" % (what, mask.__name__))
    fin = np.isfinite(want)
    err = np.abs(got[fin].astype(np.longdouble) - want[fin])
    print(what, "largest error %.3g of %.3g" % (err.max() if err.size else 0, u.tol(what, got.dtype)))
    assert (err <= u.tol(what, got.dtype)).all(), (what, err.max())
    return got


def _dense(x, sl, W, P, merge, **kw):
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), device=DEV)
    kw.setdefault("batch_first", False)
    out = ctcext_amd.decode_dense(x, torch.as_tensor(np.asarray(sl, np.int32), device=DEV), W, P, merge_repeated=merge,
                                  token_scores=True, **KW, **kw)
    return out, ctcext_amd.dense_path_scores()


@pytest.mark.parametrize("name", list(u.BUILDERS))
def test_dense_matches_definition(name, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    c = u.case(name)
    for k, v in c.get("env", {}).items():
        monkeypatch.setenv(k, v)
    x, sl, W, P = c["x"], c["sl"], c["W"], c["P"]
    T, B, C = x.shape
    kw = {} if "skip" not in c else dict(skip_blank=c["skip"])
    xd = np.array(x)
    if c.get("half"):   # a batch-major two-byte view with gaps in both dimensions, read in place
        full = torch.zeros((B, T, 40), dtype=getattr(torch, c["half"]), device=DEV)
        full[:, :, 5:5 + C] = torch.as_tensor(xd.transpose(1, 0, 2).copy(), device=DEV)
        xd = full[:, :, 5:5 + C]
        kw["batch_first"] = True
    out, ps = _dense(xd, sl, W, P, c["merge"], **kw)
    assert ps.is_cuda and tuple(ps.shape) == (B, P) and ps.dtype == getattr(torch, x.dtype.name)
    _check(ps, c["want"], name)
    assert out.status.cpu().tolist() == [0] * B
    ctcext_amd.dense_check()
    if "skip" in c:   # the synchronous form after a skipping call: the staged rows, the plan's normaliser
        ctcext_amd.decode_logits(np.array(x), sl, W, P, batch_first=False, merge_repeated=True, skip_blank=c["skip"],
                                 token_scores=True, **KW)
        _check(ctcext_amd.path_scores(), c["want"], name + ", synchronous")


def test_item_with_a_status_bit_is_nan_and_alone(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    c = u.case("peaky-12x6x5x8x3-plain")
    bad = np.array(c["sl"])
    bad[1] = c["x"].shape[0] + 1
    out, ps = _dense(np.array(c["x"]), bad, c["W"], c["P"], False)
    want = c["want"].copy()
    want[1] = np.nan
    _check(ps, want, "status")
    assert out.status.cpu().tolist() == [0, _lib.CTCEXT_ITEM_LENGTH, 0, 0, 0, 0]


def test_preconditions_and_the_blank_label_rule(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C = 6, 2, 4
    xd = torch.as_tensor(u.family(np.random.default_rng(7), "gaussian", T, B, C), device=DEV)
    ctcext_amd.decode_dense(xd, [T, T], 8, 1, batch_first=False)   # no opt-in
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.dense_path_scores()
    assert e.value.message == "path scores need a decode with token_scores=True"
    ctcext_amd.decode_logits(xd, [T, T], 8, 1, batch_first=False, token_scores=True)   # ends any dense call
    d, ms = ctcext_amd.get_decoder(0), ctypes.c_double()
    assert d.lib.ctcext_dense_path_scores(d.handle, xd.data_ptr()) == _lib.CTCEXT_FAILED_PRECONDITION
    assert d.lib.ctcext_last_error().decode() == "ctcext_dense_path_scores without a ctcext_decode_dense"
    with ctcext_amd.StreamDecoder(B, C, 8, 1, T, device=DEV) as s:   # a stream without the store
        s.push_dense(xd[:3], batch_first=False)
        with pytest.raises(ctcext_amd.FailedPreconditionError):
            s.path_scores_dense()
        s.push(xd[3:], batch_first=False)   # a stream's push keeps no logits for the synchronous form
        with pytest.raises(ctcext_amd.FailedPreconditionError):
            ctcext_amd.path_scores()
        assert d.lib.ctcext_fetch_path_scores(d.handle, xd.data_ptr(), 1) == _lib.CTCEXT_FAILED_PRECONDITION
        assert d.lib.ctcext_last_error().decode().startswith("ctcext_fetch_path_scores after a stream's push")
    ctcext_amd.decode_dense(xd, [T, T], 8, 1, batch_first=False, blank_label=3, token_scores=True)
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.dense_path_scores()
    assert e.value.message == "token times need a blank_label that is no class label"
    ctcext_amd.decode_dense(xd, [T, T], 8, 1, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True)
    ctcext_amd.dense_path_scores()
    assert d.lib.ctcext_dense_path_scores_ms(d.handle, ctypes.byref(ms)) == _lib.CTCEXT_OK and ms.value > 0
    ctcext_amd.dense_check()


def test_graph_capture_and_replay(monkeypatch):
    """Decode, token times and path scores captured together and replayed on new logits."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 3, 20, 100, 3
    side = torch.cuda.Stream(device=DEV)
    kw = dict(batch_first=False, merge_repeated=True, token_scores=True)
    with torch.cuda.stream(side):
        ctcext_amd.decode_dense(torch.zeros((4, 1, C), device=DEV), torch.full((1,), 4, dtype=torch.int32, device=DEV),
                                W, P, **kw)
        ctcext_amd.dense_token_times()
        ctcext_amd.dense_path_scores()   # loads the kernels
    side.synchronize()
    xs = torch.zeros((T, B, C), device=DEV)
    sls = torch.zeros((B,), dtype=torch.int32, device=DEV)
    dec = ctcext_amd.get_decoder(0)
    a = ctcext_amd.ops._args(xs.data_ptr(), (T, B, C), _lib.CTCEXT_F32, True, sls.data_ptr(), (B,), W, P, True, 0, -1, 0, None)
    assert dec.lib.ctcext_dense_reserve(dec.handle, ctypes.byref(a)) == _lib.CTCEXT_OK
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctcext_amd.decode_dense(xs, sls, W, P, **kw)
        ctcext_amd.dense_token_times()
        ps = ctcext_amd.dense_path_scores()
    for sl in ([T, T - 7, 3], [5, T, T - 1], [T, 9, T - 2]):
        x = u.family(np.random.default_rng(sl[1]), "sticky", T, B, C)
        xs.copy_(torch.as_tensor(x))
        sls.copy_(torch.as_tensor(np.asarray(sl, np.int32)))
        torch.cuda.synchronize()
        g.replay()
        rows = u.oracle.raw_decode(x, np.asarray(sl, np.int32), W, P, True, 0, -1)[0]
        _check(ps, u.scores(x, sl, rows, P), "replay %s" % (sl,))


def test_synchronous_form_equals_the_dense_form_bit_for_bit(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    c = u.case("sticky-40x4x29x16x3-merge")
    x, sl, W, P = np.array(c["x"]), c["sl"], c["W"], c["P"]
    dense = _check(_dense(x, sl, W, P, True)[1], c["want"], "dense").view(np.uint32)
    ctcext_amd.decode_logits(torch.as_tensor(x, device=DEV), torch.as_tensor(sl, device=DEV), W, P, batch_first=False,
                             merge_repeated=True, token_scores=True, **KW)
    got = ctcext_amd.path_scores()
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), dense, err_msg="device inputs")
    ctcext_amd.decode_logits(np.ascontiguousarray(x.transpose(1, 0, 2)), sl, W, P, merge_repeated=True, token_scores=True, **KW)
    got = ctcext_amd.path_scores()
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), dense, err_msg="host inputs, batch-major")


@pytest.mark.parametrize("store", [None, "bfloat16"], ids=["float", "bf16"])
def test_stream_equals_the_one_shot_dense_value_after_every_push(store, monkeypatch):
    """Three ragged pushes, one reset: after each, bit for bit one dense decode of the frames each item holds."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 24, 3, 6, 16, 3
    x = u.family(np.random.default_rng(62), "sticky", T, B, C)
    if store:
        x = torch.as_tensor(x).to(torch.bfloat16).float().numpy()
    xd = torch.as_tensor(x, device=DEV)
    held = [[] for _ in range(B)]   # the frames each item holds
    got, want = [], []
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, token_scores=True, score_store=store, merge_repeated=True, **KW) as s:
        for i, n in enumerate(([8, 5, 8], [8, 3, 6], [8, 8, 0])):
            reset = [0, 1, 0] if i == 1 else [0, 0, 0]
            chunk = xd[8 * i:8 * i + 8]
            s.push_dense(chunk.to(torch.bfloat16) if store else chunk, torch.as_tensor(n, dtype=torch.int32, device=DEV),
                         batch_first=False, reset=torch.as_tensor(reset, dtype=torch.int32, device=DEV))
            got.append(s.path_scores_dense())
            held = [([] if reset[b] else held[b]) + list(range(8 * i, 8 * i + n[b])) for b in range(B)]
            want.append(held)
        s.check()
    for i, held in enumerate(want):
        one = torch.zeros((T, B, C), device=DEV)
        for b in range(B):
            one[:len(held[b]), b] = xd[held[b], b]
        want[i] = _dense(one, [len(h) for h in held], W, P, True)[1]
    torch.cuda.synchronize()
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.isfinite(w).any()
        np.testing.assert_array_equal(g.cpu().numpy().view(np.uint32), w.cpu().numpy().view(np.uint32), err_msg="push %d" % i)
