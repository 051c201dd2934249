"""Target gradients on the GPU (target_grads, dense_target_grads, score_targets_autograd): the scores' NaN and -inf
cells and the slab's zero cells exactly, finite ones within 4 E of the "Target gradients" definition in longdouble
(tgrad_util.expected)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
import tgrad_util
import tie_inputs
from ctcext_amd import _lib
from test_gpu_target_scores import RENORM, _case, _lists, _tile
from token_times_util import family

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K, K64, F = 16, 8, _tile(6)   # the checkpoint tiles (CTCEXT_TARGET_GRADS_TILE_*) and the target scores' staged tile
# E_G (the slab) and E_S (the scores): the largest |definition in the compute dtype with numpy - the same in
# longdouble| over the finite expected cells of CASES, measured on the CPU; the kernel gets 4 times that.  The
# times-20 case has bounds of its own (E_OWN), so that it widens no other case's.
# float32: E_G 6.3055e-5 (pack-N33-ones), E_S 3.4324e-5 (time-2F+1); float64: E_G 6.3182e-15, E_S 6.7897e-15 (float64);
# time-2F+1-x20: 4.8100e-4 and 3.6527e-4.
E_G = {np.float32: 6.31e-5, np.float64: 6.32e-15}
E_S = {np.float32: 3.44e-5, np.float64: 6.79e-15}
E_OWN = {"time-2F+1-x20": (4.82e-4, 3.66e-4)}


def _weights(c, seed):
    """[B, N] in [-1, 1] of the compute dtype with some exact zeros, so the scale of a cell stays O(N)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1, 1, size=c["n"].shape)
    w[rng.random(w.shape) < 0.2] = 0
    return w.astype(c["x"].dtype)


def _build(T, sl, L, weights=True, labels=None, **kw):
    c = _case(T, sl, L, **kw)
    B, N = c["n"].shape
    if N < 7:   # the lists' bad length has no room: item 1's first row takes it
        c["n"][1, 0] = L + 1
    if labels == "equal":   # the longest lists of lanes a class
        c["y"][:] = (1 + np.arange(N) % 3)[None, :, None]
    elif labels == "distinct":   # ... and the shortest
        c["y"][:] = np.stack([np.stack([np.random.default_rng(b * N + i).permutation(c["x"].shape[2] - 1)[:L] + 1
                                        for i in range(N)]) for b in range(B)])
    c["w"] = _weights(c, T + L) if weights else None
    return c


def _planted(name, kind, edges=False, **kw):
    c = tie_inputs.planted_case("target grads " + name, kind, 15, 12, edges=edges)
    return dict(c, w=_weights(c, 5), **kw)


SL = [20, 13, 0]
CASES = {"seg-L%d-%s" % (L, k): functools.partial(_build, 20, SL, L, kind=k) for L in (7, 8, 15, 16, 31, 32, 63)
         for k in ("gaussian", "sticky")}
CASES.update({"pack-N%d-%s" % (N, "w" if w else "ones"): functools.partial(_build, 20, SL, 7, N=N, weights=w)
              for N in (1, 31, 32, 33) for w in (False, True)})
CASES.update({"time-%s" % k: functools.partial(_build, T, [T, min(RENORM + 1, T - 1), T - 3], 15)
              for k, T in (("K-1", K - 1), ("K", K), ("K+1", K + 1), ("2K+1", 2 * K + 1), ("F-1", F - 1), ("F", F), ("F+1", F + 1),
                           ("2F+1", 2 * F + 1))})
CASES.update({
    "time-2F+1-x20": functools.partial(_build, 2 * F + 1, [2 * F + 1, RENORM + 1, 2 * F - 2], 15, scale=20.0),
    "labels-equal": functools.partial(_build, 33, [33, 17, 4], 15, labels="equal"),
    "labels-distinct": functools.partial(_build, 33, [33, 17, 4], 15, C=17, labels="distinct"),
    "gathered": functools.partial(_build, 33, [33, 17, 0], 15, route=2, env="gathered"),
    "C1100": functools.partial(_build, 8, [8, 5], 7, C=1100, route=2),
    "C300-short-tile": functools.partial(_build, 2 * K + 1, [2 * K + 1, 9], 7, C=300, N=8),
    "float64": functools.partial(_build, 2 * K64 + 1, [2 * K64 + 1, K64, 0], 15, dtype=np.float64),
    "float64-gathered": functools.partial(_build, 2 * K64 + 1, [2 * K64 + 1, K64, 0], 15, dtype=np.float64, route=2, env="gathered"),
    "bf16-slice": functools.partial(_build, 24, [24, 21, 12], 15, kind="sticky", half="bfloat16"),
    "blank5": functools.partial(_build, 22, [22, 17, 0], 15, kind="sticky", blank=5),
    "blank2": functools.partial(_build, 22, [22, 17, 0], 15, kind="sticky", blank=2),
    "masked": functools.partial(_planted, "masked", "masked"),
    "masked-gathered": functools.partial(_planted, "masked", "masked", route=2, env="gathered"),
    "nonfinite": functools.partial(_planted, "nonfinite", "nonfinite"),
    "nonfinite-edges": functools.partial(_planted, "nonfinite-edges", "nonfinite", edges=True),
})


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    if c.get("half"):   # values the two-byte format holds exactly
        c["x"] = torch.as_tensor(c["x"]).to(getattr(torch, c["half"])).float().numpy()
    c["scores"], c["slab"] = tgrad_util.expected(c["x"], c["sl"], c["y"], c["n"], c["w"], c.get("blank", 0))
    s, g, T = c["scores"], c["slab"], c["x"].shape[0]
    assert np.isfinite(s).any() and not np.isfinite(s).all() and np.isfinite(g).all(), name
    assert (g != 0).any() and min(c["sl"]) < T and not g[min(c["sl"]):, int(np.argmin(c["sl"]))].any(), name
    if c.get("kind") == "masked":   # -inf logits under a feasible target: zero cells inside a live item
        assert (g[np.isneginf(c["x"])] == 0).all() and np.isneginf(c["x"]).any(), name
    if c.get("kind") == "nonfinite":   # an item with a NaN: all zeros
        assert any(np.isnan(c["x"][:, b]).any() and not g[:, b].any() for b in range(len(c["sl"]))), name
    return c


def _grads(x, sl, y, n, w=None, **kw):
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), device=DEV)
    kw.setdefault("batch_first", False)
    return ctcext_amd.target_grads(x, torch.as_tensor(np.asarray(sl, np.int32), device=DEV), torch.as_tensor(y, device=DEV),
                                   torch.as_tensor(n, device=DEV), None if w is None else torch.as_tensor(w, device=DEV), **kw)


def _check(got, scores, slab, what, own=None):
    torch.cuda.synchronize()
    s, g = got.scores.cpu().numpy(), got.grad.cpu().numpy()
    assert g.shape == slab.shape and s.shape == scores.shape and g.dtype == s.dtype, what
    e_g, e_s = own or (E_G[g.dtype.type], E_S[g.dtype.type])
    for mask in (np.isnan, np.isneginf, np.isposinf):
        np.testing.assert_array_equal(mask(s), mask(scores), err_msg="%s: %s scores" % (what, mask.__name__))
    # (the definition's zero cells exactly; a cell that merely underflows in the compute dtype is a finite cell)
    assert not g[slab == 0].any(), "%s: zero cells" % what
    fin = np.isfinite(scores)
    err_s = np.abs(s[fin].astype(np.longdouble) - scores[fin]).max()
    err_g = np.abs(g.astype(np.longdouble) - slab).max()
    print(what, "largest errors: slab %.3g of %.3g, scores %.3g of %.3g" % (err_g, 4 * e_g, err_s, 4 * e_s))
    assert err_g <= 4 * e_g and err_s <= 4 * e_s, what
    return s, g


def _route():
    d, r = ctcext_amd.get_decoder(0), ctypes.c_int32(-1)
    assert d.lib.ctcext_dense_target_grads_route(d.handle, ctypes.byref(r)) == _lib.CTCEXT_OK
    return r.value


@pytest.mark.parametrize("name", list(CASES))
def test_matches_definition(name, monkeypatch):
    c = case(name)
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    monkeypatch.delenv("CTCEXT_TGRADS", raising=False)
    if "env" in c:
        monkeypatch.setenv("CTCEXT_TARGETS", c["env"])
    x, kw, slab = np.array(c["x"]), dict(blank_index=c.get("blank", 0)), c["slab"]
    T, B, C = x.shape
    if c.get("half"):   # a batch-major two-byte view with gaps in both dimensions, read in place; the slab follows it
        full = torch.zeros((B, T, 40), dtype=getattr(torch, c["half"]), device=DEV)
        full[:, :, 5:5 + C] = torch.as_tensor(x.transpose(1, 0, 2).copy(), device=DEV)
        x, slab = full[:, :, 5:5 + C], slab.transpose(1, 0, 2)
        kw["batch_first"] = True
    got = _grads(x, c["sl"], c["y"], c["n"], c["w"], **kw)
    assert got.grad.is_contiguous() and got.grad.dtype == getattr(torch, c["x"].dtype.name)
    _check(got, c["scores"], slab, name, E_OWN.get(name))
    assert _route() == c.get("route", 1)


@pytest.mark.parametrize("N", [1, 33])
def test_shared_lists_and_int32_labels_give_the_same_bits_and_so_does_a_second_call(N, monkeypatch):
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    c = case("pack-N%d-w" % N)
    B = len(c["sl"])
    y, n = np.repeat(c["y"][:1], B, 0), np.repeat(c["n"][:1], B, 0)
    want = tgrad_util.expected(c["x"], c["sl"], y, n, c["w"])
    s0, g0 = _check(_grads(c["x"], c["sl"], y, n, c["w"]), *want, "broadcast")
    for what, got in (("again", _grads(c["x"], c["sl"], y, n, c["w"])), ("shared", _grads(c["x"], c["sl"], y[0], n[0], c["w"])),
                      ("int32", _grads(c["x"], c["sl"], y.astype(np.int32), n, c["w"]))):
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.grad.cpu().numpy().view(np.uint32), g0.view(np.uint32), err_msg=what)
        np.testing.assert_array_equal(got.scores.cpu().numpy().view(np.uint32), s0.view(np.uint32), err_msg=what)


def test_item_with_a_status_bit_is_nan_with_a_zero_slab_and_alone(monkeypatch):
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    c = case("seg-L15-gaussian")
    bad = np.array(c["sl"])
    bad[0] = c["x"].shape[0] + 1
    scores, slab = c["scores"].copy(), c["slab"].copy()
    scores[0], slab[:, 0] = np.nan, 0
    _check(_grads(c["x"], bad, c["y"], c["n"], c["w"]), scores, slab, "status")


def test_autograd_backward_is_the_weighted_slab(monkeypatch):
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    c = case("seg-L15-sticky")
    x = torch.as_tensor(np.array(c["x"]), device=DEV).requires_grad_()
    args = [torch.as_tensor(np.asarray(a), device=DEV) for a in (c["sl"], c["y"], c["n"])]
    v = torch.as_tensor(c["w"], device=DEV)
    out = ctcext_amd.score_targets_autograd(x, *args, batch_first=False)
    out.backward(v)
    want = ctcext_amd.target_grads(x, *args, v, batch_first=False)
    torch.cuda.synchronize()
    assert torch.equal(x.grad, want.grad) and torch.equal(out.detach().nan_to_num(), want.scores.nan_to_num())
    _check(want, c["scores"], c["slab"], "autograd")


def test_graph_capture_and_replay(monkeypatch):
    """decode_greedy and dense_target_grads captured together after one call of the shape, replayed on new logits,
    lengths, targets and weights."""
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    T, B, C, N, L = 40, 3, 6, 20, 15
    side = torch.cuda.Stream(device=DEV)
    xs = torch.zeros((T, B, C), device=DEV)
    sls = torch.zeros((B,), dtype=torch.int32, device=DEV)
    ys = torch.zeros((B, N, L), dtype=torch.int64, device=DEV)
    ns = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    ws = torch.zeros((B, N), device=DEV)
    with torch.cuda.stream(side):
        ctcext_amd.target_grads(xs, sls, ys, ns, ws, batch_first=False)   # one call of the shape
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        got = ctcext_amd.target_grads(xs, sls, ys, ns, ws, batch_first=False)
    for sl in ([T, T - 7, 3], [5, T, T - 1], [T, 9, 0]):
        rng = np.random.default_rng(sl[1])
        x = family(rng, "sticky", T, B, C)
        y, n = _lists(rng, B, N, L, C, L)
        w = rng.uniform(-1, 1, size=n.shape).astype(np.float32)
        for dst, src in ((xs, x), (sls, np.asarray(sl, np.int32)), (ys, y), (ns, n), (ws, w)):
            dst.copy_(torch.as_tensor(src))
        torch.cuda.synchronize()
        g.replay()
        _check(got, *tgrad_util.expected(x, sl, y, n, w), "replay %s" % (sl,))


def test_preconditions_and_the_packed_limit():
    T, B, C = 6, 2, 4
    xd = torch.as_tensor(family(np.random.default_rng(7), "gaussian", T, B, C), device=DEV)
    y = torch.ones((B, 3, 2), dtype=torch.int64, device=DEV)
    n = torch.ones((B, 3), dtype=torch.int32, device=DEV)
    ctcext_amd.decode_dense(xd, [T, T], 8, 1, batch_first=False)   # no opt-in
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.dense_target_grads(y, n)
    assert e.value.message == "target gradients need a decode with token_scores=True"
    ctcext_amd.decode_logits(xd, [T, T], 8, 1, batch_first=False, token_scores=True)   # ends any dense call
    d, ms = ctcext_amd.get_decoder(0), ctypes.c_double()
    t = _lib.Targets(y.data_ptr(), n.data_ptr(), 3, 2, 0, 1)
    assert d.lib.ctcext_dense_target_grads(d.handle, ctypes.byref(t), None, xd.data_ptr(), xd.data_ptr(), 0) == \
        _lib.CTCEXT_FAILED_PRECONDITION
    assert d.lib.ctcext_last_error().decode() == "ctcext_dense_target_grads without a ctcext_decode_dense"
    ctcext_amd.decode_greedy(xd, [T, T], batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True)
    none = ctcext_amd.dense_target_grads(y[:, :0], n[:, :0])   # n_targets == 0: a zero slab
    got = ctcext_amd.dense_target_grads(y, n)
    assert d.lib.ctcext_dense_target_grads_ms(d.handle, ctypes.byref(ms)) == _lib.CTCEXT_OK and ms.value > 0
    torch.cuda.synchronize()
    assert tuple(none.scores.shape) == (B, 0) and tuple(none.grad.shape) == (T, B, C) and not none.grad.any()
    assert torch.isfinite(got.scores).all() and got.grad.any()
    with pytest.raises(ctcext_amd.InvalidArgumentError):
        ctcext_amd.dense_target_grads(y[:1], n[:1])   # not the decode's batch
    with pytest.raises(ctcext_amd.UnimplementedError, match="63"):
        ctcext_amd.dense_target_grads(torch.ones((B, 1, 64), dtype=torch.int64, device=DEV), n[:, :1])
