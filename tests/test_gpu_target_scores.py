"""Target scores on the GPU (dense_target_scores, score_targets): NaN, -inf and
+inf cells exactly, finite ones within 4 E_T of the "Path scores" definition in
longdouble (path_scores_util.path_score) applied to every supplied target."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
import oracle
import path_scores_util as psu
from ctcext_amd import _lib
from token_times_util import family

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RENORM = psu.RENORM
# E_T: the largest |definition in the compute dtype with numpy's logaddexp -
# the same in longdouble| over the finite expected cells of CASES below,
# measured on the CPU (float32 3.7874e-4, on L140-T300, with 3.653e-4 on
# time-2F+1-x20; float64 3.0601e-14, on float64).  The kernels get 4 E_T, as
# the path-scores kernels do.
E_T = {np.float32: 3.788e-4, np.float64: 3.07e-14}


def _tile(C, f64=0):
    return _lib.load().ctcext_target_scores_tile(C, f64)


def _lists(rng, B, N, L, C, full):
    """[B, N, L] labels and [B, N] lengths: lengths 0 and 1, two adjacent rows of `full` labels without a repeat,
    "aa", a label == C, a length L + 1 (where N has room for them), the rest random."""
    y = rng.integers(0, C, size=(B, N, L)).astype(np.int64)
    n = rng.integers(0, L + 1, size=(B, N)).astype(np.int32)
    for b in range(B):
        fixed = [(0, None), (1, None), (full, "walk"), (full, "walk"), (2, [1, 1]), (min(3, L), "bad"), (L + 1, None)]
        for i, (length, what) in enumerate(fixed[:N]):
            n[b, i] = length
            if what == "walk":   # no two neighbours equal: feasible in `full` frames
                y[b, i, :full] = (np.arange(full) + b + i) % (C - 1) + 1
            elif what == "bad":
                y[b, i, length - 1] = C
            elif what:
                y[b, i, :2] = what
    return y, n


def _case(T, sl, L, C=6, N=12, kind="gaussian", scale=1.0, dtype=np.float32, full=None, seed=0, **extra):
    rng = np.random.default_rng(100 * T + L + seed)
    x = (family(rng, kind, T, len(sl), C) * scale).astype(dtype)
    y, n = _lists(rng, len(sl), N, L, C, min(L, T) if full is None else full)
    return dict(x=x, sl=np.array(sl, np.int32), y=y, n=n, **extra)


def _long():
    c = _case(300, [300, 290], 140, C=29, N=3, full=140, route=0)
    c["n"][1, 2] = 64
    return c


F = _tile(6)
CASES = {"seg-L%d-%s" % (L, k): functools.partial(_case, 20, [20, 13, 0], L, kind=k, route=1)
         for L in (7, 8, 15, 16, 31, 32, 63) for k in ("gaussian", "sticky")}
CASES.update({"pack-N%d" % N: functools.partial(_case, 20, [20, 13, 0], 7, N=N, route=1) for N in (1, 31, 32, 33)})
CASES.update({"time-%s" % k: functools.partial(_case, T, [T, RENORM + 1, T - 3], 15, route=1)
              for k, T in (("F-1", F - 1), ("F", F), ("F+1", F + 1), ("2F+1", 2 * F + 1))})
CASES.update({
    "time-2F+1-x20": functools.partial(_case, 2 * F + 1, [2 * F + 1, RENORM + 1, 2 * F - 2], 15, scale=20.0, route=1),
    "gathered": functools.partial(_case, 33, [33, 17, 0], 15, route=2, env="gathered"),
    "rows": functools.partial(_case, 33, [33, 17, 0], 15, route=0, env="rows"),
    "C1100": functools.partial(_case, 8, [8, 5], 7, C=1100, route=2),
    "L64": functools.partial(_case, 70, [70, 66, 3], 64, route=0),
    "L140-T300": _long,
    "float64": functools.partial(_case, 2 * _tile(6, 1) + 1, [2 * _tile(6, 1) + 1, 17, 0], 15, dtype=np.float64, route=1),
    "bf16-slice": functools.partial(_case, 24, [24, 21, 12], 15, kind="sticky", half="bfloat16", route=1),
})


def expected(x, sl, y, n, ftype=np.longdouble, blank=0):
    out = np.full(n.shape, np.nan, ftype)
    for b in range(x.shape[1]):
        xb = np.ascontiguousarray(x[:max(int(sl[b]), 0), b])
        norm = oracle.row_norm(xb) if len(xb) else np.zeros((0,), x.dtype)
        for i in range(n.shape[1]):
            if 0 <= n[b, i] <= y.shape[2]:
                out[b, i] = psu.path_score(xb, norm, list(y[b, i, :n[b, i]]), len(xb), blank, ftype)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    if c.get("half"):   # values the two-byte format holds exactly
        c["x"] = torch.as_tensor(c["x"]).to(getattr(torch, c["half"])).float().numpy()
    c["want"] = expected(c["x"], c["sl"], c["y"], c["n"])
    w = c["want"]
    assert np.isfinite(w).any(), name
    if c["n"].shape[1] >= 7:   # the lists' bad label and bad length; an item without frames
        assert np.isnan(w).any() and (min(c["sl"]) > 0 or np.isneginf(w).any()), name
    return c


def _check(got, want, what="", E=E_T):
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    for mask in (np.isnan, np.isneginf, np.isposinf):
        np.testing.assert_array_equal(mask(got), mask(want), err_msg="%s: %s cells" % (what, mask.__name__))
    fin = np.isfinite(want)
    err = np.abs(got[fin].astype(np.longdouble) - want[fin])
    tol = 4 * E[got.dtype.type]
    print(what, "largest error %.3g of %.3g" % (err.max() if err.size else 0, tol))
    assert (err <= tol).all(), (what, err.max())
    return got


# The inputs of tie_inputs and a blank_index other than 0.  E_NEW is E_T's measurement over the finite expected cells of
# NEW_CASES alone, so that no case above gets a wider bound (float32 1.9647e-5 and float64 3.1787e-14, both on the
# blank5-sticky inputs); test_cpu_alignment_inputs holds each constant to its measured figure from both sides.
E_NEW = {np.float32: 1.965e-5, np.float64: 3.18e-14}
ROUTES = {"staged": dict(route=1), "gathered": dict(route=2, env="gathered"), "rows": dict(route=0, env="rows")}


def _planted(name, kind, dtype, edges=False):
    import tie_inputs
    return tie_inputs.planted_case("target scores " + name, kind, 15, 12, dtype=dtype, edges=edges)


def _blank_case(blank, kind, dtype):
    c = _case(22, [22, 17, 0], 15, kind="sticky", dtype=dtype, blank=blank)
    if kind == "flat":
        c["x"] = np.zeros_like(c["x"])
    return c


NEW_CASES = {}
for _dt in (np.float32, np.float64):
    for _r, _kw in ROUTES.items():
        _tag = "%s-%s" % (_r, _dt.__name__)
        NEW_CASES["masked-" + _tag] = (functools.partial(_planted, "masked-" + _dt.__name__, "masked", _dt), _kw)
        NEW_CASES["nonfinite-" + _tag] = (functools.partial(_planted, "nonfinite-" + _dt.__name__, "nonfinite", _dt), _kw)
        NEW_CASES["nonfinite-edges-" + _tag] = (
            functools.partial(_planted, "nonfinite-edges-" + _dt.__name__, "nonfinite", _dt, edges=True), _kw)
        for _b in (5, 2):
            for _k in ("sticky", "flat"):
                NEW_CASES["blank%d-%s-%s" % (_b, _k, _tag)] = (functools.partial(_blank_case, _b, _k, _dt), _kw)


@functools.lru_cache(maxsize=None)
def new_case(name):
    build, kw = NEW_CASES[name]
    c = dict(build(), **kw)
    c["want"] = expected(c["x"], c["sl"], c["y"], c["n"], blank=c["blank"])
    assert np.isfinite(c["want"]).any() and np.isnan(c["want"]).any(), name
    return c


def _route():
    d, r = ctcext_amd.get_decoder(0), ctypes.c_int32(-1)
    assert d.lib.ctcext_dense_target_scores_route(d.handle, ctypes.byref(r)) == _lib.CTCEXT_OK
    return r.value


def _score(x, sl, y, n, **kw):
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), device=DEV)
    kw.setdefault("batch_first", False)
    return ctcext_amd.score_targets(x, torch.as_tensor(np.asarray(sl, np.int32), device=DEV),
                                    torch.as_tensor(y, device=DEV), torch.as_tensor(n, device=DEV), **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_matches_definition(name, monkeypatch):
    c = case(name)
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    if "env" in c:
        monkeypatch.setenv("CTCEXT_TARGETS", c["env"])
    x, kw = np.array(c["x"]), {}
    T, B, C = x.shape
    if c.get("half"):   # a batch-major two-byte view with gaps in both dimensions, read in place
        full = torch.zeros((B, T, 40), dtype=getattr(torch, c["half"]), device=DEV)
        full[:, :, 5:5 + C] = torch.as_tensor(x.transpose(1, 0, 2).copy(), device=DEV)
        x, kw = full[:, :, 5:5 + C], dict(batch_first=True)
    got = _score(x, c["sl"], c["y"], c["n"], **kw)
    assert got.is_cuda and tuple(got.shape) == c["n"].shape and got.dtype == getattr(torch, c["x"].dtype.name)
    _check(got, c["want"], name)
    assert _route() == c["route"]


@pytest.mark.parametrize("name", list(NEW_CASES))
def test_matches_definition_on_masked_nonfinite_and_other_blanks(name, monkeypatch):
    """-inf logits under a feasible target (and rows whose every alignment passes one: -inf, never NaN), an item
    with a NaN, a +inf or a frame of -inf (NaN, as the normaliser is), and blank_index 5 and 2 of 6 classes."""
    c = new_case(name)
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    if "env" in c:
        monkeypatch.setenv("CTCEXT_TARGETS", c["env"])
    got = _score(np.array(c["x"]), c["sl"], c["y"], c["n"], blank_index=c["blank"])
    assert tuple(got.shape) == c["n"].shape and got.dtype == getattr(torch, c["x"].dtype.name)
    _check(got, c["want"], name, E_NEW)
    assert _route() == c["route"]


@pytest.mark.parametrize("N", [1, 31, 32, 33])
def test_shared_lists_and_int32_labels_give_the_same_bits(N, monkeypatch):
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    c = case("pack-N%d" % N)
    B = len(c["sl"])
    y, n = np.repeat(c["y"][:1], B, 0), np.repeat(c["n"][:1], B, 0)
    per_item = _check(_score(c["x"], c["sl"], y, n), expected(c["x"], c["sl"], y, n), "broadcast").view(np.uint32)
    for what, got in (("shared", _score(c["x"], c["sl"], y[0], n[0])), ("int32", _score(c["x"], c["sl"], y.astype(np.int32), n))):
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), per_item, err_msg=what)
        assert _route() == 1


@pytest.mark.parametrize("skip", [False, True], ids=["dense", "skip"])
def test_returned_rows_fed_back_reproduce_the_path_scores(skip, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    c = psu.case("skip" if skip else "sticky-40x4x29x16x3-merge")
    W, P = (c["W"], c["P"]) if skip else (8, 2)
    kw = dict(skip_blank=c["skip"]) if skip else {}
    out = ctcext_amd.decode_dense(torch.as_tensor(np.array(c["x"]), device=DEV), torch.as_tensor(c["sl"], device=DEV), W, P,
                                  batch_first=False, merge_repeated=True, token_scores=True, blank_index=0, blank_label=-1, **kw)
    ps = ctcext_amd.dense_path_scores()
    ts = ctcext_amd.dense_target_scores(out.decoded, out.decoded_lengths)
    torch.cuda.synchronize()
    assert torch.isfinite(ps).any()
    _check(ts, ps.cpu().numpy().astype(np.longdouble), "fed back")
    if skip:   # ... and both cover the dropped frames: the definition over the caller's rows
        _check(ts, c["want"], "skip")
    ctcext_amd.dense_check()


def test_item_with_a_status_bit_is_nan_and_alone(monkeypatch):
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    c = case("seg-L15-gaussian")
    bad = np.array(c["sl"])
    bad[1] = c["x"].shape[0] + 1
    want = c["want"].copy()
    want[1] = np.nan
    _check(_score(c["x"], bad, c["y"], c["n"]), want, "status")


def test_graph_capture_and_replay(monkeypatch):
    """decode_greedy and dense_target_scores captured together, replayed on new logits, lengths and targets."""
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    T, B, C, N, L = 40, 3, 6, 20, 15
    side = torch.cuda.Stream(device=DEV)
    xs = torch.zeros((T, B, C), device=DEV)
    sls = torch.zeros((B,), dtype=torch.int32, device=DEV)
    ys = torch.zeros((B, N, L), dtype=torch.int64, device=DEV)
    ns = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    with torch.cuda.stream(side):
        ctcext_amd.score_targets(xs, sls, ys, ns, batch_first=False)   # one call of the shape
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        got = ctcext_amd.score_targets(xs, sls, ys, ns, batch_first=False)
    for sl in ([T, T - 7, 3], [5, T, T - 1], [T, 9, 0]):
        rng = np.random.default_rng(sl[1])
        x = family(rng, "sticky", T, B, C)
        y, n = _lists(rng, B, N, L, C, L)
        for dst, src in ((xs, x), (sls, np.asarray(sl, np.int32)), (ys, y), (ns, n)):
            dst.copy_(torch.as_tensor(src))
        torch.cuda.synchronize()
        g.replay()
        want = expected(x, sl, y, n)
        assert np.isfinite(want).any()
        _check(got, want, "replay %s" % (sl,))


def test_preconditions(monkeypatch):
    T, B, C = 6, 2, 4
    xd = torch.as_tensor(family(np.random.default_rng(7), "gaussian", T, B, C), device=DEV)
    y = torch.ones((B, 3, 2), dtype=torch.int64, device=DEV)
    n = torch.ones((B, 3), dtype=torch.int32, device=DEV)
    ctcext_amd.decode_dense(xd, [T, T], 8, 1, batch_first=False)   # no opt-in
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.dense_target_scores(y, n)
    assert e.value.message == "target scores need a decode with token_scores=True"
    ctcext_amd.decode_logits(xd, [T, T], 8, 1, batch_first=False, token_scores=True)   # ends any dense call
    d, ms, r = ctcext_amd.get_decoder(0), ctypes.c_double(), ctypes.c_int32()
    t = _lib.Targets(y.data_ptr(), n.data_ptr(), 3, 2, 0, 1)
    assert d.lib.ctcext_dense_target_scores(d.handle, ctypes.byref(t), xd.data_ptr()) == _lib.CTCEXT_FAILED_PRECONDITION
    assert d.lib.ctcext_last_error().decode() == "ctcext_dense_target_scores without a ctcext_decode_dense"
    ctcext_amd.decode_greedy(xd, [T, T], batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True)
    none = ctcext_amd.dense_target_scores(y[:, :0], n[:, :0])   # n_targets == 0: nothing launched
    assert tuple(none.shape) == (B, 0)
    assert d.lib.ctcext_dense_target_scores_route(d.handle, ctypes.byref(r)) == _lib.CTCEXT_FAILED_PRECONDITION
    got = ctcext_amd.dense_target_scores(y, n)
    assert d.lib.ctcext_dense_target_scores_ms(d.handle, ctypes.byref(ms)) == _lib.CTCEXT_OK and ms.value > 0
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and _route() == 1
    with pytest.raises(ctcext_amd.InvalidArgumentError):
        ctcext_amd.dense_target_scores(y[:1], n[:1])   # not the decode's batch
