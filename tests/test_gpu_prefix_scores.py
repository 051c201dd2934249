"""Prefix scores on the GPU (dense_prefix_scores, score_prefixes): NaN, -inf and
+inf cells exactly, finite ones within 4 E_P of the "Prefix scores" definition
in longdouble (prefix_scores_util.prefix_scores) for every supplied prefix."""
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
import prefix_scores_util as pxu
from ctcext_amd import _lib
from test_gpu_target_scores import _lists
from token_times_util import family

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# E_P: per case and per dtype, the largest |definition in the compute dtype with
# numpy's logaddexp - the same in longdouble| over the finite expected cells,
# measured on the CPU: E_CASE below, each figure the measurement rounded up in
# its fourth digit.  Over all cases that is float32 1.5765e-4 (sticky-x20) and
# float64 4.4818e-14; a case is held to 4 times its OWN figure, so the sharp-
# posterior case widens no other case's bound.
E_CASE = {
    "seg-L7": 5.255e-06,
    "seg-L8": 3.517e-06,
    "seg-L63": 4.828e-06,
    "C1100": 5.985e-06,
    "tile+2": 5.695e-06,
    "tile+2-last": 5.695e-06,
    "narrow-side": 2.553e-05,
    "wide-side": 1.480e-05,
    "float64": 6.544e-15,
    "float64-wide": 4.482e-14,
    "rows-L64": 2.709e-05,
    "rows-forced": 5.255e-06,
    "bf16-slice": 9.453e-06,
    "blank-mid": 1.024e-05,
    "sticky-x20": 1.577e-04,
    "forced-narrow": 1.393e-05,
    "forced-wide": 1.393e-05,
    "three-tiles": 5.028e-05,
    "tile-1-narrow": 3.433e-05,
    "tile-1-wide": 3.433e-05,
    "tile+0-narrow": 2.447e-05,
    "tile+0-wide": 2.447e-05,
    "tile+1-narrow": 5.030e-05,
    "tile+1-wide": 5.030e-05,
    "slices-1": 1.550e-06,
    "slices+0": 1.312e-06,
    "slices+1": 1.555e-06,
}

TILE, SLICES = 64, 8   # CTCEXT_PREFIX_TIME_TILE, CTCEXT_PREFIX_NARROW_SLICES (test_cpu_prefix_scores holds them to the header)
WIDE = next(C for C in range(1, 4096) if _lib.load().ctcext_prefix_scores_layout(C, 0))   # the first wide class count


def _case(T, sl1, L, C=6, N=12, kind="gaussian", scale=1.0, dtype=np.float32, last=None, **extra):
    """B = 3 with frames [T, sl1, 0]; target scores' fixed rows, then a prefix ending in a repeat (its last label
    `last`) and one of min(L, T) equal labels, which item 1 has not the frames for."""
    rng = np.random.default_rng(100 * T + L + C)
    x = (family(rng, kind, T, 3, C) * scale).astype(dtype)
    y, n = _lists(rng, 3, N, L, C, min(L, T))
    k = min(L, 3)
    y[:, 7, :k], n[:, 7] = (C - 1 if last is None else last), k
    y[:, 7, 0] = 1
    y[:, 8, :min(L, T)], n[:, 8] = 2, min(L, T)
    n[:, 9:] = np.minimum(n[:, 9:], 4)   # short enough to leave frames for an extension
    return dict(x=x, sl=np.array([T, sl1, 0], np.int32), y=y, n=n, **extra)


CASES = {"seg-L%d" % L: functools.partial(_case, 20, 12, L) for L in (7, 8, 63)}
CASES.update({
    "C1100": functools.partial(_case, 8, 5, 7, C=1100),   # gathered rows; a part-filled fifth class tile
    "tile+2": functools.partial(_case, 8, 5, 7, C=258),
    "tile+2-last": functools.partial(_case, 8, 5, 7, C=258, last=257),   # the repeated last label in the second tile
    "narrow-side": functools.partial(_case, 20, 12, 7, C=WIDE - 1, layout=0),
    "wide-side": functools.partial(_case, 20, 12, 7, C=WIDE, layout=1),
    "float64": functools.partial(_case, 20, 13, 15, dtype=np.float64),
    "float64-wide": functools.partial(_case, 20, 12, 7, C=WIDE, N=9, dtype=np.float64, layout=1),   # gathered rows too
    "rows-L64": functools.partial(_case, 70, 17, 64),   # one wave per prefix
    "rows-forced": functools.partial(_case, 20, 12, 7, targets="rows"),
    "bf16-slice": functools.partial(_case, 24, 12, 15, kind="sticky", half="bfloat16"),
    "blank-mid": functools.partial(_case, 20, 13, 15, kind="sticky", blank=3),
    "sticky-x20": functools.partial(_case, 20, 13, 15, kind="sticky", scale=20.0),
    "forced-narrow": functools.partial(_case, 20, 12, 7, C=40, env="narrow"),
    "forced-wide": functools.partial(_case, 20, 12, 7, C=40, env="wide"),
    "three-tiles": functools.partial(_case, 2 * TILE + 1, 17, 15, N=9),
})
CASES.update({"tile%+d-%s" % (d, k): functools.partial(_case, TILE + d, 17, 15, C=C, N=9, env=k)
              for d in (-1, 0, 1) for k, C in (("narrow", 6), ("wide", 6))})
CASES.update({"slices%+d" % d: functools.partial(_case, SLICES + d, 5, 7) for d in (-1, 0, 1)})


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    if c.get("half"):   # values the two-byte format holds exactly
        c["x"] = torch.as_tensor(c["x"]).to(getattr(torch, c["half"])).float().numpy()
    w = c["want"] = pxu.expected(c["x"], c["sl"], c["y"], c["n"], blank=c.get("blank", 0))
    assert np.isfinite(w).any() and np.isnan(w).any() and np.isneginf(w).any(), name
    assert np.isfinite(w[0, 7]).sum() > 2 and np.isneginf(w[1, 8]).all(), name   # the repeat row; the infeasible one
    return c


def _check(got, want, what, E):
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    for mask in (np.isnan, np.isneginf, np.isposinf):
        np.testing.assert_array_equal(mask(got), mask(want), err_msg="%s: %s cells" % (what, mask.__name__))
    fin = np.isfinite(want)
    err = np.abs(got[fin].astype(np.longdouble) - want[fin])
    tol = 4 * E
    print(what, "largest error %.3g of %.3g" % (err.max() if err.size else 0, tol))
    assert (err <= tol).all(), (what, err.max())
    return got


def _score(x, sl, y, n, **kw):
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), device=DEV)
    kw.setdefault("batch_first", False)
    return ctcext_amd.score_prefixes(x, torch.as_tensor(np.asarray(sl, np.int32), device=DEV),
                                     torch.as_tensor(y, device=DEV), torch.as_tensor(n, device=DEV), **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_matches_definition(name, monkeypatch):
    c = case(name)
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    monkeypatch.delenv("CTCEXT_PREFIX_GROUP", raising=False)
    monkeypatch.delenv("CTCEXT_PREFIX", raising=False)
    if "env" in c:
        monkeypatch.setenv("CTCEXT_PREFIX", c["env"])
    if "targets" in c:
        monkeypatch.setenv("CTCEXT_TARGETS", c["targets"])
    x, kw = np.array(c["x"]), dict(blank_index=c.get("blank", 0))
    T, B, C = x.shape
    if "layout" in c:
        assert _lib.load().ctcext_prefix_scores_layout(C, int(x.dtype == np.float64)) == c["layout"]
    if c.get("half"):   # a batch-major two-byte view with gaps in both dimensions, read in place
        full = torch.zeros((B, T, 40), dtype=getattr(torch, c["half"]), device=DEV)
        full[:, :, 5:5 + C] = torch.as_tensor(x.transpose(1, 0, 2).copy(), device=DEV)
        x, kw = full[:, :, 5:5 + C], dict(kw, batch_first=True)
    got = _score(x, c["sl"], c["y"], c["n"], **kw)
    assert got.is_cuda and tuple(got.shape) == c["n"].shape + (C,) and got.dtype == getattr(torch, c["x"].dtype.name)
    _check(got, c["want"], name, E_CASE[name])


def test_blank_column_is_the_target_score(monkeypatch):
    import test_gpu_target_scores as tgs
    monkeypatch.delenv("CTCEXT_PREFIX", raising=False)
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    c = case("seg-L8")
    ext = _score(c["x"], c["sl"], c["y"], c["n"])
    ts = ctcext_amd.dense_target_scores(torch.as_tensor(c["y"], device=DEV), torch.as_tensor(c["n"], device=DEV))
    torch.cuda.synchronize()
    ext, ts = ext[:, :, 0].cpu().numpy(), ts.cpu().numpy()
    for mask in (np.isnan, np.isneginf):
        np.testing.assert_array_equal(mask(ext), mask(ts))
    fin = np.isfinite(ts)
    assert fin.any() and (np.abs(ext[fin] - ts[fin]) <= 4 * (E_CASE["seg-L8"] + tgs.E_T[np.float32])).all()


def test_graph_capture_and_replay(monkeypatch):
    """decode_greedy and dense_prefix_scores captured together after one call of the shape, replayed on new
    logits, lengths and prefixes: the eager call's bits."""
    monkeypatch.delenv("CTCEXT_PREFIX", raising=False)
    T, B, C, N, L = 40, 3, 6, 12, 7
    side = torch.cuda.Stream(device=DEV)
    xs = torch.zeros((T, B, C), device=DEV)
    sls = torch.zeros((B,), dtype=torch.int32, device=DEV)
    ys = torch.zeros((B, N, L), dtype=torch.int64, device=DEV)
    ns = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    with torch.cuda.stream(side):
        ctcext_amd.score_prefixes(xs, sls, ys, ns, batch_first=False)   # one call of the shape
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        got = ctcext_amd.score_prefixes(xs, sls, ys, ns, batch_first=False)
    for T1 in (T, 13, 29):
        c = _case(T1, 9, L)
        xs.zero_()
        xs[:T1].copy_(torch.as_tensor(c["x"]))
        for dst, src in ((sls, c["sl"]), (ys, c["y"]), (ns, c["n"])):
            dst.copy_(torch.as_tensor(src))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        replayed = got.cpu().numpy().view(np.uint32)
        eager = _score(xs, sls.cpu().numpy(), c["y"], c["n"])
        torch.cuda.synchronize()
        assert np.isfinite(eager.cpu().numpy()).any()
        np.testing.assert_array_equal(replayed, eager.cpu().numpy().view(np.uint32), err_msg="replay T=%d" % T1)


def test_preconditions():
    T, B, C = 6, 2, 4
    xd = torch.as_tensor(family(np.random.default_rng(7), "gaussian", T, B, C), device=DEV)
    y = torch.ones((B, 3, 2), dtype=torch.int64, device=DEV)
    n = torch.ones((B, 3), dtype=torch.int32, device=DEV)
    ctcext_amd.decode_dense(xd, [T, T], 8, 1, batch_first=False)   # no opt-in
    with pytest.raises(ctcext_amd.FailedPreconditionError):
        ctcext_amd.dense_prefix_scores(y, n)
    ctcext_amd.decode_greedy(xd, [T, T], batch_first=False, token_scores=True)
    none = ctcext_amd.dense_prefix_scores(y[:, :0], n[:, :0])   # n_targets == 0: nothing launched
    assert tuple(none.shape) == (B, 0, C)
    # a shape no call has had yet: the workspace would have to grow inside the capture
    big = torch.ones((B, 4099, 2), dtype=torch.int64, device=DEV)
    nbig = torch.ones((B, 4099), dtype=torch.int32, device=DEV)
    sl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):   # sizes the decode's workspace alone
        ctcext_amd.decode_greedy(xd, sl, batch_first=False, token_scores=True)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctcext_amd.decode_greedy(xd, sl, batch_first=False, token_scores=True)
        with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
            ctcext_amd.dense_prefix_scores(big, nbig)
    assert "the stream is capturing" in e.value.message
