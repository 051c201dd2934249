"""Target alignments on the GPU (dense_target_alignments, forced_align): logp,
the token times, the token scores and the alignment row of every supplied
target equal the numpy restatements of the definitions (path_alignments_util,
token_times_util, token_scores_util) bit for bit; NaN cells match as NaN."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
import oracle
import path_alignments_util as pau
import path_scores_util as psu
from ctcext_amd import _lib
from test_gpu_target_scores import _case, _lists, _tile
from token_scores_util import token_scores
from token_times_util import family, token_times

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = _tile(6)
W10 = _lib.load().ctcext_target_alignments_word_frames()


def _ragged(T):
    return [T, (T + 1) // 2, max(T - 3, 0)]


CASES = {"seg-L%d" % L: functools.partial(_case, 20, [20, 13, 0], L, kind="sticky", route=1)
         for L in (7, 8, 15, 16, 31, 32, 63)}
CASES.update({"pack-N%d" % N: functools.partial(_case, 20, [20, 13, 0], 7, N=N, route=1) for N in (1, 31, 32, 33)})
CASES.update({"time-%d" % T: functools.partial(_case, T, _ragged(T), 15, kind="sticky", route=1)
              for T in (1, W10 - 1, W10, W10 + 1, 2 * W10 + 1, F - 1, F, F + 1, 2 * F + 1)})
CASES.update({
    "gathered": functools.partial(_case, 33, [33, 17, 0], 15, route=2, env="gathered"),
    "C1100": functools.partial(_case, 8, [8, 5], 7, C=1100, route=2),
    "float64": functools.partial(_case, 2 * _tile(6, 1) + 1, [2 * _tile(6, 1) + 1, 17, 0], 15, dtype=np.float64, route=1),
    "bf16-slice": functools.partial(_case, 24, [24, 21, 12], 15, kind="sticky", half="bfloat16", route=1),
})


def expected(x, sl, y, n, status=(), blank=0):
    """The TargetAlignments of y [B, N, L], n [B, N] over x [T, B, C] as numpy arrays."""
    T, B, _ = x.shape
    N, L, ft = y.shape[1], y.shape[2], x.dtype.type
    w = dict(logp=np.full((B, N), np.nan, ft), start=np.full((B, N, L), -1, np.int32), end=np.full((B, N, L), -1, np.int32),
             trailing_blank=np.zeros((B, N), np.int32), logp_sum=np.full((B, N, L), np.nan, ft),
             logp_min=np.full((B, N, L), np.nan, ft), alignment=np.full((B, N, T), -1, np.int32))
    for b in range(B):
        if b in status:
            continue
        fr = min(max(int(sl[b]), 0), T)
        xb = np.ascontiguousarray(x[:fr, b])
        norm = oracle.row_norm(xb) if fr else np.zeros((0,), ft)
        for i in range(N):
            m = int(n[b, i])
            if not 0 <= m <= L:
                continue
            row = [int(c) for c in y[b, i, :m]]
            a, w["logp"][b, i] = pau.align(xb, norm, row, fr, blank, -1)
            if not w["logp"][b, i] > -np.inf:
                continue
            w["alignment"][b, i, :fr] = [blank if c < 0 else c for c in a]
            s, e, w["trailing_blank"][b, i] = token_times(row, a, fr, -1, False)
            w["start"][b, i, :m], w["end"][b, i, :m] = s, e
            if m:
                w["logp_sum"][b, i, :m], w["logp_min"][b, i, :m] = token_scores(xb, norm, a, fr, s, e, blank, -1, ft)
    return w


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    if c.get("half"):   # values the two-byte format holds exactly
        c["x"] = torch.as_tensor(c["x"]).to(getattr(torch, c["half"])).float().numpy()
    for b, fr in enumerate(c["sl"]):   # a target longer than the frames, where the list has room for one
        m = min(int(fr) + 1, c["y"].shape[2])
        if c["n"].shape[1] > 7 and m > fr:
            c["n"][b, 7], c["y"][b, 7, :m] = m, np.arange(m) % (c["x"].shape[2] - 1) + 1
    if c["n"].shape[1] < 7:   # (no room for the lists' bad rows: the last item's last row gets the bad length)
        c["n"][-1, -1] = c["y"].shape[2] + 1
    c["want"] = expected(c["x"], c["sl"], c["y"], c["n"])
    logp = c["want"]["logp"]
    assert (logp > -np.inf).any() and not (logp > -np.inf).all(), name   # an aligned row and an unaligned one
    return c


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _check(got, want, what=""):
    torch.cuda.synchronize()
    have = dict(logp=got.logp, alignment=got.alignment, **got.times._asdict())
    if got.scores is not None:
        have.update(got.scores._asdict())
    for k, g in have.items():
        if g is None:
            continue
        g, w = g.cpu().numpy(), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        if g.dtype.kind == "f":
            np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg="%s: %s NaN cells" % (what, k))
            g, w = np.where(np.isnan(g), 0, g), np.where(np.isnan(w), 0, w)
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg="%s: %s" % (what, k))


def _route():
    d, r = ctcext_amd.get_decoder(0), ctypes.c_int32(-1)
    assert d.lib.ctcext_dense_target_alignments_route(d.handle, ctypes.byref(r)) == _lib.CTCEXT_OK
    return r.value


def _align(x, sl, y, n, **kw):
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), device=DEV)
    kw.setdefault("batch_first", False)
    kw.setdefault("scores", True)
    kw.setdefault("alignment", True)
    return ctcext_amd.forced_align(x, torch.as_tensor(np.asarray(sl, np.int32), device=DEV),
                                   torch.as_tensor(y, device=DEV), torch.as_tensor(n, device=DEV), **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_definition(name, monkeypatch):
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
    _check(_align(x, c["sl"], c["y"], c["n"], **kw), c["want"], name)
    assert _route() == c["route"]


def test_shared_lists_int32_labels_and_optional_outputs(monkeypatch):
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    c = case("pack-N33")
    B = len(c["sl"])
    y, n = np.repeat(c["y"][:1], B, 0), np.repeat(c["n"][:1], B, 0)
    want = expected(c["x"], c["sl"], y, n)
    _check(_align(c["x"], c["sl"], y, n), want, "broadcast")
    _check(_align(c["x"], c["sl"], y[0], n[0]), want, "shared")
    _check(_align(c["x"], c["sl"], y.astype(np.int32), n), want, "int32")
    got = _align(c["x"], c["sl"], y, n, scores=False, alignment=False)
    assert got.scores is None and got.alignment is None
    _check(got, want, "times alone")


@pytest.mark.parametrize("skip", [False, True], ids=["dense", "skip"])
def test_returned_rows_fed_back_reproduce_the_path_alignments(skip, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    c = psu.case("skip" if skip else "sticky-40x4x29x16x3-merge")
    W, P = (c["W"], c["P"]) if skip else (8, 2)
    kw = dict(skip_blank=c["skip"]) if skip else {}
    out = ctcext_amd.decode_dense(torch.as_tensor(np.array(c["x"]), device=DEV), torch.as_tensor(c["sl"], device=DEV), W, P,
                                  batch_first=False, merge_repeated=True, token_scores=True, blank_index=0, blank_label=-1, **kw)
    pa = ctcext_amd.dense_path_alignments(times=True, scores=True)
    ta = ctcext_amd.dense_target_alignments(out.decoded, out.decoded_lengths, scores=True)
    torch.cuda.synchronize()
    assert torch.isfinite(pa.logp).any()
    L = out.decoded.shape[-1]
    want = dict(logp=pa.logp, start=pa.times.start[..., :L], end=pa.times.end[..., :L],
                trailing_blank=pa.times.trailing_blank, logp_sum=pa.scores.logp_sum[..., :L],
                logp_min=pa.scores.logp_min[..., :L])
    _check(ta, {k: v.cpu().numpy() for k, v in want.items()}, "fed back")
    ctcext_amd.dense_check()


def test_item_with_a_status_bit_is_unaligned_and_alone(monkeypatch):
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    c = case("seg-L15")
    bad = np.array(c["sl"])
    bad[1] = c["x"].shape[0] + 1
    want = expected(c["x"], c["sl"], c["y"], c["n"], status=(1,))
    assert np.isnan(want["logp"][1]).all() and (want["logp"][0] > -np.inf).any()
    _check(_align(c["x"], bad, c["y"], c["n"]), want, "status")


def test_graph_capture_and_replay(monkeypatch):
    """On a handle of its own: a first call of a shape inside a capture is refused; after a warm-up, decode_greedy and
    dense_target_alignments are captured together and replayed on new logits, lengths and targets."""
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    ctcext_amd.get_decoder(0)
    monkeypatch.setitem(ctcext_amd.ops._tls.decoders, 0, ctcext_amd.Decoder(0))   # (no decision words yet)
    T, B, C, N, L = 40, 3, 6, 20, 15
    side = torch.cuda.Stream(device=DEV)
    xs = torch.zeros((T, B, C), device=DEV)
    sls = torch.zeros((B,), dtype=torch.int32, device=DEV)
    ys = torch.zeros((B, N, L), dtype=torch.int64, device=DEV)
    ns = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    kw = dict(batch_first=False, scores=True, alignment=True)
    with torch.cuda.stream(side):   # sizes the decode's workspace alone
        ctcext_amd.decode_greedy(xs, sls, batch_first=False, token_scores=True)
    side.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=side):
        with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
            ctcext_amd.forced_align(xs, sls, ys, ns, **kw)
    assert "the stream is capturing" in e.value.message
    with torch.cuda.stream(side):   # the warm-up: loads the kernel, sizes the decision words
        ctcext_amd.forced_align(xs, sls, ys, ns, **kw)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        got = ctcext_amd.forced_align(xs, sls, ys, ns, **kw)
    for sl in ([T, T - 7, 3], [5, T, T - 1], [T, 9, 0]):
        rng = np.random.default_rng(sl[1])
        x = family(rng, "sticky", T, B, C)
        y, n = _lists(rng, B, N, L, C, L)
        for dst, src in ((xs, x), (sls, np.asarray(sl, np.int32)), (ys, y), (ns, n)):
            dst.copy_(torch.as_tensor(src))
        torch.cuda.synchronize()
        g.replay()
        want = expected(x, sl, y, n)
        assert (want["logp"] > -np.inf).any()
        _check(got, want, "replay %s" % (sl,))


def test_preconditions(monkeypatch):
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    T, B, C = 6, 2, 4
    xd = torch.as_tensor(family(np.random.default_rng(7), "gaussian", T, B, C), device=DEV)
    y = torch.ones((B, 3, 2), dtype=torch.int64, device=DEV)
    n = torch.ones((B, 3), dtype=torch.int32, device=DEV)
    ctcext_amd.decode_dense(xd, [T, T], 8, 1, batch_first=False)   # no opt-in
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.dense_target_alignments(y, n)
    assert e.value.message == "target alignments need a decode with token_scores=True"
    ctcext_amd.decode_logits(xd, [T, T], 8, 1, batch_first=False, token_scores=True)   # ends any dense call
    d, ms, r = ctcext_amd.get_decoder(0), ctypes.c_double(), ctypes.c_int32()
    t = _lib.Targets(y.data_ptr(), n.data_ptr(), 3, 2, 0, 1)
    o = _lib.TargetAlignmentsOut(*[xd.data_ptr()] * 4)
    call = d.lib.ctcext_dense_target_alignments
    assert call(d.handle, ctypes.byref(t), ctypes.byref(o)) == _lib.CTCEXT_FAILED_PRECONDITION
    assert d.lib.ctcext_last_error().decode() == "ctcext_dense_target_alignments without a ctcext_decode_dense"
    ctcext_amd.decode_greedy(xd, [T, T], batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True)
    none = ctcext_amd.dense_target_alignments(y[:, :0], n[:, :0])   # n_targets == 0: nothing launched
    assert tuple(none.logp.shape) == (B, 0)
    assert d.lib.ctcext_dense_target_alignments_route(d.handle, ctypes.byref(r)) == _lib.CTCEXT_FAILED_PRECONDITION
    assert call(d.handle, ctypes.byref(t), ctypes.byref(_lib.TargetAlignmentsOut())) == _lib.CTCEXT_INVALID_ARGUMENT
    assert d.lib.ctcext_last_error().decode() == "target alignments need logp, start, end and trailing_blank"
    got = ctcext_amd.dense_target_alignments(y, n)
    assert d.lib.ctcext_dense_target_alignments_ms(d.handle, ctypes.byref(ms)) == _lib.CTCEXT_OK and ms.value > 0
    torch.cuda.synchronize()
    assert torch.isfinite(got.logp).all() and (got.times.start[..., 0] >= 0).all() and _route() == 1
    with pytest.raises(ctcext_amd.InvalidArgumentError):
        ctcext_amd.dense_target_alignments(y[:1], n[:1])   # not the decode's batch
    with pytest.raises(ctcext_amd.UnimplementedError):   # max_target >= 64 has no route yet
        ctcext_amd.dense_target_alignments(torch.ones((B, 1, 64), dtype=torch.int64, device=DEV), n[:, :1])
