"""Path alignments on the GPU (dense_path_alignments, path_alignments): the
alignment, its length, logp, the token times and the token scores equal the
numpy restatement of the definition exactly (path_alignments_util)."""
import ctypes

import numpy as np
import pytest
import torch

import ctcext_amd
import path_alignments_util as u
from ctcext_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KW = dict(blank_index=0, blank_label=-1)


def _np(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _whole(t, frames, rows, what):
    """Every aligned row is whole and timed: its length is the item's frames, every token has a start, and the
    starts increase strictly."""
    alen, logp, start = _np(t["alignment_lengths"]), _np(t["logp"]), t.get("start")
    aligned = logp > -np.inf
    np.testing.assert_array_equal(alen, np.where(aligned, np.maximum(np.asarray(frames), 0)[:, None], 0), err_msg=what)
    for b, p in zip(*np.nonzero(aligned)):
        if start is not None:
            s = _np(start)[b, p, :len(rows[b][p])]
            assert (s >= 0).all() and (np.diff(s) > 0).all(), (what, b, p)


def _check(got, want, frames, rows, what):
    """Exact equality (NaN equals NaN, the bits of every other float); the outputs and the expected values alike
    have every aligned row whole and timed."""
    torch.cuda.synchronize()
    have = dict(alignment=got.alignment, alignment_lengths=got.alignment_lengths, logp=got.logp)
    if got.times is not None:
        have.update(got.times._asdict())
    if got.scores is not None:
        have.update(got.scores._asdict())
    for k, g in have.items():
        g, w = _np(g), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        np.testing.assert_array_equal(g, w, err_msg="%s: %s" % (what, k))
        if g.dtype.kind == "f":
            np.testing.assert_array_equal(np.signbit(g), np.signbit(w), err_msg="%s: %s signs" % (what, k))
    _whole(want, frames, rows, what + ", expected")
    _whole(have, frames, rows, what)


def _dense(x, sl, W, P, merge, times=True, scores=True, **kw):
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), device=DEV)
    kw.setdefault("batch_first", False)
    out = ctcext_amd.decode_dense(x, torch.as_tensor(np.asarray(sl, np.int32), device=DEV), W, P, merge_repeated=merge,
                                  token_scores=True, **KW, **kw)
    return out, ctcext_amd.dense_path_alignments(times=times, scores=scores)


@pytest.mark.parametrize("name", u.CASES)
def test_dense_equals_the_definition(name, monkeypatch):
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
    out, pa = _dense(xd, sl, W, P, c["merge"], **kw)
    _check(pa, c["want"], sl, c["rows"], name)
    assert out.status.cpu().tolist() == [0] * B
    if "skip" in c:   # the synchronous form after a skipping call: the staged rows, the plan's normaliser
        ctcext_amd.decode_logits(np.array(x), sl, W, P, batch_first=False, merge_repeated=True, skip_blank=c["skip"],
                                 token_scores=True, **KW)
        _check(ctcext_amd.path_alignments(scores=True), c["want"], sl, c["rows"], name + ", synchronous")


def test_item_with_a_status_bit_is_unaligned_and_alone(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    c = u.case("peaky-12x6x5x8x3-plain")
    bad = np.array(c["sl"])
    bad[1] = c["x"].shape[0] + 1
    out, pa = _dense(np.array(c["x"]), bad, c["W"], c["P"], False)
    want = {k: v.copy() for k, v in c["want"].items()}
    for k, fill in (("alignment", -1), ("alignment_lengths", 0), ("logp", np.nan), ("start", -1), ("end", -1),
                    ("trailing_blank", 0), ("logp_sum", np.nan), ("logp_min", np.nan)):
        want[k][1] = fill
    frames = np.array(c["sl"])
    frames[1] = 0
    _check(pa, want, frames, c["rows"], "status")
    assert out.status.cpu().tolist() == [0, _lib.CTCEXT_ITEM_LENGTH, 0, 0, 0, 0]


def test_preconditions_and_the_blank_label_rule(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C = 6, 2, 4
    xd = torch.as_tensor(u.family(np.random.default_rng(7), "gaussian", T, B, C), device=DEV)
    ctcext_amd.decode_dense(xd, [T, T], 8, 1, batch_first=False)   # no opt-in
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.dense_path_alignments()
    assert e.value.message == "path alignments need a decode with token_scores=True"
    ctcext_amd.decode_logits(xd, [T, T], 8, 1, batch_first=False, token_scores=True)   # ends any dense call
    d, ms, o = ctcext_amd.get_decoder(0), (ctypes.c_double * 5)(), _lib.PathAlignmentsOut()
    o.alignment = o.alignment_length = o.logp = xd.data_ptr()
    assert d.lib.ctcext_dense_path_alignments(d.handle, ctypes.byref(o)) == _lib.CTCEXT_FAILED_PRECONDITION
    assert d.lib.ctcext_last_error().decode() == "ctcext_dense_path_alignments without a ctcext_decode_dense"
    with ctcext_amd.StreamDecoder(B, C, 8, 1, T, device=DEV) as s:
        s.push(xd, batch_first=False)   # a stream's push keeps no logits for the synchronous form
        with pytest.raises(ctcext_amd.FailedPreconditionError):
            ctcext_amd.path_alignments()
        assert d.lib.ctcext_fetch_path_alignments(d.handle, ctypes.byref(o), 1) == _lib.CTCEXT_FAILED_PRECONDITION
        assert d.lib.ctcext_last_error().decode().startswith("ctcext_fetch_path_alignments after a stream's push")
    ctcext_amd.decode_dense(xd, [T, T], 8, 1, batch_first=False, blank_label=3, token_scores=True)
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.dense_path_alignments()
    assert e.value.message == "token times need a blank_label that is no class label"
    ctcext_amd.decode_dense(xd, [T, T], 8, 1, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True)
    ctcext_amd.dense_path_alignments(scores=True)
    assert d.lib.ctcext_dense_path_alignments_ms(d.handle, ms) == _lib.CTCEXT_OK and min(ms) > 0
    ctcext_amd.dense_check()


def test_times_and_scores_are_optional(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    c = u.case("sticky-40x4x29x16x3-merge")
    pa = _dense(np.array(c["x"]), c["sl"], c["W"], c["P"], True, times=True, scores=False)[1]
    assert pa.scores is None and pa.times is not None
    _check(pa, c["want"], c["sl"], c["rows"], "times alone")
    ctcext_amd.decode_dense(torch.as_tensor(np.array(c["x"]), device=DEV), torch.as_tensor(c["sl"], device=DEV), c["W"],
                            c["P"], batch_first=False, merge_repeated=True, token_scores=True,
                            flags=_lib.CTCEXT_FLAG_PROFILE, **KW)
    pa = ctcext_amd.dense_path_alignments(times=False)
    assert pa.times is None and pa.scores is None
    _check(pa, c["want"], c["sl"], c["rows"], "alignment alone")
    d, ms = ctcext_amd.get_decoder(0), (ctypes.c_double * 5)()
    assert d.lib.ctcext_dense_path_alignments_ms(d.handle, ms) == _lib.CTCEXT_OK
    assert ms[0] > 0 and ms[2] > 0 and ms[3] == 0 and ms[4] == 0   # nothing was launched for the times or the scores
    with pytest.raises(ValueError):
        ctcext_amd.dense_path_alignments(times=False, scores=True)


def test_graph_capture_and_replay(monkeypatch):
    """On a handle of its own: a first call of a shape inside a capture is refused; after a warm-up of the shape,
    decode and path alignments are captured together and replayed on new logits and lengths."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    ctcext_amd.get_decoder(0)
    monkeypatch.setitem(ctcext_amd.ops._tls.decoders, 0, ctcext_amd.Decoder(0))   # (no alignment workspace yet)
    T, B, C, W, P = 40, 3, 20, 100, 3
    side = torch.cuda.Stream(device=DEV)
    kw = dict(batch_first=False, merge_repeated=True, token_scores=True)
    xs = torch.zeros((T, B, C), device=DEV)
    sls = torch.full((B,), T, dtype=torch.int32, device=DEV)
    with torch.cuda.stream(side):   # sizes the decode's workspace alone
        ctcext_amd.decode_dense(xs, sls, W, P, **kw)
    side.synchronize()
    torch.cuda.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=side):
        ctcext_amd.decode_dense(xs, sls, W, P, **kw)
        with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
            ctcext_amd.dense_path_alignments()
    assert "the stream is capturing" in e.value.message
    with torch.cuda.stream(side):   # the warm-up: loads the kernels, sizes the alignments' workspace
        ctcext_amd.decode_dense(xs, sls, W, P, **kw)
        ctcext_amd.dense_path_alignments(scores=True)
    side.synchronize()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctcext_amd.decode_dense(xs, sls, W, P, **kw)
        pa = ctcext_amd.dense_path_alignments(scores=True)
    for sl in ([T, T - 7, 3], [5, T, T - 1], [T, 9, T - 2]):
        x = u.family(np.random.default_rng(sl[1]), "sticky", T, B, C)
        xs.copy_(torch.as_tensor(x))
        sls.copy_(torch.as_tensor(np.asarray(sl, np.int32)))
        torch.cuda.synchronize()
        g.replay()
        rows = u.oracle.raw_decode(x, np.asarray(sl, np.int32), W, P, True, 0, -1)[0]
        _check(pa, u.expected(x, sl, rows, P), sl, rows, "replay %s" % (sl,))
    torch.cuda.synchronize()
