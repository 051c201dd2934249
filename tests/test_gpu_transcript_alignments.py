"""Transcript alignments on the GPU (dense_transcript_alignments,
align_transcripts): logp, the token times, the token scores and the alignment
row of every supplied target equal the numpy restatements of the definitions
(test_gpu_target_alignments.expected) bit for bit, at every wave edge, every K
and its edges, and on both sides of a forward block and of a decision word."""
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
from ctcext_amd import _lib
from test_gpu_target_alignments import _check, expected
from test_gpu_target_scores import _case, _lists
from token_times_util import family

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = _lib.load().ctcext_transcript_alignments_block_frames()
FPW3 = _lib.load().ctcext_transcript_alignments_word_frames(3)


def _tcase(L, T, edit=None, **kw):
    """B = 3 with frames [T, T - 5, 0], N = 3 sticky rows of 0, 1 and min(L, T) labels (the last without a repeat)."""
    opts = {k: kw.pop(k) for k in ("half", "labels32", "shared", "plain", "status") if k in kw}
    c = _case(T, [T, max(T - 5, 0), 0], L, N=3, kind="sticky", **kw)
    if edit:
        edit(c)
    return dict(c, **opts)


def _equal_at(pos):
    def edit(c):   # the full-length row's labels pos - 1 and pos are equal: one more frame, and no s - 2 across them
        c["y"][:, 2, pos] = c["y"][:, 2, pos - 1]
    return edit


def _set(key, index, value):
    return lambda c: c[key].__setitem__(index, value)


CASES = {"wave-L%d" % L: functools.partial(_tcase, L, L + 6) for L in (63, 64, 65, 127, 128, 255)}
CASES.update({"K-L%d" % L: functools.partial(_tcase, L, L + 8) for L in (256, 511, 512, 1023, 1024, 2047)})
CASES.update({"time4-%d" % T: functools.partial(_tcase, 70, T) for T in (4 * F - 1, 4 * F, 4 * F + 1, 4 * F + 2, 5 * F + 1)})
CASES.update({"time1-%d" % T: functools.partial(_tcase, 3, T)
              for T in (1, 2, FPW3, FPW3 + 1, F, F + 1, F + 2, 2 * F + 1)})
CASES.update({
    "equal-63-64": functools.partial(_tcase, 127, 135, _equal_at(64)),
    "equal-127-128": functools.partial(_tcase, 300, 308, _equal_at(128)),
    "float64": functools.partial(_tcase, 70, 76, dtype=np.float64),
    "bf16-slice": functools.partial(_tcase, 70, 76, half="bfloat16"),
    "int32": functools.partial(_tcase, 70, 76, labels32=True),
    "shared": functools.partial(_tcase, 70, 76, shared=True),
    "times-alone": functools.partial(_tcase, 70, 76, plain=True),
    "status": functools.partial(_tcase, 70, 76, status=1),
    "bad-label": functools.partial(_tcase, 70, 76, _set("y", (0, 2, 65), 6)),
    "bad-length": functools.partial(_tcase, 70, 76, _set("n", (1, 1), 71)),
    "m-above-frames": functools.partial(_tcase, 70, 60, _set("n", (0, 1), 70)),
})


def _align(fn, x, sl, y, n, **kw):
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), device=DEV)
    kw.setdefault("batch_first", False)
    kw.setdefault("scores", True)
    kw.setdefault("alignment", True)
    return fn(x, torch.as_tensor(np.asarray(sl, np.int32), device=DEV), torch.as_tensor(y, device=DEV),
              torch.as_tensor(n, device=DEV), **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_definition(name):
    c = CASES[name]()
    x, sl, y, n, kw = c["x"], np.array(c["sl"]), c["y"], c["n"], {}
    T, B, C = x.shape
    status = ()
    if "status" in c:   # an item longer than max_time gets a status bit: its rows are NaN, the others untouched
        status, sl = (c["status"],), sl.copy()
        sl[c["status"]] = T + 1
    if c.get("shared"):
        y, n = np.repeat(y[:1], B, 0), np.repeat(n[:1], B, 0)
    if c.get("half"):   # values the two-byte format holds exactly, in a batch-major view with gaps, read in place
        x = torch.as_tensor(x).to(getattr(torch, c["half"])).float().numpy()
        full = torch.zeros((B, T, 40), dtype=getattr(torch, c["half"]), device=DEV)
        full[:, :, 5:5 + C] = torch.as_tensor(x.transpose(1, 0, 2).copy(), device=DEV)
        xd, kw = full[:, :, 5:5 + C], dict(batch_first=True)
    else:
        xd = x
    want = expected(x, c["sl"], y, n, status=status)
    assert (want["logp"] > -np.inf).any() and not (want["logp"] > -np.inf).all(), name   # an aligned and an unaligned row
    if c.get("plain"):
        kw.update(scores=False, alignment=False)
    yd, nd = (y[0], n[0]) if c.get("shared") else (y.astype(np.int32) if c.get("labels32") else y, n)
    got = _align(ctcext_amd.align_transcripts, xd, sl, yd, nd, **kw)
    assert not c.get("plain") or (got.scores is None and got.alignment is None)
    _check(got, want, name)


def test_short_lists_equal_the_target_alignments():
    c = _case(40, [40, 33, 0], 63, N=12, kind="sticky")   # the lists' bad label and bad length included
    want = _align(ctcext_amd.forced_align, c["x"], c["sl"], c["y"], c["n"])
    got = _align(ctcext_amd.align_transcripts, c["x"], c["sl"], c["y"], c["n"])
    torch.cuda.synchronize()
    assert torch.isfinite(want.logp).any()
    _check(got, {k: v.cpu().numpy() for k, v in dict(logp=want.logp, alignment=want.alignment, **want.times._asdict(),
                                                      **want.scores._asdict()).items()}, "L63")


def test_greedy_rows_fed_back_reproduce_the_path_alignments():
    x = torch.as_tensor(family(np.random.default_rng(3), "gaussian", 150, 3, 29), device=DEV)
    out = ctcext_amd.decode_greedy(x, [150, 147, 90], batch_first=False, token_scores=True)
    pa = ctcext_amd.dense_path_alignments(times=True, scores=True)
    ta = ctcext_amd.dense_transcript_alignments(out.decoded, out.decoded_lengths, scores=True)
    torch.cuda.synchronize()
    assert int(out.decoded_lengths.max()) > 64 and torch.isfinite(pa.logp).all()
    L = out.decoded.shape[-1]
    want = dict(logp=pa.logp, start=pa.times.start[..., :L], end=pa.times.end[..., :L],
                trailing_blank=pa.times.trailing_blank, logp_sum=pa.scores.logp_sum[..., :L],
                logp_min=pa.scores.logp_min[..., :L])
    _check(ta, {k: v.cpu().numpy() for k, v in want.items()}, "fed back")
    ctcext_amd.dense_check()


def test_graph_capture_and_replay(monkeypatch):
    """On a handle of its own: a first call of a shape inside a capture is refused; after a warm-up, decode_greedy and
    dense_transcript_alignments are captured together and replayed on new logits, lengths and targets."""
    ctcext_amd.get_decoder(0)
    monkeypatch.setitem(ctcext_amd.ops._tls.decoders, 0, ctcext_amd.Decoder(0))   # (no decision words yet)
    T, B, C, N, L = 90, 3, 6, 3, 70
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
            ctcext_amd.align_transcripts(xs, sls, ys, ns, **kw)
    assert "the stream is capturing" in e.value.message
    with torch.cuda.stream(side):   # the warm-up: loads the kernel, sizes the decision words
        ctcext_amd.align_transcripts(xs, sls, ys, ns, **kw)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        got = ctcext_amd.align_transcripts(xs, sls, ys, ns, **kw)
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


def test_refusals():
    x = torch.as_tensor(family(np.random.default_rng(7), "gaussian", 6, 2, 4), device=DEV)
    n = torch.ones((2, 1), dtype=torch.int32, device=DEV)
    ctcext_amd.decode_greedy(x, [6, 6], batch_first=False)   # no opt-in
    with pytest.raises(ctcext_amd.FailedPreconditionError):
        ctcext_amd.dense_transcript_alignments(torch.ones((2, 1, 2), dtype=torch.int64, device=DEV), n)
    with pytest.raises(ctcext_amd.UnimplementedError):
        ctcext_amd.align_transcripts(x, [6, 6], torch.ones((2, 1, 2048), dtype=torch.int64, device=DEV), n, batch_first=False)
    got = ctcext_amd.align_transcripts(x, [6, 6], torch.ones((2, 1, 2047), dtype=torch.int64, device=DEV), n, batch_first=False)
    torch.cuda.synchronize()
    assert torch.isfinite(got.logp).all()
