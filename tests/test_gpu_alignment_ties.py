"""The forced-alignment kernels where the definition's comparisons decide
(forced_align, align_transcripts, and dense_path_alignments beside them):
logits on which trellis states tie, -inf logits under a feasible target, a NaN,
a +inf or a frame of -inf in an item, and a blank_index other than 0.  Every
output equals test_gpu_target_alignments.expected bit for bit, NaN cells as
NaN.  "Strictly greater", "a comparison with a NaN is false" and the end state
are what these inputs pin: test_cpu_alignment_inputs shows, on the CPU, that a
kernel with any one comparison turned into >= would fail each tie case."""
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
import path_alignments_util as pau
import tie_inputs
from ctcext_amd import _lib
from test_gpu_path_alignments import _check as _check_paths
from test_gpu_target_alignments import _align as _forced
from test_gpu_target_alignments import _check, _route, expected
from test_gpu_target_scores import _lists, _tile
from test_gpu_transcript_alignments import _align, _equal_at
from token_times_util import family as real_family

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W10 = _lib.load().ctcext_target_alignments_word_frames()
TILE = _tile(6)
F = _lib.load().ctcext_transcript_alignments_block_frames()


def _block(L):
    """The label pairs a thread of the transcript kernel holds at max_target L."""
    return next(k for k in (1, 2, 4, 8) if 256 * k > L)


def _logits(name, kind, T, B, C, dtype):
    if kind in tie_inputs.TIE_FAMILIES:
        return tie_inputs.family(name, kind, T, B, C, dtype)
    return real_family(tie_inputs.rng_for(name), kind, T, B, C, dtype)


def _fcase(name, kind, L, T=None, N=12, C=6, dtype=np.float32, blank=0, **extra):
    """A forced_align tie case: B = 3 with frames [T, T - 5, 0], the lists of test_gpu_target_scores; `edges` are the
    label indices of the full-length rows in the first and the last lane of a segment that holds a label."""
    T = L + 7 if T is None else T
    sl = [T, max(T - 5, 0), 0]
    y, n = _lists(tie_inputs.rng_for(name + " lists"), 3, N, L, C, min(L, T))
    return dict(x=_logits(name, kind, T, 3, C, dtype), sl=np.array(sl, np.int32), y=y, n=n, blank=blank, entry="forced",
                edges=[0, min(L, T) - 1], **dict(dict(route=1), **extra))


def _tcase(name, kind, L, T=None, C=6, dtype=np.float32, blank=0, thread=None, **extra):
    """An align_transcripts tie case: B = 3 with frames [T, T - 5, 0], N = 3 rows: one label, a full-length walk
    without a repeat, and a full-length walk with an equal pair across every wave boundary.  `edges` are the label
    indices either side of each wave boundary, and of the boundary in front of thread `thread`."""
    T = L + 8 if T is None else T
    K = _block(L)
    y, n = _lists(tie_inputs.rng_for(name + " lists"), 3, 4, L, C, min(L, T))
    c = dict(x=_logits(name, kind, T, 3, C, dtype), sl=np.array([T, max(T - 5, 0), 0], np.int32), y=y[:, 1:].copy(),
             n=n[:, 1:].copy(), blank=blank, entry="transcripts", **extra)
    waves = [64 * K * w for w in (1, 2, 3) if 64 * K * w < L]
    for pos in waves:
        _equal_at(pos)(c)
    c["edges"] = [j for pos in waves + ([thread * K] if thread else []) for j in (pos - 1, pos)]
    return c


FAMILIES3, FAMILIES2 = ("flat", "grid_hot", "onehot"), ("flat", "grid_hot")
FORCED = {"seg-L%d-%s" % (L, k): dict(kind=k, L=L) for L in (7, 15, 31, 63) for k in FAMILIES3}
FORCED.update({"pack-N33-%s" % k: dict(kind=k, L=7, N=33) for k in FAMILIES2})
FORCED.update({"time-%d-%s" % (T, k): dict(kind=k, L=L, T=T)   # (L = 7 at the word: frames to spare, or nothing ties)
               for L, T in ((7, W10), (7, W10 + 1), (15, TILE), (15, TILE + 1)) for k in FAMILIES2})
FORCED.update({"gathered-%s" % k: dict(kind=k, L=15, route=2, env="gathered") for k in FAMILIES2})
FORCED.update({"C1100-%s" % k: dict(kind=k, L=7, T=8, C=1100, route=2) for k in FAMILIES2})
FORCED.update({"float64-%s" % k: dict(kind=k, L=15, dtype=np.float64) for k in FAMILIES2 + ("flatgrid",)})
FORCED.update({"bf16-slice-grid_hot": dict(kind="grid_hot", L=15, half="bfloat16"),
               "flatgrid-L31": dict(kind="flatgrid", L=31)})
TRANSCRIPTS = {"wave-L%d-%s" % (L, k): dict(kind=k, L=L) for L in (63, 64, 65, 128, 255) for k in FAMILIES2}
TRANSCRIPTS.update({"K%d-L%d-%s" % (_block(L), L, k): dict(kind=k, L=L, thread=5)
                    for L in (256, 300, 600, 1100) for k in FAMILIES2})
TRANSCRIPTS.update({"time-%d-%s" % (T, k): dict(kind=k, L=70, T=T) for T in (4 * F - 1, 4 * F, 4 * F + 1) for k in FAMILIES2})
TRANSCRIPTS.update({
    "float64-flat": dict(kind="flat", L=70, dtype=np.float64),
    "float64-grid_hot": dict(kind="grid_hot", L=70, dtype=np.float64),
    "flatgrid-L70": dict(kind="flatgrid", L=70),
    "bf16-slice-grid_hot": dict(kind="grid_hot", L=70, half="bfloat16"),
    "shared-grid_hot": dict(kind="grid_hot", L=70, shared=True),
})
# a second draw where the first one's end state never ties on an aligned row (test_cpu_alignment_inputs asserts what
# every case must do): the seed's name gets a suffix, the case keeps its name
REDRAWN = {"transcripts-wave-L65-grid_hot": " #1", "transcripts-wave-L255-grid_hot": " #1", "transcripts-K8-L1100-grid_hot": " #1"}
TIE_CASES = {"forced-" + k: functools.partial(_fcase, "forced-" + k, **v) for k, v in FORCED.items()}
TIE_CASES.update({"transcripts-" + k: functools.partial(_tcase, "transcripts-" + k + REDRAWN.get("transcripts-" + k, ""), **v)
                  for k, v in TRANSCRIPTS.items()})
# The comparisons a case is meant for, where not all three.  On flat logits every reachable state holds the same value, so
# the definition's walk stays in the final blank for as long as that is reachable and then runs down the trellis's lower
# edge s = 2 f + 1, where v[s] and v[s - 1] are -inf and the skip is forced: it meets no label state at which decision 2
# has a choice, and >= there changes nothing.  The flat cases are for decision 1 and the end state (each ties at every
# reachable state), and so are the flatgrid ones, whose frames differ but whose states do not; the grid_hot and onehot
# cases of the same shapes separate all three.
MEANT_FOR = {k: ("decision 1", "end state") for k in TIE_CASES if "flat" in k}


PLANTED = {"%s-%s-L%d" % (entry, k, L): functools.partial(tie_inputs.planted_case, "%s-%s-L%d" % (entry, k, L), k.split("-")[0], L,
                                                          N, entry=entry, edges=k.endswith("edges"))
           for entry, L, N in (("forced", 15, 12), ("transcripts", 70, 4), ("transcripts", 300, 4))
           for k in ("masked", "nonfinite", "nonfinite-edges")}
BLANKS = {"%s-blank%d-%s" % (entry, blank, k): functools.partial(
    _fcase if entry == "forced" else _tcase, "%s-blank%d-%s" % (entry, blank, k), k, L, blank=blank)
    for entry, L in (("forced", 15), ("transcripts", 70)) for blank in (5, 2) for k in ("sticky", "flat")}
CASES = dict(TIE_CASES, **PLANTED, **BLANKS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    if c.get("half"):   # values the two-byte format holds exactly
        c["x"] = torch.as_tensor(c["x"]).to(getattr(torch, c["half"])).float().numpy()
    if c.get("shared"):
        c["y"], c["n"] = np.repeat(c["y"][:1], 3, 0), np.repeat(c["n"][:1], 3, 0)
    c["want"] = expected(c["x"], c["sl"], c["y"], c["n"], blank=c["blank"])
    logp = c["want"]["logp"]
    assert (logp > -np.inf).any() and not (logp > -np.inf).all(), name   # an aligned row and an unaligned one
    return c


def _device_logits(c):
    x, kw = np.array(c["x"]), {}
    T, B, C = x.shape
    if c.get("half"):   # a batch-major two-byte view with gaps in both dimensions, read in place
        full = torch.zeros((B, T, 40), dtype=getattr(torch, c["half"]), device=DEV)
        full[:, :, 5:5 + C] = torch.as_tensor(x.transpose(1, 0, 2).copy(), device=DEV)
        x, kw = full[:, :, 5:5 + C], dict(batch_first=True)
    return x, kw


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_definition(name, monkeypatch):
    c = case(name)
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    if "env" in c:
        monkeypatch.setenv("CTCEXT_TARGETS", c["env"])
    x, kw = _device_logits(c)
    y, n = (c["y"][0], c["n"][0]) if c.get("shared") else (c["y"], c["n"])
    if c["entry"] == "forced":
        _check(_forced(x, c["sl"], y, n, blank_index=c["blank"], **kw), c["want"], name)
        assert _route() == c.get("route", 1)   # (staged, unless the case says otherwise)
    else:
        _check(_align(ctcext_amd.align_transcripts, x, c["sl"], y, n, blank_index=c["blank"], **kw), c["want"], name)


@pytest.mark.parametrize("kind", ["flat", "masked"])
def test_short_lists_agree_between_the_two_kernels(kind, monkeypatch):
    monkeypatch.delenv("CTCEXT_TARGETS", raising=False)
    c = case("forced-seg-L63-flat") if kind == "flat" else tie_inputs.planted_case("both-masked-L63", "masked", 63, 12)
    want = expected(c["x"], c["sl"], c["y"], c["n"])
    assert (want["logp"] > -np.inf).any()
    _check(_forced(c["x"], c["sl"], c["y"], c["n"]), want, kind + ", forced_align")
    _check(_align(ctcext_amd.align_transcripts, c["x"], c["sl"], c["y"], c["n"]), want, kind + ", align_transcripts")


@pytest.mark.parametrize("lds", [False, True], ids=["registers", "lds"])
def test_path_alignments_of_greedy_rows_under_ties(lds, monkeypatch):
    """The two older alignment kernels on the same ties: dense_path_alignments behind a greedy decode equals the
    definition for the greedy rows, and dense_transcript_alignments of those rows fed back."""
    monkeypatch.delenv("CTCEXT_PATHS_LDS", raising=False)
    if lds:
        monkeypatch.setenv("CTCEXT_PATHS_LDS", "1")
    T, B, C = 150, 3, 6
    x, sl = tie_inputs.family("greedy rows under ties", "grid_hot", T, B, C), np.array([150, 147, 90], np.int32)
    out = ctcext_amd.decode_greedy(torch.as_tensor(x, device=DEV), torch.as_tensor(sl, device=DEV), batch_first=False,
                                   token_scores=True)
    pa = ctcext_amd.dense_path_alignments(times=True, scores=True)
    ta = ctcext_amd.dense_transcript_alignments(out.decoded, out.decoded_lengths, scores=True)
    torch.cuda.synchronize()
    dec, lens = out.decoded.cpu().numpy(), out.decoded_lengths.cpu().numpy()
    rows = [[[int(v) for v in dec[b, 0, :lens[b, 0]]]] for b in range(B)]
    assert min(len(r[0]) for r in rows) > 8
    cs = tie_inputs.census(x, sl, np.stack([np.pad(r[0], (0, T - len(r[0]))) for r in rows])[:, None, :],
                           np.array([[len(r[0])] for r in rows], np.int32))
    assert cs["aligned"] == B and all(cs["separates"].values()), cs["separates"]
    _check_paths(pa, pau.expected(x, sl, rows, 1), sl, rows, "greedy rows")
    L = out.decoded.shape[-1]
    want = dict(logp=pa.logp, start=pa.times.start[..., :L], end=pa.times.end[..., :L],
                trailing_blank=pa.times.trailing_blank, logp_sum=pa.scores.logp_sum[..., :L],
                logp_min=pa.scores.logp_min[..., :L])
    _check(ta, {k: v.cpu().numpy() for k, v in want.items()}, "fed back")
    ctcext_amd.dense_check()
