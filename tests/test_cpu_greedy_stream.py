"""The greedy stream without a GPU: what ctcext_greedy_stream_validate refuses, and that the inputs test_gpu_greedy_stream
pushes hold, in the reference, what they are there for.  The cases, their chunkings and the host model of a stream
(the host definitions over the frames an item has taken so far) are shared with that file."""
import ctypes
import functools

import numpy as np
import pytest

import ctcext_amd
import oracle
import range_inputs
from ctcext_amd import _lib
from test_cpu_greedy import greedy, quantised, special, sticky


def ranged(rng, T, B, C, dtype=np.float32):
    """Finite logits over the whole float range (its +-0 ties included) with NaN and infinite cells on top."""
    cells = special(rng, T, B, C, dtype)
    x = np.where(np.isfinite(cells), range_inputs.family(rng, "edges", T, B, C, dtype), cells)
    x[3::8] = np.where(rng.random(x[3::8].shape) < 0.5, 0.0, -0.0)   # every class ties at a zero of either sign ...
    x[3::8, :, 0] = -1                                               # ... but the blank: class 1 must win
    return x.astype(dtype)


# name: (family, [T, B, C], dtype of the chunks, chunking, merge_repeated).  "all": one push; "ones": pushes of one
# frame; "ragged": the sizes below, 130 being more than the 64 chunk rows a step of the kernel covers.  C = 33 is one
# past the LDS tile of 32 classes, 1000 and 1091 are rows of many tiles, whole and not.
RAGGED = (3, 0, 64, 1, 65, 63, 130)
CASES = {
    "quantised-7x3x5-ones": (quantised, (7, 3, 5), "float32", "ones", True),
    "ranged-7x3x5-ragged": (ranged, (7, 3, 5), "float32", "ragged", False),
    "quantised-1x1x1-all": (quantised, (1, 1, 1), "float32", "all", False),
    "quantised-70x130x29-ragged": (quantised, (70, 130, 29), "float32", "ragged", True),
    "sticky-70x130x29-bf16-all": (sticky, (70, 130, 29), "bfloat16", "all", True),
    "quantised-70x130x29-f16-ragged": (quantised, (70, 130, 29), "float16", "ragged", False),
    "sticky-600x2x33-ragged": (sticky, (600, 2, 33), "float32", "ragged", True),
    "sticky-600x2x33-ragged-nomerge": (sticky, (600, 2, 33), "float32", "ragged", False),
    "sticky-600x2x33-f64-all": (sticky, (600, 2, 33), "float64", "all", True),
    "ranged-600x2x33-f64-ragged": (ranged, (600, 2, 33), "float64", "ragged", True),
    "quantised-40x2x300-ones": (quantised, (40, 2, 300), "float32", "ones", True),
    "ranged-40x2x300-ragged": (ranged, (40, 2, 300), "float32", "ragged", False),
    "ranged-10x3x1000-ragged": (ranged, (10, 3, 1000), "float32", "ragged", True),
    "quantised-9x2x1091-all": (quantised, (9, 2, 1091), "float32", "all", True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The widened logits [T, B, C] of a case and its pushes: (chunk_time, lengths [B]) each.  Item 0 takes every
    chunk whole; the others take, in turn, all of it, half of it, nothing, and a negative length (which reads as 0)."""
    fam, (T, B, C), dt, how, _ = CASES[name]
    import torch
    x = torch.as_tensor(fam(range_inputs.rng_for(name), T, B, C, np.float64 if dt == "float64" else np.float32))
    x = x.to(getattr(torch, dt))
    wide = x.numpy() if dt == "float64" else x.float().numpy()
    sizes = {"all": (T,), "ones": (1,), "ragged": RAGGED}[how]
    pushes, done = [], 0
    while done < T:
        t = min(sizes[len(pushes) % len(sizes)], T - done)
        i = len(pushes)
        pushes.append((t, np.array([t] + [(t, t // 2, 0, -2)[(i + b) % 4] for b in range(1, B)], np.int32)))
        done += t
    return wide, pushes


class Model:
    """The frames each item of a stream has taken since its last reset, and from them what the stream must hold:
    greedy_row, token_times_row and token_scores_row over oracle.row_norm."""

    def __init__(self, B, C, F, dtype, merge):
        self.B, self.F, self.merge = B, F, merge
        self.rows, self.memo = [np.zeros((0, C), dtype) for _ in range(B)], [None] * B

    def take(self, b, rows):
        if len(rows):
            self.rows[b], self.memo[b] = np.concatenate([self.rows[b], rows]), None

    def reset(self, b):
        self.rows[b], self.memo[b] = self.rows[b][:0], None

    def item(self, b):
        if self.memo[b] is None:
            x, n = np.ascontiguousarray(self.rows[b]), len(self.rows[b])
            norm = oracle.row_norm(x) if n else np.zeros((0,), x.dtype)
            d, a, logp = ctcext_amd.greedy_row(x, norm, n, 0, -1, self.merge)
            s, e, trail = ctcext_amd.token_times_row(d, a, n, -1, merge_repeated=self.merge)
            lsum, lmin = ctcext_amd.token_scores_row(x, norm, a, n, s, e, 0, -1)
            self.memo[b] = (d, a, logp, s, e, trail, lsum, lmin)
        return self.memo[b]

    def expected(self, status):
        """GreedyPush as numpy arrays, times and scores flattened into it."""
        B, F, ft = self.B, self.F, self.rows[0].dtype
        out = dict(decoded=np.full((B, 1, F), -1, np.int64), decoded_lengths=np.zeros((B, 1), np.int32),
                   alignment=np.full((B, 1, F), -1, np.int64), alignment_lengths=np.zeros((B, 1), np.int32),
                   log_probability=np.zeros((B, 1), ft), status=np.asarray(status, np.int32),
                   frames=np.zeros((B,), np.int32), start=np.full((B, 1, F), -1, np.int32),
                   end=np.full((B, 1, F), -1, np.int32), trailing_blank=np.zeros((B, 1), np.int32),
                   logp_sum=np.full((B, 1, F), np.nan, ft), logp_min=np.full((B, 1, F), np.nan, ft))
        for b in range(B):
            d, a, logp, s, e, trail, lsum, lmin = self.item(b)
            m, n = len(d), len(a)
            out["decoded"][b, 0, :m], out["alignment"][b, 0, :n], out["log_probability"][b, 0] = d, a, logp
            out["decoded_lengths"][b, 0], out["alignment_lengths"][b, 0], out["frames"][b] = m, n, n
            out["start"][b, 0, :m], out["end"][b, 0, :m], out["trailing_blank"][b, 0] = s, e, trail
            out["logp_sum"][b, 0, :m], out["logp_min"][b, 0, :m] = lsum, lmin
        return out


@pytest.mark.parametrize("name", ["sticky-600x2x33-ragged", "quantised-70x130x29-ragged"])
def test_the_inputs_hold_what_they_are_there_for(name):
    """In the reference: a run split by a push boundary, a merged A-blank-A and a dropped repeat."""
    (wide, pushes), merge = case(name), CASES[name][4]
    xb = np.ascontiguousarray(wide[:, 0])
    norm = oracle.row_norm(xb)
    dec, ali, _ = greedy(xb, norm, len(xb), 0, -1, merge)
    bounds = np.cumsum([t for t, _ in pushes])[:-1]
    runs = sum(1 for f in range(1, len(ali)) if ali[f] != -1 and ali[f] != ali[f - 1]) + (ali[0] != -1)
    assert len(dec) < len(ali) - ali.count(-1)                                # a dropped repeat
    if name.startswith("sticky"):
        assert len(dec) < runs                                                # a merged A-blank-A
        assert any(ali[f] != -1 and ali[f] == ali[f - 1] for f in bounds)     # a run split by a push boundary


def _args(**change):
    a, w = _lib.StreamArgs(), _lib.GreedyStreamWant()
    a.dtype, a.on_device, a.batch_size, a.num_classes, a.max_frames = _lib.CTCEXT_F32, 1, 2, 5, 8
    a.beam_width, a.top_paths, a.blank_index, a.blank_label = 1, 1, 0, -1
    w.token_times, w.pad_value = 1, -1
    for k, v in change.items():
        setattr(w if hasattr(w, k) else a, k, v)
    return a, w


TABLE = np.full((6, 5), -1.0, np.float32)


@pytest.mark.parametrize("change, message", [
    (dict(top_paths=2, beam_width=2), "top_paths must be 1"),
    (dict(scorer=_lib.CTCEXT_SCORER_BIGRAM, scorer_table=TABLE.ctypes.data), "takes no beam scorer"),
    (dict(on_device=0), "needs device chunks"),
    (dict(blank_label=3), "token times need a blank_label that is no class label"),
    (dict(blank_label=3, token_times=0, token_scores=1), "token times need a blank_label that is no class label"),
    (dict(flags=_lib.CTCEXT_FLAG_GLOBAL_STATE), "flags may hold only CTCEXT_FLAG_PROFILE"),
])
def test_validate_refuses(change, message):
    lib = _lib.load()
    a, w = _args(**change)
    assert lib.ctcext_greedy_stream_validate(ctypes.byref(a), ctypes.byref(w)) == _lib.CTCEXT_INVALID_ARGUMENT
    assert message in lib.ctcext_last_error().decode()


def test_validate_accepts_and_the_class_validates_at_once():
    lib = _lib.load()
    for change in (dict(), dict(blank_label=3, token_times=0), dict(blank_label=0, token_scores=1)):
        a, w = _args(**change)
        assert lib.ctcext_greedy_stream_validate(ctypes.byref(a), ctypes.byref(w)) == _lib.CTCEXT_OK
    with pytest.raises(ctcext_amd.InvalidArgumentError, match="no class label"):
        ctcext_amd.GreedyStream(2, 5, 8, blank_label=3)   # (on the host, before any device is touched)
