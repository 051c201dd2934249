"""Shared by the stream token-scores tests (include/ctcext.h, "Streaming: token
scores"): what each item of a stream holds after a push, the expected times
and scores of that (token_scores_util.expected / expected_skip applied to the
rows committed so far, width max_frames), the push schedules of the GPU cases
and the properties the CPU tests assert on them."""
import functools

import numpy as np

import skip_util
import stream_skip_util as ssu
import token_scores_util as tsu
from token_times_util import family


class Held:
    """Host mirror of a stream: the rows each item has committed since its last
    reset, in the compute dtype."""

    def __init__(self, B, C, dtype=np.float32):
        self.B, self.C, self.dtype = B, C, np.dtype(dtype)
        self.rows = [np.zeros((0, C), self.dtype) for _ in range(B)]

    def take(self, b, rows):
        self.rows[b] = np.concatenate([self.rows[b], np.asarray(rows, self.dtype).reshape(-1, self.C)])

    def take_chunk(self, chunk, n, items=None):
        """Item b takes the first n[b] rows of chunk [t, B, C] (items: those that do; all)."""
        for b in (range(self.B) if items is None else items):
            self.take(b, chunk[:int(n[b]), b])

    def reset(self, b):
        self.rows[b] = np.zeros((0, self.C), self.dtype)

    def frames(self):
        return [len(r) for r in self.rows]

    def tensor(self, items=None):
        """([T, len(items), C], frames) of the named items (all), T their longest, at least 1."""
        items = list(range(self.B)) if items is None else list(items)
        fr = [len(self.rows[b]) for b in items]
        x = np.zeros((max(fr + [1]), len(items), self.C), self.dtype)
        for i, b in enumerate(items):
            x[:fr[i], i] = self.rows[b]
        return x, np.array(fr, np.int32)


def expected_held(held, W, P, width, skip_thr=None, **kw):
    """(times, scores) of what `held` holds, every array over all B items.  An
    item without frames has no timed token (and, with top_paths > 1, a
    few-leaves bit): times of -1 / 0 and NaN rows, as tiled_case builds them."""
    B = held.B
    live = [b for b in range(B) if len(held.rows[b]) > 0]
    start = np.full((B, P, width), -1, np.int32)
    end = np.full((B, P, width), -1, np.int32)
    trail = np.zeros((B, P), np.int32)
    lsum = np.full((B, P, width), np.nan, held.dtype)
    lmin = np.full((B, P, width), np.nan, held.dtype)
    if live:
        x, fr = held.tensor(live)
        if skip_thr is None:
            _, _, t, s = tsu.expected(x, fr, W, P, width, **kw)
        else:
            t, s = tsu.expected_skip(x, skip_util.expected(x, fr, W, P, skip_thr, **kw), fr, P, width, **kw)
        start[live], end[live], trail[live] = t
        lsum[live], lmin[live] = s
    return (start, end, trail), (lsum, lmin)


def run_schedule(x, sl, push, W, P, width, skip_thr=None, **kw):
    """The pushes of stream_skip_util.schedule(sl, push) over x [T, B, C]: per
    push (chunk [push, B, C], n [B], frames after it, times, scores)."""
    T, B, C = x.shape
    held = Held(B, C, x.dtype)
    pos = [0] * B
    out = []
    for n in ssu.schedule(sl, push):
        chunk = ssu.chunk(x, pos, n, width=push)
        held.take_chunk(chunk, n)
        pos = [p + k for p, k in zip(pos, n)]
        times, scores = expected_held(held, W, P, width, skip_thr, **kw)
        out.append((chunk, np.array(n, np.int32), list(pos), times, scores))
    return out


def crossing_spans(times, scores, push):
    """(scored spans that start in one push of `push` frames and end in a later
    one, timed tokens) of the expectations after the last push."""
    start, end, _ = times
    timed = (start >= 0) & ~np.isnan(scores[0])
    cross = timed & (start // push != end // push)
    return int(cross.sum()), int(timed.sum())


# ---- the schedules of the GPU cases, built once per process

# case 1: (family, (T, B, C, W, P), merge_repeated, frames per push)
EVERY_PUSH = [("sticky", (12, 6, 5, 8, 3), True, 5), ("sticky", (40, 4, 29, 16, 3), True, 7),
              ("peaky", (40, 4, 29, 16, 3), True, 7), ("sticky", (60, 3, 29, 128, 3), True, 16),
              ("gaussian", (60, 3, 29, 128, 3), False, 16), ("neg_inf", (12, 6, 5, 8, 3), True, 5)]
# case 2: ((T, B, C, W, P), soft, frames per push)
TILED_PUSH = [(tsu.TILED[0], True, 100), (tsu.TILED[1], False, 64)]
# crossing spans of timed tokens measured on the oracle, per schedule
CROSSING = {("sticky", (12, 6, 5, 8, 3), 5): (6, 35), ("sticky", (40, 4, 29, 16, 3), 7): (50, 107),
            ("peaky", (40, 4, 29, 16, 3), 7): (4, 122), ("sticky", (60, 3, 29, 128, 3), 16): (20, 146),
            ("tiled", tsu.TILED[0], 100): (15, 724), ("tiled", tsu.TILED[1], 64): (20, 242),
            ("gaussian", (60, 3, 29, 128, 3), 16): (0, None)}


def case_id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


@functools.lru_cache(maxsize=None)
def every_push_case(kind, shape, merge, push):
    T, B, C, W, P = shape
    x, sl, kw, _ = tsu.family_case(kind, shape, merge)
    return x, sl, kw, run_schedule(x, sl, push, W, P, T, **kw)


@functools.lru_cache(maxsize=None)
def tiled_push_case(shape, soft, push):
    T, B, C, W, P = shape
    x, sl, kw = tsu.tiled_case(shape, soft)[:3]
    return x, sl, kw, run_schedule(x, sl, push, W, P, T, **kw)


@functools.lru_cache(maxsize=None)
def skip_push_case(push):
    """token_scores_util.skip_case() in pushes of `push` frames, with the
    threshold of the skipping tests."""
    T, B, C, W, P = tsu.SKIP_SHAPE
    x, sl, kw, e = tsu.skip_case()[:4]
    return x, sl, kw, e, run_schedule(x, sl, push, W, P, T, skip_thr=skip_util.THR, **kw)


# case 5, first part: chunk 1, a decoy the stream must forget, chunk 2
ROLLBACK_SHAPE = (32, 3, 29, 128, 3)   # W = 128, C = 29: the two-wave kernel, whose hand-over the test flag fails
ROLLBACK_PUSH = 16


@functools.lru_cache(maxsize=None)
def rollback_case():
    """(x [32, B, C], decoy [16, B, C], kw, expectations after chunk 1, after
    chunk 1 + chunk 2, and those a store that kept the decoy's rows in place of
    chunk 2's would give for the true alignment and times)."""
    T, B, C, W, P = ROLLBACK_SHAPE
    n = ROLLBACK_PUSH
    x = family(np.random.default_rng(515), "sticky", T, B, C)
    decoy = family(np.random.default_rng(516), "gaussian", n, B, C)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    held = Held(B, C)
    held.take_chunk(x[:n], [n] * B)
    first = expected_held(held, W, P, T, **kw)
    held.take_chunk(x[n:], [n] * B)
    both = expected_held(held, W, P, T, **kw)
    # the true rows' alignment and times over a store whose second half is the decoy's rows
    wrong = np.concatenate([x[:n], decoy])
    dec, ali, times, _ = tsu.expected(x, [T] * B, W, P, T, **kw)
    dl = [[len(dec[b][p]) for p in range(P)] for b in range(B)]
    mixed = tsu.expected_from_rows_and_times(wrong, ali, [T] * B, times[0], times[1], dl, B, P, T, 0, -1)
    # (the normaliser is the wrong rows' own there; with the true one the terms differ all the same)
    return x, decoy, kw, first, both, mixed
