"""Shared by the stream blank-skipping tests (include/ctcext.h, "Streaming:
blank-frame skipping"): push schedules over a batch of ragged items, the chunks
they feed, and what the oracle-side plan (skip_util.plan) says a schedule
exercises -- the share of frames dropped, the (item, push) pairs whose frames
are all dropped, and the pushes that begin inside a run."""
import numpy as np


def schedule(sl, push):
    """Frames per item for each push: every item takes its next `push` frames
    (None: all of them) until its sl[b] are gone; [pushes][B]."""
    sl = [max(int(v), 0) for v in sl]
    if push is None:
        return [sl]
    out, pos = [], [0] * len(sl)
    while any(p < n for p, n in zip(pos, sl)):
        step = [min(push, n - p) for p, n in zip(pos, sl)]
        out.append(step)
        pos = [p + s for p, s in zip(pos, step)]
    return out


def chunk(x, pos, n, width=None):
    """The [width, B, C] chunk that holds item b's frames pos[b] .. pos[b] + n[b] - 1
    of x [T, B, C] (zeros behind them); width defaults to max(n), at least 1."""
    B, C = x.shape[1], x.shape[2]
    w = max(max(n), 1) if width is None else width
    c = np.zeros((w, B, C), x.dtype)
    for b in range(B):
        c[:n[b], b] = x[pos[b]:pos[b] + n[b], b]
    return c


def kept_between(kmap, lo, hi):
    """The entries of the ascending kmap in [lo, hi)."""
    return [t for t in kmap if lo <= t < hi]


def exercised(kmaps, sched):
    """(wholly dropped (item, push) pairs, (item, push) pairs that begin with a
    dropped frame) of the schedule, from the items' kmaps of all their frames."""
    B = len(kmaps)
    pos = [0] * B
    kept = [set(k) for k in kmaps]
    whole = straddle = 0
    for n in sched:
        for b in range(B):
            if n[b] > 0:
                whole += not any(t in kept[b] for t in range(pos[b], pos[b] + n[b]))
                straddle += pos[b] not in kept[b]
            pos[b] += n[b]
    return whole, straddle
