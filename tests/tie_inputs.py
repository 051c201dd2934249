"""Logits on which the alignment recursions tie or meet -inf, NaN and +inf,
shared by the alignment-ties tests.

The other alignment tests draw real-valued gaussian and sticky logits: no two
trellis states ever hold the same value there, so a kernel that compared with
>= where the definition of include/ctcext.h, "Path alignments", says "strictly
greater" would pass them all.  The families here make states tie (flat,
flatgrid, onehot, grid_hot), put -inf logits under a target that stays feasible
(masked), or put one NaN, one +inf or one frame of -inf into an item
(nonfinite).  align_variant is the definition with each of its three
comparisons switchable to >=, and a map of where the inputs tie: what
test_cpu_alignment_inputs asserts about every case is a condition on the
inputs, not a measurement of the code under test.

Every seed comes from range_inputs.rng_for(name)."""
import numpy as np

import oracle
import range_inputs
from range_inputs import rng_for
from token_times_util import family as _family

TIE_FAMILIES = ("flat", "flatgrid", "onehot", "grid_hot")
MUTANTS = {"decision 1": (False, True, True), "decision 2": (True, False, True), "end state": (True, True, False)}


def family(name, kind, T, B, C, dtype=np.float32):
    """[T, B, C] logits of one tie family.
    flat      every logit 0: every reachable state ties with its neighbours at every frame;
    flatgrid  per frame and item one constant of {0, -0.25, ..., -2} for all classes;
    onehot    range_inputs' onehot: norm == max on every row, totals on a 0.5 grid;
    grid_hot  flat rows, about one frame in five replaced by an onehot row: ties appear and break along the row."""
    rng = rng_for(name)
    if kind == "flat":
        x = np.zeros((T, B, C))
    elif kind == "flatgrid":
        x = np.repeat(rng.integers(0, 9, size=(T, B, 1)) * -0.25, C, axis=2)
    elif kind == "onehot":
        x = range_inputs.family(rng, "onehot", T, B, C, np.float64)
    elif kind == "grid_hot":
        x = np.zeros((T, B, C))
        hot = range_inputs.family(rng, "onehot", T, B, C, np.float64)
        pick = rng.random((T, B)) < 0.2
        x[pick] = hot[pick]
    else:
        raise ValueError(kind)
    return x.astype(dtype)


def collapse(path, blank):
    """The CTC collapse of a per-frame class path: repeats merged, then blanks dropped."""
    return [int(c) for i, c in enumerate(path) if c != blank and (i == 0 or c != path[i - 1])]


def plant(rng, xb, blank):
    """A target that is feasible over xb [frames, C] by construction: a class drawn among the frame's finite ones is
    held 2 to 7 frames (less where it meets a -inf), and the path is collapsed the CTC way."""
    path, t = [], 0
    while t < len(xb):
        c, hold = int(rng.choice(np.nonzero(np.isfinite(xb[t]))[0])), int(rng.integers(2, 8))
        for _ in range(hold):
            if t == len(xb) or not np.isfinite(xb[t, c]):
                break
            path.append(c)
            t += 1
    return collapse(path, blank)


def masked(name, T, sl, C, blank=0, dtype=np.float32):
    """(x [T, B, C], planted): sticky logits with -inf at p = 0.15 and the blank additionally at p = 0.15 (a row left
    without a finite logit gets its largest one back), and per item one planted target over its frames."""
    rng = rng_for(name)
    B = len(sl)
    x = _family(rng, "sticky", T, B, C, dtype)
    keep = x.copy()
    x[rng.random(x.shape) < 0.15] = -np.inf
    x[rng.random((T, B)) < 0.15, blank] = -np.inf
    for t, b in zip(*np.nonzero(~np.isfinite(x).any(axis=2))):
        x[t, b, keep[t, b].argmax()] = keep[t, b].max()
    return x, [plant(rng, x[:max(int(sl[b]), 0), b], blank) for b in range(B)]


def nonfinite(name, T, sl, C, blank=0, dtype=np.float32, edges=False):
    """(x [T, 4, C], planted): sticky logits and a planted target per item; item 0 stays clean, item 1 gets one NaN
    logit, item 2 one +inf logit and item 3 one frame of -inf, each in a frame of the planted target's alignment (the
    NaN and the +inf at that frame's class): the middle one, or with `edges` frame 0 (items 1 and 3) and the last
    frame (item 2)."""
    import path_alignments_util as pau
    rng = rng_for(name)
    assert len(sl) == 4 and min(sl) > 0
    x = _family(rng, "sticky", T, 4, C, dtype)
    planted = [plant(rng, x[:int(sl[b]), b], blank) for b in range(4)]
    for b in (1, 2, 3):
        fr = int(sl[b])
        xb = np.ascontiguousarray(x[:fr, b])
        ali, logp = pau.align(xb, oracle.row_norm(xb), planted[b], fr, blank, blank)
        assert np.isfinite(logp) and len(ali) == fr
        f = (0, fr - 1, 0)[b - 1] if edges else fr // 2
        if b == 3:
            x[f, b, :] = -np.inf
        else:
            x[f, b, ali[f]] = np.nan if b == 1 else np.inf
    return x, planted


def planted_case(name, kind, L, N, dtype=np.float32, blank=0, edges=False, entry="forced"):
    """B = 4 with frames [T, T - 5, T - 1, T], T = L + 10, C = 6: masked or nonfinite logits, the lists of
    test_gpu_target_scores and, in the last row of every item, its planted target."""
    from test_gpu_target_scores import _lists
    T, C = L + 10, 6
    sl = np.array([T, T - 5, T - 1, T], np.int32)
    x, planted = masked(name, T, sl, C, blank, dtype) if kind == "masked" else nonfinite(name, T, sl, C, blank, dtype, edges)
    y, n = _lists(rng_for(name + " lists"), 4, N, L, C, min(L, T))
    for b, row in enumerate(planted):
        assert len(row) <= L, name
        n[b, -1], y[b, -1, :len(row)] = len(row), row
    return dict(x=x, sl=sl, y=y, n=n, blank=blank, entry=entry, kind=kind, planted=planted)


def align_variant(x, norm, y, frames, blank, strict=(True, True, True), maps=None):
    """The definition of "Path alignments" for one row, in numpy in x's dtype, with each of its three comparisons
    (decision 1, decision 2, end state) strict as the definition has it or, where strict[i] is False, >=.
    Returns (alignment, logp, ties): the alignment with -1 at a blank frame (empty for an unaligned row), and ties
    [frames, S], true where the state's step or skip source holds a finite value equal to the best so far: where > and >=
    part.  maps (a dict) receives `end_tie`, `states` (the walked state per frame) and `sibling` (the (frame, state)
    pairs of the walk at which a source of the step is -inf while the best is finite)."""
    ft = x.dtype.type
    gt = [np.greater if s else np.greater_equal for s in strict]
    m, C, ninf = len(y), x.shape[1], ft(-np.inf)
    if maps is None:
        maps = {}
    maps.update(end_tie=False, states=[], sibling=[])
    if any(c < 0 or c >= C for c in y):
        return [], ft(np.nan), np.zeros((frames, 2 * m + 1), bool)
    if frames == 0:
        return [], (ft(0) if m == 0 else ninf), np.zeros((0, 2 * m + 1), bool)
    z = np.full(2 * m + 1, blank, np.int64)
    z[1::2] = y
    S = z.size
    skip = np.zeros(S, bool)
    skip[3::2] = z[3::2] != z[1:-2:2]
    dec, ties, lone = np.zeros((frames, S), np.int8), np.zeros((frames, S), bool), np.zeros((frames, S), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        lp = (x[:frames][:, z] - np.asarray(norm)[:frames, None]).astype(ft)
        v = np.full(S, ninf)
        v[:2] = lp[0, :2]
        for f in range(1, frames):
            one, two = np.concatenate(([ninf], v))[:-1], np.concatenate(([ninf, ninf], v))[:-2]
            best = v.copy()
            t1 = np.isfinite(one) & (one == best)
            d1 = gt[0](one, best)
            d1[0] = False                                   # (state 0 has no state in front)
            best[d1] = one[d1]
            t2 = skip & np.isfinite(two) & (two == best)
            d2 = skip & gt[1](two, best)
            best[d2] = two[d2]
            dec[f], ties[f] = np.where(d2, 2, d1), t1 | t2
            lone[f] = np.isfinite(best) & ((np.isneginf(one) & (np.arange(S) > 0)) | (skip & np.isneginf(two)))
            v = best + lp[f]
        maps["end_tie"] = bool(m and np.isfinite(v[-1]) and v[-2] == v[-1])
        s = S - 1 - (1 if m and gt[2](v[-2], v[-1]) else 0)
    logp = v[s]
    if not logp > ninf:
        return [], logp, ties
    out = []
    for f in range(frames - 1, -1, -1):
        out.append(int(z[s]) if s % 2 else -1)
        maps["states"].append(s)
        if lone[f][s]:
            maps["sibling"].append((f, s))
        s -= int(dec[f][s])
    maps["states"].reverse()
    return out[::-1], logp, ties


def in_band(ties, frames):
    """ties with everything below the band s >= S - 2 (frames - f) cleared: the states that still reach the end."""
    S = ties.shape[1]
    f, s = np.arange(frames)[:, None], np.arange(S)[None, :]
    return ties[:frames] & (s >= S - 2 * (frames - f))


def census(x, sl, y, n, blank=0):
    """What a tie case's inputs do, over its aligned rows: `ties` (finite in-band ties, all states), `end_ties`,
    `labels` (the label indices with such a tie at their label state on some aligned row) and `separates`: per
    mutant of MUTANTS the number of aligned rows whose alignment it changes."""
    out = dict(ties=0, end_ties=0, labels=set(), separates={k: 0 for k in MUTANTS}, aligned=0)
    for b in range(x.shape[1]):
        fr = min(max(int(sl[b]), 0), x.shape[0])
        xb = np.ascontiguousarray(x[:fr, b])
        norm = oracle.row_norm(xb) if fr else np.zeros((0,), x.dtype)
        for i in range(n.shape[1]):
            if not 0 <= n[b, i] <= y.shape[2]:
                continue
            row, info = [int(c) for c in y[b, i, :n[b, i]]], {}
            ali, logp, ties = align_variant(xb, norm, row, fr, blank, maps=info)
            if not logp > -np.inf:
                continue
            band = in_band(ties, fr)
            out["aligned"] += 1
            out["ties"] += int(band.sum())
            out["end_ties"] += info["end_tie"]
            out["labels"].update(int(s) // 2 for s in np.nonzero(band[:, 1::2].any(axis=0))[0] * 2 + 1)
            for k, strict in MUTANTS.items():
                out["separates"][k] += align_variant(xb, norm, row, fr, blank, strict)[0] != ali
    return out
