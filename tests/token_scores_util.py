"""Shared by the token-scores tests: the definition restated in Python
(include/ctcext.h, "Token scores") in numpy scalars of the compute dtype, and
the expected tensors from the oracle's rows, the token times of those rows and
the oracle's normaliser of the item's rows."""
import functools

import numpy as np

import oracle
import skip_util
from token_times_util import NEG_INF_SEEDS, expected_from_rows, family
from token_times_util import expected as expected_times

nan = float("nan")


def token_scores(x, norm, ali, frames, start, end, blank_index, blank_label, ftype=np.float32):
    """The normative definition, verbatim; ftype is the compute dtype, norm
    holds numpy scalars of it, and every float below is one."""
    base, m = frames - len(ali), len(start)
    lsum, lmin = [nan] * m, [nan] * m
    for i in range(m):
        if start[i] < 0: continue                      # untimed token: NaN
        for f in range(start[i], end[i] + 1):          # ascending frames, every frame of the span
            v = ali[f - base]
            c = blank_index if v == blank_label else v
            lp = ftype(x[f][c]) - norm[f]              # one rounded subtraction in ftype
            if f == start[i]: acc = mn = lp
            else:
                acc = ftype(acc + lp)                  # one rounded add, this order, no fma
                if lp < mn: mn = lp                    # a NaN never replaces, a leading NaN stays
        lsum[i], lmin[i] = acc, mn
    return lsum, lmin


def item_norm(x, b, frames):
    """The oracle's normaliser of item b's first `frames` rows of x [T, B, C]."""
    if frames <= 0:
        return np.zeros((0,), x.dtype)
    return oracle.row_norm(np.ascontiguousarray(x[:frames, b]))


def expected_from_rows_and_times(x, ali, frames, start, end, dec_len, B, P, width, blank_index, blank_label):
    """TokenScores as numpy (logp_sum, logp_min), [B, P, width] of x's dtype,
    NaN outside the row's decoded length, from rows ali[b][p] (lists), their
    times start / end [B, P, width] and x [T, B, C] of the compute dtype."""
    ftype = x.dtype.type
    lsum = np.full((B, P, width), np.nan, x.dtype)
    lmin = np.full((B, P, width), np.nan, x.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            n = int(frames[b])
            norm = item_norm(x, b, n)
            xb = x[:, b]
            for p in range(P):
                m = int(dec_len[b][p])
                s, mn = token_scores(xb, norm, ali[b][p], n, start[b, p, :m].tolist(), end[b, p, :m].tolist(),
                                     blank_index, blank_label, ftype)
                lsum[b, p, :m] = s
                lmin[b, p, :m] = mn
    return lsum, lmin


def expected(x, sl, W, P, width, **kw):
    """The oracle's rows of x / sl (x of the compute dtype), their token times
    and their scores: (dec, ali, (start, end, trailing_blank), (logp_sum, logp_min))."""
    sl = np.asarray(sl, np.int32)
    dec, ali, times = expected_times(x, sl, W, P, width, **kw)
    B = x.shape[1]
    dl = [[len(dec[b][p]) for p in range(P)] for b in range(B)]
    scores = expected_from_rows_and_times(x, ali, np.maximum(sl, 0), times[0], times[1], dl, B, P, width,
                                          kw.get("blank_index", 0), kw.get("blank_label", -1))
    return dec, ali, times, scores


def expected_skip(x, e, sl, P, width, **kw):
    """The same after a skipping decode, on the original time axis: e is
    skip_util.expected's (its ali rows are the expanded ones), x the caller's
    rows, the normaliser theirs."""
    sl = np.maximum(np.asarray(sl, np.int32), 0)
    B = x.shape[1]
    times = expected_from_rows(e.dec, e.ali, sl, B, P, width, kw.get("blank_label", -1),
                               bool(kw.get("merge_repeated", False)))
    dl = [[len(e.dec[b][p]) for p in range(P)] for b in range(B)]
    scores = expected_from_rows_and_times(x, e.ali, sl, times[0], times[1], dl, B, P, width,
                                          kw.get("blank_index", 0), kw.get("blank_label", -1))
    return times, scores


def descending_sum(x, norm, ali, frames, start, end, blank_index, blank_label, ftype=np.float32):
    """One token's terms added from the last frame to the first: what a kernel
    that adds in another order would return."""
    base = frames - len(ali)
    acc = None
    for f in range(end, start - 1, -1):
        v = ali[f - base]
        c = blank_index if v == blank_label else v
        lp = ftype(x[f][c]) - norm[f]
        acc = lp if acc is None else ftype(acc + lp)
    return acc


# ---- the input cases of the GPU tests, built once per process (the CPU tests
# assert on them the properties the GPU tests rely on)

# (T, B, C, W, P)
SHAPES = [(1, 2, 3, 2, 1), (12, 6, 5, 8, 3), (40, 4, 29, 16, 3), (60, 3, 29, 128, 3)]
FAMILY_CASES = ([(k, s, m) for k in ("gaussian", "peaky", "sticky") for s in SHAPES for m in (False, True)]
                + [("neg_inf", s, True) for s in sorted(NEG_INF_SEEDS)])
TILED = [(700, 3, 5, 8, 3), (257, 2, 4, 4, 4)]


def lengths(T, B):
    return np.array([T] + [max(T - 1 - 2 * b, 0) for b in range(1, B)], np.int32)


@functools.lru_cache(maxsize=None)
def family_case(kind, shape, merge, dtype="float32"):
    T, B, C, W, P = shape
    rng = np.random.default_rng(NEG_INF_SEEDS[shape] if kind == "neg_inf" else sum(kind.encode()) + T)
    x = family(rng, kind, T, B, C, np.dtype(dtype))
    x.setflags(write=False)
    sl = lengths(T, B)
    kw = dict(merge_repeated=merge, blank_index=0, blank_label=-1)
    return x, sl, kw, expected(x, sl, W, P, T, **kw)


def nan_cells_inside_decoded_length(dec, scores):
    """Cells of logp_sum below their row's decoded length that are NaN."""
    return sum(int(np.isnan(scores[0][b, p, :len(row)]).sum()) for b, rows in enumerate(dec) for p, row in enumerate(rows))


SOFT_SEED = 3   # (picked on the CPU: test_cpu_token_scores asserts what it was picked for)


@functools.lru_cache(maxsize=None)
def tiled_case(shape, soft=False):
    """Rows of several kernel tiles, merge on; an item without frames has fewer
    leaves than top_paths, a status bit, and NaN rows.

    The sticky family's held class stands 5 above unit noise, so x and norm lie
    in one binade around 5, every x - norm is a multiple of 2^-22 below 1 in
    magnitude, and a token's float32 sum is exact in any order.  `soft` scales
    that family by 0.37: the terms then have mantissas of their own and sums of
    several units, every addition rounds, and the order shows."""
    T, B, C, W, P = shape
    x = family(np.random.default_rng(SOFT_SEED if soft else 17 if T == 700 else T), "sticky", T, B, C)
    if soft:
        x = (x * np.float32(0.37)).astype(np.float32)
    x.setflags(write=False)
    sl = np.array([T, T - 177, 0] if B == 3 else [T, T - 1], np.int32)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    live = [b for b in range(B) if sl[b] > 0]
    dec, ali, times_live, scores_live = expected(np.ascontiguousarray(x[:, live]), sl[live], W, P, T, **kw)
    scores = [np.full((B,) + w.shape[1:], np.nan, w.dtype) for w in scores_live]
    for w, wl in zip(scores, scores_live):
        w[live] = wl
    return x, sl, kw, live, dec, ali, times_live, scores


def tile_properties(case, tile):
    """(scored spans that cross a multiple of `tile`, tokens among them whose
    float32 sum differs from the same terms added in descending order)."""
    x, sl, kw, live, dec, ali, (start, end, _), scores = case
    crossing = differ = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i, b in enumerate(live):
            n = int(sl[b])
            norm = item_norm(x, b, n)
            for p in range(len(dec[i])):
                for j in range(len(dec[i][p])):
                    s, e = int(start[i, p, j]), int(end[i, p, j])
                    if s < 0 or s // tile == e // tile:
                        continue
                    crossing += 1
                    down = descending_sum(x[:, b], norm, ali[i][p], n, s, e, 0, -1, x.dtype.type)
                    up = scores[0][b, p, j]
                    differ += bool(np.isfinite(up) and up != down)
    return crossing, differ


SKIP_SHAPE = (20, 2, 4, 8, 2)


@functools.lru_cache(maxsize=None)
def skip_case():
    """Hand-built logits, merge on: in item 0 label 1 holds frames 0-1 and 6-7
    with the blank far above log 0.9 on frames 2-5 between them, so the merged
    token's span holds frames the plan drops."""
    T, B, C, W, P = SKIP_SHAPE
    x = (np.random.default_rng(20).standard_normal((T, B, C)) * 0.1).astype(np.float32)
    plan0 = [1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 2, 2, 2, 0, 0, 0, 3, 3, 0, 0]
    plan1 = [0, 0, 0, 2, 2, 0, 0, 0, 0, 2, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    for b, plan in enumerate((plan0, plan1)):
        for t, c in enumerate(plan):
            x[t, b, c] += 9.0
    x.setflags(write=False)
    sl = np.array([T, T - 3], np.int32)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    e = skip_util.expected(x, sl, W, P, skip_util.THR, **kw)
    times, scores = expected_skip(x, e, sl, P, T, **kw)
    return x, sl, kw, e, times, scores


def skip_properties(case):
    """(scored spans that hold a dropped frame, items with kept < frames, runs
    of >= 3 frames above log 0.9 between two runs of one label in item 0)."""
    x, sl, kw, e, (start, end, _), scores = case
    spans = 0
    for b in range(x.shape[1]):
        kept = set(e.kmaps[b])
        for p in range(len(e.dec[b])):
            for j in range(len(e.dec[b][p])):
                s, en = int(start[b, p, j]), int(end[b, p, j])
                if s >= 0 and not np.isnan(scores[0][b, p, j]) and any(f not in kept for f in range(s, en + 1)):
                    spans += 1
    fewer = sum(int(e.kept[b]) < int(sl[b]) for b in range(x.shape[1]))
    lp = skip_util.logp_blank(x)
    return spans, fewer, int((lp[2:6, 0] > skip_util.THR).sum())
