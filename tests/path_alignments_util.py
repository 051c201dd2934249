"""Shared by the path-alignments tests: the definition of include/ctcext.h,
"Path alignments", restated in plain numpy in the compute dtype (and, for the
optimum, in np.longdouble), and the GPU cases with their expected tensors,
built once from path_scores_util's inputs and rows."""
import functools

import numpy as np

import ctcext_amd
import oracle
import path_scores_util as psu
from token_times_util import family

# E: the largest |logp in the compute dtype - optimum of the same recursion in
# longdouble| over the GPU cases below, measured on the CPU (float32 8.345e-5;
# float64 1.008e-13); the 1200-frame rows have a figure of their own (2.869e-3:
# nothing is renormalised, so the error grows with the magnitude of logp).
# test_cpu_path_alignments holds each constant to its measured figure from both
# sides.
E = {np.float32: 8.4e-5, np.float64: 1.02e-13}
E_1200 = 2.9e-3


def bound(name, dtype):
    return E_1200 if "1200" in name else E[np.dtype(dtype).type]


def align(x, norm, y, frames, blank, blank_label=-1, ftype=None):
    """The normative definition for one row: (alignment, logp).  x [T, C] and norm [frames] of the compute dtype
    (lp is their one rounded difference); the recursion in ftype (None: the compute dtype)."""
    ft = ftype or x.dtype.type
    m, C, ninf = len(y), x.shape[1], ft(-np.inf)
    if any(c < 0 or c >= C for c in y):
        return [], ft(np.nan)
    if frames == 0:
        return [], (ft(0) if m == 0 else ninf)
    z = np.full(2 * m + 1, blank, np.int64)
    z[1::2] = y
    skip = np.zeros(z.size, bool)
    skip[3::2] = z[3::2] != z[1:-2:2]
    dec = np.zeros((frames, z.size), np.int8)
    with np.errstate(invalid="ignore", over="ignore"):
        lp = (x[:frames][:, z] - np.asarray(norm)[:frames, None]).astype(ft)
        v = np.full(z.size, ninf)
        v[:2] = lp[0, :2]
        for f in range(1, frames):
            one, two = np.concatenate(([ninf], v))[:-1], np.concatenate(([ninf, ninf], v))[:-2]
            best = v.copy()
            d1 = one > best                      # strictly greater; a comparison with a NaN is false
            best[d1] = one[d1]
            d2 = skip & (two > best)
            best[d2] = two[d2]
            dec[f] = np.where(d2, 2, d1)
            v = best + lp[f]
    s = z.size - 1 - (1 if m and v[-2] > v[-1] else 0)
    logp = v[s]
    if not logp > ninf:                          # -inf or NaN: unaligned
        return [], logp
    out = []
    for f in range(frames - 1, -1, -1):
        out.append(int(z[s]) if s % 2 else blank_label)
        s -= int(dec[f][s])
    return out[::-1], logp


def expected(x, sl, rows, P, blank=0, blank_label=-1, pad=-1):
    """The PathAlignments of rows[b][p] over x [T, B, C] as numpy arrays."""
    T, B, _ = x.shape
    ft = x.dtype.type
    ali, alen = np.full((B, P, T), pad, np.int64), np.zeros((B, P), np.int32)
    logp = np.full((B, P), np.nan, ft)
    start, end, trail = np.full((B, P, T), -1, np.int32), np.full((B, P, T), -1, np.int32), np.zeros((B, P), np.int32)
    lsum, lmin = np.full((B, P, T), np.nan, ft), np.full((B, P, T), np.nan, ft)
    for b in range(B):
        n = max(int(sl[b]), 0)
        xb = np.ascontiguousarray(x[:n, b])
        norm = oracle.row_norm(xb) if n else np.zeros((0,), ft)
        for p, y in enumerate(rows[b][:P]):
            a, logp[b, p] = align(xb, norm, y, n, blank, blank_label)
            if not logp[b, p] > -np.inf:
                continue
            ali[b, p, :n], alen[b, p] = a, n
            s, e, trail[b, p] = ctcext_amd.token_times_row(y, a, n, blank_label, merge_repeated=False)
            start[b, p, :len(y)], end[b, p, :len(y)] = s, e
            if len(y):
                lsum[b, p, :len(y)], lmin[b, p, :len(y)] = ctcext_amd.token_scores_row(xb, norm, a, n, s, e, blank,
                                                                                       blank_label)
    return dict(alignment=ali, alignment_lengths=alen, logp=logp, start=start, end=end, trailing_blank=trail,
                logp_sum=lsum, logp_min=lmin)


def _frames():
    """Items of 1, 63, 64 and 65 frames: the walk back's block stores and its prefetch run-in."""
    x = family(np.random.default_rng(65), "sticky", 65, 4, 6)
    return dict(x=x, sl=np.array([1, 63, 64, 65], np.int32), W=8, P=2, merge=True)


OWN = {"frames-1-63-64-65": _frames,
       "lds-lanes-1200": lambda: dict(psu.case("lanes-1200"), env={"CTCEXT_PATHS_LDS": "1"})}   # crosses the ten-chunk word
CASES = [n for n in psu.BUILDERS if n.split("-")[0] in ("gaussian", "peaky", "sticky", "neg_inf")] + [
    "tight", "frames-1-63-64-65", "lanes-70", "lanes-140", "lanes-300", "lanes-1200", "lds-lanes-140", "lds-lanes-1200",
    "float64", "float64-lanes-140", "bf16-slice", "f16-slice", "C1100", "range-edges", "range-huge", "skip"]


@functools.lru_cache(maxsize=None)
def case(name):
    """One GPU case: path_scores_util's inputs and rows (or the two above) with `want`, the expected tensors."""
    if name in OWN:
        c = dict(OWN[name]())
        if "rows" not in c:
            c["rows"] = oracle.raw_decode(c["x"], c["sl"], c["W"], c["P"], c["merge"], 0, -1)[0]
    else:
        c = dict(psu.case(name))
    c["want"] = expected(c["x"], c["sl"], c["rows"], c["P"])
    return c
