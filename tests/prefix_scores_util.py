"""Shared by the prefix-scores tests: the definition of include/ctcext.h,
"Prefix scores", in plain numpy at a given float type.  It does not restate the
forward recursion: with S_f = path_scores_util.path_score over the first f + 1
frames (which is LSE(bl_f, nb_f)), bl_f = S_{f-1} + lp[f][blank]."""
import numpy as np

import oracle
import path_scores_util as psu


def prefix_scores(x, norm, g, frames, blank, ftype=np.longdouble):
    """ext [C] of ftype for one prefix: x [T, C] and norm [frames] of the compute dtype."""
    g, C, ninf = [int(c) for c in g], x.shape[1], ftype(-np.inf)
    m = len(g)
    if any(c < 0 or c >= C for c in g):
        return np.full(C, np.nan, ftype)
    ext = np.full(C, ninf)
    if frames == 0:
        if m == 0:
            ext[blank] = 0
        return ext
    with np.errstate(invalid="ignore", over="ignore"):
        lp = (x[:frames] - np.asarray(norm)[:frames, None]).astype(ftype)
        S = np.array([psu.path_score(x, norm, g, f + 1, blank, ftype) for f in range(frames)], ftype)
        phi = np.repeat(S[:, None], C, 1)
        if m:   # the class equal to the last label extends the blank tail only
            phi[:, g[-1]] = np.concatenate(([ninf], S[:-1] + lp[1:, blank]))
        first = lp[:1] if m == 0 else np.full((1, C), ninf)
        ext = np.logaddexp.reduce(np.concatenate((first, phi[:-1] + lp[1:])), axis=0)
    ext[blank] = S[-1]
    return ext


def expected(x, sl, y, n, ftype=np.longdouble, blank=0):
    """[B, N, C] of ftype for prefixes y [B, N, L], lengths n [B, N] over x [T, B, C]; a bad length: NaN."""
    out = np.full(n.shape + (x.shape[2],), np.nan, ftype)
    for b in range(x.shape[1]):
        xb = np.ascontiguousarray(x[:max(int(sl[b]), 0), b])
        norm = oracle.row_norm(xb) if len(xb) else np.zeros((0,), x.dtype)
        for i in range(n.shape[1]):
            if 0 <= n[b, i] <= y.shape[2]:
                out[b, i] = prefix_scores(xb, norm, y[b, i, :n[b, i]], len(xb), blank, ftype)
    return out
