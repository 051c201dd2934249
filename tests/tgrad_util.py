"""Shared by the target-gradients tests: the definition of include/ctcext.h,
"Target gradients", in plain numpy at a given float type (np.longdouble: the
reference; the compute dtype: the tolerance's yardstick), and the slab builder."""
import numpy as np

import oracle


def target_grad(x, norm, y, frames, blank, ftype=np.longdouble):
    """(logp, g [frames, C]) of ftype for one target: x [T, C] and norm [frames] of the compute dtype (lp is their one
    rounded difference); a row without a finite score has g == 0."""
    y, C, ninf = [int(c) for c in y], x.shape[1], ftype(-np.inf)
    m, g = len(y), np.zeros((frames, C), ftype)
    if any(c < 0 or c >= C for c in y):
        return ftype(np.nan), g
    if frames == 0:
        return (ftype(0) if m == 0 else ninf), g
    z = np.full(2 * m + 1, blank, np.int64)
    z[1::2] = y
    skip = np.zeros(z.size + 2, bool)   # skip[s], and False for the two states behind the last
    skip[3:-2:2] = z[3::2] != z[1:-2:2]
    with np.errstate(invalid="ignore", over="ignore"):
        lpa = (x[:frames] - np.asarray(norm)[:frames, None]).astype(ftype)
        lp = lpa[:, z]
        a, bt = np.full(lp.shape, ninf), np.full(lp.shape, ninf)
        a[0, :2] = lp[0, :2]
        for f in range(1, frames):
            one = np.concatenate(([ninf], a[f - 1]))[:-1]
            two = np.where(skip[:-2], np.concatenate(([ninf, ninf], a[f - 1]))[:-2], ninf)
            a[f] = np.logaddexp(np.logaddexp(a[f - 1], one), two) + lp[f]
        logp = np.logaddexp(a[-1, -1], a[-1, -2]) if m else a[-1, 0]
        if not np.isfinite(logp):
            return logp, g
        bt[-1, -2:] = lp[-1, -2:]
        for f in range(frames - 2, -1, -1):
            one = np.concatenate((bt[f + 1], [ninf]))[1:]
            two = np.where(skip[2:], np.concatenate((bt[f + 1], [ninf, ninf]))[2:], ninf)
            bt[f] = np.logaddexp(np.logaddexp(bt[f + 1], one), two) + lp[f]
        ab = a + bt
        occ = np.where(ab > ninf, np.exp(ab - lp - logp), 0)
        for s, c in enumerate(z):
            g[:, c] += occ[:, s]
        return logp, g - np.exp(lpa)


def expected(x, sl, y, n, w, blank=0, ftype=np.longdouble):
    """(scores [B, N], slab [T, B, C]) of ftype for targets y [B, N, L], lengths n [B, N] and weights w [B, N] (None:
    ones) over x [T, B, C]; a bad length: NaN; rows without a finite score add nothing."""
    scores, slab = np.full(n.shape, np.nan, ftype), np.zeros(x.shape, ftype)
    for b in range(x.shape[1]):
        xb = np.ascontiguousarray(x[:max(int(sl[b]), 0), b])
        norm = oracle.row_norm(xb) if len(xb) else np.zeros((0,), x.dtype)
        for i in range(n.shape[1]):
            if 0 <= n[b, i] <= y.shape[2]:
                scores[b, i], g = target_grad(xb, norm, y[b, i, :n[b, i]], len(xb), blank, ftype)
                if np.isfinite(scores[b, i]):
                    slab[:len(xb), b] += g if w is None else ftype(w[b, i]) * g
    return scores, slab
