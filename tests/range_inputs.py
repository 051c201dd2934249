"""Logits over the whole float range, shared by the GPU tests.

The other tests draw N(0,1) logits times a small scale, so every softmax term
x_j - max they hand a kernel lies in about [-30, 0] or is -inf.  The families
here put terms where the normalisers, lse and the exact-skip bounds change
path: expf's subnormal-result band and its underflow bound, exp's
(double) |x| >= 512, subnormal results and underflow bound, sums so near 1
that log takes its near-1 branch or returns 0 outright, rows with one
dominant class (norm == max), logits near 1e6..3e7 whose differences cancel
on a coarse grid, finite logits whose difference overflows, subnormal
logits, and totals of exactly 0 to which lse adds log1pf of a subnormal expf.
`family` draws one, `census` counts on the host which of those
conditions an array meets (each test asserts the ones its family exists for:
a condition on the inputs, not a measurement of the code under test).

Values are built in float64 and cast last; every seed comes from
zlib.crc32 of a name (rng_for), never from hash()."""
import math
import zlib

import numpy as np

import oracle

FAMILIES = ("logsoftmax", "edges", "banded", "onehot", "offset", "huge", "subnormal", "peaked")   # banded: float32 only

# below BOUND the libm exp of the type returns 0; from BOUND up to LOGMIN (the
# log of the smallest normal number) its result is subnormal
BOUND = {np.dtype(np.float32): float.fromhex("-0x1.9fe368p6"),            # glibc_math.h kExpfUnder
         np.dtype(np.float64): float.fromhex("-0x1.74910d52d3051p9")}
LOGMIN = {np.dtype(np.float32): float(np.float32(math.log(2.0 ** -126))),
          np.dtype(np.float64): -1022 * math.log(2.0)}
# log's near-1 branch (glibc_math_f64.h): sums in [1 - 2^-4, 1 + 0x1.09p-4)
LOG_NEAR_ONE = (1.0 - 2.0 ** -4, 1.0 + float.fromhex("0x1.09p-4"))


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _neighbours(v, dtype):
    """v and its two nextafter neighbours on both sides, in dtype."""
    t = np.dtype(dtype).type
    out = [t(v)]
    for to in (t(-np.inf), t(np.inf)):
        w = t(v)
        for _ in range(2):
            w = np.nextafter(w, to)
            out.append(w)
    return [float(w) for w in out]


def _edge_values(dtype):
    dt = np.dtype(dtype)
    if dt == np.float32:
        vals = []
        for v in (BOUND[dt], LOGMIN[dt], -88.0):
            vals += _neighbours(v, np.float32)
        vals += [-95.5, -100.25, -103.0, -104.0, -150.0, -1e4, -1e30]
        vals += [-2.0 ** -29, -2.0 ** -30, -2.0 ** -54, -2.0 ** -60, -0.0, -1e-45]
        vals += [-17.0, -20.2, -37.5, -0.41422, -0.6931472]
    else:
        vals = []
        for v in (BOUND[dt], LOGMIN[dt], -512.0, -1024.0):
            vals += _neighbours(v, np.float64)
        vals += [-700.0, -720.5, -744.0, -746.0, -1e4, -1e300]
        vals += [-2.0 ** -53, -2.0 ** -54, -2.0 ** -55, -0.0, -5e-324]
        vals += [-17.0, -36.8, -88.0, -103.97, -0.0625, -0.03]
    return np.array(vals, np.float64)


def _edges(rng, T, B, C, dtype, banded):
    vals = _edge_values(dtype)
    x = rng.choice(vals, size=(T, B, C))
    if banded:
        # classes [0, C/2): only values at or above the bound (the
        # subnormal-result band included); [C/2, C): below it as well
        half = C // 2
        x[:, :, :half] = rng.choice(vals[vals >= BOUND[np.dtype(dtype)]], size=(T, B, half))
    hot = rng.integers(C, size=(T, B))
    np.put_along_axis(x, hot[:, :, None], 0.0, axis=2)          # the row's maximum: exactly 0
    shift = rng.choice(np.array([0.0, 0.0, 64.0, -128.0]), size=(T, B, 1))   # powers of two: most differences stay exact
    return x + shift


def family(rng, kind, T, B, C, dtype):
    """[T, B, C] logits of `dtype` (float32 or float64) of one family."""
    dt = np.dtype(dtype)
    assert dt in BOUND, dtype
    if kind == "logsoftmax":       # what a trained model's log_softmax hands over: [-400, 0] and below, sums near 1
        s = rng.choice(np.array([8.0, 30.0, 120.0] if dt == np.float32 else [8.0, 120.0, 900.0]), size=(T, B, 1))
        z = rng.standard_normal((T, B, C)) * s
        m = z.max(axis=2, keepdims=True)
        x = z - (m + np.log(np.exp(z - m).sum(axis=2, keepdims=True)))
    elif kind in ("edges", "banded"):
        assert kind == "edges" or dt == np.float32
        x = _edges(rng, T, B, C, dt, kind == "banded")
    elif kind == "onehot":         # one dominant class; totals on a 0.5 grid (ties), p == 0 for the best label
        x = np.full((T, B, C), -1000.0)
        np.put_along_axis(x, rng.integers(C, size=(T, B))[:, :, None], 0.0, axis=2)
        lower = rng.choice(np.array([0.5, 1.0, 1.5]), size=(T, B, C))
        x = x - np.where(rng.random((T, B, C)) < 0.3, lower, 0.0)
    elif kind == "offset":         # x - norm cancels where the float grid is 1/16 to 2
        x = rng.standard_normal((T, B, C)) * 2 + rng.choice(np.array([1e6, -1e6, 3e7]), size=(T, B, 1))
    elif kind == "huge":           # finite logits whose difference overflows; two classes at the maximum
        big = float(np.finfo(dt).max)
        x = rng.standard_normal((T, B, C)) * (1e37 if dt == np.float32 else 1e307)
        u = rng.random((T, B, C))
        x[u < 0.05] = big
        x[u > 0.95] = -big
    elif kind == "subnormal":
        x = rng.integers(-8, 8, size=(T, B, C)) * float(np.finfo(dt).smallest_subnormal)
    elif kind == "peaked":
        # 0 on one of three classes (so that a label repeats and the blank
        # wins frames), every other class where float expf's result is
        # subnormal: norm == max, the best path's total stays exactly 0, and
        # lse (float expf / log1pf for either type) adds log1pf(subnormal) to
        # it when alignments merge: log-probabilities that are subnormal, > 0
        f32 = np.dtype(np.float32)
        band = _edge_values(np.float32)
        band = band[(band >= BOUND[f32]) & (band < LOGMIN[f32])]
        x = rng.choice(band, size=(T, B, C))
        hot = rng.choice(np.array([0, 1, C // 2]), size=(T, B))
        np.put_along_axis(x, hot[:, :, None], 0.0, axis=2)
    else:
        raise ValueError(kind)
    out = x.astype(dt)
    assert np.isfinite(out).all(), kind
    return out


def census(x):
    """Counts, over the rows of x [..., C] (float32 or float64, no NaN), of the
    conditions the families exist for: with d = x - rowmax computed in x's type,
    sub (bound <= d < log(min normal): exp's result is subnormal), at_bound
    (d == bound), below (finite d < bound: exp's result is 0), overflowed
    (d == -inf from a finite x), and norm_is_max (rows whose normaliser,
    oracle.row_norm, equals their maximum)."""
    dt = x.dtype
    rows = np.ascontiguousarray(x.reshape(-1, x.shape[-1]))
    mx = rows.max(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        d = rows - mx[:, None]
    assert d.dtype == dt
    bound, logmin = dt.type(BOUND[dt]), dt.type(LOGMIN[dt])
    fin = np.isfinite(d)
    return {"rows": int(rows.shape[0]),
            "sub": int(((d >= bound) & (d < logmin)).sum()),
            "at_bound": int((d == bound).sum()),
            "below": int((fin & (d < bound)).sum()),
            "overflowed": int((np.isneginf(d) & np.isfinite(rows)).sum()),
            "norm_is_max": int((oracle.row_norm(rows) == mx).sum())}


def row_sums64(x):
    """sum_j exp(x_j - rowmax) of each row of a float64 x [..., C], added in
    class order as the normalisers do."""
    rows = x.reshape(-1, x.shape[-1]).astype(np.float64)
    with np.errstate(over="ignore"):
        e = np.exp(rows - rows.max(axis=1, keepdims=True))
    return np.cumsum(e, axis=1)[:, -1]


# what each family must make happen, as census keys that are >= 1 (onehot and
# peaked: norm_is_max on every row; banded: per half of the classes; see
# assert_census)
EXPECT = {"logsoftmax": ("below", "norm_is_max"), "edges": ("sub", "at_bound", "below"), "banded": (),
          "onehot": (), "offset": (), "huge": ("overflowed",), "subnormal": (), "peaked": ()}


def assert_census(kind, x, wide_rows=False):
    """The conditions family `kind` exists for hold on x; returns the census.
    wide_rows (C >= 1000): a log_softmax row of that many classes need not
    have norm == max, only `below` is required."""
    cs = census(x)
    for key in EXPECT[kind]:
        if wide_rows and kind == "logsoftmax" and key == "norm_is_max":
            continue
        assert cs[key] >= 1, (kind, x.shape, key, cs)
    if kind in ("onehot", "peaked"):
        assert cs["norm_is_max"] == cs["rows"], (kind, x.shape, cs)
    if kind == "peaked":   # every other class in float expf's subnormal band (lse is float for either type)
        f32 = np.dtype(np.float32)
        rows = x.reshape(-1, x.shape[-1])
        d = rows - rows.max(axis=1, keepdims=True)
        assert (((d >= BOUND[f32]) & (d < LOGMIN[f32])).sum(axis=1) == x.shape[-1] - 1).all(), (kind, x.shape)
    if kind == "banded":
        # per half of the classes, against the whole row's maximum
        half = x.shape[-1] // 2
        rows = x.reshape(-1, x.shape[-1])
        d = rows - rows.max(axis=1, keepdims=True)
        bound, logmin = x.dtype.type(BOUND[x.dtype]), x.dtype.type(LOGMIN[x.dtype])
        lo = {"sub": int(((d[:, :half] >= bound) & (d[:, :half] < logmin)).sum()),
              "below": int((d[:, :half] < bound).sum())}
        hi = {"below": int((d[:, half:] < bound).sum())}
        assert lo["sub"] >= 1 and lo["below"] == 0 and hi["below"] >= 1, (kind, x.shape, lo, hi)
    return cs
