"""Shared by the path-scores tests: the definition of include/ctcext.h, "Path
scores", in plain numpy (np.longdouble: the reference; the compute dtype with
libm's logaddexp: the tolerance's yardstick), and the GPU cases, built once."""
import functools

import numpy as np

import oracle
import range_inputs
import skip_util
import token_scores_util as tsu
from token_times_util import family

# E: the largest |plain recursion in the compute dtype - longdouble reference|
# over the finite expected values of the issue's cases, measured on the CPU
# (1.1044e-4 on lanes-300; 9.658e-16).  The longer rows added here have an E of
# their own (E_OWN: 1.1333e-3; 1.5737e-13), so they widen no other case's
# bound.  The kernels pass within 4 E (the hardware exp / log against libm,
# another grouping of the three-way LSE).
E = {np.float32: 1.105e-4, np.float64: 1.0e-15}
E_OWN = {"lanes-1200": 1.14e-3, "float64-lanes-140": 1.6e-13, "lds-float64-140": 1.6e-13}


def tol(name, dtype):
    return 4 * E_OWN.get(name, E[np.dtype(dtype).type])


RENORM = 16   # frames between the float32 kernels' renormalisations (kPathsRenorm)


def path_score(x, norm, y, frames, blank, ftype=np.longdouble):
    """The normative definition for one row: x [T, C] and norm [frames] of the
    compute dtype (lp is their one rounded difference), the recursion in ftype."""
    m, C, ninf = len(y), x.shape[1], ftype(-np.inf)
    if any(c < 0 or c >= C for c in y):
        return ftype(np.nan)
    if frames == 0:
        return ftype(0) if m == 0 else ninf
    z = np.full(2 * m + 1, blank, np.int64)
    z[1::2] = y
    skip = np.zeros(z.size, bool)
    skip[3::2] = z[3::2] != z[1:-2:2]
    with np.errstate(invalid="ignore", over="ignore"):
        lp = (x[:frames][:, z] - np.asarray(norm)[:frames, None]).astype(ftype)
        a = np.full(z.size, ninf)
        a[:2] = lp[0, :2]
        for f in range(1, frames):
            one = np.concatenate(([ninf], a[:-1]))
            two = np.where(skip, np.concatenate(([ninf, ninf], a[:-2])), ninf)
            a = np.logaddexp(np.logaddexp(a, one), two) + lp[f]
        return np.logaddexp(a[-1], a[-2]) if m else a[0]


def scores(x, sl, rows, P, blank=0, ftype=np.longdouble, frames_of=None):
    """[B, P] of ftype for rows[b][p] over x [T, B, C]; frames_of(b): a subset of the item's frames instead of all."""
    out = np.full((x.shape[1], P), np.nan, ftype)
    for b in range(x.shape[1]):
        xb = x[:max(int(sl[b]), 0), b] if frames_of is None else x[frames_of(b), b]
        norm = oracle.row_norm(np.ascontiguousarray(xb)) if len(xb) else np.zeros((0,), x.dtype)
        for p, y in enumerate(rows[b][:P]):
            out[b, p] = path_score(xb, norm, y, len(xb), blank, ftype)
    return out


def _gauss(T, sl, C=29, W=16, P=3, scale=1.0, kind="gaussian", dtype=np.float32, merge=False):
    x = (family(np.random.default_rng(1000 + T + C), kind, T, len(sl), C) * scale).astype(dtype)
    return dict(x=x, sl=np.array(sl, np.int32), W=W, P=P, merge=merge)


def _family(kind, shape, merge, dtype="float32"):
    x, sl, kw, _ = tsu.family_case(kind, shape, merge, dtype)
    return dict(x=np.array(x), sl=sl, W=shape[3], P=shape[4], merge=merge)


def _range(kind):
    x = range_inputs.family(range_inputs.rng_for("path scores " + kind), kind, 12, 3, 5, np.float32)
    return dict(x=x, sl=np.array([12, 11, 7], np.int32), W=8, P=2, merge=True)


def _tight():
    """"aa" in three frames (one alignment: a, blank, a); an item of one frame with three rows."""
    x = np.full((3, 2, 4), -4.0, np.float32)
    x[0, 0, 1] = x[1, 0, 0] = x[2, 0, 1] = 3.0
    x[0, 1] = [0.5, 1.5, 1.0, -1.0]
    return dict(x=x, sl=np.array([3, 1], np.int32), W=4, P=3, merge=False)


def _skip():
    x, sl, kw, e, times, sc = tsu.skip_case()
    return dict(x=np.array(x), sl=sl, W=tsu.SKIP_SHAPE[3], P=tsu.SKIP_SHAPE[4], merge=True, skip=skip_util.THR, rows=e.dec,
                kmaps=e.kmaps)


BUILDERS = {"%s-%s-%s" % (k, "x".join(map(str, s)), "merge" if m else "plain"): functools.partial(_family, k, s, m)
            for k, s, m in tsu.FAMILY_CASES}
BUILDERS.update({
    "lanes-70": lambda: _gauss(70, [70, 67, 65]),
    "lanes-140": lambda: _gauss(140, [140, 137, 135, 60]),
    "lanes-300": lambda: _gauss(300, [300, 297, 270, 150]),
    "lanes-1200": lambda: _gauss(1200, [1200, 1100], P=2),
    "lds-lanes-140": lambda: dict(_gauss(140, [140, 137, 135, 60]), env={"CTCEXT_PATHS_LDS": "1"}),   # two chunks of slots
    "float64-lanes-140": lambda: _gauss(140, [140, 137, 135, 60], dtype=np.float64),
    "lds-float64-140": lambda: dict(_gauss(140, [140, 137, 135, 60], dtype=np.float64), env={"CTCEXT_PATHS_LDS": "1"}),
    "lds-forced": lambda: dict(_family("sticky", (40, 4, 29, 16, 3), False), env={"CTCEXT_PATHS_LDS": "1"}),
    "renorm-300x20": lambda: _gauss(300, [300, 297, 270, 150], scale=20.0),
    "renorm-17": lambda: _gauss(RENORM + 1, [RENORM + 1, RENORM, RENORM - 1], C=5, W=8),
    "tight": _tight,
    "range-edges": lambda: _range("edges"),
    "range-huge": lambda: _range("huge"),
    "float64": lambda: _family("gaussian", (12, 6, 5, 8, 3), True, "float64"),
    "bf16-slice": lambda: dict(_gauss(24, [24, 21, 12], kind="sticky", merge=True), half="bfloat16"),
    "f16-slice": lambda: dict(_gauss(24, [24, 21, 12], kind="sticky", merge=True), half="float16"),
    "C80": lambda: _gauss(20, [20, 17], C=80, W=8, P=2, kind="peaky", merge=True),
    "C1100": lambda: _gauss(8, [8, 5], C=1100, W=8, P=2),
    "skip": _skip,
})


@functools.lru_cache(maxsize=None)
def case(name):
    """One GPU case: inputs, rows, `want` (longdouble) and `plain` (the compute dtype)."""
    c = BUILDERS[name]()
    if c.get("half"):   # values the two-byte format holds exactly
        import torch
        c["x"] = torch.as_tensor(c["x"]).to(getattr(torch, c["half"])).float().numpy()
    x, sl, P = c["x"], c["sl"], c["P"]
    if "rows" not in c:
        c["rows"] = oracle.raw_decode(x, sl, c["W"], P, c["merge"], 0, -1)[0]
    c["want"] = scores(x, sl, c["rows"], P)
    c["plain"] = scores(x, sl, c["rows"], P, ftype=x.dtype.type)
    x.setflags(write=False)
    return c
