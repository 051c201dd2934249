"""Bigram beam-scorer tables, shared by the oracle, reference and GPU tests.

A table is [C + 1, C] of the logits' dtype: entry [a + 1][b] is added to the
total a prefix ending in label a hands the child that appends b, row 0 is the
root's (ctc_oracle.cpp, expand_state; BigramBeamScorer::expand).  -inf forbids
the bigram.  `table` draws one of a kind:

  continuous   -abs(normal) * 2: what the suite fed every bigram kernel before
               this module; no two children ever have equal totals
  grid         entries from {0, -0.5, -1, -1.5}: with logits on the half grid
               (the `ties` kind) totals repeat, so the kernels' tie order runs
  forbidden    continuous with 30% of the entries -inf, one whole row after
               row 0 -inf (a label without a successor), one whole column -inf
               (a label never offered) and tab[l + 1][l] -inf for half of the
               labels (no immediate repeat: the child that repeats its
               parent's label is refused on the blank-separated route too)
  extreme      continuous with 5% of the entries -max and 5% -max / 2 of the
               dtype (sums that stay finite, reach -max or overflow to -inf),
               10% -tiny / 4 (subnormal) and 10% -0.0

and, for single semantic cases: zero (every entry 0: the base scorer's
results), root_forbidden (continuous, row 0 all -inf: nothing can leave the
root), chain (label l may only be followed by l + 1 mod C, the root by any
label) and grid_forbidden (grid with 30% -inf: what the run-time-W cells of
the kernel matrix add).

Past 5000 classes a table is gigabytes.  There only row 0 and every seventh
row after it are written (the rest stays the zero pages it was allocated as),
continuous entries are the sum of a row and a column term, and the kind
applies to those rows alone.

Values are drawn in the order below and nowhere else, so a (seed, kind, C,
dtype) names one table; `forbidden_pairs` checks decoded paths against one.
"""
import numpy as np

KINDS = ("continuous", "grid", "forbidden", "extreme")
SEMANTIC = ("zero", "root_forbidden", "chain", "grid_forbidden")
SPARSE_ABOVE = 5000     # classes past which only every SPARSE_STEP-th row is written
SPARSE_STEP = 7
GRID = (0.0, -0.5, -1.0, -1.5)


def _mask(rng, shape, frac):
    return rng.random(shape, dtype=np.float32) < np.float32(frac)


def _grid(rng, shape, dt):
    return (rng.integers(0, len(GRID), size=shape, dtype=np.int8) * dt.type(-0.5)).astype(dt)


def _apply(rng, kind, sub, rows, dt):
    """Turns the continuous rows `sub` (table rows `rows`, ascending, rows[0]
    == 0) into `kind`, in place."""
    R, C = sub.shape
    if kind in ("grid", "grid_forbidden"):
        sub[...] = _grid(rng, (R, C), dt)
        if kind == "grid_forbidden":
            sub[_mask(rng, (R, C), 0.3)] = -np.inf
    elif kind == "forbidden":
        sub[_mask(rng, (R, C), 0.3)] = -np.inf
        if R > 1:
            sub[1 + int(rng.integers(R - 1))] = -np.inf       # a label without a successor
        sub[:, int(rng.integers(C))] = -np.inf                # a label never offered
        labels = rows[1:] - 1                                 # row l + 1 is label l's
        half = rng.random(labels.shape[0]) < 0.5
        sub[1:][half, labels[half]] = -np.inf                 # no immediate repeat of these labels
    elif kind == "extreme":
        big, tiny = float(np.finfo(dt).max), float(np.finfo(dt).tiny)
        u = rng.random((R, C), dtype=np.float32)
        sub[u < 0.05] = -big
        sub[(u >= 0.05) & (u < 0.10)] = -big / 2
        sub[(u >= 0.10) & (u < 0.20)] = -tiny / 4
        sub[(u >= 0.20) & (u < 0.30)] = -0.0
    elif kind == "zero":
        sub[...] = 0
    elif kind == "root_forbidden":
        sub[0] = -np.inf
    elif kind == "chain":
        keep = np.zeros((R, C), bool)
        keep[0] = True
        keep[np.arange(1, R), rows[1:] % C] = True            # row l + 1: only column l + 1 mod C
        sub[~keep] = -np.inf
    else:
        assert kind == "continuous", kind


def table(rng, kind, C, dtype):
    """A [C + 1, C] table of `dtype` (float32 or float64) of one kind."""
    dt = np.dtype(dtype)
    assert dt in (np.dtype(np.float32), np.dtype(np.float64)), dtype
    assert kind in KINDS + SEMANTIC, kind
    if C <= SPARSE_ABOVE:
        tab = (-np.abs(rng.standard_normal((C + 1, C))) * 2).astype(dt)
        _apply(rng, kind, tab, np.arange(C + 1), dt)
        return tab
    tab = np.zeros((C + 1, C), dt)
    ra = np.abs(rng.standard_normal(((C + SPARSE_STEP) // SPARSE_STEP, 1))).astype(dt)
    rb = np.abs(rng.standard_normal((1, C))).astype(dt)
    if kind == "continuous":
        np.negative(ra + rb, out=tab[::SPARSE_STEP])
        return tab
    sub = -(ra + rb)
    _apply(rng, kind, sub, np.arange(0, C + 1, SPARSE_STEP), dt)
    tab[::SPARSE_STEP] = sub
    return tab


def forbidden_pairs(tab, paths):
    """The (a, b) steps of `paths` (label lists; a == -1 at a path's start)
    whose entry tab[a + 1][b] is -inf."""
    bad = []
    for path in paths:
        prev = -1
        for label in path:
            if np.isneginf(tab[prev + 1][label]):
                bad.append((prev, int(label)))
            prev = int(label)
    return bad
