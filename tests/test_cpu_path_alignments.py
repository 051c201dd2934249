"""Path alignments without a GPU: ctcext_path_alignment_row against the numpy
restatement of the definition, bit for bit, and both against the optimum of
the same recursion in np.longdouble."""
import numpy as np
import pytest

import ctcext_amd
import oracle
import path_alignments_util as u


def _same(x, norm, y, frames, what):
    """path_alignment_row == the restatement: alignment, length, and the bits of logp."""
    x = np.asarray(x)
    a, logp = u.align(x, np.asarray(norm, x.dtype), list(y), frames, 0)
    ga, glogp = ctcext_amd.path_alignment_row(x, norm, y, frames, 0)
    assert ga.tolist() == a, what
    assert np.array([glogp]).view(np.uint8).tolist() == np.array([logp]).view(np.uint8).tolist(), (what, glogp, logp)
    return a, logp


@pytest.mark.parametrize("name", [n for n in u.CASES if not n.startswith(("lanes", "lds"))])
def test_row_equals_the_restatement_on_the_cases(name):
    c = u.case(name)
    x, sl = c["x"], c["sl"]
    for b in range(x.shape[1]):
        n = max(int(sl[b]), 0)
        xb = np.ascontiguousarray(x[:n, b])
        norm = oracle.row_norm(xb) if n else np.zeros((0,), x.dtype)
        for p, y in enumerate(c["rows"][b][:c["P"]]):
            a, logp = _same(xb, norm, y, n, (name, b, p))
            assert len(a) == c["want"]["alignment_lengths"][b, p]


ROWS = {   # x [frames][3] with norm 0, blank 0: (x, y, frames, alignment or None, logp or None)
    "aa in three frames": ([[-4, 3, -4], [3, -4, -4], [-4, 3, -4]], [1, 1], 3, [1, -1, 1], 9.0),
    "m = 0": ([[-1, 0, 0], [-2, 0, 0]], [], 2, [-1, -1], -3.0),
    "frames = 0, m = 0": (np.zeros((0, 3)), [], 0, [], 0.0),
    "frames = 0, m = 1": (np.zeros((0, 3)), [1], 0, [], -np.inf),
    "infeasible": ([[0, 0, 0], [0, 0, 0]], [1, 1], 2, [], -np.inf),
    "label outside the classes": ([[0, 0, 0]], [3], 1, [], np.nan),
    # ties keep the lower decision: stay (0) over s - 1 (1) over s - 2 (2)
    "tie between 0 and 1": ([[-1, -1, -9], [-2, -1, -9]], [1], 2, [1, 1], -2.0),
    "tie between 1 and 2": ([[-9, -1, -9], [-1, -1, -9], [-9, -9, -1]], [1, 2], 3, [1, -1, 2], -3.0),
    "tie between 0 and 2": ([[-9, -1, -9], [-9, -1, -1], [-9, -9, -1]], [1, 2], 3, [1, 2, 2], -3.0),
    "tie at the end state": ([[-9, -1, -9], [-1, -1, -9]], [1], 2, [1, -1], -2.0),
}


@pytest.mark.parametrize("name", list(ROWS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_row_equals_the_restatement_on_hand_written_rows(name, dtype):
    x, y, frames, ali, logp = ROWS[name]
    x = np.asarray(x, dtype).reshape(frames, 3)
    a, got = _same(x, np.zeros((frames,), dtype), y, frames, name)
    assert a == ali and (got == logp or (np.isnan(got) and np.isnan(logp))), (name, a, got)


def test_optimum_in_long_double_and_the_measured_e():
    """path_alignment_row against the optimum of the same recursion in long double, on every GPU case: its
    alignment's own lp, re-summed in long double, is within 2 E of that optimum; E is the measured
    |path_alignment_row's logp - long-double optimum|."""
    worst = {np.float32: 0.0, np.float64: 0.0, "1200": 0.0}
    L = np.longdouble
    for name in u.CASES:
        c = u.case(name)
        x, sl = c["x"], c["sl"]
        key = "1200" if "1200" in name else x.dtype.type
        for b in range(x.shape[1]):
            n = int(sl[b])
            xb = np.ascontiguousarray(x[:n, b])
            norm = oracle.row_norm(xb)
            for p, y in enumerate(c["rows"][b][:c["P"]]):
                a, logp = ctcext_amd.path_alignment_row(xb, norm, y, n, 0)
                best = u.align(xb, norm, y, n, 0, ftype=L)[1]
                if not np.isfinite(best):
                    assert not logp > -np.inf and len(a) == 0, (name, b, p)
                    continue
                assert len(a) == n, (name, b, p)
                worst[key] = max(worst[key], float(abs(L(logp) - best)))
                own = (xb[np.arange(n), np.where(a < 0, 0, a)] - norm).astype(L).sum()
                assert own <= best + 1e-15 * abs(best) and best - own <= 2 * u.bound(name, x.dtype), (name, b, p, own, best)
    print(worst)
    for key, e in ((np.float32, u.E[np.float32]), (np.float64, u.E[np.float64]), ("1200", u.E_1200)):
        assert 0.9 * e < worst[key] <= e, (key, worst[key], e)   # the constant is the measured figure, rounded up
