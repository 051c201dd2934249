"""Path scores without a GPU: ctcext_path_score_row against the numpy restatement
of include/ctcext.h, "Path scores", on oracle rows and hand-written rows, and
the properties of path_scores_util's cases the GPU tests rely on."""
import numpy as np
import pytest

import ctcext_amd
import oracle
import path_scores_util as u

LOG = np.log


def _row(x, y, frames, blank=0, blank_label=-1):
    x = np.asarray(x, np.float64)
    norm = oracle.row_norm(np.ascontiguousarray(x[:frames])) if frames else np.zeros((0,))
    return ctcext_amd.path_score_row(x, norm, y, frames, blank, blank_label), u.path_score(x[:frames], norm, y, frames, blank)


@pytest.mark.parametrize("name", ["gaussian-40x4x29x16x3-plain", "sticky-12x6x5x8x3-plain", "neg_inf-12x6x5x8x3-merge",
                                  "float64", "lanes-70"])
def test_row_function_matches_the_definition_on_oracle_rows(name):
    c = u.case(name)
    x, sl = c["x"], c["sl"]
    for b in range(x.shape[1]):
        n = int(sl[b])
        norm = oracle.row_norm(np.ascontiguousarray(x[:n, b])) if n else np.zeros((0,), x.dtype)
        for p, y in enumerate(c["rows"][b]):
            got, want = ctcext_amd.path_score_row(x[:, b], norm, y, n, 0), c["want"][b, p].astype(x.dtype)
            assert got.dtype == x.dtype and (got == want or abs(got - want) <= 2 * np.spacing(abs(want))), (b, p, got, want)


def test_hand_written_rows():
    flat = np.log(np.full((4, 3), 1 / 3))
    got, want = _row(flat, [], 3)                      # m = 0: the all-blank alignment
    assert got == pytest.approx(3 * LOG(1 / 3), abs=1e-14) and got == pytest.approx(float(want), abs=1e-14)
    assert _row(flat, [], 0) == (0.0, 0.0)             # frames = 0
    assert _row(flat, [1, 1], 2) == (-np.inf, -np.inf)   # "aa" in two frames: infeasible
    got, want = _row(flat, [1, 1], 3)                  # "aa" in three: a, blank, a alone
    assert got == pytest.approx(3 * LOG(1 / 3), abs=1e-14) and got == pytest.approx(float(want), abs=1e-14)
    dead = flat.copy()
    dead[1, 0] = -np.inf                               # a -inf logit on the only path of "aa"
    assert _row(dead, [1, 1], 3) == (-np.inf, -np.inf)
    assert np.isnan(_row(flat, [1, 3], 3)[0]) and np.isnan(_row(flat, [-1], 3)[0])   # no such class
    got, want = _row(flat, [0, 1], 3, blank=2, blank_label=2)   # blank_label == blank_index is no error
    assert got == pytest.approx(LOG(5) + 3 * LOG(1 / 3), abs=1e-14)
    with pytest.raises(ctcext_amd.InvalidArgumentError):
        _row(flat, [1], 3, blank=0, blank_label=1)     # the blank_label rule


def test_plain_recursion_stays_inside_e_on_the_gpu_cases():
    worst = dict.fromkeys(list(u.E) + list(u.E_OWN), 0.0)
    for name in u.BUILDERS:
        c = u.case(name)
        want, plain = c["want"], c["plain"]
        fin = np.isfinite(want)
        np.testing.assert_array_equal(np.isneginf(plain), np.isneginf(want), err_msg=name)
        np.testing.assert_array_equal(np.isnan(plain), np.isnan(want), err_msg=name)
        assert not np.isnan(want).any(), name           # (every item of every case has status 0)
        key = name if name in u.E_OWN else c["x"].dtype.type
        if fin.any():
            worst[key] = max(worst[key], float(np.abs(plain[fin] - want[fin]).max()))
    for key, e in {**u.E, **u.E_OWN}.items():
        assert 0.9 * e < worst[key] <= e, (key, worst[key], e)   # the constant is the measured figure, rounded up


def test_the_cases_hold_what_the_gpu_tests_rely_on():
    m = {n: [len(y) for r in u.case(n)["rows"] for y in r] for n in u.BUILDERS}
    for name, mult in (("lanes-70", 64), ("lanes-140", 64), ("lanes-300", 256), ("lanes-1200", 1024)):
        assert min(m[name]) < mult < max(m[name]), (name, sorted(m[name]))
    sticky = [r for n in u.BUILDERS if n.startswith("sticky") and n.endswith("plain") for r in u.case(n)["rows"]]
    assert any(a == b for r in sticky for y in r for a, b in zip(y, y[1:]))   # a forbidden s - 2 step
    assert any(0 in m[n] for n in m if n.startswith("sticky"))
    assert np.isneginf(u.case("neg_inf-12x6x5x8x3-merge")["want"]).any()
    tight = u.case("tight")
    assert tight["rows"][0][0] == [1, 1] and len(tight["rows"][1]) == 3 and np.isfinite(tight["want"]).all()
    # after a skipping decode the score covers the dropped frames: the kept frames alone give another number
    c = u.case("skip")
    kept = u.scores(c["x"], c["sl"], c["rows"], c["P"], frames_of=lambda b: np.asarray(c["kmaps"][b], np.int64))
    assert (np.abs(kept - c["want"]) > u.tol("skip", np.float32)).all()

