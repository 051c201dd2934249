"""The greedy decode without a GPU: ctcext_greedy_row against the numpy
restatement of the definition (include/ctcext.h, "Greedy decode"), exactly.
The restatement and the input families are shared with test_gpu_greedy."""
import numpy as np
import pytest

import ctcext_amd
import oracle


def greedy(x, norm, n, blank, blank_label, merge):
    """The normative definition for one item: x [T, C] and norm [n] of the compute dtype."""
    ft = x.dtype.type
    dec, ali, prev_k, prev_lab, logp = [], [], None, None, ft(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(n):
            m, k = x[f, 0], 0
            for j in range(1, x.shape[1]):           # class order, strict: the lowest index wins a tie;
                if x[f, j] > m: m, k = x[f, j], j    # a comparison with NaN is false (a leading NaN stays, k = 0)
            lp = ft(m - norm[f])
            logp = lp if f == 0 else ft(logp + lp)
            ali.append(blank_label if k == blank else k)
            if k != blank and k != prev_k:
                if not (merge and k == prev_lab):
                    dec.append(k)
                prev_lab = k
            prev_k = k
    return dec, ali, logp


def quantised(rng, T, B, C, dtype=np.float32):
    """Integer logits in [-2, 2]: equal maxima are common, the lowest index must win."""
    return rng.integers(-2, 3, size=(T, B, C)).astype(dtype)


def sticky(rng, T, B, C, dtype=np.float32):
    """A class held for 10..120 frames, then the blank for 1..40, then with p = 0.5 the same class again.  Item 0
    starts with a fixed schedule: a run over frames 63/64, a blank gap, the same class over frames 255/256."""
    x = rng.standard_normal((T, B, C)) * 0.5
    for b in range(B):
        c = int(rng.integers(0, C))
        plan = [(c, 40, 70), (0, 70, 250), (c, 250, 262), (0, 262, 300)] if b == 0 else []
        t = plan[-1][2] if plan else 0
        while t < T:
            n = int(rng.integers(10, 121))
            plan.append((c, t, t + n))
            g = int(rng.integers(1, 41))
            plan.append((0, t + n, t + n + g))
            t += n + g
            if rng.random() < 0.5:
                c = int(rng.integers(0, C))
        for k, lo, hi in plan:
            x[lo:hi, b, k] += 6
    return x.astype(dtype)


def special(rng, T, B, C, dtype=np.float32):
    """Gaussian logits with NaN, -inf and +inf cells; every eighth frame starts with a NaN."""
    x = rng.standard_normal((T, B, C)).astype(dtype)
    u = rng.random((T, B, C))
    x[u < 0.03], x[(u >= 0.03) & (u < 0.10)], x[u > 0.97] = np.nan, -np.inf, np.inf
    x[::8, :, 0] = np.nan
    return x


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(got, want, err_msg=str(what))
    if got.dtype.kind == "f":
        # every sign but a NaN's: inf - inf is a NaN of the adder's own default sign (set on this host's, clear on
        # the GPU's), which the definition does not fix; a NaN that came in with the logits keeps its sign on both
        ok = ~np.isnan(want)
        np.testing.assert_array_equal(np.signbit(got)[ok], np.signbit(want)[ok], err_msg="%s: signs" % (what,))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("family", [quantised, sticky, special])
def test_row_equals_the_restatement(family, merge, dtype):
    T, B, C = (300, 2, 6) if family is sticky else (41, 3, 7)
    x = family(np.random.default_rng(11), T, B, C, dtype)
    differ = 0
    for b, n in enumerate([T, T - 5, 0][:B]):
        xb = np.ascontiguousarray(x[:, b])
        norm = oracle.row_norm(xb)
        dec, ali, logp = greedy(xb, norm, n, 0, -1, merge)
        gd, ga, gl = ctcext_amd.greedy_row(xb, norm, n, 0, -1, merge)
        assert gd.tolist() == dec and ga.tolist() == ali and len(ali) == n, (family.__name__, b)
        same_bits(np.array([gl]), np.array([logp]), (family.__name__, b))
        differ += dec != greedy(xb, norm, n, 0, -1, not merge)[0]
    assert differ or family is special   # the rows hold A blank A, which the two merge settings decode differently


def test_hand_written_rows():
    x = np.array([[0, 2, 2], [0, 2, 2], [3, 0, 0], [0, 1, 0], [0, 0, 5], [0, 0, 5]], np.float32)   # 1 1 _ 1 2 2
    for merge, want in ((False, [1, 1, 2]), (True, [1, 2])):
        dec, ali, logp = ctcext_amd.greedy_row(x, np.ones(6, np.float32), 6, 0, -7, merge)
        assert dec.tolist() == want and ali.tolist() == [1, 1, -7, 1, 2, 2] and logp == np.float32(12)
    dec, ali, logp = ctcext_amd.greedy_row(np.zeros((0, 3), np.float32), [], 0, 0)
    assert dec.size == 0 and ali.size == 0 and logp == 0 and not np.signbit(logp)
    dec, ali, logp = ctcext_amd.greedy_row(np.array([[-0.0, -1]], np.float64), [0.0], 1, 1)   # logp = lp, not 0 + lp
    assert dec.tolist() == [0] and ali.tolist() == [0] and logp == 0 and np.signbit(logp)
