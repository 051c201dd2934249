"""Prefix scores without a GPU: the symbols and the header's macros, and the host
definition (prefix_score_row) against the enumeration of all C^T alignments."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import ctcext_amd
from ctcext_amd import _lib

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def test_symbols_are_exported_and_the_header_says_so(tmp_path):
    lib = _lib.load()
    for s in _lib.PREFIX_SCORES_SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    (tmp_path / "abi.c").write_text('#include "ctcext.h"\nint main(void) { return (CTCEXT_HAS_PREFIX_SCORES - 1) | '
                                    '(CTCEXT_ABI_VERSION - 8) | (CTCEXT_PREFIX_TIME_TILE - 64) | '
                                    '(CTCEXT_PREFIX_NARROW_SLICES - 8); }\n')
    subprocess.check_call(["gcc", "-I", INCLUDE, str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")])
    subprocess.check_call([str(tmp_path / "abi")])


def _inputs(T, C=3):
    x = np.random.default_rng(T).normal(size=(T, C)) * 2
    return x, np.logaddexp.reduce(x, axis=1)


def _enumerated(x, norm, g, blank):
    """log of the mass of all alignments whose collapsed labels start with g + (c,); at c == blank: equal g."""
    T, C = x.shape
    mass = np.zeros(C)
    for a in itertools.product(range(C), repeat=T):
        y = tuple(k for k, _ in itertools.groupby(a) if k != blank)
        p = np.exp(sum(x[f, c] - norm[f] for f, c in enumerate(a)))
        if y == g:
            mass[blank] += p
        elif y[:len(g)] == g:
            mass[y[len(g)]] += p
    with np.errstate(divide="ignore"):
        return np.log(mass)


@pytest.mark.parametrize("blank", [0, 2])
@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_row_matches_the_enumeration_of_all_alignments(T, blank):
    a, b = [c for c in range(3) if c != blank]
    x, norm = _inputs(T)
    for g in ((), (a,), (a, a), (a, b), (b, a, b)):
        got = ctcext_amd.prefix_score_row(x, norm, g, T, blank)
        want = _enumerated(x, norm, g, blank)
        assert got.dtype == np.float64
        np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want), err_msg=str(g))
        fin = np.isfinite(want)
        np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=1e-12, err_msg=str(g))
        assert got[blank] == ctcext_amd.path_score_row(x, norm, g, T, blank)   # the end score
        if not g:
            assert abs(np.logaddexp.reduce(got)) <= 1e-12


def test_row_conventions():
    x, norm = _inputs(4)
    x32 = x.astype(np.float32)
    none = ctcext_amd.prefix_score_row(x32, norm, (), 0, 1)   # frames == 0
    assert none.dtype == np.float32 and none[1] == 0 and np.isneginf(none[[0, 2]]).all()
    assert np.isneginf(ctcext_amd.prefix_score_row(x, norm, (0,), 0, 1)).all()
    for bad in ((3,), (0, -1)):   # a label outside [0, C): the whole row
        assert np.isnan(ctcext_amd.prefix_score_row(x, norm, bad, 4, 1)).all()
    assert np.isneginf(ctcext_amd.prefix_score_row(x, norm, (0, 0, 0), 4, 1)).all()   # infeasible: five frames
    with pytest.raises(ctcext_amd.InvalidArgumentError):
        ctcext_amd.prefix_score_row(x, norm, (), 4, 3)
