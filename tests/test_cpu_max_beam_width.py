"""ctcext_max_beam_width(C, dtype) is part of the C ABI: the widest beam whose
decode layout fits the LDS.  The small-C scored kernels' second row buffer
(round 16) sits after the helper's queue, outside that layout, so every value
must be what it was: compared with tests/golden/max_beam_width.json, recorded
on the CPU from the library of commit 50d534b (the parent of round 16).
"""
import json
import os

import pytest

from ctcext_amd import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "max_beam_width.json")
CLASSES = list(range(1, 65)) + [65, 1000, 5000, 65535]
DTYPES = {"float32": _lib.CTCEXT_F32, "float64": _lib.CTCEXT_F64}


def _gold():
    with open(GOLD) as f:
        return json.load(f)


def test_golden_covers_the_cases():
    g = _gold()
    assert g["classes"] == CLASSES
    for name in DTYPES:
        assert len(g[name]) == len(CLASSES)


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_max_beam_width_is_the_parents(name):
    lib = _lib.load()
    got = [int(lib.ctcext_max_beam_width(C, DTYPES[name])) for C in CLASSES]
    assert got == _gold()[name]
