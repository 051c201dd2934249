"""Target scores without a GPU: ctcext_targets_validate's messages through the
C ABI, the ctypes mirror of ctcext_targets against the header, and the host-only
tile query."""
import ctypes
import os
import subprocess

import pytest

from ctcext_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctcext.h")


@pytest.mark.parametrize("fields,code,msg", [
    (dict(n_targets=-1), _lib.CTCEXT_INVALID_ARGUMENT, "target scores: n_targets must not be negative"),
    (dict(n_targets=2, max_target=-3), _lib.CTCEXT_INVALID_ARGUMENT, "target scores: max_target must not be negative"),
    (dict(n_targets=2, max_target=3, targets=8), _lib.CTCEXT_INVALID_ARGUMENT, "target scores: target_length is null"),
    (dict(n_targets=2, max_target=3, target_length=8), _lib.CTCEXT_INVALID_ARGUMENT, "target scores: targets is null"),
    (dict(n_targets=2, max_target=0, target_length=8), _lib.CTCEXT_OK, ""),   # rows of no labels need no targets
    (dict(n_targets=0, max_target=5), _lib.CTCEXT_OK, ""),
    (dict(n_targets=2, max_target=3, targets=8, target_length=8, shared=1, labels_i64=1), _lib.CTCEXT_OK, ""),
])
def test_validate(fields, code, msg):
    lib = _lib.load()
    assert lib.ctcext_targets_validate(ctypes.byref(_lib.Targets(**fields))) == code
    assert lib.ctcext_last_error().decode() == msg
    assert lib.ctcext_targets_validate(None) == _lib.CTCEXT_INVALID_ARGUMENT


def test_struct_matches_header_and_symbols_are_exported(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ctcext.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(ctcext_targets));']
    lines += ['printf("%s %%zu\\n", offsetof(ctcext_targets, %s));' % (f, f) for f, _ in _lib.Targets._fields_]
    lines.append("return CTCEXT_HAS_TARGET_SCORES - 1; }")
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "abi")]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.Targets)
    for f, _ in _lib.Targets._fields_:
        assert int(got[f]) == getattr(_lib.Targets, f).offset, f
    lib = _lib.load()
    for s in _lib.TARGET_SCORES_SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s


def test_tile_is_host_only_and_states_the_bound():
    tile = _lib.load().ctcext_target_scores_tile
    assert [tile(c, 0) for c in (1, 29, 64, 65, 512, 513, 1100)] == [32, 32, 32, 31, 4, 0, 0]
    assert [tile(c, 1) for c in (6, 32, 33, 256, 257)] == [32, 32, 31, 4, 0]
    assert tile(0, 0) == 0 and tile(-4, 1) == 0
