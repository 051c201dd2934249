"""Target alignments without a GPU: the symbols, the ctypes mirror of
ctcext_target_alignments_out against the header, the workspace formula, the
frames of a decision word, and the argument errors that need no device."""
import ctypes
import os
import subprocess

import pytest

from ctcext_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctcext.h")


def test_struct_matches_header_and_symbols_are_exported(tmp_path):
    out = _lib.TargetAlignmentsOut
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ctcext.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(ctcext_target_alignments_out));']
    lines += ['printf("%s %%zu\\n", offsetof(ctcext_target_alignments_out, %s));' % (f, f) for f, _ in out._fields_]
    lines.append("return CTCEXT_HAS_TARGET_ALIGNMENTS - 1; }")
    (tmp_path / "abi.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "abi")]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(out)
    for f, _ in out._fields_:
        assert int(got[f]) == getattr(out, f).offset, f
    lib = _lib.load()
    for s in _lib.TARGET_ALIGNMENTS_SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s


@pytest.mark.parametrize("B,N,L,T", [(1, 1, 0, 1), (3, 12, 7, 20), (3, 33, 7, 20), (2, 5, 8, 10), (2, 5, 15, 11), (4, 9, 31, 0),
                                     (1, 4, 32, 65), (64, 64, 15, 1500), (2, 0, 63, 9)])
def test_bytes_equal_the_formula(B, N, L, T):
    lib = _lib.load()
    assert lib.ctcext_target_alignments_word_frames() == 10
    per = 256 // next(g for g in (8, 16, 32, 64) if L < g)
    assert lib.ctcext_target_alignments_bytes(B, N, L, T) == B * -(-N // per) * -(-T // 10) * 1024


def test_bytes_refuse_what_no_segment_holds():
    size = _lib.load().ctcext_target_alignments_bytes
    assert [size(2, 3, 64, 10), size(-1, 3, 7, 10), size(2, -3, 7, 10), size(2, 3, -1, 10), size(2, 3, 7, -1)] == [-1] * 5


def test_argument_errors_need_no_device():
    lib = _lib.load()
    t, o = _lib.Targets(n_targets=-1), _lib.TargetAlignmentsOut()
    assert lib.ctcext_dense_target_alignments(None, ctypes.byref(t), ctypes.byref(o)) == _lib.CTCEXT_INVALID_ARGUMENT
    assert lib.ctcext_last_error().decode() == "null argument"
    assert lib.ctcext_dense_target_alignments_route(None, None) == _lib.CTCEXT_INVALID_ARGUMENT
    assert lib.ctcext_dense_target_alignments_ms(None, None) == _lib.CTCEXT_INVALID_ARGUMENT
