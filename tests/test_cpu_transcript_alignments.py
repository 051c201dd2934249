"""Transcript alignments without a GPU: the symbols and the header's macro, the
workspace formula, the frames of a block and of a decision word, and the
argument errors that need no device."""
import ctypes
import os
import subprocess

import pytest

from ctcext_amd import _lib

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def test_symbols_are_exported_and_the_header_says_so(tmp_path):
    lib = _lib.load()
    for s in _lib.TRANSCRIPT_ALIGNMENTS_SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    (tmp_path / "abi.c").write_text('#include "ctcext.h"\nint main(void) { return CTCEXT_HAS_TRANSCRIPT_ALIGNMENTS - 1; }\n')
    subprocess.check_call(["gcc", "-I", INCLUDE, str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")])
    subprocess.check_call([str(tmp_path / "abi")])


@pytest.mark.parametrize("B,N,L,T", [(1, 1, 0, 1), (3, 3, 63, 69), (3, 3, 255, 261), (2, 5, 256, 11), (256, 1, 511, 1500),
                                     (1, 4, 512, 3), (1, 2, 1023, 13000), (2, 1, 1024, 7), (1, 1, 2047, 2055), (2, 0, 70, 9)])
def test_bytes_equal_the_formula(B, N, L, T):
    lib = _lib.load()
    K = next(k for k in (1, 2, 4, 8) if 256 * k > L)
    fpw = 32 // (3 * K)
    assert lib.ctcext_transcript_alignments_block_frames() == 20
    assert lib.ctcext_transcript_alignments_word_frames(L) == fpw == {1: 10, 2: 5, 4: 2, 8: 1}[K]
    assert lib.ctcext_transcript_alignments_bytes(B, N, L, T) == B * N * -(-T // fpw) * 1024


def test_bytes_refuse_what_no_block_holds():
    lib = _lib.load()
    size = lib.ctcext_transcript_alignments_bytes
    assert [size(2, 3, 2048, 10), size(-1, 3, 7, 10), size(2, -3, 7, 10), size(2, 3, -1, 10), size(2, 3, 7, -1)] == [-1] * 5
    assert lib.ctcext_transcript_alignments_word_frames(2048) == 0
    assert size(256, 1, 511, 1500) == 78643200   # cfg3, one transcript of up to 511 labels per item


def test_argument_errors_need_no_device():
    lib = _lib.load()
    t, o = _lib.Targets(n_targets=-1), _lib.TargetAlignmentsOut()
    assert lib.ctcext_dense_transcript_alignments(None, ctypes.byref(t), ctypes.byref(o)) == _lib.CTCEXT_INVALID_ARGUMENT
    assert lib.ctcext_last_error().decode() == "null argument"
    assert lib.ctcext_dense_transcript_alignments_ms(None, None) == _lib.CTCEXT_INVALID_ARGUMENT
