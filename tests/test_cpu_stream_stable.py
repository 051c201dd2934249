"""The stable-prefix query of a stream at the C boundary, without a GPU: the
two symbols, their ctypes declarations against the header's signatures, the
null-argument answers, and StreamDecoder.stable() before a push and after
close."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ctcext_amd
from ctcext_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctcext.h")
SYMBOLS = ("ctcext_stream_stable", "ctcext_stream_stable_reference")
CTYPES = {"ctcext_stream*": ctypes.c_void_p, "int32_t*": ctypes.POINTER(ctypes.c_int32),
          "int64_t*": ctypes.POINTER(ctypes.c_int64)}


def test_library_exports_both_symbols():
    lib = _lib.load()
    assert lib.ctcext_abi_version() == 8 == _lib.CTCEXT_ABI_VERSION
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and s in _lib.STREAM_STABLE_SYMBOLS
        assert ctypes.cast(getattr(lib, s), ctypes.c_void_p).value
    assert "StablePrefix" in ctcext_amd.__all__
    assert ctcext_amd.StablePrefix._fields == ("decoded_length", "frames")


def test_header_defines_the_feature_macro(tmp_path):
    src = tmp_path / "has.c"
    src.write_text('#include <stdio.h>\n#include "ctcext.h"\n'
                   'int main(void) { printf("%d %d\\n", CTCEXT_HAS_STREAM_STABLE, CTCEXT_ABI_VERSION);\n'
                   '  int (*f)(ctcext_stream*, int32_t*, int64_t*, int64_t*) = ctcext_stream_stable;\n'
                   '  int (*g)(ctcext_stream*, int32_t*, int64_t*) = ctcext_stream_stable_reference;\n'
                   '  return f == 0 || g == 0; }\n')
    # (compiled only: the declarations have the pointer types the test names; not linked)
    subprocess.check_call(["gcc", "-Werror", "-c", "-I", os.path.dirname(HEADER), str(src), "-o",
                           str(tmp_path / "has.o")])
    txt = open(HEADER).read()
    assert re.search(r"#define\s+CTCEXT_HAS_STREAM_STABLE\s+1\b", txt)
    assert re.search(r"#define\s+CTCEXT_ABI_VERSION\s+8\b", txt)


def test_lib_declares_the_header_signatures():
    """_lib's argtypes are the header's parameter types, in order."""
    lib = _lib.load()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name
        want = []
        for prm in m.group(1).split(","):
            typ = re.sub(r"\s*\w+\s*$", "", prm.strip())   # drop the parameter's name
            want.append(CTYPES[typ.replace(" ", "")])
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want, name
        assert fn.restype is ctypes.c_int


def test_null_arguments_are_refused_with_a_message():
    lib = _lib.load()
    n = (ctypes.c_int32 * 3)()
    f = (ctypes.c_int64 * 3)()
    w = (ctypes.c_int64 * 3)()
    assert lib.ctcext_stream_stable(None, n, f, w) == _lib.CTCEXT_INVALID_ARGUMENT
    assert lib.ctcext_last_error().decode() == "null argument"
    assert lib.ctcext_stream_stable(None, None, None, None) == _lib.CTCEXT_INVALID_ARGUMENT
    assert lib.ctcext_last_error().decode() == "null argument"
    assert lib.ctcext_stream_stable_reference(None, n, f) == _lib.CTCEXT_INVALID_ARGUMENT
    assert lib.ctcext_last_error().decode() == "null argument"
    assert lib.ctcext_stream_stable_reference(None, None, None) == _lib.CTCEXT_INVALID_ARGUMENT
    assert lib.ctcext_last_error().decode() == "null argument"


def test_stable_before_the_first_push_and_after_close():
    """A stream that has not opened yet answers zeros (no device work); a
    closed one raises FailedPreconditionError, as push does."""
    s = ctcext_amd.StreamDecoder(3, 6, 8, 2, 16)
    r = s.stable()
    assert isinstance(r, ctcext_amd.StablePrefix)
    assert r.decoded_length.dtype == np.int32 and r.frames.dtype == np.int64
    assert r.decoded_length.tolist() == [0, 0, 0] and r.frames.tolist() == [0, 0, 0]
    r, walked = s.stable(walked=True)
    assert walked.dtype == np.int64 and walked.tolist() == [0, 0, 0] and r.frames.tolist() == [0, 0, 0]
    assert s._stable_reference().decoded_length.tolist() == [0, 0, 0]
    s.close()
    for call in (s.stable, s._stable_reference):
        with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
            call()
        assert e.value.message == "the stream is closed"
