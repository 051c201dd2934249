"""The enqueue-only push of a stream at the C boundary, without a GPU: the
struct layout and constants against the header, the host-only rejections with
their messages in their order (before any device work: there is no device
here), the unchanged ABI version, and what the Python entry points refuse on
the host."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ctcext_amd
from ctcext_amd import _lib
from test_cpu_stream import _chunk, _sargs

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctcext.h")
INV = _lib.CTCEXT_INVALID_ARGUMENT
HYP = ("decoded", "decoded_length", "alignment", "alignment_length", "log_probability")
M_DEVICE = "ctcext_stream_push_dense needs device chunks"
M_FLAGS = "chunk flags: CTCEXT_FLAG_TEST_HELPER_DEAD, _PROFILE and _DENSE_NULL_STREAM only"
M_NULL = "null dense output pointer"
M_ALIGN = "dense outputs decoded and alignment need 8-byte alignment"


def _outs(null=(), stable=True, off=None):
    """Well-formed outputs (never written: the validation reads the pointers'
    values only); `null` names fields left NULL, `off` one moved 4 bytes."""
    buf = (ctypes.c_int64 * 8)()
    base = ctypes.addressof(buf)
    o = _lib.StreamDenseOutputs()
    for f, _ in _lib.StreamDenseOutputs._fields_[:-1]:
        if f in null or (not stable and f.startswith("stable_")):
            continue
        setattr(o, f, base + (4 if f == off else 0))
    o.pad_value = -1
    return o, buf


def _validate(a, c, o):
    lib = _lib.load()
    rc = lib.ctcext_stream_dense_validate(ctypes.byref(a) if a is not None else None,
                                          ctypes.byref(c) if c is not None else None,
                                          ctypes.byref(o) if o is not None else None)
    return rc, lib.ctcext_last_error().decode()


def _dargs(**kw):
    a = _sargs(**kw)
    a.on_device = 1
    return a


def test_struct_matches_header(tmp_path):
    """The ctypes mirror of ctcext_stream_dense_outputs has the C header's
    size and field offsets, the new constants its values, CTCEXT_HAS_STREAM_DENSE
    is defined and the ABI version is still 8 (gcc on include/ctcext.h)."""
    src = tmp_path / "abi.c"
    consts = {"CTCEXT_HAS_STREAM_DENSE": 1, "CTCEXT_ITEM_CAPACITY": _lib.CTCEXT_ITEM_CAPACITY,
              "CTCEXT_FLAG_DENSE_NULL_STREAM": _lib.CTCEXT_FLAG_DENSE_NULL_STREAM, "CTCEXT_ABI_VERSION": 8}
    py = _lib.StreamDenseOutputs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ctcext.h"',
             "#ifndef CTCEXT_HAS_STREAM_DENSE", '#error "CTCEXT_HAS_STREAM_DENSE is not defined"', "#endif",
             "int main(void) {", 'printf("size %zu\\n", sizeof(ctcext_stream_dense_outputs));']
    for f, _ in py._fields_:
        lines.append('printf("%%s %%zu\\n", "%s", offsetof(ctcext_stream_dense_outputs, %s));' % (f, f))
    for c in consts:
        lines.append('printf("%%s %%d\\n", "%s", (int)%s);' % (c, c))
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(py)
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset, f
    for c, v in consts.items():
        assert int(got[c]) == v, c
    assert _lib.CTCEXT_ITEM_CAPACITY == 16
    bits = (_lib.CTCEXT_ITEM_LENGTH, _lib.CTCEXT_ITEM_FEW_LEAVES, _lib.CTCEXT_ITEM_HELPER_TIMEOUT,
            _lib.CTCEXT_ITEM_TABLE, _lib.CTCEXT_ITEM_CAPACITY)
    assert len({b for b in bits}) == 5 and all(b & (b - 1) == 0 for b in bits)


def test_abi_version_unchanged_and_symbols_exist():
    lib = _lib.load()
    assert lib.ctcext_abi_version() == 8 == _lib.CTCEXT_ABI_VERSION
    for s in ("ctcext_stream_dense_validate", "ctcext_stream_reserve", "ctcext_stream_push_dense",
              "ctcext_stream_check", "ctcext_stream_commit_ms"):
        assert s in _lib.EXPORTED_SYMBOLS
        getattr(lib, s)
    assert "StreamDense" in ctcext_amd.__all__
    assert ctcext_amd.StreamDense._fields == ("decoded", "decoded_lengths", "alignment", "alignment_lengths",
                                              "log_probability", "status", "frames", "stable_length",
                                              "stable_frames")
    for name in ("push_dense", "reserve", "check"):
        assert callable(getattr(ctcext_amd.StreamDecoder, name))


def test_validate_accepts():
    a = _dargs()
    c, _k = _chunk(a)
    for o in (_outs()[0], _outs(stable=False)[0], _outs(null=("frames",))[0], _outs(null=HYP)[0], None):
        assert _validate(a, c, o) == (_lib.CTCEXT_OK, ""), o
    for flags in (_lib.CTCEXT_FLAG_TEST_HELPER_DEAD, _lib.CTCEXT_FLAG_PROFILE, _lib.CTCEXT_FLAG_DENSE_NULL_STREAM):
        c.flags = flags
        assert _validate(a, c, _outs()[0]) == (_lib.CTCEXT_OK, "")
    # rows need 8-byte alignment only: a base 8 bytes off a 16-byte boundary is fine
    buf = (ctypes.c_int64 * 8)()
    base = (ctypes.addressof(buf) + 15) & ~15
    o, _b = _outs()
    c.flags = 0
    o.decoded = o.alignment = base + 8
    assert _validate(a, c, o) == (_lib.CTCEXT_OK, "")
    # batch_size 0: nothing is addressed, null outputs are fine
    a0 = _dargs(B=0)
    assert _validate(a0, _chunk(a0)[0], _lib.StreamDenseOutputs()) == (_lib.CTCEXT_OK, "")


# Each row breaks one more thing than the row below it needs; the earlier check wins.
ORDER = [
    (dict(attr="W"), "Value for attr 'beam_width' of 0 must be at least minimum 1"),
    (dict(host=True), M_DEVICE),
    (dict(flags=_lib.CTCEXT_FLAG_FORCE_LITERAL), M_FLAGS),
    (dict(t=-1), "inputs has a negative dimension"),
    (dict(fmt=9), "inputs_format must be CTCEXT_IN_NATIVE, CTCEXT_IN_F16 or CTCEXT_IN_BF16"),
    (dict(null="status"), M_NULL),
    (dict(off="decoded"), M_ALIGN),
]


@pytest.mark.parametrize("first", range(len(ORDER)))
def test_host_rejections_in_order(first):
    """Everything from ORDER[first] down is broken at once; ORDER[first]'s message comes."""
    broken = {}
    for kw, _ in ORDER[first:]:
        broken.update(kw)
    a = _dargs(W=0) if "attr" in broken else _dargs()
    if "host" in broken:
        a.on_device = 0
    c, _k = _chunk(a, t=broken.get("t", 4), fmt=broken.get("fmt", _lib.CTCEXT_IN_NATIVE))
    c.flags = broken.get("flags", 0)
    o, _b = _outs(null=(broken["null"],) if "null" in broken else (), off=broken.get("off"))
    assert _validate(a, c, o) == (INV, ORDER[first][1])


@pytest.mark.parametrize("null", [("status",), ("decoded",), ("alignment_length", "log_probability"),
                                  ("stable_length",), ("stable_frames",)])
def test_null_output_pointers(null):
    """status always; the five hypothesis pointers all or none; the stable pair both or neither."""
    a = _dargs()
    c, _k = _chunk(a)
    o, _b = _outs(null=null)
    assert _validate(a, c, o) == (INV, M_NULL)


@pytest.mark.parametrize("field", ["decoded", "alignment"])
def test_misaligned_rows(field):
    a = _dargs()
    c, _k = _chunk(a)
    o, _b = _outs(off=field)
    assert _validate(a, c, o) == (INV, M_ALIGN)


def test_null_arguments():
    """A null stream handle (and a null chunk) is refused by every new entry
    point before anything is read through it."""
    lib = _lib.load()
    a = _dargs()
    c, _k = _chunk(a)
    o, _b = _outs()
    assert _validate(None, c, o) == (INV, "null argument")
    assert _validate(a, None, o) == (INV, "null argument")
    assert lib.ctcext_stream_push_dense(None, ctypes.byref(c), None, ctypes.byref(o)) == INV
    assert lib.ctcext_last_error().decode() == "null argument"
    assert lib.ctcext_stream_reserve(None, 4) == INV
    assert lib.ctcext_stream_check(None) == INV
    ms = ctypes.c_double()
    assert lib.ctcext_stream_commit_ms(None, ctypes.byref(ms)) == INV


def test_python_refuses_host_chunks_before_any_device_work():
    s = ctcext_amd.StreamDecoder(3, 6, 8, 2, 16)
    with pytest.raises(ValueError, match="push_dense takes CUDA torch tensors"):
        s.push_dense(np.zeros((3, 4, 6), np.float32))
    assert s.handle is None   # nothing was opened
    assert s.check() is None  # no push yet: nothing to wait for
    s.close()
    with pytest.raises(ctcext_amd.OpError):
        s.check()
