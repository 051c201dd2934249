"""The dense, enqueue-only decode at the C boundary, without a GPU: the struct
layout and constants against the header, the host-only validation in the
reference's order followed by the two dense messages, and what the Python
entry points refuse before any device work."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ctcext_amd
from ctcext_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctcext.h")

INV, PRE = _lib.CTCEXT_INVALID_ARGUMENT, _lib.CTCEXT_FAILED_PRECONDITION


def _args(T=5, B=3, C=6, W=8, P=2, dims=3, sl_dims=1, sl_size=None, blank=0, dtype=_lib.CTCEXT_F32,
          on_device=1, fmt=_lib.CTCEXT_IN_NATIVE, st=(0, 0), scorer=0, table=False):
    """A well-formed call (the pointers are never read by the validation)."""
    buf = (ctypes.c_float * 4)()
    a = _lib.DecodeArgs()
    a.dtype, a.inputs_on_device = dtype, on_device
    a.inputs = a.sequence_length = ctypes.cast(buf, ctypes.c_void_p)
    a.max_time, a.batch_size, a.num_classes = T, B, C
    a.beam_width, a.top_paths, a.blank_index, a.blank_label = W, P, blank, -1
    a.inputs_dims, a.sequence_length_dims = dims, sl_dims
    a.sequence_length_size = B if sl_size is None else sl_size
    a.inputs_format = fmt
    a.inputs_stride_t, a.inputs_stride_b = st
    a.scorer = scorer
    if table:
        a.scorer_table = ctypes.cast(buf, ctypes.c_void_p)
    return a, buf


def _outs(null=None):
    buf = (ctypes.c_int64 * 4)()
    o = _lib.DenseOutputs()
    for f, _ in _lib.DenseOutputs._fields_[:-1]:
        setattr(o, f, None if f == null else ctypes.cast(buf, ctypes.c_void_p))
    o.pad_value = -1
    return o, buf


def _validate(a, o):
    lib = _lib.load()
    rc = lib.ctcext_dense_validate(ctypes.byref(a), ctypes.byref(o))
    return rc, lib.ctcext_last_error().decode()


def test_dense_struct_matches_header(tmp_path):
    """The ctypes mirror of ctcext_dense_outputs has the C header's size and
    field offsets, the constants its values (gcc on include/ctcext.h), and the
    ABI version is still 8."""
    src = tmp_path / "abi.c"
    consts = {"CTCEXT_HAS_DENSE": 1, "CTCEXT_FLAG_DENSE_NULL_STREAM": _lib.CTCEXT_FLAG_DENSE_NULL_STREAM,
              "CTCEXT_ITEM_LENGTH": _lib.CTCEXT_ITEM_LENGTH, "CTCEXT_ITEM_FEW_LEAVES": _lib.CTCEXT_ITEM_FEW_LEAVES,
              "CTCEXT_ITEM_HELPER_TIMEOUT": _lib.CTCEXT_ITEM_HELPER_TIMEOUT,
              "CTCEXT_ITEM_TABLE": _lib.CTCEXT_ITEM_TABLE, "CTCEXT_ABI_VERSION": 8}
    py = _lib.DenseOutputs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ctcext.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(ctcext_dense_outputs));']
    for f, _ in py._fields_:
        lines.append('printf("%%s %%zu\\n", "%s", offsetof(ctcext_dense_outputs, %s));' % (f, f))
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
    assert (_lib.CTCEXT_ITEM_LENGTH, _lib.CTCEXT_ITEM_FEW_LEAVES, _lib.CTCEXT_ITEM_HELPER_TIMEOUT,
            _lib.CTCEXT_ITEM_TABLE, _lib.CTCEXT_FLAG_DENSE_NULL_STREAM) == (1, 2, 4, 8, 512)


def test_abi_version_unchanged_and_dense_symbols_exist():
    lib = _lib.load()
    assert lib.ctcext_abi_version() == 8 == _lib.CTCEXT_ABI_VERSION
    for s in ("ctcext_dense_validate", "ctcext_dense_reserve", "ctcext_decode_dense", "ctcext_dense_check"):
        assert s in _lib.EXPORTED_SYMBOLS
        getattr(lib, s)
    for name in ("decode_dense", "dense_check", "DenseDecode"):
        assert name in ctcext_amd.__all__ and hasattr(ctcext_amd, name)
    assert ctcext_amd.DenseDecode._fields == ("decoded", "decoded_lengths", "alignment", "alignment_lengths",
                                              "log_probability", "status")


def test_dense_validate_accepts():
    o, _k = _outs()
    for kw in (dict(), dict(dtype=_lib.CTCEXT_F64), dict(fmt=_lib.CTCEXT_IN_BF16), dict(st=(6, 30)),
               dict(scorer=_lib.CTCEXT_SCORER_BIGRAM, table=True), dict(T=7)):
        a, _b = _args(**kw)
        assert _validate(a, o) == (_lib.CTCEXT_OK, ""), kw
    # batch_size 0: nothing is addressed, null outputs are fine
    a, _b = _args(B=0)
    null = _lib.DenseOutputs()
    assert _validate(a, null) == (_lib.CTCEXT_OK, "")


# The reference's messages in the reference's order: each row breaks one more
# thing than the row below it needs, and the earlier check wins.
ORDER = [
    (dict(W=0, P=0, dims=2), INV, "Value for attr 'beam_width' of 0 must be at least minimum 1"),
    (dict(P=0, dims=2), INV, "Value for attr 'top_paths' of 0 must be at least minimum 1"),
    (dict(dims=2, sl_dims=2), INV, "inputs is not a 3-Tensor"),
    (dict(sl_dims=2, sl_size=4), INV, "sequence_length is not a vector"),
    (dict(sl_size=4, blank=6), PRE, "len(sequence_length) != batch_size.  len(sequence_length):  4 batch_size: 3"),
    (dict(blank=6, W=2, P=3), INV, "blank_index out of range [0, num_classes)"),
    (dict(W=2, P=3, fmt=4), INV, "requested more paths than the beam width."),
    # ... then the ABI-7 layout messages
    (dict(fmt=4, dtype=_lib.CTCEXT_F64), INV,
     "inputs_format must be CTCEXT_IN_NATIVE, CTCEXT_IN_F16 or CTCEXT_IN_BF16"),
    (dict(fmt=_lib.CTCEXT_IN_F16, dtype=_lib.CTCEXT_F64, st=(6, 0)), INV, "half-precision inputs need dtype float32"),
    (dict(st=(6, 0), on_device=0), INV, "inputs_stride_t and inputs_stride_b must be given together"),
    (dict(st=(5, 4), on_device=0), INV, "inputs_stride_t is below num_classes"),
    (dict(st=(18, 5), on_device=0), INV, "inputs_stride_b is below num_classes"),
]


@pytest.mark.parametrize("kw,code,msg", ORDER, ids=[m[:40] for _, _, m in ORDER])
def test_dense_validate_reference_messages_in_order(kw, code, msg):
    a, _b = _args(**kw)
    o, _k = _outs(null="status")   # (and a null output: every check above comes before the dense ones)
    assert _validate(a, o) == (code, msg)
    # ctcext_validate says the same for the same arguments
    lib = _lib.load()
    if kw.get("on_device", 1):
        assert lib.ctcext_validate(ctypes.byref(a)) == code
        assert lib.ctcext_last_error().decode() == msg


def test_dense_validate_own_messages_come_last():
    o, _k = _outs()
    a, _b = _args(on_device=0)
    assert _validate(a, o) == (INV, "ctcext_decode_dense needs device inputs")
    # host inputs come before a null output
    bad, _k2 = _outs(null="decoded")
    assert _validate(a, bad) == (INV, "ctcext_decode_dense needs device inputs")
    a, _b = _args()
    for f, _ in _lib.DenseOutputs._fields_[:-1]:
        bad, _k2 = _outs(null=f)
        assert _validate(a, bad) == (INV, "null dense output pointer"), f
    assert _validate(a, o) == (_lib.CTCEXT_OK, "")


def test_dense_validate_reads_no_data():
    """The lengths and the table are device memory: a length above max_time
    and a positive table entry are not seen by the host validation."""
    sl = (ctypes.c_int32 * 3)(5, 99, 5)
    tab = np.ones((7, 6), np.float32)
    a, _b = _args(scorer=_lib.CTCEXT_SCORER_BIGRAM)
    a.sequence_length = ctypes.cast(sl, ctypes.c_void_p)
    a.scorer_table = tab.ctypes.data
    o, _k = _outs()
    assert _validate(a, o) == (_lib.CTCEXT_OK, "")


def test_decode_dense_refuses_host_tensors():
    import torch
    x = torch.zeros((3, 5, 6))
    with pytest.raises(ValueError, match="decode_logits"):
        ctcext_amd.decode_dense(x, [5, 5, 5], 8, 2)
    with pytest.raises(ValueError, match="decode_logits"):
        ctcext_amd.decode_dense(np.zeros((3, 5, 6), np.float32), [5, 5, 5], 8, 2)


def test_dense_check_before_any_dense_call():
    # (handles are per thread: a fresh thread has made no dense call, whatever ran before this test)
    import threading
    got = []

    def run():
        try:
            ctcext_amd.dense_check()
        except Exception as e:   # noqa: BLE001
            got.append(e)
    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert len(got) == 1 and isinstance(got[0], ctcext_amd.FailedPreconditionError), got
    assert got[0].error_code == _lib.CTCEXT_FAILED_PRECONDITION
    assert got[0].message == "ctcext_dense_check without a ctcext_decode_dense"
    # the C entry point itself refuses a null handle
    assert _lib.load().ctcext_dense_check(None) == _lib.CTCEXT_INVALID_ARGUMENT
