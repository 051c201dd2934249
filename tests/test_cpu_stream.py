"""The streaming entry points at the C boundary, without a GPU: the struct
layouts against the header, the host-only validation of a stream's attributes
and of a chunk, and the unchanged ABI version."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ctcext_amd
from ctcext_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctcext.h")

STREAM_SYMBOLS = ("ctcext_stream_validate", "ctcext_stream_validate_chunk", "ctcext_stream_open",
                  "ctcext_stream_push", "ctcext_stream_frames", "ctcext_stream_reset", "ctcext_stream_close")


def _sargs(dtype=_lib.CTCEXT_F32, B=3, C=6, F=16, W=8, P=2, blank=0, flags=0, scorer=0):
    a = _lib.StreamArgs()
    a.dtype = dtype
    a.batch_size, a.num_classes, a.max_frames = B, C, F
    a.beam_width, a.top_paths, a.blank_index, a.blank_label = W, P, blank, -1
    a.flags, a.scorer = flags, scorer
    return a


def _validate(a):
    lib = _lib.load()
    rc = lib.ctcext_stream_validate(ctypes.byref(a))
    return rc, lib.ctcext_last_error().decode()


def _chunk(a, t=4, fmt=_lib.CTCEXT_IN_NATIVE, st=(0, 0), lengths=None):
    c = _lib.Chunk()
    buf = (ctypes.c_float * 256)()
    c.inputs = ctypes.cast(buf, ctypes.c_void_p)
    keep = [buf]
    if lengths is not None:
        sl = (ctypes.c_int32 * len(lengths))(*lengths)
        c.chunk_length = ctypes.cast(sl, ctypes.c_void_p)
        keep.append(sl)
    c.chunk_time = t
    c.inputs_format = fmt
    c.inputs_stride_t, c.inputs_stride_b = st
    return c, keep


def _validate_chunk(a, c):
    lib = _lib.load()
    rc = lib.ctcext_stream_validate_chunk(ctypes.byref(a), ctypes.byref(c))
    return rc, lib.ctcext_last_error().decode()


def test_stream_structs_match_header(tmp_path):
    """The ctypes mirrors of ctcext_stream_args / ctcext_chunk have the C
    header's sizes and field offsets (gcc on include/ctcext.h)."""
    src = tmp_path / "abi.c"
    fields = {"ctcext_stream_args": _lib.StreamArgs, "ctcext_chunk": _lib.Chunk}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ctcext.h"', "int main(void) {"]
    for cname, py in fields.items():
        lines.append('printf("%%s size %%zu\\n", "%s", sizeof(%s));' % (cname, cname))
        for f, _ in py._fields_:
            lines.append('printf("%%s %%s %%zu\\n", "%s", "%s", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append('printf("abi %d\\n", CTCEXT_ABI_VERSION);')
    lines.append('printf("has_stream %d\\n", CTCEXT_HAS_STREAM);')
    lines.append('printf("kernel_stream %d\\n", CTCEXT_KERNEL_STREAM); return 0; }')
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, py in fields.items():
        assert int(got["%s size" % cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got["%s %s" % (cname, f)]) == getattr(py, f).offset, (cname, f)
    assert int(got["abi"]) == 8
    assert int(got["has_stream"]) == 1
    assert int(got["kernel_stream"]) == _lib.CTCEXT_KERNEL_STREAM == 0x8000


def test_abi_version_unchanged_and_stream_symbols_exist():
    lib = _lib.load()
    assert lib.ctcext_abi_version() == 8 == _lib.CTCEXT_ABI_VERSION
    for s in STREAM_SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS
        getattr(lib, s)
    assert "StreamDecoder" in ctcext_amd.__all__


def test_kernel_stat_names_the_stream_bit():
    k = _lib.decode_kernel_stat(0x800 | 0x8000 | 0x3 | (1 << 2) | (1 << 5))
    assert k["stream"] is True and k["launched"] and k["helper"] == "SQ" and k["WC"] == 128
    assert _lib.decode_kernel_stat(0x800)["stream"] is False


def test_stream_validate_accepts():
    for dtype in (_lib.CTCEXT_F32, _lib.CTCEXT_F64):
        assert _validate(_sargs(dtype=dtype)) == (_lib.CTCEXT_OK, "")
    assert _validate(_sargs(F=0)) == (_lib.CTCEXT_OK, "")
    assert _validate(_sargs(B=0)) == (_lib.CTCEXT_OK, "")


@pytest.mark.parametrize("kw,code,msg", [
    (dict(dtype=7), _lib.CTCEXT_INVALID_ARGUMENT, "dtype must be float32 or float64"),
    (dict(W=0), _lib.CTCEXT_INVALID_ARGUMENT, "Value for attr 'beam_width' of 0 must be at least minimum 1"),
    (dict(P=0), _lib.CTCEXT_INVALID_ARGUMENT, "Value for attr 'top_paths' of 0 must be at least minimum 1"),
    (dict(F=-1), _lib.CTCEXT_INVALID_ARGUMENT, "max_frames is negative"),
    (dict(blank=6), _lib.CTCEXT_INVALID_ARGUMENT, "blank_index out of range [0, num_classes)"),
    (dict(W=2, P=3), _lib.CTCEXT_INVALID_ARGUMENT, "requested more paths than the beam width."),
    (dict(scorer=5), _lib.CTCEXT_INVALID_ARGUMENT, "unknown beam scorer"),
    (dict(scorer=_lib.CTCEXT_SCORER_BIGRAM), _lib.CTCEXT_INVALID_ARGUMENT, "bigram beam scorer without a table"),
    (dict(flags=_lib.CTCEXT_FLAG_RECORD_RING), _lib.CTCEXT_INVALID_ARGUMENT,
     "stream flags: CTCEXT_FLAG_FORCE_LITERAL, _GLOBAL_STATE and _PROFILE only"),
    (dict(flags=_lib.CTCEXT_FLAG_TEST_HELPER_DEAD | _lib.CTCEXT_FLAG_PROFILE), _lib.CTCEXT_INVALID_ARGUMENT,
     "stream flags: CTCEXT_FLAG_FORCE_LITERAL, _GLOBAL_STATE and _PROFILE only"),
    # the reference's checks come first, in its order
    (dict(dtype=7, F=-1), _lib.CTCEXT_INVALID_ARGUMENT, "dtype must be float32 or float64"),
    (dict(W=0, F=-1), _lib.CTCEXT_INVALID_ARGUMENT, "Value for attr 'beam_width' of 0 must be at least minimum 1"),
])
def test_stream_validate_messages(kw, code, msg):
    assert _validate(_sargs(**kw)) == (code, msg)


def test_scorer_table_is_host_memory_wherever_the_chunks_live():
    """The bigram table is read on the host by ctcext_stream_validate, with
    on_device 0 and 1 alike: a positive entry is refused in both."""
    for on_device in (0, 1):
        for bad in (False, True):
            tab = -np.ones((7, 6), np.float32)
            if bad:
                tab[3, 2] = 0.5
            a = _sargs(scorer=_lib.CTCEXT_SCORER_BIGRAM)
            a.on_device = on_device
            a.scorer_table = tab.ctypes.data
            want = ((_lib.CTCEXT_INVALID_ARGUMENT, "beam scorer table entries must be log-probabilities (<= 0)")
                    if bad else (_lib.CTCEXT_OK, ""))
            assert _validate(a) == want, (on_device, bad)


def test_stream_decoder_device_argument():
    """device: None, an ordinal, a torch.device or a string; anything else, or
    a device that is no GPU, is refused when the stream is built."""
    import torch
    mk = lambda d: ctcext_amd.StreamDecoder(3, 6, 8, 2, 16, device=d)   # noqa: E731
    assert mk(None)._device is None
    assert mk(1)._device == 1 and mk(np.int64(2))._device == 2
    assert mk("cuda:1")._device == 1 and mk(torch.device("cuda", 0))._device == 0
    assert mk("cuda")._device is None
    with pytest.raises(ValueError):
        mk("cpu")
    with pytest.raises(TypeError):
        mk(1.5)
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.StreamDecoder(3, 6, 8, 2, 16, flags=_lib.CTCEXT_FLAG_NO_RING)
    assert e.value.message.startswith("stream flags:")


def test_chunk_validate_accepts():
    a = _sargs()
    for kw in (dict(), dict(fmt=_lib.CTCEXT_IN_F16), dict(fmt=_lib.CTCEXT_IN_BF16), dict(st=(6, 24)),
               dict(st=(17, 68), fmt=_lib.CTCEXT_IN_BF16), dict(t=0), dict(lengths=[4, 0, 2])):
        c, keep = _chunk(a, **kw)
        assert _validate_chunk(a, c) == (_lib.CTCEXT_OK, ""), kw
    c, keep = _chunk(_sargs(dtype=_lib.CTCEXT_F64), st=(6, 24))
    assert _validate_chunk(_sargs(dtype=_lib.CTCEXT_F64), c) == (_lib.CTCEXT_OK, "")


@pytest.mark.parametrize("akw,ckw,code,msg", [
    (dict(dtype=_lib.CTCEXT_F64), dict(fmt=_lib.CTCEXT_IN_F16), _lib.CTCEXT_INVALID_ARGUMENT,
     "half-precision inputs need dtype float32"),
    (dict(dtype=_lib.CTCEXT_F64), dict(fmt=_lib.CTCEXT_IN_BF16), _lib.CTCEXT_INVALID_ARGUMENT,
     "half-precision inputs need dtype float32"),
    (dict(), dict(fmt=4), _lib.CTCEXT_INVALID_ARGUMENT,
     "inputs_format must be CTCEXT_IN_NATIVE, CTCEXT_IN_F16 or CTCEXT_IN_BF16"),
    (dict(), dict(st=(6, 0)), _lib.CTCEXT_INVALID_ARGUMENT, "inputs_stride_t and inputs_stride_b must be given together"),
    (dict(), dict(st=(5, 24)), _lib.CTCEXT_INVALID_ARGUMENT, "inputs_stride_t is below num_classes"),
    (dict(), dict(st=(18, 5)), _lib.CTCEXT_INVALID_ARGUMENT, "inputs_stride_b is below num_classes"),
    (dict(), dict(lengths=[4, 5, 0]), _lib.CTCEXT_FAILED_PRECONDITION, "sequence_length(1) <= 4"),
    (dict(), dict(t=-1), _lib.CTCEXT_INVALID_ARGUMENT, "inputs has a negative dimension"),
    # the stream's own attributes are checked first
    (dict(W=0), dict(fmt=4), _lib.CTCEXT_INVALID_ARGUMENT, "Value for attr 'beam_width' of 0 must be at least minimum 1"),
])
def test_chunk_validate_messages(akw, ckw, code, msg):
    a = _sargs(**akw)
    c, keep = _chunk(a, **ckw)
    assert _validate_chunk(a, c) == (code, msg)


def test_stream_decoder_constructor_validates_on_the_host():
    """StreamDecoder checks its attributes when it is built (no device work:
    the stream opens with the first push)."""
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.StreamDecoder(3, 6, 0, 1, 16)
    assert e.value.message == "Value for attr 'beam_width' of 0 must be at least minimum 1"
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.StreamDecoder(3, 6, 8, 2, -2)
    assert e.value.message == "max_frames is negative"
    with pytest.raises(TypeError):
        ctcext_amd.StreamDecoder(3, 6, 8, 2, 16, dtype="float16")
    with pytest.raises(ValueError):
        ctcext_amd.StreamDecoder(3, 6, 8, 2, 16, scorer_table=np.zeros((6, 6), np.float32))
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.StreamDecoder(3, 6, 8, 2, 16, scorer_table=np.ones((7, 6), np.float32))
    assert e.value.message == "beam scorer table entries must be log-probabilities (<= 0)"
    s = ctcext_amd.StreamDecoder(3, 6, 8, 2, 16)
    assert s.frames.tolist() == [0, 0, 0] and s.frames.dtype == np.int64
    # shape and dtype errors of a chunk come before the stream opens
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        s.push(np.zeros((3, 2, 7), np.float32))
    assert "num_classes 7" in e.value.message
    with pytest.raises(ctcext_amd.InvalidArgumentError):
        s.push(np.zeros((2, 2, 6), np.float32))
    with pytest.raises(TypeError):
        s.push(np.zeros((3, 2, 6), np.float64))
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        s.push(np.zeros((3, 2, 6), np.float32), [2, 3, 0])
    assert e.value.message == "sequence_length(1) <= 2"
    s64 = ctcext_amd.StreamDecoder(3, 6, 8, 2, 16, dtype="float64")
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        s64.push(np.zeros((3, 2, 6), np.float16))
    assert e.value.message == "half-precision inputs need dtype float32"
    s.close()
    with pytest.raises(ctcext_amd.OpError):
        s.push(np.zeros((3, 2, 6), np.float32))
