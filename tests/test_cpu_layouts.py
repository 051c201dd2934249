"""The ABI-7 input fields (inputs_format, inputs_stride_t / _b) at the C
boundary, and decode_logits' stride/contiguity decision.  No GPU:
ctcext_validate is host-only and the layout decision is a pure helper."""
import ctypes

import numpy as np
import pytest
import torch

import ctcext_amd
from ctcext_amd import _lib
from ctcext_amd.ops import logits_layout

M_FORMAT = "inputs_format must be CTCEXT_IN_NATIVE, CTCEXT_IN_F16 or CTCEXT_IN_BF16"
M_HALF = "half-precision inputs need dtype float32"
M_PAIR = "inputs_stride_t and inputs_stride_b must be given together"
M_ST = "inputs_stride_t is below num_classes"
M_SB = "inputs_stride_b is below num_classes"


def _args(shape=(3, 2, 4), sl=(3, 3), W=4, P=1, blank=0, dtype=_lib.CTCEXT_F32, fmt=0, st=(0, 0), dims=3):
    a = _lib.DecodeArgs()   # zero-initialised, as every caller's
    a.dtype = dtype
    buf = (ctypes.c_float * 64)()
    a.inputs = ctypes.cast(buf, ctypes.c_void_p)
    sla = (ctypes.c_int32 * max(len(sl), 1))(*sl)
    a.sequence_length = ctypes.cast(sla, ctypes.c_void_p)
    a.max_time, a.batch_size, a.num_classes = shape
    a.inputs_dims, a.sequence_length_dims, a.sequence_length_size = dims, 1, len(sl)
    a.beam_width, a.top_paths, a.blank_index, a.blank_label = W, P, blank, -1
    a.inputs_format = fmt
    a.inputs_stride_t, a.inputs_stride_b = st
    return a, (buf, sla)


def _validate(a):
    lib = _lib.load()
    rc = lib.ctcext_validate(ctypes.byref(a))
    return rc, lib.ctcext_last_error().decode()


def test_abi_version_and_constants():
    assert _lib.CTCEXT_ABI_VERSION == 8 == _lib.load().ctcext_abi_version()
    assert (_lib.CTCEXT_IN_NATIVE, _lib.CTCEXT_IN_F16, _lib.CTCEXT_IN_BF16) == (0, 1, 2)
    # appended: every earlier field keeps its offset
    assert _lib.DecodeArgs.inputs_format.offset > _lib.DecodeArgs.scorer_table.offset
    assert _lib.DecodeArgs.inputs_stride_b.offset + 8 == ctypes.sizeof(_lib.DecodeArgs)


def test_zeroed_fields_accept_as_before():
    for dtype in (_lib.CTCEXT_F32, _lib.CTCEXT_F64):
        a, keep = _args(dtype=dtype)
        assert _validate(a) == (_lib.CTCEXT_OK, "")


@pytest.mark.parametrize("kw", [
    dict(fmt=_lib.CTCEXT_IN_F16), dict(fmt=_lib.CTCEXT_IN_BF16),
    dict(st=(8, 4)),                       # the dense layout, spelled out
    dict(st=(4, 12)),                      # batch-major dense
    dict(st=(15, 45), fmt=_lib.CTCEXT_IN_BF16),   # a vocabulary slice of [B, T, 15]
    dict(st=(4, 4)),                       # overlapping rows are still addressable
    dict(shape=(1, 2, 4), sl=(1, 1), st=(1, 4)),   # extent 1: its stride addresses nothing
    dict(shape=(3, 1, 4), sl=(3,), st=(4, -7)),
    dict(dtype=_lib.CTCEXT_F64, st=(4, 12)),
])
def test_new_fields_accepted(kw):
    a, keep = _args(**kw)
    assert _validate(a) == (_lib.CTCEXT_OK, "")


@pytest.mark.parametrize("kw,msg", [
    (dict(fmt=3), M_FORMAT),
    (dict(fmt=-1), M_FORMAT),
    (dict(fmt=_lib.CTCEXT_IN_F16, dtype=_lib.CTCEXT_F64), M_HALF),
    (dict(fmt=_lib.CTCEXT_IN_BF16, dtype=_lib.CTCEXT_F64), M_HALF),
    (dict(st=(8, 0)), M_PAIR),
    (dict(st=(0, 4)), M_PAIR),
    (dict(st=(3, 12)), M_ST),
    (dict(st=(-8, 12)), M_ST),
    (dict(st=(8, 3)), M_SB),
    # in this order when several are wrong
    (dict(fmt=9, dtype=_lib.CTCEXT_F64, st=(1, 0)), M_FORMAT),
    (dict(fmt=_lib.CTCEXT_IN_F16, dtype=_lib.CTCEXT_F64, st=(1, 0)), M_HALF),
    (dict(st=(1, 1)), M_ST),
])
def test_new_errors(kw, msg):
    a, keep = _args(**kw)
    assert _validate(a) == (_lib.CTCEXT_INVALID_ARGUMENT, msg)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(dtype=7), _lib.CTCEXT_INVALID_ARGUMENT, "dtype must be float32 or float64"),
    (dict(W=0), _lib.CTCEXT_INVALID_ARGUMENT, "Value for attr 'beam_width' of 0 must be at least minimum 1"),
    (dict(dims=2), _lib.CTCEXT_INVALID_ARGUMENT, "inputs is not a 3-Tensor"),
    (dict(shape=(0, 2, 4)), _lib.CTCEXT_INVALID_ARGUMENT, "max_time is 0"),
    (dict(sl=(3,)), _lib.CTCEXT_FAILED_PRECONDITION,
     "len(sequence_length) != batch_size.  len(sequence_length):  1 batch_size: 2"),
    (dict(sl=(3, 4)), _lib.CTCEXT_FAILED_PRECONDITION, "sequence_length(1) <= 3"),
    (dict(blank=4), _lib.CTCEXT_INVALID_ARGUMENT, "blank_index out of range [0, num_classes)"),
    (dict(W=2, P=3), _lib.CTCEXT_INVALID_ARGUMENT, "requested more paths than the beam width."),
])
@pytest.mark.parametrize("new", [dict(fmt=5), dict(st=(1, 0)), dict(st=(1, 1), fmt=_lib.CTCEXT_IN_F16)])
def test_existing_errors_win(kw, code, msg, new):
    """The new checks come after every existing one: with an old and a new
    error in the same struct the old message is reported, as before."""
    merged = dict(new)
    merged.update(kw)
    a, keep = _args(**merged)
    assert _validate(a) == (code, msg)


# ---------------------------------------------------------------------------
# decode_logits' layout decision

B, T, C = 3, 5, 7


def _layout(t, batch_first):
    return logits_layout(tuple(t.shape), t.stride(), batch_first)


def test_layout_dense_time_major():
    t = torch.zeros(T, B, C, dtype=torch.bfloat16)
    assert _layout(t, False) == (False, (T, B, C), B * C, C)


def test_layout_dense_batch_major():
    t = torch.zeros(B, T, C, dtype=torch.float16)
    assert _layout(t, True) == (False, (T, B, C), C, T * C)


def test_layout_transpose_view():
    t = torch.zeros(B, T, C).transpose(0, 1)   # [T, B, C] over batch-major storage
    assert not t.is_contiguous()
    assert _layout(t, False) == (False, (T, B, C), C, T * C)
    u = torch.zeros(T, B, C).transpose(0, 1)   # [B, T, C] over time-major storage
    assert _layout(u, True) == (False, (T, B, C), B * C, C)


def test_layout_vocabulary_slice():
    big = torch.zeros(B, T, C + 11)
    t = big[:, :, :C]
    assert not t.is_contiguous()
    assert _layout(t, True) == (False, (T, B, C), C + 11, T * (C + 11))
    assert _layout(big[:, :, 4:4 + C], True) == (False, (T, B, C), C + 11, T * (C + 11))


def test_layout_class_stride_forces_copy():
    t = torch.zeros(B, C, T).transpose(1, 2)   # [B, T, C] with stride(-1) == T
    assert t.stride(-1) != 1
    assert _layout(t, True) == (True, (T, B, C), C, T * C)
    assert _layout(torch.zeros(B, T, 2 * C)[:, :, ::2], True) == (True, (T, B, C), C, T * C)


def test_layout_expanded_view_forces_copy():
    t = torch.zeros(1, T, C).expand(B, T, C)   # stride 0 over the batch
    assert _layout(t, True) == (True, (T, B, C), C, T * C)


def test_layout_extent_one_takes_dense_stride():
    t = torch.zeros(4, T, C)[1:2]              # B == 1: whatever stride torch reports is unused
    copy, shape, st_t, st_b = _layout(t, True)
    assert (copy, shape, st_t) == (False, (T, 1, C), C) and st_b >= C
    assert _layout(torch.zeros(B, 1, C), True) == (False, (1, B, C), C, C)
    assert _layout(torch.zeros(1, 1, C), True) == (False, (1, 1, C), C, C)


def test_layout_numpy_strides_in_elements():
    x = np.zeros((B, T, C + 1), np.float16)[:, :, :C]
    st = tuple(s // x.itemsize for s in x.strides)
    assert logits_layout(x.shape, st, True) == (False, (T, B, C), C + 1, T * (C + 1))


def test_decode_logits_type_errors_and_dropin_unchanged():
    with pytest.raises(TypeError) as e:
        ctcext_amd.decode_logits(np.zeros((1, 3, 4), np.int32), [3], 2, 1)
    assert "float16, bfloat16, float32, float64" in str(e.value)
    with pytest.raises(TypeError):
        ctcext_amd.decode_logits(torch.zeros(1, 3, 4, dtype=torch.int64), [3], 2, 1)
    # the drop-in still registers float and double only
    with pytest.raises(TypeError):
        ctcext_amd.ctc_ext_beam_search_decoder(np.zeros((3, 1, 4), np.float16), [3], 2, 1)
    with pytest.raises(TypeError):
        ctcext_amd.ctc_ext_beam_search_decoder(torch.zeros(3, 1, 4, dtype=torch.bfloat16), [3], 2, 1)


def test_decode_logits_shape_errors_before_device_work():
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.decode_logits(torch.zeros(3, 4, dtype=torch.bfloat16), [3], 2, 1)
    assert e.value.message == "inputs is not a 3-Tensor"
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.decode_logits(np.zeros((2, 3, 4), np.float16), [3, 4], 2, 1)
    assert e.value.message == "sequence_length(1) <= 3"
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.decode_logits(np.zeros((2, 3, 4), np.float16), [3, 4], 2, 1, batch_first=False)
    assert e.value.message == "len(sequence_length) != batch_size.  len(sequence_length):  2 batch_size: 3"
