"""``ctc_ext_beam_search_decoder`` — the reference's Python op, on MI355X.

Same signature, argument meaning, output structure and error messages as the
TF-generated wrapper the reference exports
(python/ops/ctc_ext_beam_search_decoder_ops.py:12, op definition
cc/ops/ctc_ext_beam_search_decoder_ops.cc:9-63):

    ctc_ext_beam_search_decoder(inputs, sequence_length, beam_width, top_paths,
                                merge_repeated=False, blank_index=0,
                                blank_label=-1, name=None)
      -> (decoded_indices, decoded_values, decoded_shape,
          alignment_indices, alignment_values, alignment_shape,
          log_probability)

The six list outputs are Python lists of ``top_paths`` int64 arrays (the
SparseTensor components of kernels.cc:163-257); ``log_probability`` is
[batch_size, top_paths] of the input dtype.  Host inputs (numpy, lists, CPU
torch tensors) give numpy outputs; device (HBM) torch tensors give device
torch tensors.  Decoding always runs on the GPU through libctcext.so.

``decode_dense`` is the enqueue-only form for GPU logits: padded
``[B, top_paths, T]`` tensors instead of SparseTensor components, no host
synchronisation, data-dependent errors deferred to ``dense_check``.
"""
import collections
import ctypes
import threading
import warnings

import numpy as np

from . import _lib

CTCExtBeamSearchDecoder = collections.namedtuple(
    "CTCExtBeamSearchDecoder",
    ["decoded_indices", "decoded_values", "decoded_shape",
     "alignment_indices", "alignment_values", "alignment_shape",
     "log_probability"])


class OpError(Exception):
    """Mirror of tf.errors.OpError: ``.message`` holds the reference's text."""

    def __init__(self, message, code):
        super().__init__(message)
        self.message = message
        self.error_code = code


class InvalidArgumentError(OpError):
    pass


class FailedPreconditionError(OpError):
    pass


class UnimplementedError(OpError):
    pass


class InternalError(OpError):
    pass


_ERRORS = {_lib.CTCEXT_INVALID_ARGUMENT: InvalidArgumentError,
           _lib.CTCEXT_FAILED_PRECONDITION: FailedPreconditionError,
           _lib.CTCEXT_UNIMPLEMENTED: UnimplementedError,
           _lib.CTCEXT_INTERNAL: InternalError}

_tls = threading.local()


def _raise(lib, rc):
    msg = lib.ctcext_last_error().decode()
    raise _ERRORS.get(rc, InternalError)(msg, rc)


class Decoder:
    """One libctcext handle (device workspace + HIP stream per device) per
    device set and thread, like one OpKernel instance per device.  With more
    than one device the handle decodes contiguous batch shards on each and
    assembles the outputs on ``devices[0]`` (ctcext_create_sharded)."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        devs = tuple(int(d) for d in (device if isinstance(device, (tuple, list)) else (device,)))
        h = ctypes.c_void_p()
        if len(devs) == 1:
            rc = self.lib.ctcext_create(devs[0], ctypes.byref(h))
        else:
            arr = (ctypes.c_int * len(devs))(*devs)
            rc = self.lib.ctcext_create_sharded(arr, len(devs), ctypes.byref(h))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)
        self.handle = h
        self.devices = devs
        self.device = devs[0]
        self.last_stats = None

    def close(self):
        if self.handle:
            self.lib.ctcext_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        s = _lib.Stats()
        _lib.get_stats(self.lib, self.handle, s)
        st = {k: getattr(s, k) for k, _ in _lib.Stats._fields_}
        # "kernel" decoded into named fields (the raw value stays as "kernel_raw")
        st["kernel_raw"] = st["kernel"]
        st["kernel"] = _lib.decode_kernel_stat(st["kernel_raw"])
        return st

    # -- phase 1 ---------------------------------------------------------
    def decode(self, args, skip=None):
        P = max(int(args.top_paths), 1)
        sizes = (_lib.PathSizes * P)()
        if skip is None:
            rc = self.lib.ctcext_decode_sharded(self.handle, ctypes.byref(args), sizes)
        else:   # a _lib.SkipArgs: blank-frame skipping
            rc = self.lib.ctcext_decode_skip(self.handle, ctypes.byref(args), ctypes.byref(skip), sizes)
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)
        self.last_stats = self.stats()
        if self.last_stats.get("helper_redecodes", 0) > 0:
            # a two-wave kernel's hand-over wait ran out of time (never in a
            # correct run): the outputs are right, decoded again by the
            # one-wave kernels, but the call took up to ~2x its time
            warnings.warn("ctc_ext_beam_search_decoder: a helper-wave hand-over wait timed out; the call was "
                          "decoded again with the one-wave kernels (ctcext_stats.helper_redecodes = %d)"
                          % self.last_stats["helper_redecodes"], RuntimeWarning, stacklevel=3)
        return [(s.num_decoded, s.max_decoded, s.num_alignment, s.max_alignment) for s in sizes]

    # -- phase 2 ---------------------------------------------------------
    def fetch(self, ptr_lists, log_prob_ptr, on_device):
        P = len(ptr_lists[0])
        arrs = [(ctypes.c_void_p * P)(*pl) for pl in ptr_lists]
        o = _lib.Outputs()
        o.outputs_on_device = 1 if on_device else 0
        o.decoded_indices, o.decoded_values, o.decoded_shape = arrs[0], arrs[1], arrs[2]
        o.alignment_indices, o.alignment_values, o.alignment_shape = arrs[3], arrs[4], arrs[5]
        o.log_probability = log_prob_ptr
        rc = self.lib.ctcext_fetch(self.handle, ctypes.byref(o))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)


def get_decoder(device=0):
    """The calling thread's handle for ``device`` (an ordinal, or a tuple of
    ordinals for a sharded multi-device handle)."""
    cache = getattr(_tls, "decoders", None)
    if cache is None:
        cache = _tls.decoders = {}
    key = tuple(device) if isinstance(device, (tuple, list)) else int(device)
    d = cache.get(key)
    if d is None:
        d = cache[key] = Decoder(key)
    return d


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _print_no_label(n):
    # ctc_beam_entry.h:148-150 prints once per path without any candidate
    for _ in range(int(n)):
        print("No label seq available")


def _type_error(name, got, allowed):
    # the message TF's op wrapper raises for a dtype outside the op's type list
    # (ops.cc:17-18: T in {float, double}; sequence_length: int32)
    raise TypeError("Value passed to parameter '%s' has DataType %s not in list of allowed values: %s"
                    % (name, got, allowed))


def _current_device():
    try:
        import torch
        if torch.cuda.is_available():
            return torch.cuda.current_device()
    except ImportError:
        pass
    return 0


def _skip_args(lib, skip_blank):
    """The ctcext_skip_args of ``skip_blank`` (a log-probability threshold),
    checked on the host; its ``kept`` pointer is left to the caller."""
    if not hasattr(lib, "ctcext_decode_skip"):
        raise UnimplementedError("this libctcext.so has no blank-frame skipping (CTCEXT_HAS_BLANK_SKIP)",
                                 _lib.CTCEXT_UNIMPLEMENTED)
    k = _lib.SkipArgs()
    k.logp_threshold = float(skip_blank)
    rc = lib.ctcext_skip_validate(ctypes.byref(k))
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return k


def _args(x_ptr, shape, dtype_code, on_device, sl_ptr, sl_shape, beam_width, top_paths, merge_repeated,
          blank_index, blank_label, flags, stream):
    a = _lib.DecodeArgs()
    a.dtype = dtype_code
    a.inputs_on_device = 1 if on_device else 0
    a.inputs = x_ptr
    a.sequence_length = sl_ptr
    dims = list(shape) + [0, 0, 0]
    a.max_time, a.batch_size, a.num_classes = int(dims[0]), int(dims[1]), int(dims[2])
    a.inputs_dims = len(shape)
    a.sequence_length_dims = len(sl_shape)
    a.sequence_length_size = int(sl_shape[0]) if len(sl_shape) >= 1 else 0
    a.beam_width = int(beam_width)
    a.top_paths = int(top_paths)
    a.merge_repeated = 1 if merge_repeated else 0
    a.blank_index = int(blank_index)
    a.blank_label = int(blank_label)
    a.flags = int(flags)
    a.stream = stream
    return a


def ctc_ext_beam_search_decoder(inputs, sequence_length, beam_width, top_paths,
                                merge_repeated=False, blank_index=0, blank_label=-1,
                                name=None, *, flags=0, outputs="auto", devices=None, scorer_table=None,
                                skip_blank=None, token_scores=False):
    """Drop-in for the reference op.  See the module docstring.

    Keyword-only extensions (not in the reference):
      outputs: "auto" (device tensors for device inputs, numpy for host
        inputs), "host" (numpy, copied from the GPU into pinned host memory;
        the reference op's own output placement) or "device".
      devices: a list of device ordinals to decode contiguous batch shards on,
        in one process (ctcext_create_sharded); device inputs must live on
        devices[0], where the outputs are assembled.
      scorer_table: a [num_classes + 1, num_classes] table of log-probabilities
        (<= 0) for the decoder's beam-scorer hook (util/ctc_beam_scorer.h:31-65):
        expanding a beam that ends in label a (row 0: the empty beam) by label
        b adds table[a + 1, b] to the score it extends.  The reference op
        always uses the identity scorer (kernels.cc:260), which None selects.
      flags: CTCEXT_FLAG_* diagnostics.
      skip_blank: None, or a log-probability threshold (<= 0) for blank-frame
        skipping (include/ctcext.h, "Blank-frame skipping"): a frame whose
        blank log-probability is above it, directly after another such frame,
        is dropped before the decode.  The outputs are the decode's of the
        kept frames, with the alignments put back on the original time axis
        (dropped frames read blank_label); log_probability is that of the kept
        frames, not corrected for the dropped ones.  ``kept_frames()`` returns
        the frames kept per item.  One device only.
      token_scores: True keeps what ``token_scores()`` reads after this call:
        for device inputs a reference to the tensor the kernels read (which
        may be a contiguous copy of ``inputs``), until the calling thread's
        next decode on that device.  Without it ``token_scores()`` raises
        ``FailedPreconditionError``.  One device only.
    """
    del name
    if outputs not in ("auto", "host", "device"):
        raise ValueError("outputs must be 'auto', 'host' or 'device'")
    lib = _lib.load()
    keep = []   # arrays whose memory the C call reads
    on_device = _is_torch(inputs) and inputs.is_cuda
    if on_device:
        import torch
        if inputs.dtype not in (torch.float32, torch.float64):
            _type_error("inputs", str(inputs.dtype).replace("torch.", ""), "float32, float64")
        x = inputs.contiguous()
        dev = x.device
        sl = _lengths_device(sequence_length, dev)
        keep += [x, sl]
        shape, sl_shape = tuple(x.shape), tuple(sl.shape)
        code = _lib.CTCEXT_F32 if x.dtype == torch.float32 else _lib.CTCEXT_F64
        x_ptr, sl_ptr = x.data_ptr(), sl.data_ptr()
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        stream = torch.cuda.current_stream(dev).cuda_stream
    else:
        if _is_torch(inputs):
            inputs = inputs.detach().cpu().numpy()
        if isinstance(inputs, np.ndarray):
            if inputs.dtype not in (np.float32, np.float64):
                _type_error("inputs", inputs.dtype.name, "float32, float64")
            x = np.ascontiguousarray(inputs)
        else:   # Python numbers convert to float32, as tf.convert_to_tensor does
            x = np.ascontiguousarray(np.asarray(inputs, dtype=np.float32))
        sl = _lengths_host(sequence_length)
        keep += [x, sl]
        shape, sl_shape = x.shape, sl.shape
        code = _lib.CTCEXT_F32 if x.dtype == np.float32 else _lib.CTCEXT_F64
        x_ptr, sl_ptr = x.ctypes.data, sl.ctypes.data
        index = None
        stream = None
    a = _args(x_ptr, shape, code, on_device, sl_ptr, sl_shape, beam_width, top_paths, merge_repeated,
              blank_index, blank_label, flags, stream)
    return _decode_and_fetch(lib, a, keep, shape, on_device, x.device if on_device else None,
                             x.dtype if on_device else np.dtype(x.dtype), index, outputs, devices, scorer_table,
                             skip_blank, token_scores)


def logits_layout(shape, strides, batch_first=True):
    """The stride/contiguity decision of ``decode_logits``, on plain numbers:
    ``shape`` and ``strides`` (in elements) of a 3-D logits tensor, batch-major
    ``[B, T, C]`` with ``batch_first`` else time-major ``[T, B, C]``.

    Returns ``(copy, (max_time, batch, num_classes), stride_t, stride_b)``.
    ``copy`` is False when the C ABI can address the tensor in place: classes
    contiguous (``strides[-1] == 1``) and, on every dimension of extent > 1, a
    stride of at least ``num_classes`` (an expanded or reversed view has to be
    materialised).  With ``copy`` the strides returned are those of the dense
    copy in the same dimension order; the stride of a dimension of extent 1
    is the dense one."""
    d0, d1, C = (int(v) for v in shape)
    s0, s1, sc = (int(v) for v in strides)
    copy = sc != 1 or (d0 > 1 and s0 < C) or (d1 > 1 and s1 < C)
    if copy:
        s0, s1 = d1 * C, C
    elif d0 <= 1 and d1 <= 1:
        s0 = s1 = C
    elif d1 <= 1:
        s1 = C
    elif d0 <= 1:
        s0 = d1 * s1
    if batch_first:
        return copy, (d1, d0, C), s1, s0
    return copy, (d0, d1, C), s0, s1


def decode_logits(logits, lengths, beam_width, top_paths, *, batch_first=True,
                  merge_repeated=False, blank_index=0, blank_label=-1,
                  flags=0, outputs="auto", devices=None, scorer_table=None, skip_blank=None, token_scores=False):
    """Decode the logits tensor an acoustic model produces, as it is.

    ``logits`` is a torch tensor of dtype float16, bfloat16, float32 or
    float64, on the GPU or the host, or a numpy float16 / float32 / float64
    array; ``[B, T, C]`` with ``batch_first`` (the default), else ``[T, B, C]``.
    It may be a view (a vocabulary slice, a transpose, a padded batch): when
    its classes are contiguous (``logits.stride(-1) == 1``) the kernels read
    it in place through its strides and nothing is copied or converted;
    otherwise it is made contiguous first.  Half-precision logits are widened
    to float32 as the kernels read them, which is exact: the result is that of
    ``ctc_ext_beam_search_decoder(logits.float().transpose(0, 1), ...)``, and
    ``log_probability`` is float32.  The other arguments (``skip_blank`` and
    ``token_scores`` among them) and the returned ``CTCExtBeamSearchDecoder``
    tuple are the drop-in function's.
    """
    if outputs not in ("auto", "host", "device"):
        raise ValueError("outputs must be 'auto', 'host' or 'device'")
    lib = _lib.load()
    allowed = "float16, bfloat16, float32, float64"
    if _is_torch(logits):
        import torch
        formats = {torch.float16: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_F16),
                   torch.bfloat16: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_BF16),
                   torch.float32: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_NATIVE),
                   torch.float64: (_lib.CTCEXT_F64, _lib.CTCEXT_IN_NATIVE)}
        if logits.dtype not in formats:
            _type_error("logits", str(logits.dtype).replace("torch.", ""), allowed)
        x = logits.detach()
        strides = x.stride()
    else:
        x = logits if isinstance(logits, np.ndarray) else np.asarray(logits, dtype=np.float32)
        formats = {np.dtype(np.float16): (_lib.CTCEXT_F32, _lib.CTCEXT_IN_F16),
                   np.dtype(np.float32): (_lib.CTCEXT_F32, _lib.CTCEXT_IN_NATIVE),
                   np.dtype(np.float64): (_lib.CTCEXT_F64, _lib.CTCEXT_IN_NATIVE)}
        if x.dtype not in formats:
            _type_error("logits", x.dtype.name, allowed)
        strides = tuple(s // x.itemsize if s % x.itemsize == 0 else 0 for s in x.strides)
    code, fmt = formats[x.dtype]
    if len(x.shape) == 3:
        copy, shape, st_t, st_b = logits_layout(tuple(x.shape), strides, batch_first)
        if copy:
            x = x.contiguous() if _is_torch(x) else np.ascontiguousarray(x)
    else:   # the C ABI raises the reference's "inputs is not a 3-Tensor"
        x = x.contiguous() if _is_torch(x) else np.ascontiguousarray(x)
        shape, st_t, st_b = tuple(x.shape), 0, 0
    on_device = _is_torch(x) and x.is_cuda
    if on_device:
        dev = x.device
        sl = _lengths_device(lengths, dev)
        x_ptr, sl_ptr = x.data_ptr(), sl.data_ptr()
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        stream = torch.cuda.current_stream(dev).cuda_stream
        table_dtype = torch.float32 if code == _lib.CTCEXT_F32 else torch.float64
    else:
        dev = None
        sl = _lengths_host(lengths)
        # (a CPU torch tensor is read where it lies: numpy has no bfloat16)
        x_ptr, sl_ptr = (x.data_ptr() if _is_torch(x) else x.ctypes.data), sl.ctypes.data
        index = stream = None
        table_dtype = np.dtype(np.float32 if code == _lib.CTCEXT_F32 else np.float64)
    a = _args(x_ptr, shape, code, on_device, sl_ptr, tuple(sl.shape), beam_width, top_paths, merge_repeated,
              blank_index, blank_label, flags, stream)
    a.inputs_format = fmt
    a.inputs_stride_t, a.inputs_stride_b = int(st_t), int(st_b)
    return _decode_and_fetch(lib, a, [x, sl], shape, on_device, dev, table_dtype, index, outputs, devices,
                             scorer_table, skip_blank, token_scores)


DenseDecode = collections.namedtuple(
    "DenseDecode",
    ["decoded", "decoded_lengths", "alignment", "alignment_lengths", "log_probability", "status"])


def decode_dense(logits, lengths, beam_width, top_paths, *, batch_first=True,
                 merge_repeated=False, blank_index=0, blank_label=-1, pad_value=-1,
                 flags=0, scorer_table=None, out=None, skip_blank=None, token_scores=False):
    """Decode GPU logits into padded GPU tensors without waiting for anything.

    The call validates what it can on the host, enqueues the whole decode on
    ``torch.cuda.current_stream()`` and returns: no ``synchronize()``, no
    ``.item()``, no ``.cpu()``.  It can be queued behind the acoustic model
    and captured into a ``torch.cuda.graph`` (after one call, or a
    ``ctcext_dense_reserve``, of the same shape has sized the workspace).

    ``logits`` is a CUDA torch tensor, with the dtypes, strides and in-place
    rules of ``decode_logits`` (a host tensor raises ``ValueError``: use
    ``decode_logits`` for those).  ``lengths`` should be an int32 CUDA tensor;
    any other form is converted, and that conversion copies and may block.
    ``scorer_table`` must be a CUDA tensor.

    Returns ``DenseDecode(decoded, decoded_lengths, alignment,
    alignment_lengths, log_probability, status)``: ``decoded`` and
    ``alignment`` are int64 ``[B, top_paths, T]``, row ``[b, p]`` holding path
    ``p``'s labels in its first ``decoded_lengths[b, p]`` (``alignment_lengths
    [b, p]``) elements and ``pad_value`` in the rest; the lengths are int32
    ``[B, top_paths]``, ``log_probability`` ``[B, top_paths]`` of the compute
    dtype, ``status`` int32 ``[B]``.  The tensors come from torch's caching
    allocator on the current stream; ``out`` (a ``DenseDecode`` of contiguous
    CUDA tensors of those shapes and dtypes) is written instead when given.

    Errors that depend on the data are deferred.  ``status[b]`` is 0 for a
    good item, else ``CTCEXT_ITEM_*`` bits (``_lib``): such an item has all
    its rows empty -- lengths 0, rows all ``pad_value``, ``log_probability``
    ``-inf`` -- and the other items are untouched by it.  ``dense_check()``
    waits and raises what the synchronous call would have raised.

    ``skip_blank`` is ``ctc_ext_beam_search_decoder``'s: with it the call is
    still enqueue-only, alignment rows stay ``T`` wide, and ``kept_frames()``
    returns an int32 CUDA tensor this call writes without waiting.

    ``token_scores=True`` keeps a reference to the tensor the kernels read
    (``logits`` itself, or the contiguous copy made of it) until the calling
    thread's next decode on that device, so that ``dense_token_scores()`` can
    read it; without it that call raises ``FailedPreconditionError``.  In a
    captured graph the scores read the static input the decode read.
    """
    lib = _lib.load()
    skip = None if skip_blank is None else _skip_args(lib, skip_blank)
    if not (_is_torch(logits) and logits.is_cuda):
        raise ValueError("decode_dense takes CUDA torch tensors; use decode_logits for host inputs")
    import torch
    formats = {torch.float16: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_F16),
               torch.bfloat16: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_BF16),
               torch.float32: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_NATIVE),
               torch.float64: (_lib.CTCEXT_F64, _lib.CTCEXT_IN_NATIVE)}
    if logits.dtype not in formats:
        _type_error("logits", str(logits.dtype).replace("torch.", ""), "float16, bfloat16, float32, float64")
    code, fmt = formats[logits.dtype]
    x = logits.detach()
    if x.dim() == 3:
        copy, shape, st_t, st_b = logits_layout(tuple(x.shape), x.stride(), batch_first)
        if copy:
            x = x.contiguous()
    else:   # the C ABI raises the reference's "inputs is not a 3-Tensor"
        x = x.contiguous()
        shape, st_t, st_b = tuple(x.shape), 0, 0
    dev = x.device
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    sl = _lengths_device(lengths, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if not stream:   # torch's legacy default stream: the null stream itself, not the decoder's own
        flags = int(flags) | _lib.CTCEXT_FLAG_DENSE_NULL_STREAM
    a = _args(x.data_ptr(), shape, code, True, sl.data_ptr(), tuple(sl.shape), beam_width, top_paths,
              merge_repeated, blank_index, blank_label, flags, stream)
    a.inputs_format = fmt
    a.inputs_stride_t, a.inputs_stride_b = int(st_t), int(st_b)
    fdt = torch.float32 if code == _lib.CTCEXT_F32 else torch.float64
    tab = None
    if scorer_table is not None:
        if not (_is_torch(scorer_table) and scorer_table.is_cuda):
            raise ValueError("decode_dense: scorer_table must be a CUDA torch tensor")
        C = int(shape[2]) if len(shape) == 3 else 0
        tab = scorer_table.detach().to(device=dev, dtype=fdt).contiguous()
        if tuple(tab.shape) != (C + 1, C):
            raise ValueError("scorer_table must be [num_classes + 1, num_classes] = [%d, %d], got %s"
                             % (C + 1, C, tuple(tab.shape)))
        a.scorer = _lib.CTCEXT_SCORER_BIGRAM
        a.scorer_table = tab.data_ptr()
    # every check that needs no data, on the host, before anything is allocated
    rc = lib.ctcext_validate(ctypes.byref(a))
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    T, B, P = int(shape[0]), int(shape[1]), int(top_paths)
    want = (((B, P, T), torch.int64), ((B, P), torch.int32), ((B, P, T), torch.int64), ((B, P), torch.int32),
            ((B, P), fdt), ((B,), torch.int32))
    if out is None:
        with torch.cuda.device(dev):
            out = DenseDecode(*[torch.empty(s, dtype=dt, device=dev) for s, dt in want])
    else:
        out = DenseDecode(*out)
        for name, t, (s, dt) in zip(DenseDecode._fields, out, want):
            if not (_is_torch(t) and t.is_cuda and t.device == dev and tuple(t.shape) == s and t.dtype == dt
                    and t.is_contiguous()):
                raise ValueError("out.%s must be a contiguous %s tensor of shape %s on %s"
                                 % (name, str(dt).replace("torch.", ""), s, dev))
    o = _lib.DenseOutputs()
    (o.decoded, o.decoded_length, o.alignment, o.alignment_length, o.log_probability,
     o.status) = [t.data_ptr() for t in out]
    o.pad_value = int(pad_value)
    dec = get_decoder(index)
    dec._scores_keep = dec._scores_dense = dec._scores_sync = None
    if skip is None:
        rc = lib.ctcext_decode_dense(dec.handle, ctypes.byref(a), ctypes.byref(o))
    else:
        with torch.cuda.device(dev):
            kept = torch.empty((B,), dtype=torch.int32, device=dev)
        skip.kept = kept.data_ptr()
        rc = lib.ctcext_decode_dense_skip(dec.handle, ctypes.byref(a), ctypes.byref(skip), ctypes.byref(o))
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    dec._kept = None if skip is None else kept
    dec.last_stats = dec.stats()
    dec._times_dense = (B, P, T, dev)   # (dense_token_times' output shapes)
    if token_scores:   # (dense_token_scores' output shapes and dtype, and the rows its kernel reads)
        dec._scores_keep = x
        dec._scores_dense = (B, P, T, dev, fdt)
        dec._scores_batch_first = bool(batch_first) and x.dim() == 3   # (dense_target_grads' slab follows it)
    # x, sl and tab may be temporaries: they were allocated on this stream, and
    # the caching allocator hands their memory out again in stream order
    del x, sl, tab
    return out


def _greedy_lib(lib):
    if not hasattr(lib, "ctcext_decode_greedy"):
        raise UnimplementedError("this libctcext.so has no greedy decode (CTCEXT_HAS_GREEDY)",
                                 _lib.CTCEXT_UNIMPLEMENTED)
    return lib


def decode_greedy(logits, lengths, *, batch_first=True, merge_repeated=False, blank_index=0, blank_label=-1,
                  pad_value=-1, flags=0, out=None, token_scores=False):
    """The best-path ("greedy") decode of GPU logits into padded GPU tensors,
    without waiting for anything: per frame the class of the largest logit
    (the lowest index of a tie), repeats and blanks collapsed, and with
    ``merge_repeated`` a label equal to the one before it in the collapsed row
    dropped as the op drops it.  Two kernels read the logits once, where the
    beam search walks a serial chain per item: use it for partial results
    between beam decodes, as a first pass, or for large vocabularies.

    ``logits``, ``lengths``, ``out`` and the deferred errors are
    ``decode_dense``'s (CUDA torch tensors, its dtypes, strides and in-place
    rules; a host tensor raises ``ValueError``), the call is enqueued on
    ``torch.cuda.current_stream()`` and can be captured into a
    ``torch.cuda.graph`` after one call of the shape.  Returns ``DenseDecode``
    with ``top_paths`` 1: ``alignment`` row ``[b, 0]`` holds the item's frames
    (``blank_label`` at a blank frame), ``log_probability`` the best path's
    log-probability under the decoder's own normaliser.  The definition is in
    ``include/ctcext.h``, "Greedy decode" (``greedy_row`` on the host).

    ``dense_check``, ``dense_token_times``, ``dense_token_scores``,
    ``dense_path_scores`` and ``dense_path_alignments`` follow it as they
    follow ``decode_dense`` (the last three with ``token_scores=True``)."""
    lib = _greedy_lib(_lib.load())
    if not (_is_torch(logits) and logits.is_cuda):
        raise ValueError("decode_greedy takes CUDA torch tensors")
    import torch
    formats = {torch.float16: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_F16),
               torch.bfloat16: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_BF16),
               torch.float32: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_NATIVE),
               torch.float64: (_lib.CTCEXT_F64, _lib.CTCEXT_IN_NATIVE)}
    if logits.dtype not in formats:
        _type_error("logits", str(logits.dtype).replace("torch.", ""), "float16, bfloat16, float32, float64")
    code, fmt = formats[logits.dtype]
    x = logits.detach()
    if x.dim() == 3:
        copy, shape, st_t, st_b = logits_layout(tuple(x.shape), x.stride(), batch_first)
        if copy:
            x = x.contiguous()
    else:   # the C ABI raises the reference's "inputs is not a 3-Tensor"
        x = x.contiguous()
        shape, st_t, st_b = tuple(x.shape), 0, 0
    dev = x.device
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    sl = _lengths_device(lengths, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if not stream:   # torch's legacy default stream: the null stream itself, not the decoder's own
        flags = int(flags) | _lib.CTCEXT_FLAG_DENSE_NULL_STREAM
    a = _args(x.data_ptr(), shape, code, True, sl.data_ptr(), tuple(sl.shape), 1, 1, merge_repeated, blank_index,
              blank_label, flags, stream)
    a.inputs_format = fmt
    a.inputs_stride_t, a.inputs_stride_b = int(st_t), int(st_b)
    fdt = torch.float32 if code == _lib.CTCEXT_F32 else torch.float64
    # every check that needs no data, on the host, before anything is allocated
    rc = lib.ctcext_validate(ctypes.byref(a))
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    T, B = int(shape[0]), int(shape[1])
    want = (((B, 1, T), torch.int64), ((B, 1), torch.int32), ((B, 1, T), torch.int64), ((B, 1), torch.int32),
            ((B, 1), fdt), ((B,), torch.int32))
    if out is None:
        with torch.cuda.device(dev):
            out = DenseDecode(*[torch.empty(s, dtype=dt, device=dev) for s, dt in want])
    else:
        out = DenseDecode(*out)
        for name, t, (s, dt) in zip(DenseDecode._fields, out, want):
            if not (_is_torch(t) and t.is_cuda and t.device == dev and tuple(t.shape) == s and t.dtype == dt
                    and t.is_contiguous()):
                raise ValueError("out.%s must be a contiguous %s tensor of shape %s on %s"
                                 % (name, str(dt).replace("torch.", ""), s, dev))
    o = _lib.DenseOutputs()
    (o.decoded, o.decoded_length, o.alignment, o.alignment_length, o.log_probability,
     o.status) = [t.data_ptr() for t in out]
    o.pad_value = int(pad_value)
    dec = get_decoder(index)
    dec._scores_keep = dec._scores_dense = dec._scores_sync = None
    rc = lib.ctcext_decode_greedy(dec.handle, ctypes.byref(a), ctypes.byref(o))
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    dec._kept = None
    dec.last_stats = dec.stats()
    dec._times_dense = (B, 1, T, dev)   # (the follow-up calls' state, as decode_dense sets it)
    if token_scores:
        dec._scores_keep = x
        dec._scores_dense = (B, 1, T, dev, fdt)
        dec._scores_batch_first = bool(batch_first) and x.dim() == 3
    del x, sl
    return out


def greedy_row(x, norm, frames, blank_index, blank_label=-1, merge_repeated=False):
    """The definition of the greedy decode for one item, on the host (no GPU),
    in the compute dtype: ``x`` is the item's logits ``[frames, num_classes]``
    (float32 or float64), ``norm`` its rows' normaliser ``[frames]``.  Returns
    ``(decoded, alignment, logp)``: two int64 arrays and a numpy scalar of
    ``x``'s dtype."""
    lib = _greedy_lib(_lib.load())
    x = np.asarray(x)
    dt = np.float64 if x.dtype == np.float64 else np.float32
    frames = int(frames)
    if x.ndim != 2:
        raise ValueError("greedy_row: x must be [frames, num_classes]")
    C = int(x.shape[1])
    x = np.ascontiguousarray(x[:frames], dtype=dt)
    nm = np.ascontiguousarray(np.asarray(norm).reshape(-1)[:frames], dtype=dt)
    if x.shape[0] != frames or nm.size != frames:
        raise ValueError("greedy_row: x and norm must hold the item's frames")
    dec, ali = np.empty((max(frames, 1),), np.int64), np.empty((max(frames, 1),), np.int64)
    nd, na = ctypes.c_int64(), ctypes.c_int64()
    logp = np.empty((1,), dt)
    rc = lib.ctcext_greedy_row(x.ctypes.data, nm.ctypes.data, 1 if dt == np.float64 else 0, frames, C,
                               int(blank_index), int(blank_label), 1 if merge_repeated else 0,
                               _ptr(dec, ctypes.c_int64), ctypes.byref(nd), _ptr(ali, ctypes.c_int64),
                               ctypes.byref(na), logp.ctypes.data)
    if rc != _lib.CTCEXT_OK:
        raise InvalidArgumentError("ctcext_greedy_row: bad arguments", rc)
    return dec[:nd.value].copy(), ali[:na.value].copy(), logp[0]


TokenTimes = collections.namedtuple("TokenTimes", ["start", "end", "trailing_blank"])
TokenScores = collections.namedtuple("TokenScores", ["logp_sum", "logp_min"])


def _times_lib(lib):
    if not hasattr(lib, "ctcext_dense_token_times"):
        raise UnimplementedError("this libctcext.so has no token times (CTCEXT_HAS_TOKEN_TIMES)",
                                 _lib.CTCEXT_UNIMPLEMENTED)
    return lib


def _thread_decoder(device, what):
    index = _device_index(device)
    if index is None:
        index = _current_device()
    dec = getattr(_tls, "decoders", {}).get(int(index))
    if dec is None:   # no handle yet on this thread: no decode either
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    return dec


def _times_device(dev, B, P, width):
    """Uninitialised CUDA outputs of a token-times call and their struct."""
    import torch
    with torch.cuda.device(dev):
        out = TokenTimes(torch.empty((B, P, width), dtype=torch.int32, device=dev),
                         torch.empty((B, P, width), dtype=torch.int32, device=dev),
                         torch.empty((B, P), dtype=torch.int32, device=dev))
    o = _lib.TokenTimesOut()
    o.start, o.end, o.trailing_blank = [t.data_ptr() for t in out]
    return out, o


def dense_token_times(device=None):
    """Start and end frames of every decoded token of the calling thread's
    last ``decode_dense`` on ``device`` (None: the current one), and the blank
    frames each best path ends in, without waiting for anything: one small
    kernel enqueued behind the decode, on the stream the decode went to (so it
    can be captured into the same ``torch.cuda.graph``).

    Returns ``TokenTimes(start, end, trailing_blank)``: int32 CUDA tensors,
    ``start`` and ``end`` ``[B, top_paths, T]`` and ``trailing_blank``
    ``[B, top_paths]``.  Token ``i`` of row ``[b, p]`` of ``decoded`` spans
    frames ``start[b, p, i]`` .. ``end[b, p, i]`` of item b (a token merged by
    ``merge_repeated`` spans the blanks between its runs).  Tokens the
    alignment does not reach, and everything past the row's decoded length, are
    -1; an item with a status bit has rows of -1 and ``trailing_blank`` 0.  The
    definition (``include/ctcext.h``, "Token times") needs a ``blank_label``
    that is no class label: ``InvalidArgumentError`` otherwise."""
    what = "ctcext_dense_token_times without a ctcext_decode_dense"
    dec = _thread_decoder(device, what)
    lib = _times_lib(dec.lib)
    shape = getattr(dec, "_times_dense", None)
    if shape is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, dev = shape
    out, o = _times_device(dev, B, P, T)
    rc = lib.ctcext_dense_token_times(dec.handle, ctypes.byref(o))
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return out


def token_times(device=None):
    """``dense_token_times`` for the synchronous calls: the token times of the
    hypotheses the calling thread's last ``ctc_ext_beam_search_decoder``,
    ``decode_logits`` or ``StreamDecoder.push`` on ``device`` returned.  Waits.
    Rows are ``max_time`` (``max_frames`` after a push) wide.  Returns numpy
    arrays, or CUDA tensors where that call's outputs were."""
    what = "ctcext_fetch_token_times without a successful ctcext_decode"
    dec = _thread_decoder(device, what)
    lib = _times_lib(dec.lib)
    shape = getattr(dec, "_times_sync", None)
    if shape is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, to_device = shape
    if to_device:
        import torch
        out, o = _times_device(torch.device("cuda", dec.device), B, P, T)
    else:
        out = TokenTimes(np.empty((B, P, T), np.int32), np.empty((B, P, T), np.int32), np.empty((B, P), np.int32))
        o = _lib.TokenTimesOut()
        o.start, o.end, o.trailing_blank = [t.ctypes.data for t in out]
    rc = lib.ctcext_fetch_token_times(dec.handle, ctypes.byref(o), 1 if to_device else 0)
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return out


def _scores_lib(lib):
    if not hasattr(lib, "ctcext_dense_token_scores"):
        raise UnimplementedError("this libctcext.so has no token scores (CTCEXT_HAS_TOKEN_SCORES)",
                                 _lib.CTCEXT_UNIMPLEMENTED)
    return lib


_NO_SCORES = "token scores need a decode with token_scores=True"


def _scores_device(dev, B, P, width, dtype):
    """Uninitialised CUDA outputs of a token-scores call and their struct."""
    import torch
    with torch.cuda.device(dev):
        out = TokenScores(torch.empty((B, P, width), dtype=dtype, device=dev),
                          torch.empty((B, P, width), dtype=dtype, device=dev))
    o = _lib.TokenScoresOut()
    o.logp_sum, o.logp_min = [t.data_ptr() for t in out]
    return out, o


def dense_token_scores(times=None, device=None):
    """How sure the decoder is of every decoded token of the calling thread's
    last ``decode_dense(..., token_scores=True)`` on ``device`` (None: the
    current one), without waiting for anything: one small kernel enqueued
    behind the decode and its token times, on the stream the decode went to
    (so it can be captured into the same ``torch.cuda.graph``).

    ``times`` is what ``dense_token_times()`` returned for that decode; None
    calls it here.  Returns ``TokenScores(logp_sum, logp_min)``: CUDA tensors
    of the compute dtype, ``[B, top_paths, T]``.  For token ``i`` of row
    ``[b, p]``, over the frames ``start[b, p, i] .. end[b, p, i]`` of the best
    alignment, ``logp_sum`` is the sum and ``logp_min`` the minimum of the
    log-posterior of the class the alignment holds at that frame (the blank's
    at the blank frames inside a merged token), from the decoder's own
    normaliser.  Tokens without times, everything past the row's decoded
    length and every row of an item with a status bit are NaN.  The mean
    confidence of a token is ``exp(logp_sum / (end - start + 1))``.  The
    definition is in ``include/ctcext.h``, "Token scores"; the ``blank_label``
    rule of the token times applies."""
    what = "ctcext_dense_token_scores without a ctcext_decode_dense"
    dec = _thread_decoder(device, what)
    lib = _scores_lib(dec.lib)
    if getattr(dec, "_times_dense", None) is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    shape = getattr(dec, "_scores_dense", None)
    if shape is None:
        raise FailedPreconditionError(_NO_SCORES, _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, dev, fdt = shape
    if times is None:
        times = dense_token_times(device)
    for name, v in (("start", times.start), ("end", times.end)):
        if not (_is_torch(v) and v.is_cuda and v.device == dev and tuple(v.shape) == (B, P, T)
                and str(v.dtype) == "torch.int32" and v.is_contiguous()):
            raise ValueError("times.%s must be a contiguous int32 tensor of shape %s on %s" % (name, (B, P, T), dev))
    t = _lib.TokenTimesOut()
    t.start, t.end = times.start.data_ptr(), times.end.data_ptr()
    out, o = _scores_device(dev, B, P, T, fdt)
    rc = lib.ctcext_dense_token_scores(dec.handle, ctypes.byref(t), ctypes.byref(o))
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return out


def token_scores(device=None):
    """``dense_token_scores`` for the synchronous calls: the scores of the
    hypotheses the calling thread's last ``ctc_ext_beam_search_decoder`` or
    ``decode_logits`` with ``token_scores=True`` on ``device`` returned (a
    stream keeps no logits: not after a push).  Waits.  Returns numpy arrays,
    or CUDA tensors where that call's outputs were."""
    what = "ctcext_fetch_token_scores without a successful ctcext_decode"
    dec = _thread_decoder(device, what)
    lib = _scores_lib(dec.lib)
    if getattr(dec, "_times_sync", None) is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    shape = getattr(dec, "_scores_sync", None)
    if shape is None:
        raise FailedPreconditionError(_NO_SCORES, _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, to_device, f64 = shape
    if to_device:
        import torch
        out, o = _scores_device(torch.device("cuda", dec.device), B, P, T, torch.float64 if f64 else torch.float32)
    else:
        dt = np.float64 if f64 else np.float32
        out = TokenScores(np.empty((B, P, T), dt), np.empty((B, P, T), dt))
        o = _lib.TokenScoresOut()
        o.logp_sum, o.logp_min = [t.ctypes.data for t in out]
    rc = lib.ctcext_fetch_token_scores(dec.handle, ctypes.byref(o), 1 if to_device else 0)
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return out


def token_scores_row(x, norm, alignment, frames, start, end, blank_index, blank_label):
    """The definition of the token scores for one row, on the host (no GPU):
    ``x`` is one item's logits ``[frames, num_classes]`` (float32 or float64,
    the compute dtype), ``norm`` its rows' normaliser ``[frames]``,
    ``alignment`` one path's alignment row in label order (without padding),
    ``start`` / ``end`` that path's token times.  Returns ``(logp_sum,
    logp_min)``: arrays of ``len(start)`` of ``x``'s dtype."""
    lib = _scores_lib(_lib.load())
    x = np.asarray(x)
    dt = np.float64 if x.dtype == np.float64 else np.float32
    frames = int(frames)
    x = np.ascontiguousarray(x[:frames], dtype=dt)
    if x.ndim != 2:
        raise ValueError("token_scores_row: x must be [frames, num_classes]")
    nm = np.ascontiguousarray(np.asarray(norm).reshape(-1)[:frames], dtype=dt)
    if x.shape[0] != frames or nm.size != frames:
        raise ValueError("token_scores_row: x and norm must hold the item's frames")
    al = np.ascontiguousarray(np.asarray(alignment, dtype=np.int64).reshape(-1))
    st = np.ascontiguousarray(np.asarray(start, dtype=np.int32).reshape(-1))
    en = np.ascontiguousarray(np.asarray(end, dtype=np.int32).reshape(-1))
    if st.size != en.size:
        raise ValueError("token_scores_row: start and end must have one length")
    lsum = np.empty((st.size,), dt)
    lmin = np.empty((st.size,), dt)
    rc = lib.ctcext_token_scores_row(x.ctypes.data, nm.ctypes.data, 1 if dt == np.float64 else 0, frames,
                                     int(x.shape[1]), _ptr(al, ctypes.c_int64), int(al.size),
                                     _ptr(st, ctypes.c_int32), _ptr(en, ctypes.c_int32), int(st.size),
                                     int(blank_index), int(blank_label), lsum.ctypes.data, lmin.ctypes.data)
    if rc != _lib.CTCEXT_OK:
        raise InvalidArgumentError("ctcext_token_scores_row: bad arguments", rc)
    return lsum, lmin


def _paths_lib(lib):
    if not hasattr(lib, "ctcext_dense_path_scores"):
        raise UnimplementedError("this libctcext.so has no path scores (CTCEXT_HAS_PATH_SCORES)",
                                 _lib.CTCEXT_UNIMPLEMENTED)
    return lib


_NO_PATHS = "path scores need a decode with token_scores=True"


def dense_path_scores(device=None):
    """How sure the decoder is of every whole hypothesis of the calling
    thread's last ``decode_dense(..., token_scores=True)`` on ``device`` (None:
    the current one), without waiting for anything: the exact CTC
    log-likelihood ``log p(y | x)`` of each returned label row over all of the
    item's frames, by the forward recursion on the device, enqueued behind the
    decode on the stream the decode went to (so it can be captured into the
    same ``torch.cuda.graph``).

    Returns a CUDA tensor ``[B, top_paths]`` of the compute dtype.  Unlike
    ``log_probability`` it does not depend on ``beam_width``, and after
    ``skip_blank`` it covers the dropped frames too.  An infeasible row is
    ``-inf``; every row of an item with a status bit is NaN.  The definition
    is in ``include/ctcext.h``, "Path scores"; the ``blank_label`` rule of the
    token times applies."""
    what = "ctcext_dense_path_scores without a ctcext_decode_dense"
    dec = _thread_decoder(device, what)
    lib = _paths_lib(dec.lib)
    if getattr(dec, "_times_dense", None) is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    shape = getattr(dec, "_scores_dense", None)
    if shape is None:
        raise FailedPreconditionError(_NO_PATHS, _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, dev, fdt = shape
    import torch
    with torch.cuda.device(dev):
        out = torch.empty((B, P), dtype=fdt, device=dev)
    rc = lib.ctcext_dense_path_scores(dec.handle, out.data_ptr())
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return out


def path_scores(device=None):
    """``dense_path_scores`` for the synchronous calls: the path scores of the
    hypotheses the calling thread's last ``ctc_ext_beam_search_decoder`` or
    ``decode_logits`` with ``token_scores=True`` on ``device`` returned (not
    after a stream's push).  Waits.  Returns a numpy array ``[B, top_paths]``,
    or a CUDA tensor where that call's outputs were."""
    what = "ctcext_fetch_path_scores without a successful ctcext_decode"
    dec = _thread_decoder(device, what)
    lib = _paths_lib(dec.lib)
    if getattr(dec, "_times_sync", None) is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    shape = getattr(dec, "_scores_sync", None)
    if shape is None:
        raise FailedPreconditionError(_NO_PATHS, _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, to_device, f64 = shape
    if to_device:
        import torch
        dev = torch.device("cuda", dec.device)
        with torch.cuda.device(dev):
            out = torch.empty((B, P), dtype=torch.float64 if f64 else torch.float32, device=dev)
        ptr = out.data_ptr()
    else:
        out = np.empty((B, P), np.float64 if f64 else np.float32)
        ptr = out.ctypes.data
    rc = lib.ctcext_fetch_path_scores(dec.handle, ptr, 1 if to_device else 0)
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return out


_NO_TARGETS = "target scores need a decode with token_scores=True"


def dense_target_scores(targets, target_lengths, device=None):
    """What the model thinks of label rows it did NOT return: the exact CTC
    log-likelihood ``log p(y | x)`` of every supplied target under the logits
    of the calling thread's last ``decode_dense(..., token_scores=True)`` or
    ``decode_greedy(..., token_scores=True)`` on ``device`` (None: the current
    one) -- a keyword list, another pass's N-best, an expected transcript.
    Enqueued behind that decode on its stream without waiting for anything, so
    it can be captured into the same ``torch.cuda.graph``.

    ``targets`` is a CUDA int64 or int32 tensor ``[B, N, L]``, or ``[N, L]``
    for one list shared by all items; ``target_lengths`` is a CUDA int32 tensor
    ``[B, N]`` or ``[N]`` to match.  Returns a CUDA tensor ``[B, N]`` of the
    compute dtype: the "Path scores" definition of ``include/ctcext.h`` applied
    to each row.  An infeasible row is ``-inf``; a row with a label outside
    ``[0, C)`` or a length outside ``[0, L]`` is NaN, as is every row of an
    item with a status bit.  No ``blank_label`` is involved.  Lists with
    ``L <= 63`` run in the packed kernel ("Target scores"), longer ones one
    wave per target."""
    what = "ctcext_dense_target_scores without a ctcext_decode_dense"
    dec = _thread_decoder(device, what)
    lib = dec.lib
    if not hasattr(lib, "ctcext_dense_target_scores"):
        raise UnimplementedError("this libctcext.so has no target scores (CTCEXT_HAS_TARGET_SCORES)",
                                 _lib.CTCEXT_UNIMPLEMENTED)
    if getattr(dec, "_times_dense", None) is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    shape = getattr(dec, "_scores_dense", None)
    if shape is None:
        raise FailedPreconditionError(_NO_TARGETS, _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, dev, fdt = shape
    import torch
    if not (_is_torch(targets) and _is_torch(target_lengths) and targets.is_cuda and target_lengths.is_cuda):
        raise TypeError("dense_target_scores: targets and target_lengths must be CUDA tensors")
    if targets.dtype not in (torch.int64, torch.int32):
        _type_error("targets", str(targets.dtype).replace("torch.", ""), "int32, int64")
    if target_lengths.dtype != torch.int32:
        _type_error("target_lengths", str(target_lengths.dtype).replace("torch.", ""), "int32")
    if targets.device != dev or target_lengths.device != dev:
        raise InvalidArgumentError("target scores: the targets must be on the decode's device", _lib.CTCEXT_INVALID_ARGUMENT)
    shared = targets.dim() == 2
    if targets.dim() not in (2, 3) or tuple(target_lengths.shape) != tuple(targets.shape[:-1]) or \
            (not shared and targets.shape[0] != B):
        raise InvalidArgumentError("target scores: targets must be [B, N, L] or [N, L], and target_lengths [B, N] or [N]",
                                   _lib.CTCEXT_INVALID_ARGUMENT)
    targets, target_lengths = targets.contiguous(), target_lengths.contiguous()
    N, L = int(targets.shape[-2]), int(targets.shape[-1])
    t = _lib.Targets(targets.data_ptr(), target_lengths.data_ptr(), N, L, 1 if shared else 0,
                     1 if targets.dtype == torch.int64 else 0)
    with torch.cuda.device(dev):
        out = torch.empty((B, N), dtype=fdt, device=dev)
    rc = lib.ctcext_dense_target_scores(dec.handle, ctypes.byref(t), out.data_ptr())
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return out


def score_targets(logits, lengths, targets, target_lengths, *, blank_index=0, batch_first=True):
    """``dense_target_scores`` for logits nothing has decoded yet:
    ``decode_greedy(..., token_scores=True)`` supplies the normaliser (its two
    small kernels), then the targets are scored behind it on the same stream.
    Arguments as for ``decode_greedy`` and ``dense_target_scores``; returns the
    CUDA tensor ``[B, N]``.  Nothing is waited for."""
    decode_greedy(logits, lengths, batch_first=batch_first, blank_index=blank_index, token_scores=True)
    return dense_target_scores(targets, target_lengths, device=logits.device)


def _prefix_lib(lib):
    if not hasattr(lib, "ctcext_dense_prefix_scores"):
        raise UnimplementedError("this libctcext.so has no prefix scores (CTCEXT_HAS_PREFIX_SCORES)",
                                 _lib.CTCEXT_UNIMPLEMENTED)
    return lib


def dense_prefix_scores(prefixes, prefix_lengths, device=None):
    """What an external beam search asks at every step: for every partial
    hypothesis ``g`` supplied and every class ``c`` at once, the CTC prefix
    score ``log p(transcript begins with g, c | x)`` under the logits of the
    calling thread's last ``decode_dense(..., token_scores=True)`` or
    ``decode_greedy(..., token_scores=True)`` on ``device`` (None: the current
    one).  Enqueued behind that decode on its stream; after one call of a
    shape nothing is allocated or waited for, so it can be captured into the
    same ``torch.cuda.graph``.

    ``prefixes`` is a CUDA int64 or int32 tensor ``[B, N, L]``, or ``[N, L]``
    for one list shared by all items; ``prefix_lengths`` is a
    CUDA int32 tensor ``[B, N]`` or ``[N]`` to match.  Returns a CUDA tensor
    ``[B, N, C]`` of the compute dtype: the "Prefix scores" definition of
    ``include/ctcext.h``.  The blank column holds the end score, the path score
    of ``g`` itself.  An infeasible prefix gives a row of ``-inf``; a label
    outside ``[0, C)``, a length outside ``[0, L]`` or an item with a status
    bit a row of NaN.  Acoustic scores only."""
    what = "ctcext_dense_prefix_scores without a ctcext_decode_dense"
    dec = _thread_decoder(device, what)
    lib = _prefix_lib(dec.lib)
    if getattr(dec, "_times_dense", None) is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    shape = getattr(dec, "_scores_dense", None)
    if shape is None:
        raise FailedPreconditionError("prefix scores need a decode with token_scores=True",
                                      _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, dev, fdt = shape
    import torch
    if not (_is_torch(prefixes) and _is_torch(prefix_lengths) and prefixes.is_cuda and prefix_lengths.is_cuda):
        raise TypeError("dense_prefix_scores: prefixes and prefix_lengths must be CUDA tensors")
    if prefixes.dtype not in (torch.int64, torch.int32):
        _type_error("prefixes", str(prefixes.dtype).replace("torch.", ""), "int32, int64")
    if prefix_lengths.dtype != torch.int32:
        _type_error("prefix_lengths", str(prefix_lengths.dtype).replace("torch.", ""), "int32")
    if prefixes.device != dev or prefix_lengths.device != dev:
        raise InvalidArgumentError("prefix scores: the prefixes must be on the decode's device",
                                   _lib.CTCEXT_INVALID_ARGUMENT)
    shared = prefixes.dim() == 2
    if prefixes.dim() not in (2, 3) or tuple(prefix_lengths.shape) != tuple(prefixes.shape[:-1]) or \
            (not shared and prefixes.shape[0] != B):
        raise InvalidArgumentError("prefix scores: prefixes must be [B, N, L] or [N, L], and prefix_lengths [B, N] or [N]",
                                   _lib.CTCEXT_INVALID_ARGUMENT)
    prefixes, prefix_lengths = prefixes.contiguous(), prefix_lengths.contiguous()
    N, L = int(prefixes.shape[-2]), int(prefixes.shape[-1])
    t = _lib.Targets(prefixes.data_ptr(), prefix_lengths.data_ptr(), N, L, 1 if shared else 0,
                     1 if prefixes.dtype == torch.int64 else 0)
    with torch.cuda.device(dev):
        out = torch.empty((B, N, int(dec._scores_keep.shape[-1])), dtype=fdt, device=dev)   # (the kept logits: classes last)
    rc = lib.ctcext_dense_prefix_scores(dec.handle, ctypes.byref(t), out.data_ptr())
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return out


def score_prefixes(logits, lengths, prefixes, prefix_lengths, *, blank_index=0, batch_first=True):
    """``dense_prefix_scores`` for logits nothing has decoded yet:
    ``decode_greedy(..., token_scores=True)`` supplies the normaliser, then the
    prefixes are scored behind it on the same stream.  Arguments as for
    ``decode_greedy`` and ``dense_prefix_scores``; returns the CUDA tensor
    ``[B, N, C]``."""
    decode_greedy(logits, lengths, batch_first=batch_first, blank_index=blank_index, token_scores=True)
    return dense_prefix_scores(prefixes, prefix_lengths, device=logits.device)


def prefix_score_row(x, norm, prefix, frames, blank_index):
    """The definition of the prefix scores for one prefix, on the host (no
    GPU), in long double: ``x`` is one item's logits ``[frames, num_classes]``
    (float32 or float64, the compute dtype), ``norm`` its rows' normaliser
    ``[frames]``, ``prefix`` the label row (without padding).  Returns a numpy
    array ``[num_classes]`` of ``x``'s dtype."""
    lib = _prefix_lib(_lib.load())
    x = np.asarray(x)
    dt = np.float64 if x.dtype == np.float64 else np.float32
    frames = int(frames)
    if x.ndim != 2:
        raise ValueError("prefix_score_row: x must be [frames, num_classes]")
    C = int(x.shape[1])
    x = np.ascontiguousarray(x[:frames], dtype=dt)
    nm = np.ascontiguousarray(np.asarray(norm).reshape(-1)[:frames], dtype=dt)
    if x.shape[0] != frames or nm.size != frames:
        raise ValueError("prefix_score_row: x and norm must hold the item's frames")
    g = np.ascontiguousarray(np.asarray(prefix, dtype=np.int64).reshape(-1))
    out = np.empty((max(C, 1),), dt)
    rc = lib.ctcext_prefix_score_row(x.ctypes.data, nm.ctypes.data, 1 if dt == np.float64 else 0, frames, C,
                                     _ptr(g, ctypes.c_int64), int(g.size), int(blank_index), out.ctypes.data)
    if rc != _lib.CTCEXT_OK:
        raise InvalidArgumentError("ctcext_prefix_score_row: bad arguments", rc)
    return out[:C]


TargetGrads = collections.namedtuple("TargetGrads", ["scores", "grad"])


def _tgrad_lib(lib):
    if not hasattr(lib, "ctcext_dense_target_grads"):
        raise UnimplementedError("this libctcext.so has no target gradients (CTCEXT_HAS_TARGET_GRADS)",
                                 _lib.CTCEXT_UNIMPLEMENTED)
    return lib


def dense_target_grads(targets, target_lengths, weights=None, device=None):
    """CTC forward-backward over supplied targets: ``dense_target_scores`` and,
    with it, ``sum_n weights[b, n] * d log p(y_n | x) / d logits[b]`` under the
    logits of the calling thread's last ``decode_dense(..., token_scores=True)``
    or ``decode_greedy(..., token_scores=True)`` on ``device`` (None: the
    current one) -- what minimum-risk training over a rescored N-best, a
    keyword list trained against a list or a CTC loss on short utterances
    needs.  Enqueued behind that decode on its stream; after one call of a
    shape nothing is allocated or waited for, so it can be captured into the
    same ``torch.cuda.graph``.

    ``targets`` and ``target_lengths`` are ``dense_target_scores``'s;
    ``weights`` is a CUDA tensor ``[B, N]`` of the compute dtype, or None for
    ones.  Returns ``TargetGrads(scores, grad)``: ``scores`` is
    ``dense_target_scores``'s ``[B, N]``, ``grad`` a contiguous CUDA tensor of
    the compute dtype, ``[B, T, C]`` or ``[T, B, C]`` as the logits the decode
    read were oriented, every cell written (zeros past an item's length).  Rows
    without a finite score (``-inf`` or NaN) add nothing; the definition is in
    ``include/ctcext.h``, "Target gradients".  Targets of more than 63 labels
    raise ``UnimplementedError``."""
    what = "ctcext_dense_target_grads without a ctcext_decode_dense"
    dec = _thread_decoder(device, what)
    lib = _tgrad_lib(dec.lib)
    if getattr(dec, "_times_dense", None) is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    shape = getattr(dec, "_scores_dense", None)
    if shape is None:
        raise FailedPreconditionError("target gradients need a decode with token_scores=True",
                                      _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, dev, fdt = shape
    import torch
    if not (_is_torch(targets) and _is_torch(target_lengths) and targets.is_cuda and target_lengths.is_cuda):
        raise TypeError("dense_target_grads: targets and target_lengths must be CUDA tensors")
    if targets.dtype not in (torch.int64, torch.int32):
        _type_error("targets", str(targets.dtype).replace("torch.", ""), "int32, int64")
    if target_lengths.dtype != torch.int32:
        _type_error("target_lengths", str(target_lengths.dtype).replace("torch.", ""), "int32")
    if targets.device != dev or target_lengths.device != dev:
        raise InvalidArgumentError("target gradients: the targets must be on the decode's device",
                                   _lib.CTCEXT_INVALID_ARGUMENT)
    shared = targets.dim() == 2
    if targets.dim() not in (2, 3) or tuple(target_lengths.shape) != tuple(targets.shape[:-1]) or \
            (not shared and targets.shape[0] != B):
        raise InvalidArgumentError("target gradients: targets must be [B, N, L] or [N, L], and target_lengths [B, N] or [N]",
                                   _lib.CTCEXT_INVALID_ARGUMENT)
    targets, target_lengths = targets.contiguous(), target_lengths.contiguous()
    N, L = int(targets.shape[-2]), int(targets.shape[-1])
    if weights is not None:
        if not (_is_torch(weights) and weights.is_cuda and weights.device == dev):
            raise TypeError("dense_target_grads: weights must be a CUDA tensor on the decode's device")
        if weights.dtype != fdt:
            _type_error("weights", str(weights.dtype).replace("torch.", ""), str(fdt).replace("torch.", ""))
        if tuple(weights.shape) != (B, N):
            raise InvalidArgumentError("target gradients: weights must be [B, N]", _lib.CTCEXT_INVALID_ARGUMENT)
        weights = weights.detach().contiguous()
    t = _lib.Targets(targets.data_ptr(), target_lengths.data_ptr(), N, L, 1 if shared else 0,
                     1 if targets.dtype == torch.int64 else 0)
    C = int(dec._scores_keep.shape[-1])   # (the kept logits: classes last)
    bf = bool(getattr(dec, "_scores_batch_first", False))
    with torch.cuda.device(dev):
        scores = torch.empty((B, N), dtype=fdt, device=dev)
        grad = torch.empty((B, T, C) if bf else (T, B, C), dtype=fdt, device=dev)
    rc = lib.ctcext_dense_target_grads(dec.handle, ctypes.byref(t), None if weights is None else weights.data_ptr(),
                                       scores.data_ptr(), grad.data_ptr(), 1 if bf else 0)
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return TargetGrads(scores, grad)


def target_grads(logits, lengths, targets, target_lengths, weights=None, *, blank_index=0, batch_first=True):
    """``dense_target_grads`` for logits nothing has decoded yet:
    ``decode_greedy(..., token_scores=True)`` supplies the normaliser, then the
    forward-backward runs behind it on the same stream.  Arguments as for
    ``decode_greedy`` and ``dense_target_grads``; returns ``TargetGrads``.
    Nothing is waited for."""
    decode_greedy(logits, lengths, batch_first=batch_first, blank_index=blank_index, token_scores=True)
    return dense_target_grads(targets, target_lengths, weights, device=logits.device)


def score_targets_autograd(logits, lengths, targets, target_lengths, *, blank_index=0, batch_first=True):
    """``score_targets`` that ``torch.autograd`` can differentiate with respect
    to ``logits``: the forward is ``score_targets``; the backward runs the
    greedy pre-pass on the saved logits again (the handle may have moved on)
    and ``dense_target_grads`` with the incoming gradient as the weights, and
    returns the slab in the logits' dtype.  Rows without a finite score pass no
    gradient."""
    import torch

    class _ScoreTargets(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.save_for_backward(x)
            return score_targets(x, lengths, targets, target_lengths, blank_index=blank_index, batch_first=batch_first)

        @staticmethod
        def backward(ctx, v):
            x, = ctx.saved_tensors
            g = target_grads(x, lengths, targets, target_lengths, v.contiguous(), blank_index=blank_index,
                             batch_first=batch_first).grad
            return g.to(x.dtype)

    return _ScoreTargets.apply(logits)


def target_grad_row(x, norm, target, frames, blank_index):
    """The definition of the target gradients for one target, on the host (no
    GPU), in long double: ``x`` is one item's logits ``[frames, num_classes]``
    (float32 or float64, the compute dtype), ``norm`` its rows' normaliser
    ``[frames]``, ``target`` the label row (without padding).  Returns
    ``(logp, g)``: a scalar and a numpy array ``[frames, num_classes]`` of
    ``x``'s dtype; a row without a finite score has an all-zero ``g``."""
    lib = _tgrad_lib(_lib.load())
    x = np.asarray(x)
    dt = np.float64 if x.dtype == np.float64 else np.float32
    frames = int(frames)
    if x.ndim != 2:
        raise ValueError("target_grad_row: x must be [frames, num_classes]")
    C = int(x.shape[1])
    x = np.ascontiguousarray(x[:frames], dtype=dt)
    nm = np.ascontiguousarray(np.asarray(norm).reshape(-1)[:frames], dtype=dt)
    if x.shape[0] != frames or nm.size != frames:
        raise ValueError("target_grad_row: x and norm must hold the item's frames")
    y = np.ascontiguousarray(np.asarray(target, dtype=np.int64).reshape(-1))
    logp, g = np.empty((1,), dt), np.empty((max(frames, 1), max(C, 1)), dt)
    rc = lib.ctcext_target_grad_row(x.ctypes.data, nm.ctypes.data, 1 if dt == np.float64 else 0, frames, C,
                                    _ptr(y, ctypes.c_int64), int(y.size), int(blank_index), logp.ctypes.data,
                                    g.ctypes.data)
    if rc != _lib.CTCEXT_OK:
        raise InvalidArgumentError("ctcext_target_grad_row: bad arguments", rc)
    return logp[0], g[:frames, :C]


TargetAlignments = collections.namedtuple("TargetAlignments", ["logp", "times", "scores", "alignment"])


def dense_target_alignments(targets, target_lengths, scores=False, alignment=False, device=None):
    """Where in the audio each label of a supplied row lies: the forced Viterbi
    alignment of every target under the logits of the calling thread's last
    ``decode_dense(..., token_scores=True)`` or ``decode_greedy(...,
    token_scores=True)`` on ``device`` (None: the current one) -- subtitle
    timing, corpus segmentation, word timings for another pass's N-best.
    Enqueued behind that decode on its stream without waiting for anything.
    The first call of a shape sizes a workspace (``include/ctcext.h``, "Target
    alignments") and may block; inside a ``torch.cuda.graph`` capture a call
    that would have to grow it raises ``FailedPreconditionError``: call once
    with the shape before capturing.

    ``targets`` and ``target_lengths`` are as for ``dense_target_scores``.
    Returns ``TargetAlignments(logp, times, scores, alignment)``: ``logp``
    ``[B, N]`` of the compute dtype (the best alignment's log-probability),
    ``times`` a ``TokenTimes`` of int32 ``[B, N, L]`` start and end frames and
    ``[B, N]`` trailing blanks, ``scores`` a ``TokenScores`` ``[B, N, L]``
    (``scores=True``, else None) and ``alignment`` int32 ``[B, N, T]``
    (``alignment=True``, else None): per frame the class index, ``blank_index``
    at a blank frame, -1 past the item's frames.  A row whose ``logp`` is
    ``-inf`` (infeasible) or NaN (a label outside ``[0, C)``, a length outside
    ``[0, L]``, an item with a status bit) is unaligned: times -1, scores NaN,
    alignment -1.  Lists with ``L >= 64`` raise ``UnimplementedError``: whole
    transcripts go to ``dense_transcript_alignments``."""
    return _target_alignments("ctcext_dense_target_alignments", "target alignments", "CTCEXT_HAS_TARGET_ALIGNMENTS",
                              targets, target_lengths, scores, alignment, device)


def _target_alignments(entry, name, macro, targets, target_lengths, scores, alignment, device):
    """The body ``dense_target_alignments`` and ``dense_transcript_alignments`` share: the C entry point differs."""
    what = entry + " without a ctcext_decode_dense"
    dec = _thread_decoder(device, what)
    lib = dec.lib
    if not hasattr(lib, entry):
        raise UnimplementedError("this libctcext.so has no %s (%s)" % (name, macro), _lib.CTCEXT_UNIMPLEMENTED)
    if getattr(dec, "_times_dense", None) is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    shape = getattr(dec, "_scores_dense", None)
    if shape is None:
        raise FailedPreconditionError(name + " need a decode with token_scores=True", _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, dev, fdt = shape
    import torch
    if not (_is_torch(targets) and _is_torch(target_lengths) and targets.is_cuda and target_lengths.is_cuda):
        raise TypeError("dense_%s: targets and target_lengths must be CUDA tensors" % name.replace(" ", "_"))
    if targets.dtype not in (torch.int64, torch.int32):
        _type_error("targets", str(targets.dtype).replace("torch.", ""), "int32, int64")
    if target_lengths.dtype != torch.int32:
        _type_error("target_lengths", str(target_lengths.dtype).replace("torch.", ""), "int32")
    if targets.device != dev or target_lengths.device != dev:
        raise InvalidArgumentError(name + ": the targets must be on the decode's device", _lib.CTCEXT_INVALID_ARGUMENT)
    shared = targets.dim() == 2
    if targets.dim() not in (2, 3) or tuple(target_lengths.shape) != tuple(targets.shape[:-1]) or \
            (not shared and targets.shape[0] != B):
        raise InvalidArgumentError(name + ": targets must be [B, N, L] or [N, L], and target_lengths [B, N] or [N]",
                                   _lib.CTCEXT_INVALID_ARGUMENT)
    targets, target_lengths = targets.contiguous(), target_lengths.contiguous()
    N, L = int(targets.shape[-2]), int(targets.shape[-1])
    t = _lib.Targets(targets.data_ptr(), target_lengths.data_ptr(), N, L, 1 if shared else 0,
                     1 if targets.dtype == torch.int64 else 0)
    with torch.cuda.device(dev):
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        logp = new((B, N), fdt)
        tt = TokenTimes(new((B, N, L), torch.int32), new((B, N, L), torch.int32), new((B, N), torch.int32))
        sc = TokenScores(new((B, N, L), fdt), new((B, N, L), fdt)) if scores else None
        ali = new((B, N, T), torch.int32) if alignment else None
    o = _lib.TargetAlignmentsOut(logp.data_ptr(), tt.start.data_ptr(), tt.end.data_ptr(), tt.trailing_blank.data_ptr(),
                                 sc.logp_sum.data_ptr() if scores else None, sc.logp_min.data_ptr() if scores else None,
                                 ali.data_ptr() if alignment else None)
    rc = getattr(lib, entry)(dec.handle, ctypes.byref(t), ctypes.byref(o))
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return TargetAlignments(logp, tt, sc, ali)


def forced_align(logits, lengths, targets, target_lengths, *, blank_index=0, batch_first=True, scores=False,
                 alignment=False):
    """``dense_target_alignments`` for logits nothing has decoded yet:
    ``decode_greedy(..., token_scores=True)`` supplies the normaliser (its two
    small kernels), then the targets are aligned behind it on the same stream.
    Arguments as for ``decode_greedy`` and ``dense_target_alignments``; returns
    the ``TargetAlignments``.  Nothing is waited for."""
    decode_greedy(logits, lengths, batch_first=batch_first, blank_index=blank_index, token_scores=True)
    return dense_target_alignments(targets, target_lengths, scores=scores, alignment=alignment, device=logits.device)


def dense_transcript_alignments(targets, target_lengths, scores=False, alignment=False, device=None):
    """``dense_target_alignments`` for whole transcripts: the same arguments,
    preconditions, definition and ``TargetAlignments`` result for targets of up
    to 2047 labels, in a kernel of its own that gives every target a workgroup
    (``include/ctcext.h``, "Transcript alignments").  Any ``L`` from 0 to 2047
    runs there; for ``L <= 63`` the results equal ``dense_target_alignments``
    bit for bit, which packs many short targets into a workgroup and is the
    better choice for lists of them.  ``L > 2047`` or a decode with
    ``max_time > 13000`` raises ``UnimplementedError``.  The workspace rule
    under a ``torch.cuda.graph`` capture is that of
    ``dense_target_alignments``, with a buffer of its own."""
    return _target_alignments("ctcext_dense_transcript_alignments", "transcript alignments",
                              "CTCEXT_HAS_TRANSCRIPT_ALIGNMENTS", targets, target_lengths, scores, alignment, device)


def align_transcripts(logits, lengths, targets, target_lengths, *, blank_index=0, batch_first=True, scores=False,
                      alignment=False):
    """``dense_transcript_alignments`` for logits nothing has decoded yet, as
    ``forced_align`` is to ``dense_target_alignments``: ``decode_greedy(...,
    token_scores=True)`` supplies the normaliser, then the transcripts are
    aligned behind it on the same stream.  Nothing is waited for."""
    decode_greedy(logits, lengths, batch_first=batch_first, blank_index=blank_index, token_scores=True)
    return dense_transcript_alignments(targets, target_lengths, scores=scores, alignment=alignment,
                                       device=logits.device)


def path_score_row(x, norm, decoded, frames, blank_index, blank_label=-1):
    """The definition of the path score for one row, on the host (no GPU), in
    long double: ``x`` is one item's logits ``[frames, num_classes]`` (float32
    or float64, the compute dtype), ``norm`` its rows' normaliser ``[frames]``,
    ``decoded`` one path's label row (without padding).  Returns a numpy
    scalar of ``x``'s dtype."""
    lib = _paths_lib(_lib.load())
    x = np.asarray(x)
    dt = np.float64 if x.dtype == np.float64 else np.float32
    frames = int(frames)
    if x.ndim != 2:
        raise ValueError("path_score_row: x must be [frames, num_classes]")
    C = int(x.shape[1])
    x = np.ascontiguousarray(x[:frames], dtype=dt)
    nm = np.ascontiguousarray(np.asarray(norm).reshape(-1)[:frames], dtype=dt)
    if x.shape[0] != frames or nm.size != frames:
        raise ValueError("path_score_row: x and norm must hold the item's frames")
    y = np.ascontiguousarray(np.asarray(decoded, dtype=np.int64).reshape(-1))
    out = np.empty((1,), dt)
    rc = lib.ctcext_path_score_row(x.ctypes.data, nm.ctypes.data, 1 if dt == np.float64 else 0, frames, C,
                                   _ptr(y, ctypes.c_int64), int(y.size), int(blank_index), int(blank_label),
                                   out.ctypes.data)
    if rc != _lib.CTCEXT_OK:
        raise InvalidArgumentError("ctcext_path_score_row: bad arguments", rc)
    return out[0]


PathAlignments = collections.namedtuple("PathAlignments", ["alignment", "alignment_lengths", "logp", "times", "scores"])

_NO_ALIGN = "path alignments need a decode with token_scores=True"


def _align_lib(lib):
    if not hasattr(lib, "ctcext_dense_path_alignments"):
        raise UnimplementedError("this libctcext.so has no path alignments (CTCEXT_HAS_PATH_ALIGNMENTS)",
                                 _lib.CTCEXT_UNIMPLEMENTED)
    return lib


def _align_outputs(B, P, T, fdt, times, scores, dev):
    """Uninitialised outputs of a path-alignments call (CUDA tensors on dev, numpy arrays for dev None), their
    struct, and the PathAlignments that holds them."""
    if scores and not times:
        raise ValueError("path alignments: scores=True needs times=True")
    if dev is None:
        ft = np.float64 if fdt == "float64" else np.float32
        new = lambda shape, dt: np.empty(shape, {"int64": np.int64, "int32": np.int32, "f": ft}[dt])
        ptr = lambda t: t.ctypes.data
    else:
        import torch
        ft = torch.float64 if fdt == "float64" else torch.float32
        def new(shape, dt):
            with torch.cuda.device(dev):
                return torch.empty(shape, dtype={"int64": torch.int64, "int32": torch.int32, "f": ft}[dt], device=dev)
        ptr = lambda t: t.data_ptr()
    o = _lib.PathAlignmentsOut()
    ali, alen, logp = new((B, P, T), "int64"), new((B, P), "int32"), new((B, P), "f")
    o.alignment, o.alignment_length, o.logp = ptr(ali), ptr(alen), ptr(logp)
    tt = sc = None
    if times:
        tt = TokenTimes(new((B, P, T), "int32"), new((B, P, T), "int32"), new((B, P), "int32"))
        o.start, o.end, o.trailing_blank = [ptr(t) for t in tt]
    if scores:
        sc = TokenScores(new((B, P, T), "f"), new((B, P, T), "f"))
        o.logp_sum, o.logp_min = [ptr(t) for t in sc]
    return o, PathAlignments(ali, alen, logp, tt, sc)


def dense_path_alignments(times=True, scores=False, device=None):
    """The Viterbi alignment of every returned label row of the calling
    thread's last ``decode_dense(..., token_scores=True)`` on ``device`` (None:
    the current one): the single most likely CTC alignment of the row over all
    of the item's frames, by a trellis on the device, enqueued behind the
    decode on the stream the decode went to.  It waits for nothing; the first
    call of a shape sizes a workspace (``max_time * words * 256`` bytes per
    row, ``include/ctcext.h``, "Path alignments") and may block, and inside a
    ``torch.cuda.graph`` capture a call that would have to grow it raises
    ``FailedPreconditionError``: call once with the shape before capturing.

    Returns ``PathAlignments(alignment, alignment_lengths, logp, times,
    scores)``: ``alignment`` int64 ``[B, top_paths, T]`` padded with the
    decode's ``pad_value``, ``alignment_lengths`` int32 ``[B, top_paths]``
    (the item's frames, or 0 for an unaligned row), ``logp`` ``[B, top_paths]``
    of the compute dtype (the alignment's log-probability), ``times`` a
    ``TokenTimes`` and ``scores`` a ``TokenScores`` of that alignment (None
    when not asked for; ``scores`` needs ``times``).  Unlike the decode's
    alignment rows it is complete -- every token is timed -- does not depend on
    ``beam_width``, belongs to the returned (merged) string, and covers the
    frames ``skip_blank`` dropped.  A row with ``logp`` ``-inf`` or NaN is
    unaligned: length 0, times -1, scores NaN."""
    what = "ctcext_dense_path_alignments without a ctcext_decode_dense"
    dec = _thread_decoder(device, what)
    lib = _align_lib(dec.lib)
    if getattr(dec, "_times_dense", None) is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    shape = getattr(dec, "_scores_dense", None)
    if shape is None:
        raise FailedPreconditionError(_NO_ALIGN, _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, dev, fdt = shape
    o, out = _align_outputs(B, P, T, str(fdt).replace("torch.", ""), times, scores, dev)
    rc = lib.ctcext_dense_path_alignments(dec.handle, ctypes.byref(o))
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return out


def path_alignments(times=True, scores=False, device=None):
    """``dense_path_alignments`` for the synchronous calls: the alignments of
    the hypotheses the calling thread's last ``ctc_ext_beam_search_decoder`` or
    ``decode_logits`` with ``token_scores=True`` on ``device`` returned (not
    after a stream's push).  Waits.  Rows are padded with -1.  Returns numpy
    arrays, or CUDA tensors where that call's outputs were."""
    what = "ctcext_fetch_path_alignments without a successful ctcext_decode"
    dec = _thread_decoder(device, what)
    lib = _align_lib(dec.lib)
    if getattr(dec, "_times_sync", None) is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    shape = getattr(dec, "_scores_sync", None)
    if shape is None:
        raise FailedPreconditionError(_NO_ALIGN, _lib.CTCEXT_FAILED_PRECONDITION)
    B, P, T, to_device, f64 = shape
    dev = None
    if to_device:
        import torch
        dev = torch.device("cuda", dec.device)
    o, out = _align_outputs(B, P, T, "float64" if f64 else "float32", times, scores, dev)
    rc = lib.ctcext_fetch_path_alignments(dec.handle, ctypes.byref(o), 1 if to_device else 0)
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    return out


def path_alignment_row(x, norm, decoded, frames, blank_index, blank_label=-1):
    """The definition of the path alignment for one row, on the host (no GPU),
    in the compute dtype: ``x`` is one item's logits ``[frames, num_classes]``
    (float32 or float64), ``norm`` its rows' normaliser ``[frames]``,
    ``decoded`` one path's label row (without padding).  Returns ``(alignment,
    logp)``: an int64 array of ``frames`` values (empty for an unaligned row)
    and a numpy scalar of ``x``'s dtype."""
    lib = _align_lib(_lib.load())
    x = np.asarray(x)
    dt = np.float64 if x.dtype == np.float64 else np.float32
    frames = int(frames)
    if x.ndim != 2:
        raise ValueError("path_alignment_row: x must be [frames, num_classes]")
    C = int(x.shape[1])
    x = np.ascontiguousarray(x[:frames], dtype=dt)
    nm = np.ascontiguousarray(np.asarray(norm).reshape(-1)[:frames], dtype=dt)
    if x.shape[0] != frames or nm.size != frames:
        raise ValueError("path_alignment_row: x and norm must hold the item's frames")
    y = np.ascontiguousarray(np.asarray(decoded, dtype=np.int64).reshape(-1))
    ali = np.empty((max(frames, 1),), np.int64)
    n = ctypes.c_int64()
    logp = np.empty((1,), dt)
    rc = lib.ctcext_path_alignment_row(x.ctypes.data, nm.ctypes.data, 1 if dt == np.float64 else 0, frames, C,
                                       _ptr(y, ctypes.c_int64), int(y.size), int(blank_index), int(blank_label),
                                       _ptr(ali, ctypes.c_int64), ctypes.byref(n), logp.ctypes.data)
    if rc != _lib.CTCEXT_OK:
        raise InvalidArgumentError("ctcext_path_alignment_row: bad arguments", rc)
    return ali[:n.value].copy(), logp[0]


def kept_frames(device=None):
    """The frames each item kept in the calling thread's last decode with
    ``skip_blank`` on ``device`` (None: the current one): a numpy int32 ``[B]``
    after ``ctc_ext_beam_search_decoder`` / ``decode_logits``, an int32 CUDA
    tensor after ``decode_dense`` (written by that call in stream order; an
    item with a status bit known before the decode keeps 0)."""
    what = "kept_frames without a decode with skip_blank"
    kept = getattr(_thread_decoder(device, what), "_kept", None)
    if kept is None:
        raise FailedPreconditionError(what, _lib.CTCEXT_FAILED_PRECONDITION)
    return kept


def token_times_row(decoded, alignment, frames, blank_label, merge_repeated=False):
    """The definition of the token times for one row, on the host (no GPU):
    ``decoded`` and ``alignment`` are one path's label and alignment rows in
    label order (without padding), ``frames`` the item's frame count.  Returns
    ``(start, end, trailing_blank)``: int32 arrays of ``len(decoded)`` and an
    int."""
    lib = _times_lib(_lib.load())
    d = np.ascontiguousarray(np.asarray(decoded, dtype=np.int64).reshape(-1))
    al = np.ascontiguousarray(np.asarray(alignment, dtype=np.int64).reshape(-1))
    start = np.empty((d.size,), np.int32)
    end = np.empty((d.size,), np.int32)
    trailing = ctypes.c_int32()
    rc = lib.ctcext_token_times_row(_ptr(d, ctypes.c_int64), int(d.size), _ptr(al, ctypes.c_int64), int(al.size),
                                    int(frames), int(blank_label), 1 if merge_repeated else 0,
                                    _ptr(start, ctypes.c_int32), _ptr(end, ctypes.c_int32), ctypes.byref(trailing))
    if rc != _lib.CTCEXT_OK:
        raise InvalidArgumentError("ctcext_token_times_row: bad arguments", rc)
    return start, end, int(trailing.value)


def dense_check(device=None):
    """Wait for the calling thread's last ``decode_dense`` on ``device``
    (None: the current one) and report it as the synchronous call would have:
    raises the same ``OpError`` subclass with the same message (a bad scorer
    table, ``sequence_length(b) <= max_time``, a helper hand-over timeout,
    "Less leaves in the beam search than requested.", in that order), prints
    the reference's "No label seq available" lines, and returns the stats dict
    with every counter filled."""
    index = _device_index(device)
    if index is None:
        index = _current_device()
    dec = getattr(_tls, "decoders", {}).get(int(index))
    if dec is None:   # no handle yet on this thread: no dense call either
        raise FailedPreconditionError("ctcext_dense_check without a ctcext_decode_dense",
                                      _lib.CTCEXT_FAILED_PRECONDITION)
    rc = dec.lib.ctcext_dense_check(dec.handle)
    dec.last_stats = dec.stats()
    if rc != _lib.CTCEXT_OK:
        _raise(dec.lib, rc)
    _print_no_label(dec.last_stats["no_label_paths"])
    return dec.last_stats


def _lengths_device(sequence_length, dev):
    """sequence_length as a contiguous int32 tensor on dev."""
    import torch
    if _is_torch(sequence_length):
        if sequence_length.dtype.is_floating_point:
            _type_error("sequence_length", str(sequence_length.dtype).replace("torch.", ""), "int32")
        return sequence_length.to(device=dev, dtype=torch.int32).contiguous()
    return torch.as_tensor(np.asarray(sequence_length, dtype=np.int32), device=dev)


def _lengths_host(sequence_length):
    """sequence_length as a contiguous int32 numpy array."""
    if _is_torch(sequence_length):
        sequence_length = sequence_length.detach().cpu().numpy()
    sl_arr = np.asarray(sequence_length)
    if sl_arr.dtype.kind == "f":
        _type_error("sequence_length", sl_arr.dtype.name, "int32")
    return np.ascontiguousarray(sl_arr.astype(np.int32))


def _decode_and_fetch(lib, a, keep, shape, on_device, device, table_dtype, index, outputs, devices, scorer_table,
                      skip_blank=None, token_scores=False):
    """Everything after the inputs are described by ``a``: validation, the
    beam-scorer table, the handle, phase 1, output allocation and phase 2.
    ``shape`` is the logical (max_time, batch, num_classes); ``table_dtype``
    the compute dtype (torch for device inputs, numpy for host inputs), in
    which the scorer table is passed and log_probability comes back."""
    code, top_paths = a.dtype, a.top_paths
    skip = None if skip_blank is None else _skip_args(lib, skip_blank)
    # the reference's shape/length checks run behind the C ABI, before any
    # device work (kernels.cc:97-139)
    rc = lib.ctcext_validate(ctypes.byref(a))
    if rc != _lib.CTCEXT_OK:
        _raise(lib, rc)
    if scorer_table is not None:
        C = int(shape[2]) if len(shape) == 3 else 0
        if on_device:
            import torch
            tab = torch.as_tensor(scorer_table, device=device, dtype=table_dtype).contiguous()
            a.scorer_table = tab.data_ptr()
        else:
            tab = np.ascontiguousarray(np.asarray(
                scorer_table.detach().cpu().numpy() if _is_torch(scorer_table) else scorer_table,
                dtype=table_dtype))
            a.scorer_table = tab.ctypes.data
        if tuple(tab.shape) != (C + 1, C):
            raise ValueError("scorer_table must be [num_classes + 1, num_classes] = [%d, %d], got %s"
                             % (C + 1, C, tuple(tab.shape)))
        keep.append(tab)
        a.scorer = _lib.CTCEXT_SCORER_BIGRAM
        # the library checks the table's entries (<= 0) before decoding
        rc = lib.ctcext_validate(ctypes.byref(a))
        if rc != _lib.CTCEXT_OK:
            _raise(lib, rc)
    if devices is not None:
        devs = tuple(int(d) for d in devices)
        if on_device and devs[0] != index:
            raise ValueError("device inputs must live on devices[0] (cuda:%d), not cuda:%d" % (devs[0], index))
        dec = get_decoder(devs if len(devs) > 1 else devs[0])
    else:
        dec = get_decoder(index if index is not None else _current_device())
    if on_device and not a.stream:
        # torch's legacy default stream has handle 0, which the C ABI reads as
        # "the decoder's own (non-blocking) stream": work still pending on the
        # default stream (the kernels that produce the logits) would not be
        # waited for, so it is, here
        import torch
        torch.cuda.current_stream(device).synchronize()
    dec._kept = None
    dec._scores_keep = dec._scores_dense = dec._scores_sync = None
    if skip is not None:
        # the kept counts: device memory for device inputs, host memory otherwise
        nb = max(int(shape[1]), 0) if len(shape) == 3 else 0
        if on_device:
            import torch
            with torch.cuda.device(device):
                kept = torch.zeros((nb,), dtype=torch.int32, device=device)
            skip.kept = kept.data_ptr()
        else:
            kept = np.zeros((nb,), np.int32)
            skip.kept = kept.ctypes.data
    sizes = dec.decode(a, skip)
    if skip is not None:
        dec._kept = kept.cpu().numpy() if on_device else kept
    to_device = outputs == "device" or (outputs == "auto" and on_device)
    dec._times_sync = (int(shape[1]), int(top_paths), int(shape[0]), to_device)   # (token_times' output shapes)
    if token_scores:
        # (token_scores' output shapes and dtype; device inputs are read in place again by its kernel, host
        # inputs from the copy the library staged)
        dec._scores_keep = list(keep) if on_device else None
        dec._scores_sync = dec._times_sync + (code == _lib.CTCEXT_F64,)
    out = _fetch_outputs(dec, sizes, int(shape[1]), int(top_paths), code, to_device)
    del keep
    _print_no_label(dec.last_stats["no_label_paths"])
    return out


def _host_empty():
    """Host output allocator: numpy views of pinned torch CPU tensors (the
    caching host allocator reuses the pinned pages, so the GPU copies the
    components down at full PCIe rate without first-touch page faults), or
    plain numpy without torch."""
    try:
        import torch
        if torch.cuda.is_available():
            tdt = {np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32,
                   np.dtype(np.float64): torch.float64}

            def empty(shape, dt):
                return torch.empty(shape, dtype=tdt[np.dtype(dt)], pin_memory=True).numpy()
            return empty
    except ImportError:
        pass
    return np.empty


def _stream_chunk(a, np_dtype, fixed, chunk, lengths, batch_first, flags):
    """The ``ctcext_chunk`` of one push of a stream with attributes ``a``: ``(c, x, sl, on_device, dev, index)``,
    x and sl being the tensors or arrays c points into.  ``fixed``: where the stream's chunks live (None: not
    fixed yet)."""
    allowed = "float16, bfloat16, float32" if a.dtype == _lib.CTCEXT_F32 else "float64"
    if _is_torch(chunk):
        import torch
        formats = {torch.float16: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_F16),
                   torch.bfloat16: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_BF16),
                   torch.float32: (_lib.CTCEXT_F32, _lib.CTCEXT_IN_NATIVE),
                   torch.float64: (_lib.CTCEXT_F64, _lib.CTCEXT_IN_NATIVE)}
        if chunk.dtype not in formats:
            _type_error("chunk", str(chunk.dtype).replace("torch.", ""), allowed)
        x = chunk.detach()
        strides = x.stride()
        dname = str(x.dtype).replace("torch.", "")
    else:
        x = chunk if isinstance(chunk, np.ndarray) else np.asarray(chunk, dtype=np_dtype)
        formats = {np.dtype(np.float16): (_lib.CTCEXT_F32, _lib.CTCEXT_IN_F16),
                   np.dtype(np.float32): (_lib.CTCEXT_F32, _lib.CTCEXT_IN_NATIVE),
                   np.dtype(np.float64): (_lib.CTCEXT_F64, _lib.CTCEXT_IN_NATIVE)}
        if x.dtype not in formats:
            _type_error("chunk", x.dtype.name, allowed)
        strides = tuple(s // x.itemsize if s % x.itemsize == 0 else 0 for s in x.strides)
        dname = x.dtype.name
    code, fmt = formats[x.dtype]
    if fmt == _lib.CTCEXT_IN_NATIVE and code != a.dtype:
        _type_error("chunk", dname, allowed)
    if len(x.shape) != 3:
        raise InvalidArgumentError("inputs is not a 3-Tensor", _lib.CTCEXT_INVALID_ARGUMENT)
    copy, shape, st_t, st_b = logits_layout(tuple(x.shape), strides, batch_first)
    if (shape[1], shape[2]) != (a.batch_size, a.num_classes):
        raise InvalidArgumentError("chunk has batch_size %d and num_classes %d, the stream %d and %d"
                                   % (shape[1], shape[2], a.batch_size, a.num_classes),
                                   _lib.CTCEXT_INVALID_ARGUMENT)
    if copy:
        x = x.contiguous() if _is_torch(x) else np.ascontiguousarray(x)
    if shape[0] == 0:   # no frame: nothing is addressed, whatever strides an empty view reports
        st_t = st_b = 0
    on_device = bool(_is_torch(x) and x.is_cuda)
    if fixed is not None and on_device != fixed:
        raise ValueError("this stream's chunks live on the %s (fixed by its first push)"
                         % ("device" if fixed else "host"))
    c = _lib.Chunk()
    c.chunk_time = int(shape[0])
    c.inputs_format, c.flags = fmt, int(flags)
    c.inputs_stride_t, c.inputs_stride_b = int(st_t), int(st_b)
    sl = None
    if on_device:
        dev = x.device
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        if lengths is not None:
            sl = _lengths_device(lengths, dev)
            c.chunk_length = sl.data_ptr()
        c.inputs = x.data_ptr()
        c.stream = torch.cuda.current_stream(dev).cuda_stream
    else:
        dev = index = None
        if lengths is not None:
            sl = _lengths_host(lengths)
            c.chunk_length = sl.ctypes.data
        c.inputs = x.data_ptr() if _is_torch(x) else x.ctypes.data
    if sl is not None and tuple(sl.shape) != (int(a.batch_size),):
        raise FailedPreconditionError("len(sequence_length) != batch_size.  len(sequence_length):  %d batch_size: %d"
                                      % (sl.shape[0] if len(sl.shape) else 0, a.batch_size),
                                      _lib.CTCEXT_FAILED_PRECONDITION)
    return c, x, sl, on_device, dev, index


StablePrefix = collections.namedtuple("StablePrefix", ["decoded_length", "frames"])
StreamDense = collections.namedtuple(
    "StreamDense",
    ["decoded", "decoded_lengths", "alignment", "alignment_lengths", "log_probability", "status", "frames",
     "stable_length", "stable_frames"])


class StreamDecoder:
    """Streaming decode: push the logits of a batch in chunks of frames and
    read, after each push, the hypotheses of everything pushed so far --
    bit for bit what ``decode_logits`` returns for that prefix.

        s = StreamDecoder(batch_size, num_classes, beam_width, top_paths, max_frames)
        for chunk in chunks:              # [B, t, C] each (batch_first), t may vary
            out = s.push(chunk, lengths)  # lengths: frames of this chunk per item (None: all t)
            fin = s.stable()              # fin.decoded_length[b] leading labels of item b are final
        s.reset([1])                      # item 1 starts a new utterance; the others go on
        s.close()                         # or use it as a context manager

    ``max_frames`` is the capacity per item: the beam records of that many
    frames are kept on the device.  ``dtype`` is the compute and output type;
    ``"float32"`` streams take float16 / bfloat16 / float32 chunks, ``"float64"``
    ones float64.  Chunks are torch tensors (GPU or host) or numpy arrays, as
    ``decode_logits`` takes them, strided views included; whether they live on
    the device or the host is fixed by the first push.  The decode kernel is
    chosen at that moment (dtype, scorer, num_classes, beam_width and the
    ``CTCEXT_HELPER`` environment variable) and stays for the stream's life.

    ``skip_blank``: None, or a log-probability threshold (<= 0) for blank-frame
    skipping (include/ctcext.h, "Streaming: blank-frame skipping").  Every
    ``push_dense`` then drops runs of blank-dominant frames on the device, a
    run carried across pushes, and its outputs are those of the one-shot
    skipping decode of everything pushed so far; ``frames``, ``stable()`` and
    the token times stay on the original time axis.  Such a stream takes CUDA
    chunks through ``push_dense`` only: ``push`` raises ``UnimplementedError``.

    ``token_scores=True`` gives the stream a score store (include/ctcext.h,
    "Streaming: token scores"): the logits and the normaliser of every frame
    committed since an item's last reset stay on the device, and
    ``token_scores_dense()`` returns the per-token confidences after any
    ``push_dense``.  ``score_store`` is the store's element type: None keeps
    the compute dtype and takes chunks of any accepted dtype; ``"bfloat16"`` or
    ``"float16"`` (float32 streams) halves the store and takes chunks of that
    dtype only.  The store is ``batch_size * max_frames * (num_classes * esize
    + sizeof(dtype))`` bytes, allocated when the stream opens.  Such a stream
    takes CUDA chunks through ``push_dense`` only as well.
    """

    def __init__(self, batch_size, num_classes, beam_width, top_paths, max_frames, *,
                 dtype="float32", merge_repeated=False, blank_index=0, blank_label=-1,
                 device=None, scorer_table=None, flags=0, skip_blank=None, token_scores=False, score_store=None):
        self.lib = _lib.load()
        self._skip = self._kept = None
        self._scores = None
        if score_store is not None and not token_scores:
            raise ValueError("score_store needs token_scores=True")
        if token_scores:
            if not hasattr(self.lib, "ctcext_stream_open_scores"):
                raise UnimplementedError("this libctcext.so has no token scores for streams "
                                         "(CTCEXT_HAS_STREAM_SCORES)", _lib.CTCEXT_UNIMPLEMENTED)
            formats = {None: _lib.CTCEXT_IN_NATIVE, "float16": _lib.CTCEXT_IN_F16, "bfloat16": _lib.CTCEXT_IN_BF16}
            if score_store not in formats:
                _type_error("score_store", score_store, "None, float16, bfloat16")
            self._scores = _lib.StreamScoresArgs()
            self._scores.store_format = formats[score_store]
        if skip_blank is not None:
            if not hasattr(self.lib, "ctcext_stream_open_skip"):
                raise UnimplementedError("this libctcext.so has no blank-frame skipping for streams "
                                         "(CTCEXT_HAS_STREAM_SKIP)", _lib.CTCEXT_UNIMPLEMENTED)
            self._skip = _skip_args(self.lib, skip_blank)
        name = np.dtype(dtype).name if not isinstance(dtype, str) else dtype
        if name not in ("float32", "float64"):
            _type_error("dtype", name, "float32, float64")
        self._np_dtype = np.dtype(name)
        a = _lib.StreamArgs()
        a.dtype = _lib.CTCEXT_F32 if name == "float32" else _lib.CTCEXT_F64
        a.batch_size, a.num_classes, a.max_frames = int(batch_size), int(num_classes), int(max_frames)
        a.beam_width, a.top_paths = int(beam_width), int(top_paths)
        a.merge_repeated = 1 if merge_repeated else 0
        a.blank_index, a.blank_label, a.flags = int(blank_index), int(blank_label), int(flags)
        self._args = a
        self._table = None
        if scorer_table is not None:
            tab = np.ascontiguousarray(np.asarray(
                scorer_table.detach().cpu().numpy() if _is_torch(scorer_table) else scorer_table,
                dtype=self._np_dtype))
            C = int(num_classes)
            if tuple(tab.shape) != (C + 1, C):
                raise ValueError("scorer_table must be [num_classes + 1, num_classes] = [%d, %d], got %s"
                                 % (C + 1, C, tuple(tab.shape)))
            self._table = tab
            a.scorer = _lib.CTCEXT_SCORER_BIGRAM
            a.scorer_table = tab.ctypes.data   # (host memory wherever the chunks live: ctcext.h)
        # the attribute checks run on the host now; the stream itself opens
        # with the first push, which fixes where the chunks live
        rc = self.lib.ctcext_stream_validate(ctypes.byref(a))
        if rc == _lib.CTCEXT_OK and self._scores is not None:
            a.on_device = 1   # (device chunks only)
            rc = self.lib.ctcext_stream_scores_validate(ctypes.byref(a), ctypes.byref(self._scores))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)
        self._device = _device_index(device)
        self.dec = None
        self.handle = None
        self.on_device = None
        self.closed = False
        self.last_stats = None

    # -- lifetime ----------------------------------------------------------
    def _open(self, on_device, index):
        if self._device is not None:
            if on_device and index != self._device:
                raise ValueError("the chunk lives on cuda:%d, the stream on cuda:%d" % (index, self._device))
            index = self._device
        self.dec = get_decoder(index if index is not None else _current_device())
        a = self._args
        a.on_device = 1 if on_device else 0
        h = ctypes.c_void_p()
        if self._skip is not None and on_device:
            # the tensor every push writes its kept counts into, for the stream's life
            import torch
            self._kept = torch.zeros((int(a.batch_size),), dtype=torch.int32,
                                     device=torch.device("cuda", self.dec.device))
            self._skip.kept = self._kept.data_ptr()
        if self._scores is not None:
            rc = self.lib.ctcext_stream_open_scores(self.dec.handle, ctypes.byref(a),
                                                    None if self._skip is None else ctypes.byref(self._skip),
                                                    ctypes.byref(self._scores), ctypes.byref(h))
        elif self._skip is None:
            rc = self.lib.ctcext_stream_open(self.dec.handle, ctypes.byref(a), ctypes.byref(h))
        else:
            rc = self.lib.ctcext_stream_open_skip(self.dec.handle, ctypes.byref(a), ctypes.byref(self._skip),
                                                  ctypes.byref(h))
        if rc != _lib.CTCEXT_OK:
            self._kept = None
            _raise(self.lib, rc)
        self.handle = h
        self.on_device = on_device

    def close(self):
        if self.handle and self.dec is not None and self.dec.handle:
            self.lib.ctcext_stream_close(self.handle)
        self.handle = None
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_open(self):
        if self.closed:
            raise FailedPreconditionError("the stream is closed", _lib.CTCEXT_FAILED_PRECONDITION)

    @property
    def frames(self):
        """Frames pushed so far per item: numpy int64 [batch_size]."""
        self._check_open()
        out = np.zeros((int(self._args.batch_size),), np.int64)
        if self.handle:
            rc = self.lib.ctcext_stream_frames(self.handle, out.ctypes.data)
            if rc != _lib.CTCEXT_OK:
                _raise(self.lib, rc)
        return out

    def kept_frames(self):
        """Frames kept per item so far on a ``skip_blank`` stream (``frames``
        on any other): numpy int64 [batch_size].  Waits."""
        self._check_open()
        out = np.zeros((int(self._args.batch_size),), np.int64)
        if self.handle:
            if not hasattr(self.lib, "ctcext_stream_kept"):
                raise UnimplementedError("this libctcext.so has no ctcext_stream_kept (CTCEXT_HAS_STREAM_SKIP)",
                                         _lib.CTCEXT_UNIMPLEMENTED)
            rc = self.lib.ctcext_stream_kept(self.handle, out.ctypes.data)
            if rc != _lib.CTCEXT_OK:
                _raise(self.lib, rc)
        return out

    def kept_dense(self):
        """The int32 CUDA tensor ``[batch_size]`` that every ``push_dense`` of a
        ``skip_blank`` stream writes its kept counts into, in stream order (the
        same tensor for the stream's life, so a captured push keeps writing
        it).  Opens the stream for CUDA chunks if no push has yet."""
        self._check_open()
        if self._skip is None:
            raise FailedPreconditionError("kept_dense without skip_blank", _lib.CTCEXT_FAILED_PRECONDITION)
        if not self.handle:
            self._open(True, self._device if self._device is not None else _current_device())
        return self._kept

    def reset(self, items=None):
        """Put ``items`` (None: all) back to no frames; the others are untouched."""
        self._check_open()
        if not self.handle:
            return
        if items is None:
            rc = self.lib.ctcext_stream_reset(self.handle, None, 0)
        else:
            arr = np.ascontiguousarray(np.asarray(items, dtype=np.int32).reshape(-1))
            rc = self.lib.ctcext_stream_reset(self.handle, arr.ctypes.data, int(arr.size))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)

    # -- the stable prefix ---------------------------------------------------
    def stable(self, walked=False):
        """How much of the decoded output is final: ``StablePrefix(decoded_length,
        frames)``, numpy int32 / int64 ``[batch_size]``.  The first
        ``decoded_length[b]`` labels of item b's decoded row are the same in
        every path of this push and of every later push, until the item is
        reset; ``frames[b]`` is the frame frontier behind them (all live beam
        entries share their history up to frame ``frames[b] - 1``).  Neither
        decreases between resets.  The alignment outputs get no such
        guarantee.  With ``walked=True`` also returns, as a second value, the
        record frames the query's convergence walk visited per item (int64)."""
        self._check_open()
        B = int(self._args.batch_size)
        n = np.zeros((B,), np.int32)
        f = np.zeros((B,), np.int64)
        w = np.zeros((B,), np.int64)
        if self.handle:   # (a stream before its first push: zeros)
            rc = self.lib.ctcext_stream_stable(self.handle, _ptr(n, ctypes.c_int32), _ptr(f, ctypes.c_int64),
                                               _ptr(w, ctypes.c_int64) if walked else None)
            if rc != _lib.CTCEXT_OK:
                _raise(self.lib, rc)
        res = StablePrefix(n, f)
        return (res, w) if walked else res

    def _stable_reference(self):
        """Tests: ``stable()``'s two numbers by the naive host walk over a
        copy of the records (every live chain to frame 0, no cache)."""
        self._check_open()
        B = int(self._args.batch_size)
        n = np.zeros((B,), np.int32)
        f = np.zeros((B,), np.int64)
        if self.handle:
            rc = self.lib.ctcext_stream_stable_reference(self.handle, _ptr(n, ctypes.c_int32), _ptr(f, ctypes.c_int64))
            if rc != _lib.CTCEXT_OK:
                _raise(self.lib, rc)
        return StablePrefix(n, f)

    # -- push ---------------------------------------------------------------
    def push(self, chunk, lengths=None, *, batch_first=True, results=True, outputs="auto", flags=0):
        """Decode ``chunk`` (``[B, t, C]`` with ``batch_first``, else ``[t, B, C]``)
        on top of what the stream holds.  ``lengths``: frames of this chunk per
        item, 0..t (None: t for all).  Returns the ``CTCExtBeamSearchDecoder``
        tuple of the prefix pushed so far, or None with ``results=False``
        (no traceback, no outputs: the cheap push between two reads)."""
        self._check_open()
        if outputs not in ("auto", "host", "device"):
            raise ValueError("outputs must be 'auto', 'host' or 'device'")
        if self._skip is not None:   # (the library's own answer and message; nothing is opened or touched)
            raise UnimplementedError("a skipping stream has no synchronous push: use ctcext_stream_push_dense",
                                     _lib.CTCEXT_UNIMPLEMENTED)
        if self._scores is not None:   # (likewise)
            raise UnimplementedError("a stream with a score store has no synchronous push: use "
                                     "ctcext_stream_push_dense", _lib.CTCEXT_UNIMPLEMENTED)
        lib = self.lib
        a = self._args
        c, x, sl, on_device, dev, index = self._chunk(chunk, lengths, batch_first, flags)
        if not self.handle:
            # host-side checks of the first chunk before the stream opens
            a.on_device = 1 if on_device else 0
            rc = lib.ctcext_stream_validate_chunk(ctypes.byref(a), ctypes.byref(c))
            if rc != _lib.CTCEXT_OK:
                _raise(lib, rc)
            self._open(on_device, index)
        dec = self.dec
        if on_device and not c.stream:
            import torch
            torch.cuda.current_stream(dev).synchronize()   # (see _decode_and_fetch)
        P = int(a.top_paths)
        sizes = (_lib.PathSizes * max(P, 1))() if results else None
        rc = lib.ctcext_stream_push(self.handle, ctypes.byref(c), sizes)
        self.last_stats = dec.last_stats = dec.stats()
        if rc != _lib.CTCEXT_OK:
            _raise(lib, rc)
        del x, sl
        if not results:
            return None
        szs = [(s.num_decoded, s.max_decoded, s.num_alignment, s.max_alignment) for s in sizes]
        to_device = outputs == "device" or (outputs == "auto" and on_device)
        dec._times_sync = (int(a.batch_size), P, int(a.max_frames), to_device)   # (token_times' output shapes)
        dec._scores_keep = dec._scores_sync = None   # (a push leaves nothing for token_scores)
        out = _fetch_outputs(dec, szs, int(a.batch_size), P, a.dtype, to_device)
        _print_no_label(dec.last_stats["no_label_paths"])
        return out

    def _chunk(self, chunk, lengths, batch_first, flags):
        return _stream_chunk(self._args, self._np_dtype, self.on_device, chunk, lengths, batch_first, flags)

    # -- the enqueue-only push -----------------------------------------------
    def push_dense(self, chunk, lengths=None, *, reset=None, batch_first=True, results=True, stable=False,
                   pad_value=-1, flags=0):
        """``push`` without waiting for anything: the chunk is decoded on
        ``torch.cuda.current_stream()`` behind whatever produced it, and the
        call returns padded CUDA tensors of static shape.  No ``synchronize()``,
        no ``.item()``, no ``.cpu()``; after ``reserve(t)`` (or one push of that
        size) it can be captured into a ``torch.cuda.graph`` and replayed once
        per chunk with new data in the same tensors.

        ``chunk`` is a CUDA tensor; ``lengths`` and ``reset`` should be int32
        CUDA tensors of ``[B]`` (other forms are converted on the device).
        ``reset[b] != 0`` starts a new utterance in item b with this chunk: the
        continuous-batching slot swap without a host round trip.

        Returns ``StreamDense(decoded, decoded_lengths, alignment,
        alignment_lengths, log_probability, status, frames, stable_length,
        stable_frames)``.  The first five are ``decode_dense``'s with rows
        ``max_frames`` wide, the hypotheses of everything pushed so far, and
        None with ``results=False`` (no traceback, no pack).  ``status`` int32
        ``[B]`` holds this push's ``CTCEXT_ITEM_*`` bits (0: good) and
        ``frames`` int32 ``[B]`` the frames per item after it.
        ``stable_length`` int32 / ``stable_frames`` int64 ``[B]`` are
        ``stable()``'s two numbers after this push, None without ``stable=True``.

        Errors that depend on the data are deferred: a length above the chunk's
        frames (``CTCEXT_ITEM_LENGTH``) or past ``max_frames``
        (``CTCEXT_ITEM_CAPACITY``) and a helper hand-over timeout leave that item
        as it was before the push, with empty rows; the other items advance.
        ``check()`` waits and raises what ``push`` would have raised.

        Successive pushes are ordered by the torch stream they are made on;
        pushes of one ``StreamDecoder`` made on different streams are the
        caller's to order."""
        self._check_open()
        if not (_is_torch(chunk) and chunk.is_cuda):
            raise ValueError("push_dense takes CUDA torch tensors; use push for host chunks")
        import torch
        lib = self.lib
        a = self._args
        c, x, sl, on_device, dev, index = self._chunk(chunk, lengths, batch_first, flags)
        B, P, F = int(a.batch_size), int(a.top_paths), int(a.max_frames)
        rs = None
        if reset is not None:
            rs = _lengths_device(reset, dev)
            if tuple(rs.shape) != (B,):
                raise ValueError("reset must have shape [batch_size] = [%d], got %s" % (B, tuple(rs.shape)))
        if not c.stream:   # torch's legacy default stream: the null stream itself, not the decoder's own
            c.flags |= _lib.CTCEXT_FLAG_DENSE_NULL_STREAM
        if not self.handle:
            a.on_device = 1
            if self._scores is None:
                rc = lib.ctcext_stream_dense_validate(ctypes.byref(a), ctypes.byref(c), None)
            else:
                rc = lib.ctcext_stream_scores_validate_chunk(ctypes.byref(a), ctypes.byref(self._scores),
                                                             ctypes.byref(c))
            if rc != _lib.CTCEXT_OK:
                _raise(lib, rc)
            self._open(True, index)
        fdt = torch.float32 if a.dtype == _lib.CTCEXT_F32 else torch.float64
        with torch.cuda.device(dev):
            def empty(shape, dt):
                return torch.empty(shape, dtype=dt, device=dev)
            hyp = ([empty((B, P, F), torch.int64), empty((B, P), torch.int32), empty((B, P, F), torch.int64),
                    empty((B, P), torch.int32), empty((B, P), fdt)] if results else [None] * 5)
            status, frames = empty((B,), torch.int32), empty((B,), torch.int32)
            st = [empty((B,), torch.int32), empty((B,), torch.int64)] if stable else [None, None]
        out = StreamDense(*(hyp + [status, frames] + st))
        o = _lib.StreamDenseOutputs()
        (o.decoded, o.decoded_length, o.alignment, o.alignment_length, o.log_probability, o.status, o.frames,
         o.stable_length, o.stable_frames) = [None if t is None else t.data_ptr() for t in out]
        o.pad_value = int(pad_value)
        rc = lib.ctcext_stream_push_dense(self.handle, ctypes.byref(c), None if rs is None else rs.data_ptr(),
                                          ctypes.byref(o))
        if rc != _lib.CTCEXT_OK:
            _raise(lib, rc)
        # x, sl and rs may be temporaries: they were allocated on this stream, and
        # the caching allocator hands their memory out again in stream order
        del x, sl, rs
        return out

    def token_times_dense(self):
        """``dense_token_times`` for the last ``push_dense`` with results:
        ``TokenTimes(start, end, trailing_blank)`` of everything pushed so far,
        rows ``max_frames`` wide, enqueued behind that push on its stream (so
        the two can be captured together).  Frames count from the item's last
        reset.  ``FailedPreconditionError`` after a ``results=False`` push or
        before any ``push_dense``."""
        self._check_open()
        lib = _times_lib(self.lib)
        a = self._args
        if not self.handle:
            raise FailedPreconditionError(
                "ctcext_stream_token_times without a ctcext_stream_push_dense that had hypothesis outputs",
                _lib.CTCEXT_FAILED_PRECONDITION)
        import torch
        out, o = _times_device(torch.device("cuda", self.dec.device), int(a.batch_size), int(a.top_paths),
                               int(a.max_frames))
        rc = lib.ctcext_stream_token_times(self.handle, ctypes.byref(o))
        if rc != _lib.CTCEXT_OK:
            _raise(lib, rc)
        return out

    def token_scores_dense(self, times=None):
        """``dense_token_scores`` for the last ``push_dense`` with results of a
        ``token_scores=True`` stream: ``TokenScores(logp_sum, logp_min)`` of
        everything pushed so far, CUDA tensors of the compute dtype
        ``[B, top_paths, max_frames]``, NaN everywhere but the timed tokens,
        enqueued behind that push on its stream (so the push, the times and
        the scores can be captured together).  ``times`` is what
        ``token_times_dense()`` returned for that push; None calls it here.
        ``FailedPreconditionError`` on a stream without ``token_scores=True``,
        after a ``results=False`` push or before any ``push_dense``."""
        self._check_open()
        lib = self.lib
        if not hasattr(lib, "ctcext_stream_token_scores"):
            raise UnimplementedError("this libctcext.so has no token scores for streams "
                                     "(CTCEXT_HAS_STREAM_SCORES)", _lib.CTCEXT_UNIMPLEMENTED)
        a = self._args
        if self._scores is None:
            raise FailedPreconditionError(
                "ctcext_stream_token_scores on a stream without a score store (ctcext_stream_open_scores)",
                _lib.CTCEXT_FAILED_PRECONDITION)
        if not self.handle:
            raise FailedPreconditionError(
                "ctcext_stream_token_scores without a ctcext_stream_push_dense that had hypothesis outputs",
                _lib.CTCEXT_FAILED_PRECONDITION)
        import torch
        dev = torch.device("cuda", self.dec.device)
        B, P, F = int(a.batch_size), int(a.top_paths), int(a.max_frames)
        if times is None:
            times = self.token_times_dense()
        for name, v in (("start", times.start), ("end", times.end)):
            if not (_is_torch(v) and v.is_cuda and v.device == dev and tuple(v.shape) == (B, P, F)
                    and str(v.dtype) == "torch.int32" and v.is_contiguous()):
                raise ValueError("times.%s must be a contiguous int32 tensor of shape %s on %s" % (name, (B, P, F), dev))
        t = _lib.TokenTimesOut()
        t.start, t.end = times.start.data_ptr(), times.end.data_ptr()
        out, o = _scores_device(dev, B, P, F, torch.float32 if a.dtype == _lib.CTCEXT_F32 else torch.float64)
        rc = lib.ctcext_stream_token_scores(self.handle, ctypes.byref(t), ctypes.byref(o))
        if rc != _lib.CTCEXT_OK:
            _raise(lib, rc)
        return out

    def path_scores_dense(self):
        """``dense_path_scores`` for the last ``push_dense`` with results of a
        ``token_scores=True`` stream: the exact CTC log-likelihood of every
        hypothesis over everything pushed to its item since the item's last
        reset, a CUDA tensor ``[B, top_paths]`` of the compute dtype, enqueued
        behind that push on its stream.  ``FailedPreconditionError`` on a
        stream without ``token_scores=True``, after a ``results=False`` push
        or before any ``push_dense``."""
        self._check_open()
        lib = self.lib
        if not hasattr(lib, "ctcext_stream_path_scores"):
            raise UnimplementedError("this libctcext.so has no path scores (CTCEXT_HAS_PATH_SCORES)",
                                     _lib.CTCEXT_UNIMPLEMENTED)
        a = self._args
        if self._scores is None:
            raise FailedPreconditionError(
                "ctcext_stream_path_scores on a stream without a score store (ctcext_stream_open_scores)",
                _lib.CTCEXT_FAILED_PRECONDITION)
        if not self.handle:
            raise FailedPreconditionError(
                "ctcext_stream_path_scores without a ctcext_stream_push_dense that had hypothesis outputs",
                _lib.CTCEXT_FAILED_PRECONDITION)
        import torch
        dev = torch.device("cuda", self.dec.device)
        with torch.cuda.device(dev):
            out = torch.empty((int(a.batch_size), int(a.top_paths)),
                              dtype=torch.float32 if a.dtype == _lib.CTCEXT_F32 else torch.float64, device=dev)
        rc = lib.ctcext_stream_path_scores(self.handle, out.data_ptr())
        if rc != _lib.CTCEXT_OK:
            _raise(lib, rc)
        return out

    def scores_ms(self):
        """Diagnostics: ``(append_ms, scores_ms)``, the times of the score
        store's append kernel in the last ``flags=CTCEXT_FLAG_PROFILE``
        ``push_dense`` and of the ``token_scores_dense`` kernel behind it (0
        where there was none).  Waits."""
        self._check_open()
        if not hasattr(self.lib, "ctcext_stream_scores_ms"):
            raise UnimplementedError("this libctcext.so has no token scores for streams "
                                     "(CTCEXT_HAS_STREAM_SCORES)", _lib.CTCEXT_UNIMPLEMENTED)
        if not self.handle:
            raise FailedPreconditionError("no CTCEXT_FLAG_PROFILE enqueue-only push on this stream yet",
                                          _lib.CTCEXT_FAILED_PRECONDITION)
        a_ms, s_ms = ctypes.c_double(), ctypes.c_double()
        rc = self.lib.ctcext_stream_scores_ms(self.handle, ctypes.byref(a_ms), ctypes.byref(s_ms))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)
        return a_ms.value, s_ms.value

    def token_times_ms(self):
        """Diagnostics: the token-times kernel's time in ms of the last
        ``token_times_dense`` after a ``flags=CTCEXT_FLAG_PROFILE`` push.  Waits."""
        self._check_open()
        ms = ctypes.c_double()
        rc = self.lib.ctcext_stream_token_times_ms(self.handle, ctypes.byref(ms))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)
        return ms.value

    def reserve(self, max_chunk_time):
        """Size the stream's workspace for ``push_dense`` of chunks of up to
        ``max_chunk_time`` frames (may allocate and block; launches nothing).
        Opens the stream for CUDA chunks if no push has yet."""
        self._check_open()
        if not self.handle:
            self._open(True, self._device if self._device is not None else _current_device())
        rc = self.lib.ctcext_stream_reserve(self.handle, int(max_chunk_time))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)

    def check(self):
        """Wait for the ``push_dense`` calls made so far and report them as
        ``push`` would have: raises the same ``OpError`` subclass with the same
        message for the first of -- a length above its chunk's frames (lowest
        item), the stream's capacity exceeded (lowest item), a helper hand-over
        timeout, "Less leaves in the beam search than requested." -- over all
        pushes since the previous ``check()``, which it then forgets.  Returns
        the stats dict (cumulative counters, as after ``push``)."""
        self._check_open()
        if not self.handle:
            return self.last_stats
        rc = self.lib.ctcext_stream_check(self.handle)
        self.last_stats = self.dec.last_stats = self.dec.stats()
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)
        _print_no_label(self.last_stats["no_label_paths"])
        return self.last_stats

    def commit_ms(self):
        """Diagnostics: the commit kernel's time in ms of the last ``push_dense``
        made with ``flags=CTCEXT_FLAG_PROFILE``, after its ``check()``."""
        self._check_open()
        ms = ctypes.c_double()
        rc = self.lib.ctcext_stream_commit_ms(self.handle, ctypes.byref(ms))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)
        return ms.value


GreedyPush = collections.namedtuple(
    "GreedyPush",
    ["decoded", "decoded_lengths", "alignment", "alignment_lengths", "log_probability", "status", "frames", "times",
     "scores"])


class _DeviceRows:
    """Device memory the library owns, as ``__cuda_array_interface__``: torch wraps it without a copy."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr or 0), False),
                                         "version": 2, "strides": None}


class GreedyStream:
    """Streaming greedy decode: push the logits of a batch in chunks of frames
    and read, after each push, the best-path hypothesis of everything pushed so
    far, with its token times and token confidences -- bit for bit what
    ``decode_greedy``, ``dense_token_times`` and ``dense_token_scores`` give for
    the concatenated frames (include/ctcext.h, "Streaming: greedy").  A push is
    one kernel over the chunk alone: its cost does not grow with the frames
    pushed so far, and the stream keeps neither logits nor beam records.

        with GreedyStream(batch_size, num_classes, max_frames, token_scores=True) as s:
            for chunk in chunks:                 # [B, t, C] each (batch_first), t may vary
                out = s.push(chunk, lengths)     # lengths: frames of this chunk per item (None: all t)
            s.check()

    ``max_frames`` is the capacity per item and the width of every row.
    ``dtype`` is the compute and output type; ``"float32"`` streams take
    float16 / bfloat16 / float32 chunks, ``"float64"`` ones float64.  With
    ``token_times`` / ``token_scores`` the stream keeps ``TokenTimes`` /
    ``TokenScores`` as well; both need a ``blank_label`` that is no class label.
    Not covered: ``skip_blank``, host chunks, a scorer, path scores and path
    alignments over the stream."""

    def __init__(self, batch_size, num_classes, max_frames, *, dtype="float32", merge_repeated=False, blank_index=0,
                 blank_label=-1, pad_value=-1, device=None, token_times=True, token_scores=False, flags=0):
        self.lib = _lib.load()
        if not hasattr(self.lib, "ctcext_greedy_stream_open"):
            raise UnimplementedError("this libctcext.so has no greedy stream (CTCEXT_HAS_GREEDY_STREAM)",
                                     _lib.CTCEXT_UNIMPLEMENTED)
        name = np.dtype(dtype).name if not isinstance(dtype, str) else dtype
        if name not in ("float32", "float64"):
            _type_error("dtype", name, "float32, float64")
        self._np_dtype = np.dtype(name)
        a = _lib.StreamArgs()
        a.dtype = _lib.CTCEXT_F32 if name == "float32" else _lib.CTCEXT_F64
        a.on_device = 1
        a.batch_size, a.num_classes, a.max_frames = int(batch_size), int(num_classes), int(max_frames)
        a.beam_width, a.top_paths = 1, 1
        a.merge_repeated = 1 if merge_repeated else 0
        a.blank_index, a.blank_label, a.flags = int(blank_index), int(blank_label), int(flags)
        w = _lib.GreedyStreamWant()
        w.token_times, w.token_scores, w.pad_value = int(bool(token_times)), int(bool(token_scores)), int(pad_value)
        self._args, self._want = a, w
        # the attribute checks run on the host now; the stream itself opens with the first push
        rc = self.lib.ctcext_greedy_stream_validate(ctypes.byref(a), ctypes.byref(w))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)
        self._device = _device_index(device)
        self.on_device = True
        self.dec = self.handle = self._out = None
        self.closed = False

    # -- lifetime ----------------------------------------------------------
    def _open(self, index):
        if self._device is not None and index != self._device:
            raise ValueError("the chunk lives on cuda:%d, the stream on cuda:%d" % (index, self._device))
        self.dec = get_decoder(index)
        h = ctypes.c_void_p()
        rc = self.lib.ctcext_greedy_stream_open(self.dec.handle, ctypes.byref(self._args), ctypes.byref(self._want),
                                                ctypes.byref(h))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)
        self.handle = h

    def _wrap(self, o, dev):
        """The stream's rows as torch tensors over the library's memory (made once)."""
        import torch
        a = self._args
        B, F = int(a.batch_size), int(a.max_frames)
        f = "<f4" if a.dtype == _lib.CTCEXT_F32 else "<f8"

        def t(ptr, shape, typestr):
            return None if not ptr else torch.as_tensor(_DeviceRows(ptr, shape, typestr), device=dev)
        times = scores = None
        if self._want.token_times:
            times = TokenTimes(t(o.start, (B, 1, F), "<i4"), t(o.end, (B, 1, F), "<i4"),
                               t(o.trailing_blank, (B, 1), "<i4"))
        if self._want.token_scores:
            scores = TokenScores(t(o.logp_sum, (B, 1, F), f), t(o.logp_min, (B, 1, F), f))
        return GreedyPush(t(o.decoded, (B, 1, F), "<i8"), t(o.decoded_length, (B, 1), "<i4"),
                          t(o.alignment, (B, 1, F), "<i8"), t(o.alignment_length, (B, 1), "<i4"),
                          t(o.log_probability, (B, 1), f), t(o.status, (B,), "<i4"), t(o.frames, (B,), "<i4"),
                          times, scores)

    def close(self):
        """Frees the stream and its rows: the tensors a push returned must not be touched afterwards."""
        if self.handle and self.dec is not None and self.dec.handle:
            self.lib.ctcext_greedy_stream_close(self.handle)
        self.handle = self._out = None
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_open(self):
        if self.closed:
            raise FailedPreconditionError("the stream is closed", _lib.CTCEXT_FAILED_PRECONDITION)

    # -- the push ------------------------------------------------------------
    def push(self, chunk, lengths=None, *, reset=None, batch_first=True):
        """Take the chunk's frames without waiting for anything: one kernel on
        ``torch.cuda.current_stream()``, behind whatever produced the chunk.
        With ``lengths`` and ``reset`` None or contiguous int32 CUDA tensors,
        and a chunk whose layout needs no copy, a push after the first
        allocates nothing and can be captured into a ``torch.cuda.graph`` as a
        single kernel node; a CUDA tensor of another integer dtype or layout is
        converted on the device first, which allocates.

        ``chunk`` is a CUDA tensor ``[B, t, C]`` (``[t, B, C]`` without
        ``batch_first``), strided views included; ``lengths`` and ``reset``
        are CUDA tensors of ``[B]`` (anything else raises ``ValueError``).
        ``reset[b] != 0`` starts a new utterance in item b with this chunk.

        Returns ``GreedyPush(decoded [B, 1, max_frames], decoded_lengths,
        alignment, alignment_lengths, log_probability, status, frames, times,
        scores)``; ``times`` is a ``TokenTimes`` or None, ``scores`` a
        ``TokenScores`` or None.  These are the stream's own tensors, the same
        objects after every push, updated in place by the next one: clone what
        must outlive the next push, and touch none of them after ``close()``.

        An item whose length is above the chunk's frames
        (``CTCEXT_ITEM_LENGTH``) or would pass ``max_frames``
        (``CTCEXT_ITEM_CAPACITY``) takes no frame: ``status[b]`` carries the bit
        for this push only and its rows stay as they were.  ``check()`` waits
        and raises."""
        self._check_open()
        if not (_is_torch(chunk) and chunk.is_cuda):
            raise ValueError("GreedyStream.push takes CUDA torch tensors")
        for name, t in (("lengths", lengths), ("reset", reset)):
            if t is not None and not (_is_torch(t) and t.is_cuda):
                raise ValueError("GreedyStream.push takes %s as a CUDA torch tensor" % name)
        c, x, sl, _, dev, index = _stream_chunk(self._args, self._np_dtype, True, chunk, lengths, batch_first, 0)
        B = int(self._args.batch_size)
        rs = None
        if reset is not None:
            rs = _lengths_device(reset, dev)
            if tuple(rs.shape) != (B,):
                raise ValueError("reset must have shape [batch_size] = [%d], got %s" % (B, tuple(rs.shape)))
        if not c.stream:   # torch's legacy default stream: the null stream itself, not the decoder's own
            c.flags |= _lib.CTCEXT_FLAG_DENSE_NULL_STREAM
        if not self.handle:
            self._open(index)
        o = _lib.GreedyStreamOutputs()
        rc = self.lib.ctcext_greedy_stream_push(self.handle, ctypes.byref(c), None if rs is None else rs.data_ptr(),
                                                ctypes.byref(o))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)
        if self._out is None:
            self._out = self._wrap(o, dev)
        # x, sl and rs may be temporaries: they were allocated on this stream, and
        # the caching allocator hands their memory out again in stream order
        del x, sl, rs
        return self._out

    def check(self):
        """Wait for the torch stream of the last push (pushes made on other
        streams are the caller's to order) and raise what ``StreamDecoder.check()``
        raises for a length above its chunk's frames (lowest item) or the
        stream's capacity exceeded (lowest item), over all pushes since the
        previous ``check()``, which it then forgets."""
        self._check_open()
        if self.handle:
            rc = self.lib.ctcext_greedy_stream_check(self.handle)
            if rc != _lib.CTCEXT_OK:
                _raise(self.lib, rc)

    @property
    def frames(self):
        """Frames taken so far per item: numpy int64 [batch_size].  Waits for the stream of the last push."""
        self._check_open()
        out = np.zeros((int(self._args.batch_size),), np.int64)
        if self.handle:
            rc = self.lib.ctcext_greedy_stream_frames(self.handle, out.ctypes.data)
            if rc != _lib.CTCEXT_OK:
                _raise(self.lib, rc)
        return out

    def reset(self, items=None):
        """Put ``items`` (None: all) back to no frames and empty rows; the others' rows and state are untouched.
        Waits; afterwards ``status`` reads 0 and ``frames`` the counts, as after a push without frames."""
        self._check_open()
        if not self.handle:
            return
        if items is None:
            rc = self.lib.ctcext_greedy_stream_reset(self.handle, None, 0)
        else:
            arr = np.ascontiguousarray(np.asarray(items, dtype=np.int32).reshape(-1))
            rc = self.lib.ctcext_greedy_stream_reset(self.handle, arr.ctypes.data, int(arr.size))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)

    def push_ms(self):
        """Diagnostics: the kernel's time in ms of the last push of a stream made with ``flags=CTCEXT_FLAG_PROFILE``."""
        self._check_open()
        ms = ctypes.c_double()
        rc = self.lib.ctcext_greedy_stream_push_ms(self.handle, ctypes.byref(ms))
        if rc != _lib.CTCEXT_OK:
            _raise(self.lib, rc)
        return ms.value


def _ptr(arr, ctype):
    return arr.ctypes.data_as(ctypes.POINTER(ctype))


def _device_index(device):
    """``device`` (None, an ordinal, a ``torch.device`` or a string such as
    "cuda:1") as a device ordinal, or None when it names none."""
    if device is None:
        return None
    if isinstance(device, (int, np.integer)) and not isinstance(device, bool):
        return int(device)
    import torch
    if isinstance(device, (str, torch.device)):
        d = torch.device(device)
        if d.type != "cuda":
            raise ValueError("a StreamDecoder runs on a GPU: device must be a cuda device, not %r" % (device,))
        return d.index
    raise TypeError("device must be None, an int, a torch.device or a string, not %s" % type(device).__name__)


def _fetch_outputs(dec, sizes, B, P, code, to_device):
    """Phase 2 for a decoder whose fetch state a decode or a stream push has
    set: allocate the seven outputs (device tensors on the decoder's device, or
    pinned host arrays) from the per-path ``sizes`` and fill them."""
    if to_device:
        import torch
        dev = torch.device("cuda", dec.device)
        i64 = dict(dtype=torch.int64, device=dev)
        di = [torch.empty((s[0], 2), **i64) for s in sizes]
        dv = [torch.empty((s[0],), **i64) for s in sizes]
        ds = [torch.empty((2,), **i64) for _ in sizes]
        ai = [torch.empty((s[2], 2), **i64) for s in sizes]
        av = [torch.empty((s[2],), **i64) for s in sizes]
        ash = [torch.empty((2,), **i64) for _ in sizes]
        lp = torch.empty((B, P), dtype=torch.float32 if code == _lib.CTCEXT_F32 else torch.float64, device=dev)
        lists = [[t.data_ptr() for t in lst] for lst in (di, dv, ds, ai, av, ash)]
        dec.fetch(lists, lp.data_ptr(), True)
    else:
        empty = _host_empty()
        fdt = np.float32 if code == _lib.CTCEXT_F32 else np.float64
        di = [empty((s[0], 2), np.int64) for s in sizes]
        dv = [empty((s[0],), np.int64) for s in sizes]
        ds = [empty((2,), np.int64) for _ in sizes]
        ai = [empty((s[2], 2), np.int64) for s in sizes]
        av = [empty((s[2],), np.int64) for s in sizes]
        ash = [empty((2,), np.int64) for _ in sizes]
        lp = empty((B, P), fdt)
        lists = [[t.ctypes.data for t in lst] for lst in (di, dv, ds, ai, av, ash)]
        dec.fetch(lists, lp.ctypes.data, False)
    return CTCExtBeamSearchDecoder(di, dv, ds, ai, av, ash, lp)
