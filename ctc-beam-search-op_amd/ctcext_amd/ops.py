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
    # x, sl and tab may be temporaries: they were allocated on this stream, and
    # the caching allocator hands their memory out again in stream order
    del x, sl, tab
    return out


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
        """The ``ctcext_chunk`` of one push: ``(c, x, sl, on_device, dev, index)``,
        x and sl being the tensors or arrays c points into."""
        a = self._args
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
            x = chunk if isinstance(chunk, np.ndarray) else np.asarray(chunk, dtype=self._np_dtype)
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
        if self.on_device is not None and on_device != self.on_device:
            raise ValueError("this stream's chunks live on the %s (fixed by its first push)"
                             % ("device" if self.on_device else "host"))
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
