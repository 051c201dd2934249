"""ctypes front-end of a compiled build of the REFERENCE decoder (TEST
INFRASTRUCTURE ONLY): oracle/_ref/libctc_ref.so, made by oracle/ref/Makefile
from the reference tree's own headers where that tree is present.

``raw_decode`` takes and returns what ``oracle.raw_decode`` does, and raises
``oracle.OracleError`` with the reference Status' own message.  With a
``scorer_table`` the reference decoder runs with a scorer of the driver's,
derived from the reference's BaseBeamScorer over its default EmptyBeamState:
the per-state value lives in a side table keyed by the state object's address
(ref_driver.cpp says why that is sound), and ``hook_stats`` receives the counts
that show it held during the call.  The op's input validation is not in the
reference's headers but in kernels.cc; the checks here are the oracle's, made
before the library is called.

Keep NaN and +inf out of the inputs: the row view's maxCoeff (ref_driver.cpp)
is Eigen's only on rows without NaN.
"""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

from oracle import OracleError

_HERE = os.path.dirname(os.path.abspath(__file__))
RECIPE = os.path.join(_HERE, "ref")
LIB_PATH = os.path.join(_HERE, "_ref", "libctc_ref.so")
HEADERS = ("ctc_ext_beam_search_decoder.h", "ctc_beam_entry.h", "ctc_beam_scorer.h", "ctc_loss_util.h",
           "ctc_ext_decoder.h")


class _Result(ctypes.Structure):
    _fields_ = [("ok", ctypes.c_int32), ("failed_item", ctypes.c_int32), ("no_label_lines", ctypes.c_int32),
                ("message", ctypes.c_char * 256),
                ("total_dec", ctypes.c_int64), ("total_ali", ctypes.c_int64),
                ("dec_len", ctypes.POINTER(ctypes.c_int64)), ("ali_len", ctypes.POINTER(ctypes.c_int64)),
                ("dec_vals", ctypes.POINTER(ctypes.c_int32)), ("ali_vals", ctypes.POINTER(ctypes.c_int32)),
                ("log_prob", ctypes.POINTER(ctypes.c_double))]


_lib = None


def tree():
    """The reference tree the recipe compiles from (make's REF_TREE), or None
    where it is absent."""
    out = subprocess.check_output(["make", "-s", "-C", RECIPE, "print-ref-util"]).decode().strip()
    return out if os.path.exists(os.path.join(out, HEADERS[0])) else None


def header_sha256():
    """{header name: sha256} of the reference headers the library compiles."""
    util = tree()
    assert util is not None, "no reference tree"
    return {h: hashlib.sha256(open(os.path.join(util, h), "rb").read()).hexdigest() for h in HEADERS}


def build():
    subprocess.check_call(["make", "-s", "-C", RECIPE])


def available():
    return os.path.exists(LIB_PATH)


def _load():
    global _lib
    if _lib is None:
        lib = ctypes.CDLL(LIB_PATH)
        lib.ref_decode.restype = ctypes.POINTER(_Result)
        lib.ref_decode.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        lib.ref_decode_scored.restype = ctypes.POINTER(_Result)
        lib.ref_decode_scored.argtypes = lib.ref_decode.argtypes + [ctypes.c_void_p, ctypes.c_void_p]
        lib.ref_free.argtypes = [ctypes.POINTER(_Result)]
        _lib = lib
    return _lib


HOOK_STATS = ("initialize_state", "expand_state", "lookups", "lookups_without_state", "reexpansions_differ",
              "end_hook_calls")


def raw_decode(inputs, sequence_length, beam_width, top_paths, merge_repeated=False,
               blank_index=0, blank_label=-1, scorer_table=None, hook_stats=None):
    """(dec, ali, log_prob, no_label_events) as oracle.raw_decode: dec[b][p] and
    ali[b][p] lists of ints, log_prob [B, P] of the inputs' dtype.
    ``scorer_table`` ([C + 1, C], the inputs' dtype; row ``from_label + 1``, row 0
    the root's): the driver's table scorer; None is BaseBeamScorer through
    ref_decode, as before.  ``hook_stats`` (a dict, with a table only) receives
    the HOOK_STATS counts of the call, also when it ends in an error."""
    x = np.ascontiguousarray(inputs)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError("inputs must be float32 or float64")
    if x.ndim != 3:
        raise OracleError("inputs is not a 3-Tensor")
    T, B, C = x.shape
    if T == 0:
        raise OracleError("max_time is 0")
    sl = np.ascontiguousarray(np.asarray(sequence_length, dtype=np.int32))
    if sl.ndim != 1:
        raise OracleError("sequence_length is not a vector")
    if sl.shape[0] != B:
        raise OracleError("len(sequence_length) != batch_size.  len(sequence_length):  %d batch_size: %d"
                          % (sl.shape[0], B))
    for b in range(B):
        if not sl[b] <= T:
            raise OracleError("sequence_length(%d) <= %d" % (b, T))
    if not 0 <= blank_index < C:
        raise OracleError("blank_index out of range")
    assert not np.isnan(x).any() and not np.isposinf(x).any(), "NaN / +inf are outside the reference build's scope"
    lib = _load()
    P = int(top_paths)
    args = (0 if x.dtype == np.float32 else 1, x.ctypes.data, sl.ctypes.data, B, C,
            int(beam_width), P, int(bool(merge_repeated)), int(blank_index), int(blank_label))
    if scorer_table is None:
        assert hook_stats is None, "hook_stats needs a scorer_table"
        r = lib.ref_decode(*args)
    else:
        tab = np.ascontiguousarray(np.asarray(scorer_table, dtype=x.dtype))
        if tab.shape != (C + 1, C):
            raise ValueError("scorer_table must be [num_classes + 1, num_classes]")
        assert not np.isnan(tab).any() and not np.isposinf(tab).any(), "NaN / +inf are outside the reference build's scope"
        counts = np.full(len(HOOK_STATS), -1, np.int64)
        r = lib.ref_decode_scored(*args, tab.ctypes.data, counts.ctypes.data)
        if hook_stats is not None:
            hook_stats.update(zip(HOOK_STATS, counts.tolist()))
    try:
        res = r.contents
        if not res.ok:
            raise OracleError(res.message.decode())
        n = B * P
        dl = np.ctypeslib.as_array(res.dec_len, (n + 1,))[:n].copy()
        al = np.ctypeslib.as_array(res.ali_len, (n + 1,))[:n].copy()
        dv = np.ctypeslib.as_array(res.dec_vals, (int(res.total_dec) + 1,))[:res.total_dec].copy()
        av = np.ctypeslib.as_array(res.ali_vals, (int(res.total_ali) + 1,))[:res.total_ali].copy()
        lp = np.ctypeslib.as_array(res.log_prob, (n + 1,))[:n].copy().reshape(B, P)
        events = int(res.no_label_lines)
    finally:
        lib.ref_free(r)
    dec, ali = [], []
    od = oa = 0
    for b in range(B):
        db, ab = [], []
        for p in range(P):
            i = b * P + p
            db.append(dv[od:od + dl[i]].tolist()); od += dl[i]
            ab.append(av[oa:oa + al[i]].tolist()); oa += al[i]
        dec.append(db)
        ali.append(ab)
    return dec, ali, lp.astype(x.dtype), events
