"""Blank-frame skipping for streams without a GPU (include/ctcext.h,
"Streaming: blank-frame skipping"): the host restatement of the chunked plan,
ctcext_skip_plan_chunk_row, chained over the splits of a row against
skip_util.skip_plan of the whole; the argument errors of
ctcext_stream_open_skip that need no device; the header's constants; and what
the Python entry points decide on the host."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest

import ctcext_amd
import skip_util as su
import stream_skip_util as ssu
from ctcext_amd import _lib
from test_cpu_stream import _sargs

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctcext.h")
INV, UNIMPL = _lib.CTCEXT_INVALID_ARGUMENT, _lib.CTCEXT_UNIMPLEMENTED
M_THR = "blank skip threshold must be a log-probability (<= 0)"
NAN = float("nan")

# hand-written rows of log-probabilities of the blank against thr = log 0.9
# (D: blank-dominant, n: not, NaN: never dominant): every pattern of a run at
# the start, the end and across any boundary a split can put into it
D, N = -0.01, -3.0
ROWS = [
    [],
    [D],
    [N],
    [D, D],
    [N, D, D, D],
    [D, D, D, D, D, D, D, D],
    [N, N, N, N, N, N, N, N],
    [D, N, D, D, N, D, D, D],
    [D, D, NAN, D, D, N, D, D],
    [NAN, D, D, D, NAN, NAN, D, N],
    [N, D, D, N, N, D, N, D],
    [D, D, D, N, D, D, D],
]


def _chained(row, cuts, dtype, thr):
    """ctcext_skip_plan_chunk_row over the pieces of `row` between `cuts`
    (ascending positions, repeats allowed: an n == 0 piece), each started from
    the flag the piece before it returned: (kmap, flags after each piece)."""
    lib = _lib.load()
    arr = np.asarray(row, dtype)
    kmap, flags, dom = [], [], 0
    edges = [0] + list(cuts) + [len(row)]
    for lo, hi in zip(edges[:-1], edges[1:]):
        n = hi - lo
        piece = np.ascontiguousarray(arr[lo:hi])
        out = np.full((max(n, 1),), -99, np.int32)
        kept, last = ctypes.c_int64(-1), ctypes.c_int32(-1)
        rc = lib.ctcext_skip_plan_chunk_row(piece.ctypes.data if n else None, 1 if dtype == np.float64 else 0, n,
                                            thr, lo, dom, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                            ctypes.byref(kept), ctypes.byref(last))
        assert rc == _lib.CTCEXT_OK
        assert 0 <= kept.value <= n and last.value in (0, 1)
        if n == 0:
            assert last.value == dom   # an empty piece leaves the flag alone
        kmap += out[:kept.value].tolist()
        dom = last.value
        flags.append(dom)
    return kmap, flags


def _splits(n):
    """Every set of cut positions of a row of n frames, plus some with a repeated cut."""
    for k in range(n):
        for cuts in itertools.combinations(range(1, n), k):
            yield cuts
    for p in range(n + 1):
        yield (p, p)
    if n >= 2:
        yield (0, 0, 1, 1, n, n)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float", "double"])
def test_chunk_row_chained_over_every_split_of_the_hand_written_rows(dtype):
    assert any(math.isnan(v) for r in ROWS for v in r)
    empty = 0
    for row in ROWS:
        arr = np.asarray(row, dtype)
        want = su.skip_plan(arr, len(row), dtype(su.THR))
        for cuts in _splits(len(row)):
            got, flags = _chained(row, cuts, dtype, su.THR)
            assert got == want, (row, cuts, got, want)
            if row:
                assert flags[-1] == int(arr[-1] > dtype(su.THR)), (row, cuts)
            edges = [0] + list(cuts) + [len(row)]
            empty += sum(a == b for a, b in zip(edges[:-1], edges[1:]))
    assert empty > 20   # n == 0 pieces were in the chains
    # the rule reads the absolute frame: a dominant frame 0 is kept whatever flag is handed in ...
    lib = _lib.load()
    one = np.asarray([D], dtype)
    out = np.zeros((1,), np.int32)
    kept, last = ctypes.c_int64(), ctypes.c_int32()
    args = (out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(kept), ctypes.byref(last))
    f64 = 1 if dtype == np.float64 else 0
    assert lib.ctcext_skip_plan_chunk_row(one.ctypes.data, f64, 1, su.THR, 0, 1, *args) == 0
    assert (kept.value, out[0], last.value) == (1, 0, 1)
    # ... and any later one behind a dominant frame is not
    assert lib.ctcext_skip_plan_chunk_row(one.ctypes.data, f64, 1, su.THR, 5, 1, *args) == 0
    assert (kept.value, last.value) == (0, 1)
    assert lib.ctcext_skip_plan_chunk_row(one.ctypes.data, f64, 1, su.THR, 5, 0, *args) == 0
    assert (kept.value, out[0], last.value) == (1, 5, 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float", "double"])
def test_chunk_row_chained_over_random_rows(dtype):
    rng = np.random.default_rng(7)
    for trial in range(60):
        n = int(rng.integers(20, 400))
        lp = -np.abs(rng.standard_normal(n)).astype(dtype) * 0.3
        lp[rng.random(n) < 0.03] = np.nan
        thr = float(np.nanmedian(lp)) if trial % 2 else su.THR
        want = su.skip_plan(lp, n, dtype(thr))
        cuts = sorted(rng.integers(0, n + 1, size=int(rng.integers(0, 12))).tolist())
        got, _ = _chained(lp, cuts, dtype, thr)
        assert got == want, (trial, n, cuts)
        assert len(want) < n or trial % 2 == 0   # (the median threshold drops frames)
    # thr = 0 keeps every frame of any split
    lp = -np.abs(rng.standard_normal(50)).astype(dtype)
    lp[::7] = 0
    assert _chained(lp, (10, 10, 33), dtype, 0.0)[0] == list(range(50))


def test_chunk_row_rejects_bad_arguments():
    lib = _lib.load()
    one = np.zeros((4,), np.float32)
    out = np.zeros((4,), np.int32)
    kept, last = ctypes.c_int64(), ctypes.c_int32()
    km = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def call(lp=one.ctypes.data, n=4, thr=su.THR, first=0, dom=0, kmap=km, k=ctypes.byref(kept), l=ctypes.byref(last)):
        return lib.ctcext_skip_plan_chunk_row(lp, 0, n, thr, first, dom, kmap, k, l)

    assert call() == 0
    for bad in (dict(n=-1), dict(first=-1), dict(thr=0.1), dict(thr=NAN), dict(lp=None), dict(kmap=None),
                dict(k=None), dict(l=None), dict(first=2 ** 31 - 2)):
        assert call(**bad) == INV, bad
    assert call(lp=None, kmap=None, n=0, dom=1) == 0 and last.value == 1 and kept.value == 0


def test_schedule_helpers():
    """The test helpers themselves, on a plan small enough to read."""
    sched = ssu.schedule([5, 2, 0], 2)
    assert sched == [[2, 2, 0], [2, 0, 0], [1, 0, 0]] and ssu.schedule([5, 2, 0], None) == [[5, 2, 0]]
    # item 0 keeps frames 0, 3: push 1 (frames 2, 3) begins with a dropped frame, push 2 (frame 4) is all dropped
    assert ssu.exercised([[0, 3], [0, 1], []], sched) == (1, 2)
    x = np.arange(5 * 3 * 1, dtype=np.float32).reshape(5, 3, 1)
    c = ssu.chunk(x, [2, 0, 0], [2, 1, 0])
    assert c.shape == (2, 3, 1) and c[:, 0, 0].tolist() == [6, 9] and c[:, 1, 0].tolist() == [1, 0]


def _open_skip(a, k, handle=None):
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.ctcext_stream_open_skip(handle, ctypes.byref(a) if a is not None else None,
                                     ctypes.byref(k) if k is not None else None, ctypes.byref(h))
    assert not h.value
    return rc, lib.ctcext_last_error().decode()


def _skip(thr=su.THR):
    k = _lib.SkipArgs()
    k.logp_threshold = thr
    return k


def test_open_skip_argument_errors_need_no_device():
    """In their order, each with a message of its own; the decoder handle is
    looked at last, so all of them answer without one."""
    a = _sargs()
    a.on_device = 1
    assert _open_skip(None, _skip()) == (INV, "null argument")
    bad = _sargs(W=0)
    bad.on_device = 1
    rc, msg = _open_skip(bad, _skip())
    assert rc == INV and msg and msg != "null argument"   # ctcext_stream_validate's own
    rc, m_null = _open_skip(a, None)
    assert rc == INV and "skip arguments" in m_null
    for thr in (1e-9, NAN):
        assert _open_skip(a, _skip(thr)) == (INV, M_THR)
    host = _sargs()
    host.on_device = 0
    rc, m_host = _open_skip(host, _skip())
    assert rc == INV and "device chunks" in m_host
    assert len({m_null, M_THR, m_host}) == 3
    # all of them in order: the stream arguments first, then skip, its threshold, on_device
    assert _open_skip(host, _skip(0.5)) == (INV, M_THR)
    assert _open_skip(host, None)[1] == m_null
    # well-formed arguments without a handle
    assert _open_skip(a, _skip()) == (INV, "null argument")
    assert _open_skip(a, _skip(0.0)) == (INV, "null argument")
    lib = _lib.load()
    assert lib.ctcext_stream_kept(None, None) == INV


def test_header_and_abi():
    src = open(HEADER).read()
    assert "#define CTCEXT_HAS_STREAM_SKIP 1" in src
    for name in ("ctcext_stream_open_skip", "ctcext_stream_kept", "ctcext_skip_plan_chunk_row"):
        assert "int %s(" % name in src and hasattr(_lib.load(), name), name
    assert "#define CTCEXT_ABI_VERSION 8" in src and _lib.load().ctcext_abi_version() == 8


def test_python_entry_points_on_the_host():
    for thr in (1e-6, NAN):
        with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
            ctcext_amd.StreamDecoder(3, 6, 8, 2, 16, skip_blank=thr)
        assert e.value.message == M_THR
    s = ctcext_amd.StreamDecoder(3, 6, 8, 2, 16, skip_blank=su.THR)
    # the synchronous push is refused before anything is opened, and the stream stays as it was
    with pytest.raises(ctcext_amd.UnimplementedError) as e:
        s.push(np.zeros((3, 4, 6), np.float32))
    assert e.value.error_code == UNIMPL and "synchronous push" in e.value.message
    assert s.handle is None and not s.closed
    assert s.frames.tolist() == [0, 0, 0] and s.kept_frames().tolist() == [0, 0, 0]
    s.close()
    plain = ctcext_amd.StreamDecoder(3, 6, 8, 2, 16)
    assert plain.kept_frames().tolist() == [0, 0, 0]
    with pytest.raises(ctcext_amd.FailedPreconditionError):
        plain.kept_dense()
    plain.close()
