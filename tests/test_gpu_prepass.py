"""The large-vocabulary pre-pass alone (ctcext_row_facts, C ABI diagnostics
entry): each row's record -- maximum, NaN/+inf flag, 64-class block maxima,
the top set S and the largest non-blank value outside it -- checked against a
numpy restatement of its definition (S bit-exact, in order; the maxima and
the outside value by value, as +0.0 and -0.0 tie), on rows built to
stress the selection: ties at the boundary, -inf, signed zeros, fewer finite
labels than the set holds, the blank anywhere, C just above 64 up to 8196,
and both the register path (float, C % 4 == 0: ctcx_row_facts) and the LDS
path (ctcx_row_prep).  The decode parity tests cover the same records only
through their effect on results; S is the gather's exactness bound
(DESIGN.md "Kernels"), so it is pinned here directly.  The normaliser the
same launch writes (fused into ctcx_row_facts on the register path) is
checked bit-exact against the oracle's (oracle.row_norm, decoder.h:72-80),
NaN / +inf rows included, and rows past an item's length are left alone.
Rows of more than 8192 classes run ctcx_row_prep: with more than 64 KB of
dynamic LDS from C = 16384, with the row exactly filling its LDS stage at
C * sizeof(T) = 128 KB, and reading the row from global memory past that;
ctcext_stats.kernel says which of them ran.

The last part feeds every path the families of range_inputs (softmax terms in
expf's / exp's subnormal-result band, at and below the underflow bound, sums
near 1, one dominant class, logits near 1e6..3e7, overflowing differences,
subnormals): the normal rows above keep every term within [-30, 0] or at
-inf.  The census of each input is asserted, so a case cannot pass without
the values it exists for."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ctc-beam-search-op_amd"))

import oracle  # noqa: E402  (tests/conftest.py puts oracle/ on the path)
import range_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

K = 64   # kTopK


def _fkey(bits):
    u = bits.astype(np.uint64)
    return np.where(u >> 31, u ^ 0xFFFFFFFF, u ^ 0x80000000)


def _ref(row, blank):
    """(xmax, bad, block maxima, S bits, S label indices, xout) by definition:
    S = the non-blank labels whose order-preserving key lies above the (K+1)-th
    largest key (every label when there are at most K), in label order; xout =
    the largest non-blank value outside S (-inf: none)."""
    C = row.size
    bad = bool(np.isnan(row).any() or np.isposinf(row).any())
    xmax = np.float32(row.max())
    bmax = np.array([row[k:k + 64].max() for k in range(0, C, 64)], dtype=np.float32)
    cls = np.array([c for c in range(C) if c != blank])
    vals = row[cls]
    keys = _fkey(vals.view(np.uint32))
    lab = cls - (cls > blank)
    if C - 1 <= K:
        inS = np.ones(cls.size, bool)
        xout = np.float32(-np.inf)
    else:
        v = np.sort(keys)[::-1][K]
        inS = keys > v
        xout = vals[keys == v][0]
    return xmax, bad, bmax, vals[inS].view(np.uint32), lab[inS], np.float32(xout)


def _rows(rng, C, kind, n):
    x = rng.standard_normal((n, C)).astype(np.float32)
    if kind == "ties":
        x = (np.round(x * 2) / 2).astype(np.float32)
    elif kind == "neg_inf":
        x[rng.random((n, C)) < 0.4] = -np.inf
    elif kind == "few_finite":   # fewer finite labels than S holds
        x[:] = -np.inf
        for r in range(n):
            x[r, rng.choice(C, size=min(C, 10), replace=False)] = rng.standard_normal(min(C, 10))
    elif kind == "zeros":        # +0.0 / -0.0 (distinct keys, equal values)
        x = np.where(rng.random((n, C)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        x[:, : C // 7] = rng.standard_normal((n, C // 7)).astype(np.float32)
    elif kind == "flat":
        x[:] = np.float32(1.25)
    elif kind == "all_neg_inf":  # a row of -inf only: maximum -inf, every term NaN
        x[0, :] = -np.inf
        if n > 2:
            x[2, : C // 2] = -np.inf
    elif kind == "bad":
        x[0, C // 3] = np.nan
        if n > 1:
            x[1, C // 2] = np.inf
    return x


def _run(x_tb, C, blank, dtype=np.float32, seq_len=None):
    import torch
    import ctcext_amd
    from ctcext_amd import _lib
    T, B = x_tb.shape[:2]
    d = ctcext_amd.get_decoder(0)
    lib = d.lib
    rb = ctypes.c_int64()
    dt = _lib.CTCEXT_F64 if dtype == np.float64 else _lib.CTCEXT_F32
    xs = torch.as_tensor(np.ascontiguousarray(x_tb.astype(dtype)), device="cuda")
    if seq_len is None:
        seq_len = np.full(B, T, np.int32)
    sl = torch.as_tensor(np.asarray(seq_len, np.int32), device="cuda")
    assert lib.ctcext_row_facts(d.handle, None, dt, T, B, C, blank, None, None, None, ctypes.byref(rb)) == 0
    prep = torch.zeros(T * B * rb.value, dtype=torch.uint8, device="cuda")
    norm = torch.full((T * B,), 7.5, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    rc = lib.ctcext_row_facts(d.handle, ctypes.c_void_p(xs.data_ptr()), dt, T, B, C, blank,
                              ctypes.c_void_p(sl.data_ptr()), ctypes.c_void_p(prep.data_ptr()),
                              ctypes.c_void_p(norm.data_ptr()), ctypes.byref(rb))
    assert rc == 0, lib.ctcext_last_error()
    _run.prepass = d.stats()["kernel"]["prepass"]   # which pre-pass the launcher ran
    return prep.cpu().numpy().reshape(T * B, rb.value), norm.cpu().numpy()


def _check_norm(x_tb, norm, seq_len=None):
    T, B, C = x_tb.shape
    want = oracle.row_norm(x_tb.reshape(-1, C))
    live = np.ones((T, B), bool) if seq_len is None else np.arange(T)[:, None] < np.asarray(seq_len)[None, :]
    live = live.reshape(-1)
    got = norm
    same = (got.view(np.uint32 if got.dtype == np.float32 else np.uint64)
            == want.view(np.uint32 if want.dtype == np.float32 else np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert same[live].all(), (C, np.flatnonzero(live & ~same)[:8], got[live & ~same][:4], want[live & ~same][:4])
    assert (got[~live] == 7.5).all(), "rows past an item's length are not written"


def _check_f32(x_tb, C, blank, seq_len=None):
    rec, norm = _run(x_tb, C, blank, seq_len=seq_len)
    _check_norm(x_tb, norm, seq_len)
    rows = x_tb.reshape(-1, C)
    nblk = (C + 63) // 64
    top_off = 16 + ((nblk * 4 + 15) & ~15)
    live = None if seq_len is None else (np.arange(x_tb.shape[0])[:, None] < np.asarray(seq_len)[None, :]).reshape(-1)
    for r in range(rows.shape[0]):
        if live is not None and not live[r]:
            continue
        xmax, bad, bmax, sb, sl_, xout = _ref(rows[r], blank)
        h = rec[r]
        gmax = h[0:4].view(np.float32)[0]
        gbad = h[8:12].view(np.int32)[0]
        assert bool(gbad) == bad, (C, blank, r)
        if bad:
            continue
        # maxima by value: of equal values (+0.0 / -0.0) either may be kept
        assert gmax == xmax, (C, blank, r, gmax, xmax)
        assert np.array_equal(h[16:16 + 4 * nblk].view(np.float32), bmax), (C, blank, r)
        ns = h[12:16].view(np.int32)[0]
        gxout = h[4:8].view(np.float32)[0]
        assert ns == sb.size, (C, blank, r, ns, sb.size)
        top = h[top_off:top_off + 8 * ns].view(np.uint32).reshape(ns, 2)
        assert np.array_equal(top[:, 0], sb), (C, blank, r)
        assert np.array_equal(top[:, 1], sl_.astype(np.uint32)), (C, blank, r)
        assert gxout == xout, (C, blank, r, gxout, xout)


@pytest.mark.parametrize("C", [68, 256, 260, 1000, 2048, 5000, 8196, 65, 1001, 5001])
def test_row_facts_match_definition(C):
    rng = np.random.default_rng(7000 + C)
    for kind in ("normal", "ties", "neg_inf", "few_finite", "zeros", "flat", "all_neg_inf", "bad"):
        for blank in (0, C - 1, C // 2):
            x = _rows(rng, C, kind, 6).reshape(2, 3, C)
            _check_f32(x, C, blank)


@pytest.mark.parametrize("C", [124, 128, 512, 516, 772, 1020, 1024, 1028, 2048, 3072])
def test_row_facts_nv_boundaries(C):
    # the row widths at the edges of each compiled NV (and of the fused
    # normaliser's C <= 1024), 5 x 7 rows: the last block of eight (two rows
    # per wave, fused) or four rows only partly filled
    rng = np.random.default_rng(7200 + C)
    x = (rng.standard_normal((5, 7, C)) * 2).astype(np.float32)
    x[1, 2, :] = -np.inf
    x[3, 4, C // 3] = np.nan
    _check_f32(x, C, C // 5, seq_len=[5, 4, 5, 2, 5, 3, 1])


# (C, the pre-pass the launcher must pick): the fused facts, the facts and a
# norm kernel, ctcx_row_prep with the row in LDS (16384: more than 64 KB of
# dynamic LDS; 32768: the row exactly kPrepLdsBytes), ... read from global memory
F32_PATHS = [(68, "facts_fused"), (1024, "facts_fused"), (1028, "facts_norm"), (8192, "facts_norm"),
             (8196, "row_prep_lds"), (1001, "row_prep_lds"), (16384, "row_prep_lds"), (32768, "row_prep_lds"),
             (32769, "row_prep_global"), (32772, "row_prep_global"), (38000, "row_prep_global")]


@pytest.mark.parametrize("C,path", F32_PATHS)
def test_row_facts_path_taken(C, path):
    rng = np.random.default_rng(7400 + C)
    _check_f32(rng.standard_normal((1, 2, C)).astype(np.float32), C, 3)
    assert _run.prepass == path, (C, _run.prepass)


@pytest.mark.parametrize("C", [16384, 32768, 32769, 32772, 38000])
def test_row_facts_wide_rows(C):
    rng = np.random.default_rng(7500 + C)
    for kind in ("normal", "ties", "neg_inf", "all_neg_inf", "bad"):
        for blank in (0, C - 1):
            x = _rows(rng, C, kind, 4).reshape(2, 2, C)
            _check_f32(x, C, blank)
    assert _run.prepass == dict(F32_PATHS)[C]


@pytest.mark.parametrize("C", [68, 1000, 5000, 5001, 32772])
def test_row_facts_ragged_lengths(C):
    # items of different lengths: some of a block's four rows are past their
    # item's end (the fused kernel's waves still meet its barriers)
    rng = np.random.default_rng(7100 + C)
    T, B = 5, 7
    x = rng.standard_normal((T, B, C)).astype(np.float32) * 3
    x[2, 3, C // 5] = np.nan
    x[4, 0, 1] = np.inf
    _check_f32(x, C, 0, seq_len=[5, 1, 0, 3, 4, 2, 5])


def _check_f64(x_tb, C, blank, seq_len=None):
    # double rows carry no top set (|S| = 0: the decode takes the plain path)
    rec, norm = _run(x_tb, C, blank, np.float64, seq_len=seq_len)
    _check_norm(x_tb, norm, seq_len)
    rows = x_tb.reshape(-1, C)
    nblk = (C + 63) // 64
    live = None if seq_len is None else (np.arange(x_tb.shape[0])[:, None] < np.asarray(seq_len)[None, :]).reshape(-1)
    for r in range(rows.shape[0]):
        h = rec[r]
        if live is not None and not live[r]:
            assert not h.any(), "the record of a row past its item's length is left alone"
            continue
        bad = bool(np.isnan(rows[r]).any() or np.isposinf(rows[r]).any())
        assert bool(h[16:20].view(np.int32)[0]) == bad, (C, r)
        assert h[20:24].view(np.int32)[0] == 0, (C, r)
        if bad:
            continue
        assert h[0:8].view(np.float64)[0] == rows[r].max(), (C, r)
        bm = np.array([rows[r][k:k + 64].max() for k in range(0, C, 64)])
        assert np.array_equal(h[32:32 + 8 * nblk].view(np.float64), bm), (C, r)


# double rows: the LDS stage holds 16384 of them exactly (128 KB)
F64_PATHS = {300: "row_prep_lds", 8192: "row_prep_lds", 16384: "row_prep_lds", 16385: "row_prep_global",
             19000: "row_prep_global"}


@pytest.mark.parametrize("C", sorted(F64_PATHS))
def test_row_facts_f64_header_and_block_maxima(C):
    rng = np.random.default_rng(7300 + (C if C != 300 else 0))
    x = rng.standard_normal((2, 3, C))
    _check_f64(x, C, 5)
    assert _run.prepass == F64_PATHS[C]
    for kind in ("neg_inf", "all_neg_inf", "bad"):
        x = _rows(rng, C, kind, 6).astype(np.float64).reshape(2, 3, C)
        _check_f64(x, C, C - 1)
    # ragged lengths: rows past an item's length are neither read nor written
    x = rng.standard_normal((4, 3, C)) * 3
    x[1, 0, C // 5] = np.nan
    x[0, 2, 1] = np.inf
    _check_f64(x, C, 0, seq_len=[4, 0, 2])


# ---- the whole float range (tests/range_inputs.py)

# every pre-pass path and the NV boundary widths: (C, the pre-pass that must run)
RANGE_F32 = sorted(set(F32_PATHS) | {(1020, "facts_fused"), (2048, "facts_norm"), (3072, "facts_norm")})


@pytest.mark.parametrize("kind", range_inputs.FAMILIES)
@pytest.mark.parametrize("C,path", RANGE_F32)
def test_row_facts_numeric_range_f32(C, path, kind):
    rng = range_inputs.rng_for("prepass/f32/%d/%s" % (C, kind))
    for blank in (0, C - 1):
        x = range_inputs.family(rng, kind, 2, 3, C, np.float32)
        range_inputs.assert_census(kind, x, wide_rows=C >= 1000)
        _check_f32(x, C, blank)
        assert _run.prepass == path, (C, kind, _run.prepass)


def test_row_facts_numeric_range_mixed_wave():
    """ctcx_row_norm_v4 (facts_norm widths) sums one row per lane and picks
    expf_t_core or expf_t_le0 per 16-term batch by a wave-wide ballot: 8 x 8
    live rows fill a wave, rows of every family share it, and the banded rows
    keep the batches of their lower classes on the core path with subnormal
    results while the upper ones take the le0 path."""
    C, T, B = 1056, 8, 8
    rng = range_inputs.rng_for("prepass/mixed_wave")
    x = range_inputs.family(rng, "banded", T, B, C, np.float32)
    range_inputs.assert_census("banded", x)
    _check_f32(x, C, 0)
    assert _run.prepass == "facts_norm"
    # rows of different kinds in one wave: every fourth row stays banded
    for i, kind in enumerate(k for k in range_inputs.FAMILIES if k != "banded"):
        rows = [r for r in range(T * B) if r % 4 and r % 7 == i]
        other = range_inputs.family(rng, kind, T, B, C, np.float32)
        x.reshape(T * B, C)[rows] = other.reshape(T * B, C)[rows]
    range_inputs.assert_census("banded", x[:, 0])     # (rows 0, 8, ...: r % 4 == 0)
    _check_f32(x, C, C - 1)
    assert _run.prepass == "facts_norm"


@pytest.mark.parametrize("kind", ["logsoftmax", "edges", "onehot", "huge", "subnormal"])
@pytest.mark.parametrize("C", sorted(F64_PATHS))
def test_row_facts_numeric_range_f64(C, kind):
    rng = range_inputs.rng_for("prepass/f64/%d/%s" % (C, kind))
    x = range_inputs.family(rng, kind, 2, 3, C, np.float64)
    cs = range_inputs.assert_census(kind, x, wide_rows=C >= 1000)
    lo, hi = range_inputs.LOG_NEAR_ONE
    s = range_inputs.row_sums64(x)
    if kind == "logsoftmax":
        # log's near-1 branch proper (a sum in the interval that is not 1:
        # the runner-up of a scale-120 row lies 3 to 37 below its maximum)
        # and its == 1.0 early return (norm == max), at every width
        assert ((s >= lo) & (s < hi) & (s != 1.0)).any(), (C, s)
        assert cs["norm_is_max"] >= 1, (C, cs)
    elif kind == "onehot":
        assert (s == 1.0).all(), (C, s)
    _check_f64(x, C, 5)
    assert _run.prepass == F64_PATHS[C]
