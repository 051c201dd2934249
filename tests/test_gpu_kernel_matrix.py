"""Every compiled decode kernel against the oracle, one pytest id per
instantiation, and the edges of the LDS tier.

libctcext.so holds 40 one-wave instantiations of ctcx_beam_decode<T, RN, WC,
BIG, scorer>, six two-wave ones and the four global-state builds;
launch_decode (ctcx_decode.hip) picks one from dtype, scorer, C > 64, the beam
range and whether the compile-time layout fits the LDS.  ctcext_stats.kernel
(written by the launchers themselves) says which one a call ran: each cell
below decodes three input kinds through the public op, compares all seven
outputs bit-exactly with the oracle, and asserts that the kernel that ran is
the cell's.  TABLE lists every instantiation; test_every_instantiation_is_accounted_for
holds it to the build.

The second half walks the edges of the LDS tier (8196 < C <= ~38500 float,
300 < C <= ~19500 double), where the carve is within bytes of the 160 KB
limit: the widest beam of the tier and one past it, the two-wave layouts'
last fitting class counts, the record ring behind a run-time-W layout.  LDS
accesses past the allocation do not fault, so a disagreement between the
kernel's carve and decode_lds_bytes shows only as wrong outputs, here.

test_bigram_instantiation_table_kinds gives every bigram cell the other table
kinds of tests/scorer_tables.py: entries on a grid with half-grid logits (equal
totals: the scored kernels' tie order), forbidden bigrams (-inf entries, whole
rows and columns of them; no decoded path may hold one) and entries at the
ends of the float range.

The last part decodes the families of tests/range_inputs.py (the whole float
range: expf's and exp's subnormal band and underflow bound, one dominant
class, logits near 1e6..3e7, overflowing differences, subnormals) through
every instantiation the small shapes reach, and through one-frame decodes
whose log-probabilities are x_l - norm itself.
"""
import zlib

import numpy as np
import pytest

import ctcext_amd
from ctcext_amd import _lib
from parity_util import compare
import oracle
import range_inputs
import scorer_tables

pytestmark = pytest.mark.gpu

GS = _lib.CTCEXT_FLAG_GLOBAL_STATE
F32, F64 = "f32", "f64"
NP = {F32: np.float32, F64: np.float64}
CODE = {F32: _lib.CTCEXT_F32, F64: _lib.CTCEXT_F64}


def _row(dtype, scorer, RN, WC, BIG, helper="none", tier=0):
    return (tier, dtype, scorer, RN, WC, BIG, helper)


# One-wave shapes (T, C, W, P) by (RN, WC, BIG): the smallest that reach the
# instantiation.  WC = 0 with BIG needs a class count at which the
# compile-time layout (128 or 256 beams) no longer fits the LDS.
SMALL = {(1, 128, False): (30, 20, 100, 5), (2, 256, False): (30, 20, 200, 5), (4, 0, False): (30, 20, 400, 5),
         (1, 128, True): (20, 300, 100, 5), (2, 256, True): (20, 300, 200, 5), (4, 0, True): (20, 300, 400, 5)}

# id -> (row, [(T, C, W, P), ...], CTCEXT_HELPER or None, flags).  Every shape
# of a cell runs all three input kinds unless it names its own.
CELLS = {}


def _cell(name, row, shapes, helper_env="0", flags=0, kinds=None):
    CELLS[name] = (row, shapes, helper_env, flags, kinds)


for _dt in (F32, F64):
    for _sc in ("base", "bigram"):
        for (_rn, _wc, _big), _shape in SMALL.items():
            if _dt == F64 and _sc == "bigram" and (_rn, _wc, _big) == (4, 0, False):
                _shape = (30, 20, 380, 5)   # two branch buffers, 8-byte values and the scorer states: 400 is past the LDS
            _cell("%s_%s_rn%d_wc%d_%s" % (_dt, _sc, _rn, _wc, "big" if _big else "small"),
                  _row(_dt, _sc, _rn, _wc, _big), [_shape])
# the widest beams and the tie grid at a second class count, float
_cell("f32_base_rn4_wc0_big_c130_ties", _row(F32, "base", 4, 0, True), [(20, 130, 300, 5)], kinds=("ties",))
_cell("f32_base_rn4_wc0_big_w512_p200", _row(F32, "base", 4, 0, True), [(20, 300, 512, 200)])
# the run-time-W layouts: the class count at which 128 (256) beams no longer fit
_cell("f32_base_rn1_wc0_big", _row(F32, "base", 1, 0, True), [(8, 33000, 100, 3)])
_cell("f32_base_rn1_wc0_big_c38000", _row(F32, "base", 1, 0, True), [(8, 38000, 8, 3)])   # the last beams of the tier
_cell("f32_base_rn2_wc0_big", _row(F32, "base", 2, 0, True), [(8, 26000, 200, 3)])
_cell("f64_base_rn1_wc0_big", _row(F64, "base", 1, 0, True), [(8, 15000, 100, 3)])
_cell("f64_base_rn2_wc0_big", _row(F64, "base", 2, 0, True), [(8, 10500, 200, 3)])
# ... with the bigram scorer, whose state arrays move those class counts down
# and whose (C + 1) x C table is 0.6 to 3.9 GB there: a mostly-zero table
# (_bigram_table) keeps each decode under a second
_cell("f32_bigram_rn1_wc0_big", _row(F32, "bigram", 1, 0, True), [(8, 31400, 100, 3)])
# (T = 4: a frame the -inf kind sends down the literal path takes ~2 s at this C x W with the scorer)
_cell("f32_bigram_rn2_wc0_big", _row(F32, "bigram", 2, 0, True), [(4, 24100, 200, 3)])
_cell("f64_bigram_rn1_wc0_big", _row(F64, "bigram", 1, 0, True), [(8, 14300, 100, 3)])
_cell("f64_bigram_rn2_wc0_big", _row(F64, "bigram", 2, 0, True), [(8, 9000, 200, 3)])
# the two-wave kernels (float, the base scorer): the score table and the
# gather queue (CTCEXT_HELPER=1, and the default for beams of 129..256), the
# scored queue (the default up to 128 beams; CTCEXT_HELPER=4 above)
_cell("f32_hw_rn1_wc128_small", _row(F32, "base", 1, 128, False, "HW"), [SMALL[(1, 128, False)]], helper_env="1")
_cell("f32_hw_rn1_wc128_big", _row(F32, "base", 1, 128, True, "HW"), [SMALL[(1, 128, True)]], helper_env="1")
_cell("f32_hw_rn2_wc256_big", _row(F32, "base", 2, 256, True, "HW"), [SMALL[(2, 256, True)]], helper_env=None)
_cell("f32_sq_rn1_wc128_small", _row(F32, "base", 1, 128, False, "SQ"), [SMALL[(1, 128, False)]], helper_env=None)
_cell("f32_sq_rn1_wc128_big", _row(F32, "base", 1, 128, True, "SQ"), [SMALL[(1, 128, True)]], helper_env=None)
_cell("f32_sq_rn2_wc256_big", _row(F32, "base", 2, 256, True, "SQ"), [SMALL[(2, 256, True)]], helper_env="4")
# the global-state tier's four builds
for _dt in (F32, F64):
    for _sc in ("base", "bigram"):
        _cell("gstate_%s_%s" % (_dt, _sc), _row(_dt, _sc, 1, 0, False, tier=1), [(10, 8, 40, 3)], flags=GS)

# Every instantiation of the build: CTCX_DECODE_INSTANCES (40 one-wave), the
# six two-wave kernels and the four global-state ones -> ("covered", cell id),
# ("unreachable", why) or ("exempt", why; none today).
TABLE = {}
for _dt in (F32, F64):
    for _sc in ("base", "bigram"):
        for _rn, _wc in ((1, 128), (1, 0), (2, 256), (2, 0), (4, 0)):
            for _big in (False, True):
                _name = "%s_%s_rn%d_wc%d_%s" % (_dt, _sc, _rn, _wc, "big" if _big else "small")
                _r = _row(_dt, _sc, _rn, _wc, _big)
                if _wc == 0 and _rn < 4 and not _big:
                    TABLE[_r] = ("unreachable", "C <= 64 always fits the compile-time layout of %d beams" % (128 * _rn))
                else:
                    TABLE[_r] = ("covered", _name)
for _name in ("f32_hw_rn1_wc128_small", "f32_hw_rn1_wc128_big", "f32_hw_rn2_wc256_big", "f32_sq_rn1_wc128_small",
              "f32_sq_rn1_wc128_big", "f32_sq_rn2_wc256_big", "gstate_f32_base", "gstate_f32_bigram",
              "gstate_f64_base", "gstate_f64_bigram"):
    TABLE[CELLS[_name][0]] = ("covered", _name)

KINDS = {"normal": dict(merge_repeated=False, blank_index=0),
         "ties": dict(merge_repeated=True, blank_index=None),    # (None: C // 2, a non-zero blank)
         "neg_inf": dict(merge_repeated=True, blank_index=0),
         # the families of range_inputs (test_instantiation_numeric_range)
         "logsoftmax": dict(merge_repeated=True, blank_index=None),
         "edges": dict(merge_repeated=False, blank_index=0),
         "banded": dict(merge_repeated=False, blank_index=0),
         "onehot": dict(merge_repeated=True, blank_index=None),
         "offset": dict(merge_repeated=False, blank_index=0),
         "huge": dict(merge_repeated=True, blank_index=None),
         "subnormal": dict(merge_repeated=False, blank_index=0),
         "peaked": dict(merge_repeated=True, blank_index=None)}
BASE_KINDS = ("neg_inf", "normal", "ties")   # what every shape of a cell runs

_observed = set()


def _stat_row(k):
    return (k["tier"], k["dtype"], k["scorer"], k["RN"], k["WC"], k["BIG"], k["helper"])


def _stats():
    return ctcext_amd.get_decoder(0).last_stats


def _inputs(rng, kind, T, C, dtype):
    if kind in range_inputs.FAMILIES:
        return range_inputs.family(rng, kind, T, 2, C, NP[dtype])
    x = rng.standard_normal((T, 2, C))
    if kind == "ties":
        x = np.round(x * 2) / 2
    elif kind == "neg_inf":
        x[rng.random(x.shape) < 0.15] = -np.inf
    return x.astype(NP[dtype])


def _bigram_table(rng, C, dtype):
    """scorer_tables' continuous kind: -abs(normal) * 2 entries; past 5000
    classes (a table of gigabytes) only the root's row and every seventh row
    after it are non-zero, each entry the sum of a row and a column term: the
    rest of the table is never written, so building it stays cheap, and the
    expansions of one beam in seven are still penalised."""
    return scorer_tables.table(rng, "continuous", C, NP[dtype])


def _decode_both(x, sl, W, P, kw, tab=None, flags=0, want_ref=True):
    """The op's outputs and the oracle's for one input; the oracle must not
    fail (an error on both sides would stand in for a comparison)."""
    ref = oracle.decode(x, sl, W, P, scorer_table=tab, **kw) if want_ref else None
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, flags=flags, scorer_table=tab, **kw)
    return out, ref


def _run_cell(name, monkeypatch, kinds=None, want_ref=True):
    row, shapes, helper_env, flags, own_kinds = CELLS[name]
    tier, dtype, scorer = row[:3]
    if helper_env is None:
        monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    else:
        monkeypatch.setenv("CTCEXT_HELPER", helper_env)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    for (T, C, W, P) in shapes:
        sl = np.array([T, max(T - 3, 1)], np.int32)
        assert P >= 2
        if tier == 0 and scorer == "base":
            # the shape is inside the LDS tier by the library's own limit
            assert W <= ctcext_amd.get_decoder(0).lib.ctcext_max_beam_width(C, CODE[dtype]), (C, W)
        tab = _bigram_table(rng, C, dtype) if scorer == "bigram" else None
        for kind in kinds or own_kinds or BASE_KINDS:
            kw = dict(KINDS[kind])
            if kw["blank_index"] is None:
                kw["blank_index"] = C // 2
            x = _inputs(rng, kind, T, C, dtype)
            try:
                out, ref = _decode_both(x, sl, W, P, kw, tab, flags, want_ref)
            except (oracle.OracleError, ctcext_amd.OpError) as e:
                raise AssertionError("%s %s C=%d W=%d: %s" % (name, kind, C, W, e))
            k = _stats()["kernel"]
            assert k["launched"] and _stat_row(k) == row, (name, kind, (T, C, W, P), k)
            assert _stats()["tier"] == tier
            _observed.add(row)
            if ref is not None:
                compare(out, ref, P, lp_exact=True)


@pytest.mark.parametrize("name", sorted(CELLS))
def test_instantiation_matches_oracle(name, monkeypatch):
    _run_cell(name, monkeypatch)


# ---- the bigram cells under the other table kinds

# table kind -> (the logits it is paired with, merge_repeated).  forbidden
# decodes with merge_repeated off, so that a decoded path is its prefix's label
# sequence and every bigram of it can be looked up in the table.
TABLE_KINDS = {"grid": ("ties", True), "forbidden": ("neg_inf", False), "extreme": ("normal", False),
               # grid entries with 30% -inf under half-grid logits: no frame takes the literal path (the -inf logits
               # of the forbidden pairing send nearly every frame there), so the fast path's own -inf admission
               # tests and its tie order run.  The one kind of the run-time-W cells (tables of gigabytes, every
               # seventh row written), where a literal frame takes seconds.
               "grid_forbidden": ("ties", True)}
BIGRAM_CELLS = sorted(n for n, c in CELLS.items() if c[0][2] == "bigram")
TABLE_KIND_PARAMS = [(n, k) for n in BIGRAM_CELLS
                     for k in (("grid", "forbidden", "extreme", "grid_forbidden") if CELLS[n][1][0][1] <= 5000
                               else ("grid_forbidden",))]
assert len(BIGRAM_CELLS) == 18 and len(TABLE_KIND_PARAMS) == 14 * 4 + 4


def table_kind_case(name, tkind, B=2, reseed=""):
    """(x [T, B, C], lengths, W, P, attributes, table) of a bigram cell under
    a table kind; shared with the stream matrix (B = 3, and a suffix to the
    seed's name where its census needs another draw)."""
    row, shapes, _, _, _ = CELLS[name]
    (T, C, W, P), = shapes
    kind, merge = TABLE_KINDS[tkind]
    rng = np.random.default_rng(zlib.crc32(("%s/table/%s%s" % (name, tkind, reseed)).encode()))
    tab = scorer_tables.table(rng, tkind, C, NP[row[1]])
    kw = dict(KINDS[kind], merge_repeated=merge)
    if kw["blank_index"] is None:
        kw["blank_index"] = C // 2
    x = rng.standard_normal((T, B, C))
    if kind == "ties":
        x = np.round(x * 2) / 2
    elif kind == "neg_inf":
        x[rng.random(x.shape) < 0.15] = -np.inf
    return x.astype(NP[row[1]]), np.array([T, max(T - 3, 1), 2][:B], np.int32), W, P, kw, tab


def decoded_paths(out, B, P):
    """The op's decoded label lists, path by path and item by item."""
    paths = []
    for p in range(P):
        idx, val = (np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in (out.decoded_indices[p], out.decoded_values[p]))
        for b in range(B):
            paths.append(val[idx[:, 0] == b].tolist())
    return paths


@pytest.mark.parametrize("name,tkind", TABLE_KIND_PARAMS)
def test_bigram_instantiation_table_kinds(name, tkind, monkeypatch):
    """All seven outputs are the oracle's, bit for bit, and the kernel that ran
    is the cell's.  Under the forbidden kinds no decoded path of the op starts
    with a label the root's row forbids or holds a step (a, b) whose entry
    [a + 1][b] is -inf (asserted on the op's outputs, not only through the
    oracle), and the reference has P paths to compare."""
    row, shapes, helper_env, flags, _ = CELLS[name]
    monkeypatch.setenv("CTCEXT_HELPER", helper_env)
    x, sl, W, P, kw, tab = table_kind_case(name, tkind)
    if "forbidden" in tkind:   # (of the rows that are written; 72 entries at C = 8)
        assert np.isneginf(tab if tab.shape[1] <= scorer_tables.SPARSE_ABOVE else tab[::scorer_tables.SPARSE_STEP]).mean() > 0.2
    try:
        out, ref = _decode_both(x, sl, W, P, kw, tab, flags)
    except (oracle.OracleError, ctcext_amd.OpError) as e:
        raise AssertionError("%s %s: %s" % (name, tkind, e))
    k = _stats()["kernel"]
    assert k["launched"] and _stat_row(k) == row, (name, tkind, k)
    assert _stats()["tier"] == row[0]
    _observed.add(row)
    compare(out, ref, P, lp_exact=True)
    if "forbidden" in tkind:
        # (merge_repeated, which grid_forbidden keeps on, only drops a label
        # equal to the one before it: every step left in a path is a step of
        # its prefix)
        paths = decoded_paths(out, 2, P)
        assert any(len(p) >= 2 for p in paths)
        assert scorer_tables.forbidden_pairs(tab, paths) == [], name
    if tkind in ("grid", "grid_forbidden"):
        lp = np.asarray(ref.log_probability)
        print("%s %s: distinct log-probabilities per item %s of %d" % (name, tkind, [len(set(r.tolist())) for r in lp], P))


def test_every_instantiation_is_accounted_for(monkeypatch):
    """40 one-wave + 6 two-wave + 4 global-state rows; every one is covered by
    a cell above (its kernel id seen in this session, or by running the cell's
    first kind here), except the eight rows no shape reaches (WC = 0 at C <=
    64 below RN = 4: 128 and 256 beams always fit there).  "exempt" is open to
    the four bigram rows that need a table of gigabytes only; none uses it."""
    assert len(TABLE) == 50
    by = {}
    for row, (mark, _) in TABLE.items():
        by.setdefault(mark, []).append(row)
    assert set(by) <= {"covered", "exempt", "unreachable"}
    by.setdefault("exempt", [])
    lib = ctcext_amd.get_decoder(0).lib
    for dtype in (F32, F64):
        assert lib.ctcext_max_beam_width(64, CODE[dtype]) >= 256
    assert len(by["unreachable"]) == 8
    for (tier, dtype, scorer, RN, WC, BIG, helper) in by["unreachable"]:
        assert tier == 0 and WC == 0 and not BIG and RN in (1, 2) and helper == "none"
    assert len(by["exempt"]) <= 4
    for (tier, dtype, scorer, RN, WC, BIG, helper) in by["exempt"]:
        assert tier == 0 and scorer == "bigram" and WC == 0 and BIG and RN in (1, 2)
    assert len(by["covered"]) == 50 - 8 - len(by["exempt"])
    for row in by["covered"]:
        cell = TABLE[row][1]
        assert CELLS[cell][0] == row
        if row not in _observed:
            _run_cell(cell, monkeypatch, kinds=(CELLS[cell][4] or ("normal",))[:1], want_ref=False)
        assert row in _observed, cell
    # and no cell claims a row outside the table
    assert {c[0] for c in CELLS.values()} == set(by["covered"])


# ---- the LDS tier's edges

def _edge_case(C, W, dtype, kinds=("normal", "ties"), flags=0, T=6, P=2, seed=0):
    """Parity of a [T, 2, C] decode at beam W for each kind; returns the stats
    of the last one (the same kernel for every kind)."""
    rng = np.random.default_rng(50000 + C + W + seed)
    sl = np.array([T, max(T - 3, 1)], np.int32)
    for kind in kinds:
        kw = dict(KINDS[kind])
        if kw["blank_index"] is None:
            kw["blank_index"] = C // 2
        x = _inputs(rng, kind, T, C, dtype)
        out, ref = _decode_both(x, sl, W, P, kw, flags=flags)
        compare(out, ref, P, lp_exact=True)
    return _stats()


@pytest.mark.parametrize("dtype,C", [(F32, 20000), (F32, 30000), (F32, 35000), (F32, 38000),
                                     (F64, 29), (F64, 5000), (F64, 10000), (F64, 15000)])
def test_lds_tier_exactly_full(dtype, C):
    # the widest beam the LDS tier takes (the carve at or within bytes of the
    # 160 KB), then one more: the global-state tier
    W = ctcext_amd.get_decoder(0).lib.ctcext_max_beam_width(C, CODE[dtype])
    assert W >= 2
    st = _edge_case(C, W, dtype)
    assert st["tier"] == 0 and st["kernel"]["tier"] == 0 and st["kernel"]["launched"], st
    st = _edge_case(C, W + 1, dtype)
    assert st["tier"] == 1 and st["kernel"]["tier"] == 1, st


@pytest.mark.parametrize("C,W,helper", [(30000, 100, 3), (31000, 100, 0), (24000, 200, 2), (24900, 200, 0)])
def test_two_wave_layout_fallback(C, W, helper, monkeypatch):
    # the two-wave layout (the decode carve plus the helper's queue) stops
    # fitting before the one-wave one does: the host falls back to one wave
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    st = _edge_case(C, W, F32)
    print("C=%d W=%d helper=%d kernel=%s" % (C, W, st["helper"], st["kernel"]))
    assert st["tier"] == 0
    assert st["helper"] == helper, st
    assert st["kernel"]["helper"] == {0: "none", 2: "HW", 3: "SQ"}[helper], st


def test_ring_behind_run_time_layout():
    # C = 33000: 128 beams do not fit, the layout is carved from W itself
    st = _edge_case(33000, 60, F32, flags=_lib.CTCEXT_FLAG_RING_MIN)
    assert st["tier"] == 0 and st["ring_frames"] == 8, st
    assert st["kernel"]["WC"] == 0, st


def test_ring_dropped_when_the_layout_fills_the_lds():
    W = ctcext_amd.get_decoder(0).lib.ctcext_max_beam_width(33000, _lib.CTCEXT_F32)
    st = _edge_case(33000, W, F32, flags=_lib.CTCEXT_FLAG_RING_MIN)
    assert st["tier"] == 0 and st["ring_frames"] == 0, st


# ---- the whole float range through every instantiation of the small shapes

# the cells built from SMALL (24 one-wave, six two-wave) and the four
# global-state ones; not the run-time-W cells, whose class counts add nothing here
RANGE_CELLS = sorted(n for n, c in CELLS.items() if c[1][0] in list(SMALL.values()) + [(30, 20, 380, 5), (10, 8, 40, 3)])
RANGE_KINDS = tuple(k for k in range_inputs.FAMILIES if k != "banded")
assert len(RANGE_CELLS) == 34


def _live_rows(x, sl):
    return np.concatenate([x[:n, b] for b, n in enumerate(sl)])


@pytest.mark.parametrize("kind", RANGE_KINDS)
@pytest.mark.parametrize("name", RANGE_CELLS)
def test_instantiation_numeric_range(name, kind, monkeypatch):
    """As _run_cell: all seven outputs are the oracle's, the log-probabilities
    bit for bit, and the kernel that ran is the cell's (the family did not
    divert the call).  The all-finite families must also stay off the literal
    path's non-finite replay: no logit and no total of theirs is non-finite,
    so the fast path is the code under test."""
    row, shapes, helper_env, flags, _ = CELLS[name]
    tier, dtype, scorer = row[:3]
    if helper_env is None:
        monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    else:
        monkeypatch.setenv("CTCEXT_HELPER", helper_env)
    (T, C, W, P), = shapes
    rng = range_inputs.rng_for("%s/%s" % (name, kind))
    sl = np.array([T, max(T - 3, 1)], np.int32)
    tab = _bigram_table(rng, C, dtype) if scorer == "bigram" else None
    kw = dict(KINDS[kind])
    if kw["blank_index"] is None:
        kw["blank_index"] = C // 2
    x = _inputs(rng, kind, T, C, dtype)
    range_inputs.assert_census(kind, _live_rows(x, sl))
    try:
        out, ref = _decode_both(x, sl, W, P, kw, tab, flags)
    except (oracle.OracleError, ctcext_amd.OpError) as e:
        raise AssertionError("%s %s: %s" % (name, kind, e))
    st = _stats()
    k = st["kernel"]
    assert k["launched"] and _stat_row(k) == row, (name, kind, k)
    assert st["tier"] == tier
    compare(out, ref, P, lp_exact=True)
    assert np.isfinite(ref.log_probability).all()
    if kind == "peaked" and scorer == "base":   # (a bigram table's entries move the totals off 0)
        # merged alignments added log1pf(a subnormal expf), itself subnormal,
        # to a total of 0 (the double kernels add the same float term): a best
        # path whose log-probability is a sum of those, above 0
        lp = np.asarray(ref.log_probability)[:, 0]
        assert ((lp > 0) & (lp < 1e-30)).any(), (name, lp)
    if kind != "huge":
        assert st["literal_nonfinite"] == 0, (name, kind, st)


@pytest.mark.parametrize("dtype,kind", [(d, k) for d in (F32, F64) for k in range_inputs.FAMILIES
                                        if (d, k) != (F64, "banded")])   # (banded: expf_t_core / expf_t_le0, float only)
@pytest.mark.parametrize("C", [8, 29, 64])
def test_one_frame_log_probability_is_x_minus_norm(C, dtype, kind, monkeypatch):
    """T = 1, W = C: the leaves are the labels and the empty path, each
    log-probability x_l - norm itself.  Pins ctcx_row_norm (the decode's own
    normaliser, C <= 64) at the class counts ctcext_row_facts cannot reach;
    32 items so that every condition of the family's census is met."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    B, W, P = 32, C, min(C, 5)
    rng = range_inputs.rng_for("one_frame/%d/%s/%s" % (C, dtype, kind))
    x = range_inputs.family(rng, kind, 1, B, C, NP[dtype])
    kw = dict(KINDS[kind])
    if kw["blank_index"] is None:
        kw["blank_index"] = C // 2
    if kind == "huge":
        # a label whose x_l - norm overflows to -inf is no leaf, and one item
        # with fewer than P leaves fails the whole call on both sides: keep the
        # items with P labels left (a condition on the inputs, from the host)
        with np.errstate(over="ignore"):
            p = x[0] - oracle.row_norm(x[0])[:, None]
        p[:, kw["blank_index"]] = -np.inf
        x = np.ascontiguousarray(x[:, (p > -np.inf).sum(axis=1) >= P])
        B = x.shape[1]
        assert B >= 4, (C, dtype, B)
    range_inputs.assert_census(kind, x)
    sl = np.ones(B, np.int32)
    try:
        ref = oracle.decode(x, sl, W, P, **kw)
        out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, **kw)
    except (oracle.OracleError, ctcext_amd.OpError) as e:
        raise AssertionError("C=%d %s %s: %s" % (C, dtype, kind, e))
    compare(out, ref, P, lp_exact=True)
    if kind != "huge":
        # the best path's log-probability by its definition
        rows = x[0]
        want = (rows - oracle.row_norm(rows)[:, None]).max(axis=1)
        np.testing.assert_array_equal(np.asarray(ref.log_probability)[:, 0], want)
        assert _stats()["literal_nonfinite"] == 0, _stats()
