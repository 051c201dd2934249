"""Generates tests/golden/reference_cases.json: outputs of the REFERENCE
decoder itself (its own headers, compiled by oracle/ref into
oracle/_ref/libctc_ref.so; oracle/reference.py), recorded as data so that the
oracle (tests/test_oracle_reference.py) and every kernel route
(tests/test_gpu_reference_golden.py) are compared with the reference and not
only with the project's restatement of it.  Needs the reference tree and the
library, so it runs where those are; the tests of the recorded cases need
neither.

Format as make_fixtures_full.py: inputs are NOT stored but drawn from
numpy.random.default_rng(seed) by inputs() below (their sha256 is recorded, so
a changed numpy stream fails loudly); per item and path the decoded and
alignment label lists; log-probabilities as hex floats; where the reference
returns an error, its message; the number of "No label seq available" lines
it printed; the seconds it took; and the sha256 of each reference header that
was compiled (data: a changed reference is noticed).

Group A: one case per kernel route (the SMALL shapes of
test_gpu_kernel_matrix.py, both dtypes, three input kinds; cfg3-shaped cases
at beams 128 and 256).  Group B: semantics the restatement could have misread
(see CASES).  Group C: the oracle-made fixtures the suite already trusts,
recomputed with the reference; only the verdict and a hash of the reference's
outputs are stored (GROUP_C_SKIPPED says what was not recomputed, and why).
No case holds NaN or +inf: the library's row maximum is Eigen's only without
them.

Group S (reference_scorer_cases.json, a file of its own so that the first
stays as recorded): the reference under the driver's table scorer
(oracle/ref/ref_driver.cpp), with tables of tests/scorer_tables.py: the SMALL
shapes and cfg3 under each table kind, and the semantics of the hook (S_CASES).
Each entry also holds the table's sha256 and the hook counters of the call.

    python tests/golden/make_reference_fixtures.py            # everything (~4 min)
    python tests/golden/make_reference_fixtures.py NAME ...   # some cases / group C fixtures
    python tests/golden/make_reference_fixtures.py --scorer [NAME ...]   # group S only
"""
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_cases.json")
for _p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

RANGE_FAMILIES = ("logsoftmax", "edges", "banded", "onehot", "offset", "huge", "subnormal", "peaked")

CASES = {}


def _case(name, group, gen, seed, dtype, T, B, C, W, P, merge=False, blank=0, blabel=-1, sl=None, **gen_args):
    assert name not in CASES, name
    CASES[name] = dict(group=group, gen=gen, gen_args=gen_args, seed=seed, dtype=dtype, T=T, B=B, C=C,
                       beam_width=W, top_paths=P, merge_repeated=merge, blank_index=blank, blank_label=blabel,
                       seq_len=list(sl) if sl is not None else [T] * B)


# ---- group A: a case per kernel route
_SMALL = [(30, 20, 100, 5), (30, 20, 200, 5), (30, 20, 400, 5),
          (20, 300, 100, 5), (20, 300, 200, 5), (20, 300, 400, 5), (10, 8, 40, 3)]
_KIND = {"normal": dict(merge=False, blank=0), "ties": dict(merge=True, blank=None), "neg_inf": dict(merge=True, blank=0)}
_seed = 1000
for _T, _C, _W, _P in _SMALL:
    for _dt in ("f32", "f64"):
        for _kind, _kw in _KIND.items():
            _seed += 1
            _case("A_T%d_C%d_W%d_%s_%s" % (_T, _C, _W, _dt, _kind), "A", _kind, _seed, _dt, _T, 2, _C, _W, _P,
                  merge=_kw["merge"], blank=_C // 2 if _kw["blank"] is None else 0, sl=[_T, _T - 3])
for _W in (128, 256):
    _case("A_cfg3_W%d_normal" % _W, "A", "normal", 1100 + _W, "f32", 200, 2, 29, _W, 3, merge=True, sl=[200, 197])
    _case("A_cfg3_W%d_peaky" % _W, "A", "peaky", 1101 + _W, "f32", 200, 2, 29, _W, 3, merge=True, sl=[200, 197])
    _case("A_cfg3_W%d_ties" % _W, "A", "ties", 1102 + _W, "f32", 200, 2, 29, _W, 3, merge=True, sl=[200, 197])
    _case("A_cfg3_W%d_peaky_blank_last" % _W, "A", "peaky", 1103 + _W, "f32", 200, 2, 29, _W, 3, merge=True,
          blank=28, blabel=28, sl=[200, 197])

# ---- group B: semantics
_case("B_beam_1", "B", "normal", 2001, "f32", 25, 2, 6, 1, 1, merge=True, sl=[25, 20])
_case("B_beam_1_ties", "B", "ties", 2002, "f64", 25, 2, 6, 1, 1, blank=3, sl=[25, 20])
_case("B_paths_equal_beam", "B", "normal", 2003, "f32", 12, 2, 5, 7, 7, merge=True, blank=2, sl=[12, 9])
_case("B_paths_equal_beam_ties", "B", "ties", 2004, "f32", 12, 2, 5, 9, 9, sl=[12, 8])
_case("B_one_frame", "B", "normal", 2005, "f32", 1, 3, 9, 8, 4, blank=4)
_case("B_one_frame_f64_ties", "B", "ties", 2006, "f64", 1, 3, 9, 9, 9, merge=True)
_case("B_two_classes", "B", "normal", 2007, "f32", 14, 2, 2, 6, 3, merge=True, sl=[14, 11])
_case("B_two_classes_blank_1", "B", "ties", 2008, "f64", 14, 2, 2, 6, 3, blank=1, blabel=1, sl=[14, 11])
_case("B_blank_label_is_a_class", "B", "normal", 2009, "f32", 16, 2, 6, 10, 3, merge=True, blank=0, blabel=2, sl=[16, 13])
_case("B_blank_label_is_blank_index", "B", "normal", 2010, "f32", 16, 2, 6, 10, 3, blank=3, blabel=3, sl=[16, 13])
_case("B_repeats_merged", "B", "repeats", 2011, "f32", 24, 2, 5, 12, 4, merge=True, sl=[24, 21])
_case("B_repeats_kept", "B", "repeats", 2011, "f32", 24, 2, 5, 12, 4, merge=False, sl=[24, 21])
_case("B_repeats_merged_f64", "B", "repeats", 2012, "f64", 24, 2, 5, 12, 4, merge=True, blank=2, blabel=2, sl=[24, 21])
_case("B_repeats_kept_f64", "B", "repeats", 2012, "f64", 24, 2, 5, 12, 4, merge=False, blank=2, blabel=2, sl=[24, 21])
# 2 labels, 3 frames: 15 prefixes can exist, the beam holds 40
_case("B_beam_never_fills", "B", "normal", 2013, "f32", 3, 2, 3, 40, 5, merge=True, sl=[3, 2])
_case("B_beam_never_fills_ties", "B", "ties", 2014, "f64", 3, 2, 3, 40, 7, blank=1, sl=[3, 3])
# 19 labels offered to a beam of 4: full after the first frame
_case("B_beam_fills_on_first_frame", "B", "normal", 2015, "f32", 10, 2, 20, 4, 4, merge=True, sl=[10, 7])
_case("B_beam_fills_on_first_frame_ties", "B", "ties", 2016, "f32", 10, 2, 20, 4, 4, blank=10, sl=[10, 7])
_case("B_error_more_paths_than_beam", "B", "normal", 2017, "f32", 6, 2, 5, 3, 4)
_case("B_error_less_leaves", "B", "normal", 2018, "f32", 6, 3, 3, 10, 5, sl=[6, 1, 6])
_case("B_error_less_leaves_f64", "B", "normal", 2019, "f64", 1, 1, 3, 10, 5)
_case("B_zero_length_item", "B", "normal", 2020, "f32", 8, 3, 6, 8, 1, merge=True, sl=[8, 0, 5])
_case("B_zero_length_item_f64", "B", "ties", 2021, "f64", 8, 3, 6, 8, 1, blank=5, sl=[0, 8, 0])
_case("B_rows_all_neg_inf", "B", "neg_inf_rows", 2022, "f32", 12, 2, 6, 8, 2, merge=True, sl=[12, 10])
# -inf-heavy items chosen (by the search at the bottom of this file) so that
# frames start with one entry twice in the beam, and so that paths come back
# without an alignment
# (seed, T, B, C, W, P, -inf fraction, merge_repeated, blank_index, blank_label)
_DUP = [(24193, 27, 3, 6, 7, 4, 0.3, False, 3, 5), (24198, 19, 3, 4, 6, 5, 0.5, True, 2, 1),
        (24202, 27, 2, 6, 8, 8, 0.5, False, 1, 4), (24269, 23, 2, 4, 7, 7, 0.5, True, 3, 3),
        (24310, 23, 3, 6, 9, 8, 0.5, False, 2, 4), (24312, 8, 3, 4, 7, 5, 0.5, True, 3, 3),
        (24322, 14, 3, 4, 7, 6, 0.5, False, 3, 3), (24437, 18, 3, 6, 9, 6, 0.3, True, 4, 5)]
_NO_LABEL = [(30020, 3, 2, 5, 5, 4, 0.5, True, 4, 0), (30038, 10, 2, 6, 4, 3, 0.5, False, 5, 2),
             (30051, 9, 2, 6, 5, 5, 0.3, True, 2, 4), (30060, 6, 2, 4, 4, 3, 0.5, True, 2, -1),
             (30082, 7, 2, 5, 6, 5, 0.5, True, 1, 1), (30128, 8, 2, 6, 6, 6, 0.3, False, 0, -1)]
for _what, _rows in (("duplicate_state", _DUP), ("no_label", _NO_LABEL)):
    for (_s, _T, _B, _C, _W, _P, _frac, _merge, _blank, _blabel) in _rows:
        for _dt in ("f32", "f64"):
            _case("B_%s_%d_%s" % (_what, _s, _dt), "B", "neg_inf", _s, _dt, _T, _B, _C, _W, _P,
                  merge=_merge, blank=_blank, blabel=_blabel, frac=_frac)
for _i, _fam in enumerate(RANGE_FAMILIES):
    for _dt in ("f32", "f64"):
        if (_fam, _dt) == ("banded", "f64"):   # the family is float32 only
            continue
        _merge = _fam in ("logsoftmax", "onehot", "huge", "peaked")   # test_gpu_kernel_matrix.KINDS
        _case("B_range_%s_%s" % (_fam, _dt), "B", _fam, 2100 + _i, _dt, 20, 2, 20, 30, 3, merge=_merge,
              blank=10 if _merge else 0, sl=[20, 17])

# ---- group S: the reference under a bigram table scorer (reference_scorer_cases.json)
#
# The driver's TableScorer (oracle/ref/ref_driver.cpp) runs inside the
# reference decoder; tables come from tests/scorer_tables.py, drawn from
# default_rng(seed + TABLE_SEED).  A case is a group-A/B case dict plus "table",
# the table's kind.
S_OUT = os.path.join(HERE, "reference_scorer_cases.json")
TABLE_SEED = 5 * 10 ** 6
S_CASES = {}


def _scase(name, gen, table, seed, dtype, T, B, C, W, P, merge=False, blank=0, blabel=-1, sl=None, **gen_args):
    assert name not in S_CASES and name not in CASES, name
    S_CASES[name] = dict(group="S", gen=gen, gen_args=gen_args, seed=seed, dtype=dtype, T=T, B=B, C=C,
                         beam_width=W, top_paths=P, merge_repeated=merge, blank_index=blank, blank_label=blabel,
                         seq_len=list(sl) if sl is not None else [T] * B, table=table)


# (table kind, logits): forbidden decodes with merge_repeated off, so that a
# decoded path is its prefix's label sequence and its bigrams can be checked
_PAIRINGS = (("continuous", "normal"), ("grid", "ties"), ("forbidden", "neg_inf"), ("extreme", "normal"))
# top_paths of the grid cases: the smallest (from the shape's 5, or 3) at which
# some item's log-probabilities repeat a value, by --search-grid below
_GRID_P = {
    "S_T30_C20_W100_f32_grid": (3002, 17), "S_T30_C20_W100_f64_grid": (3006, 7),
    "S_T30_C20_W200_f32_grid": (3010, 17), "S_T30_C20_W200_f64_grid": (3014, 22),
    "S_T30_C20_W400_f32_grid": (3018, 24), "S_T30_C20_W400_f64_grid": (3022, 11),
    "S_T20_C300_W100_f32_grid": (3026, 5), "S_T20_C300_W100_f64_grid": (3030, 5),
    "S_T20_C300_W200_f32_grid": (3034, 5), "S_T20_C300_W200_f64_grid": (3038, 5),
    "S_T20_C300_W400_f32_grid": (3042, 5), "S_T20_C300_W400_f64_grid": (3046, 5),
    "S_T10_C8_W40_f32_grid": (3050, 9), "S_T10_C8_W40_f64_grid": (3054, 13),
    "S_cfg3_W128_grid": (3229, 3), "S_cfg3_W256_grid": (3357, 3),
}
_OWN_P = {}     # grid case -> the top_paths of its shape, the least --search-grid gives it
_seed = 3000
for _T, _C, _W, _P in _SMALL:
    for _dt in ("f32", "f64"):
        for _tk, _kind in _PAIRINGS:
            _seed += 1
            _kw = _KIND[_kind]
            _name = "S_T%d_C%d_W%d_%s_%s" % (_T, _C, _W, _dt, _tk)
            _s, _p = _GRID_P.get(_name, (_seed, _P))
            if _tk == "grid":
                _OWN_P[_name] = _P
            _scase(_name, _kind, _tk, _s, _dt, _T, 2, _C, _W, _p, merge=_kw["merge"] and _tk != "forbidden",
                   blank=_C // 2 if _kw["blank"] is None else 0, sl=[_T, _T - 3])
for _W in (128, 256):
    for _tk, _kind in _PAIRINGS[:2]:
        _name = "S_cfg3_W%d_%s" % (_W, _tk)
        _s, _p = _GRID_P.get(_name, (3100 + _W + (_tk == "grid"), 3))
        if _tk == "grid":
            _OWN_P[_name] = 3
        _scase(_name, _kind, _tk, _s, "f32", 200, 2, 29, _W, _p, merge=True, sl=[200, 197])

# semantics.  An all-zero table on the inputs of a group-A case: that case's outputs
S_ZERO_OF = {"S_zero_table_is_base_scorer": "A_T30_C20_W100_f32_ties", "S_zero_table_is_base_scorer_f64": "A_T20_C300_W200_f64_neg_inf"}
for _name, _of in S_ZERO_OF.items():
    S_CASES[_name] = dict(CASES[_of], group="S", table="zero")
# nothing can leave the root: the empty path alone
_scase("S_root_forbidden_one_path", "normal", "root_forbidden", 3201, "f32", 12, 2, 6, 8, 1, merge=True, sl=[12, 9])
_scase("S_root_forbidden_two_paths", "normal", "root_forbidden", 3201, "f32", 12, 2, 6, 8, 2, merge=True, sl=[12, 9])
_scase("S_root_forbidden_f64_blank_2", "ties", "root_forbidden", 3202, "f64", 12, 2, 6, 8, 1, blank=2, blabel=2, sl=[12, 9])
# label l only before l + 1 mod C
_scase("S_chain", "normal", "chain", 3203, "f32", 16, 2, 6, 10, 4, merge=True, sl=[16, 13])
_scase("S_chain_f64_blank_3", "ties", "chain", 3204, "f64", 16, 2, 6, 10, 4, blank=3, sl=[16, 13])
_scase("S_beam_1", "normal", "continuous", 3205, "f32", 25, 2, 6, 1, 1, merge=True, sl=[25, 20])
_scase("S_beam_1_extreme", "ties", "extreme", 3206, "f64", 25, 2, 6, 1, 1, blank=3, sl=[25, 20])
_scase("S_one_frame", "normal", "continuous", 3207, "f32", 1, 3, 9, 8, 4, blank=4)
_scase("S_one_frame_f64_grid", "ties", "grid", 3208, "f64", 1, 3, 9, 9, 9, merge=True)
_scase("S_one_frame_forbidden", "normal", "forbidden", 3209, "f32", 1, 3, 9, 8, 2)
_scase("S_zero_length_item", "normal", "continuous", 3210, "f32", 8, 3, 6, 8, 1, merge=True, sl=[8, 0, 5])
_scase("S_zero_length_item_f64", "ties", "forbidden", 3211, "f64", 8, 3, 6, 8, 1, blank=5, sl=[0, 8, 0])
_scase("S_blank_last", "normal", "continuous", 3212, "f32", 16, 2, 6, 10, 3, merge=True, blank=5, blabel=5, sl=[16, 13])
_scase("S_blank_middle_grid", "ties", "grid", 3213, "f64", 16, 2, 7, 10, 3, blank=3, blabel=0, sl=[16, 13])
_scase("S_blank_middle_forbidden", "neg_inf", "forbidden", 3214, "f32", 16, 2, 7, 10, 3, blank=3, sl=[16, 13])
_scase("S_error_more_paths_than_beam", "normal", "continuous", 3215, "f32", 6, 2, 5, 3, 4)
_scase("S_error_less_leaves", "normal", "forbidden", 3216, "f64", 6, 3, 3, 10, 5, sl=[6, 1, 6])
# -inf-heavy items on the half grid under a grid table, chosen (--search-scorer
# 34000 400) so that frames start with one entry twice in the beam
# (seed, T, B, C, W, P, -inf fraction, merge_repeated, blank_index, blank_label)
# (two duplicate-entry items each, and an item whose finite log-probabilities
# repeat a value; NaN rows, items that -inf left no path, do not count)
_S_DUP = [(34039, 29, 3, 5, 9, 6, 0.5, False, 0, 1), (34083, 25, 3, 5, 7, 5, 0.5, False, 3, -1)]
for (_s, _T, _B, _C, _W, _P, _frac, _merge, _blank, _blabel) in _S_DUP:
    for _dt in ("f32", "f64"):
        _scase("S_duplicate_state_%d_%s" % (_s, _dt), "neg_inf", "grid", _s, _dt, _T, _B, _C, _W, _P,
               merge=_merge, blank=_blank, blabel=_blabel, frac=_frac, ties=True)

NP = {"f32": np.float32, "f64": np.float64}


def scorer_table(c):
    """The [C + 1, C] table of a group-S case dict, of the case's dtype."""
    import scorer_tables
    return scorer_tables.table(np.random.default_rng(c["seed"] + TABLE_SEED), c["table"], c["C"], NP[c["dtype"]])


def inputs(c):
    """(x [T, B, C] of the case's dtype, seq_len int32 [B]) of a case dict."""
    T, B, C, gen, dt = c["T"], c["B"], c["C"], c["gen"], NP[c["dtype"]]
    rng = np.random.default_rng(c["seed"])
    if gen in RANGE_FAMILIES:
        import range_inputs
        x = range_inputs.family(rng, gen, T, B, C, dt)
    else:
        x = rng.standard_normal((T, B, C))
        if gen == "ties":
            x = np.round(x * 2) / 2
        elif gen == "neg_inf":
            if c["gen_args"].get("ties"):     # on the half grid first: with a grid table, totals repeat
                x = np.round(x * 2) / 2
            x[rng.random(x.shape) < c["gen_args"].get("frac", 0.15)] = -np.inf
        elif gen == "neg_inf_rows":       # 15% -inf, and every fourth frame -inf throughout
            x[rng.random(x.shape) < 0.15] = -np.inf
            x[3::4] = -np.inf
        elif gen == "peaky":              # distribution B of BASELINE.md: +6 on the blank w.p. 0.6, else on a label
            blank = c["blank_index"]
            lab = rng.integers(0, C - 1, size=(T, B))
            lab = lab + (lab >= blank)
            hot = np.where(rng.random((T, B)) < 0.6, blank, lab)
            np.put_along_axis(x, hot[..., None], np.take_along_axis(x, hot[..., None], 2) + 6.0, 2)
        elif gen == "repeats":            # +4 on a class held for runs of 1..4 frames: labels repeat, with and without a blank between
            for b in range(B):
                t = 0
                while t < T:
                    n = int(rng.integers(1, 5))
                    x[t:t + n, b, int(rng.integers(C))] += 4.0
                    t += n
        else:
            assert gen == "normal", gen
        x = x.astype(dt)
    assert not np.isnan(x).any() and not np.isposinf(x).any()
    return x, np.asarray(c["seq_len"], np.int32)


def attrs(c):
    return dict(merge_repeated=c["merge_repeated"], blank_index=c["blank_index"], blank_label=c["blank_label"])


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def hex_rows(lp):
    return [[float(v).hex() for v in row] for row in np.asarray(lp)]


def outputs_sha256(decoded, alignment, lp_hex):
    """One hash over a result's label lists and hex log-probabilities."""
    return hashlib.sha256(json.dumps([decoded, alignment, lp_hex], separators=(",", ":")).encode()).hexdigest()


def record(c):
    import oracle
    import reference
    x, sl = inputs(c)
    t0 = time.time()
    entry = {"case": c, "sha256": sha(x)}
    scored = {}
    if c.get("table") is not None:
        hooks = {}
        tab = scorer_table(c)
        entry["table_sha256"] = sha(tab)
        scored = dict(scorer_table=tab, hook_stats=hooks)
    try:
        dec, ali, lp, events = reference.raw_decode(x, sl, c["beam_width"], c["top_paths"], **attrs(c), **scored)
        entry.update(decoded=dec, alignment=ali, log_probability_hex=hex_rows(lp), error=None, no_label=events)
    except oracle.OracleError as e:
        entry.update(decoded=None, alignment=None, log_probability_hex=None, error=str(e), no_label=None)
    if scored:
        entry["hook_stats"] = hooks
    entry["reference_seconds"] = round(time.time() - t0, 3)
    return entry


# ---- group C: the oracle-made fixtures, recomputed with the reference

GROUP_C = ["paper_example", "full_length/cfg3_peaky_T1500_B2", "full_length/cfg3_T1500_B4",
           "large_vocab/cfg4_like_T100", "large_vocab/cfg4_like_T60_B2_P3", "bench_digests/cfg2_rank0"]
_ALLOC = ("the reference allocates a BeamEntry (two alignment queues, a child map) for every child of every expanded "
          "branch, keeps all of them until Reset, and copies a label sequence of the item's length per candidate: ")
GROUP_C_SKIPPED = {
    "full_length/cfg4_*": _ALLOC + "up to 64 x 999 entries a frame over 2000 frames, about 128 million an item",
    "full_length/cfg5_*": _ALLOC + "up to 256 x 4999 entries a frame over 1500 to 3000 frames, billions an item",
    "large_vocab/cfg4_like_T400_B2": _ALLOC + "up to 64 x 999 entries a frame over 400 frames, about 25 million an item",
    "large_vocab/cfg5_like_*": _ALLOC + "up to 256 x 4999 entries a frame, 25 to 128 million an item",
    "bench_digests/* but cfg2_rank0": "the reference's time grows with the square of an item's length: the other "
                                      "seven ranks of cfg2 (32 items of 1000 frames each), cfg3 (256 items of 1500 "
                                      "frames a rank) and cfg4 (entries as full_length/cfg4) were left to the oracle, "
                                      "which everything recorded here pins",
    "max_beam_width.json": "not oracle-made: the library's own LDS carve",
}


def group_c(name):
    import reference
    t0 = time.time()
    if name == "paper_example":
        # the reference's own test through its own code, with assertAllClose's defaults
        g = json.load(open(os.path.join(HERE, "paper_example.json")))
        a = g["attrs"]
        ok, n = True, 0
        for dt in (np.float32, np.float64):
            x = np.log(np.asarray(g["probs"])).astype(dt)
            dec, ali, lp, n = reference.raw_decode(x, g["sequence_length"], a["beam_width"], a["top_paths"],
                                                   a["merge_repeated"], a["blank_index"], a["blank_label"])
            for p in range(a["top_paths"]):
                ok &= dec[0][p] == g["decoded_values"][p] and ali[0][p] == g["alignment_values"][p]
            ok &= bool(np.allclose(lp, np.asarray(g["log_probability"]), rtol=1e-6, atol=1e-6))
        return {"fixture": "paper_example.json", "criterion": "labels equal, log-probabilities within rtol = atol = 1e-6, "
                "float32 and float64", "matches_reference": bool(ok), "reference_seconds": round(time.time() - t0, 1)}
    fixture, key = name.split("/")
    if fixture == "bench_digests":
        # rank 0 of a bench.py config, drawn as bench.make_inputs draws it and
        # hashed as bench.py hashes its own outputs
        import oracle
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        import bench
        cfg = key.split("_rank")[0]
        B, T, C, W, P, merge, blank = bench.CONFIGS[cfg]
        x = np.random.default_rng(20251015).standard_normal((T, B, C), dtype=np.float32)
        dec, ali, lp, n = reference.raw_decode(x, np.full(B, T, np.int32), W, P, merge, blank, -1)
        out = oracle.pack_sparse(dec, B, P) + oracle.pack_sparse(ali, B, P) + (lp.astype(np.float32),)
        digest = bench.output_digest(out, P)
        stored = json.load(open(os.path.join(HERE, "bench_digests.json")))[cfg]["digests"]["0"]
        return {"fixture": "bench_digests.json", "case": key, "items": int(B),
                "criterion": "bench.output_digest of every output", "matches_reference": digest == stored,
                "reference_digest": digest, "no_label": n, "reference_seconds": round(time.time() - t0, 1)}
    fx = json.load(open(os.path.join(HERE, fixture + ".json")))[key]
    if fixture == "full_length":
        import make_fixtures_full as gen
        _, _, T, B, C, W, P, merge, blank, blabel, _ = fx["case"]
    else:
        import make_fixtures as gen
        _, T, B, C, W, P, merge, blank, blabel, _ = fx["case"]
    x, sl = gen.inputs(fx["case"])
    assert sha(x) == fx["sha256"], "input stream changed"
    dec, ali, lp, n = reference.raw_decode(x, sl, W, P, merge, blank, blabel)
    lph = hex_rows(lp)
    if fixture == "full_length":
        same = dec == fx["decoded"] and ali == fx["alignment"] and lph == fx["log_probability_hex"]
    else:
        import oracle
        di, dv, ds = oracle.pack_sparse(dec, B, P)
        ai, av, ash = oracle.pack_sparse(ali, B, P)
        same = lph == fx["log_probability_hex"]
        for k, got in (("decoded_indices", di), ("decoded_values", dv), ("decoded_shape", ds),
                       ("alignment_indices", ai), ("alignment_values", av), ("alignment_shape", ash)):
            same &= [np.asarray(v).tolist() for v in got] == fx[k]
    return {"fixture": fixture + ".json", "case": key, "items": int(B), "criterion": "every output bit for bit",
            "matches_reference": bool(same), "reference_outputs_sha256": outputs_sha256(dec, ali, lph),
            "no_label": n, "reference_seconds": round(time.time() - t0, 1)}


def main_scorer(names):
    """Group S -> reference_scorer_cases.json (all of it, or the named cases)."""
    import reference
    assert reference.available(), "oracle/_ref/libctc_ref.so is missing: run build() where the reference tree is"
    out = json.load(open(S_OUT)) if os.path.exists(S_OUT) and names else {}
    out.setdefault("cases", {})
    out["source"] = ("the reference decoder's own headers compiled by oracle/ref (g++ -O2 -std=c++14, no -march) "
                     "with the driver's TableScorer, through oracle/reference.py")
    out["reference_headers_sha256"] = reference.header_sha256()
    for name in names or list(S_CASES):
        out["cases"][name] = record(S_CASES[name])
        print(name, out["cases"][name]["error"] or "ok", out["cases"][name]["reference_seconds"], flush=True)
    with open(S_OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("%d scorer cases, %d bytes" % (len(out["cases"]), os.path.getsize(S_OUT)))


def main(names):
    import reference
    assert reference.available(), "oracle/_ref/libctc_ref.so is missing: run build() where the reference tree is"
    if not names:
        main_scorer([])
    elif any(n in S_CASES for n in names):
        main_scorer([n for n in names if n in S_CASES])
        names = [n for n in names if n not in S_CASES]
        if not names:
            return
    out = json.load(open(OUT)) if os.path.exists(OUT) and names else {}
    out.setdefault("cases", {})
    out.setdefault("group_c", {})
    out["source"] = ("the reference decoder's own headers compiled by oracle/ref "
                     "(g++ -O2 -std=c++14, no -march), through oracle/reference.py")
    out["reference_headers_sha256"] = reference.header_sha256()
    out["group_c_skipped"] = GROUP_C_SKIPPED
    for name in names or list(CASES) + GROUP_C:
        if name in CASES:
            out["cases"][name] = record(CASES[name])
            print(name, out["cases"][name]["error"] or "ok", out["cases"][name]["reference_seconds"], flush=True)
        else:
            out["group_c"][name] = group_c(name)
            print(name, out["group_c"][name], flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("%d cases, %d bytes" % (len(out["cases"]), os.path.getsize(OUT)))


def search(first_seed, count, short=False, table=None):
    """How the rows of _DUP (--search 24100 400), _NO_LABEL (--search-short
    30000 200) and, with a table kind, _S_DUP (--search-scorer 34000 400) were
    chosen: prints seeds whose case the oracle decodes without an error, with
    duplicate-entry frames or paths without an alignment.  With a table the
    -inf-heavy logits lie on the half grid, and a seed also needs an item whose
    finite log-probabilities repeat a value.  (A condition on inputs, computed
    with the oracle.)"""
    import oracle
    for seed in range(first_seed, first_seed + count):
        rng = np.random.default_rng(seed + 10 ** 6)
        if short:
            T, B, C, W = int(rng.integers(2, 12)), 2, int(rng.integers(3, 7)), int(rng.integers(2, 7))
            P, frac = int(rng.integers(max(1, W - 1), W + 1)), float(rng.choice([0.3, 0.5]))
        else:
            T, B, C, W = int(rng.integers(8, 30)), int(rng.integers(2, 4)), int(rng.integers(4, 8)), int(rng.integers(4, 10))
            P, frac = int(rng.integers(1, W + 1)), float(rng.choice([0.3, 0.5]))
        merge, blank, blabel = bool(rng.integers(2)), int(rng.integers(C)), int(rng.integers(-1, C))
        c = dict(gen="neg_inf", gen_args=dict(frac=frac, ties=True) if table else dict(frac=frac), seed=seed, dtype="f32", T=T, B=B, C=C, seq_len=[T] * B,
                 blank_index=blank, table=table)
        x, sl = inputs(c)
        tab = scorer_table(c) if table else None
        dups = 0
        try:
            for b in range(B):
                st = {}
                oracle.raw_decode(x[:, b:b + 1], [T], W, P, merge, blank, blabel, stats=st, scorer_table=tab)
                dups += st["duplicate_frames"] > 0
            lp, events = oracle.raw_decode(x, sl, W, P, merge, blank, blabel, scorer_table=tab)[2:4]
        except oracle.OracleError:
            continue
        if table:
            rows = [[v for v in row.tolist() if np.isfinite(v)] for row in np.asarray(lp)]
            if dups and any(len(r) > len(set(r)) for r in rows):
                print((seed, T, B, C, W, P, frac, merge, blank, blabel), "dup items", dups,
                      "items with a repeated finite log-probability", sum(len(r) > len(set(r)) for r in rows))
        elif dups or events:
            print((seed, T, B, C, W, P, frac, merge, blank, blabel), "dup items", dups, "no-label", events)


def search_grid():
    """How _GRID_P was chosen: per grid case of _OWN_P its seed and the smallest
    top_paths, from the shape's own up to 50 and the beam, at which some
    item's log-probabilities repeat a value; computed with the oracle at the
    largest top_paths."""
    import oracle
    for name, own in _OWN_P.items():
        c = S_CASES[name]
        x, sl = inputs(c)
        pmax = min(50, c["beam_width"])
        lp = oracle.raw_decode(x, sl, c["beam_width"], pmax, scorer_table=scorer_table(c), **attrs(c))[2]
        need = []
        for row in np.asarray(lp):
            seen = set()
            for i, v in enumerate(row.tolist()):
                if v in seen:
                    need.append(i + 1)
                    break
                seen.add(v)
        if need:
            print('    "%s": (%d, %d),' % (name, c["seed"], max(own, min(need))), flush=True)
        else:
            print("# %s: no item repeats a value within %d paths: take another seed" % (name, pmax))


if __name__ == "__main__":
    if sys.argv[1:2] in (["--search"], ["--search-short"]):
        search(int(sys.argv[2]), int(sys.argv[3]), short=sys.argv[1] == "--search-short")
    elif sys.argv[1:2] == ["--search-scorer"]:
        search(int(sys.argv[2]), int(sys.argv[3]), table="grid")
    elif sys.argv[1:2] == ["--search-grid"]:
        search_grid()
    elif sys.argv[1:2] == ["--scorer"]:
        main_scorer(sys.argv[2:])
    else:
        main(sys.argv[1:])
