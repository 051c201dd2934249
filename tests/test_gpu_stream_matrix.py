"""Every stream-build decode kernel against the oracle across pushes, one
pytest id per cell of the kernel matrix, and the edges of the LDS tier as
streams.

libctcext.so holds every decode kernel a second time as the stream build
(-DCTCX_STREAM: namespaces ctcx_st and ctcx_gs_st), behind a dispatcher of its
own (stream_decode, part 14) and a helper choice made at open.  Between pushes
an item is the image of the launch's whole LDS allocation plus the scalars of
CtcxStreamHdr; an item without frames in a push passes both through and is
reported from the header.  LDS accesses past the allocation do not fault, so
an image that misses live words, a scalar missing from the header or a
dispatch rule that differs from launch_decode's shows only as a wrong result
after a later push: here.

1. test_stream_instantiation_matches_oracle: the cells of
   test_gpu_kernel_matrix.CELLS (imported, so the two matrices cannot drift),
   their shapes, CTCEXT_HELPER and flags unchanged, three items, a ragged
   schedule of pushes (schedule()) with
     (a) a first push of one frame,
     (b) a push of several frames,
     (c) an item that gets no frame in a push after it has had some and frames
         again in a later one (pass-through, then a resume from the image that
         was passed through),
     (d) an item that ends early and is reported from the saved header in at
         least two later pushes.
   The kinds of a cell run as streams of their own that take turns push by
   push (_run_streams: what the launch before a resume leaves in LDS is
   another stream's state, never the resumed item's own).
   After push k the reference is oracle.decode(x[:max f], f, ...) with f the
   frames each item has been given so far.  All seven outputs are compared
   bit-exactly after (a), after every pass-through push of (c), after the
   push that resumes and after the last; the other pushes return None.  After
   every push the kernel that ran is the cell's row as a stream build (the
   stream dispatcher's choice is launch_decode's) and s.frames is f.  After
   the last push the counters that travel in the header (literal_frames,
   literal_nonfinite, literal_fill, duplicate_frames) are those of one
   one-shot call on the same inputs, lengths, environment and flags; for the
   -inf kind that one-shot call must have taken literal frames (a condition
   on the inputs).

2. test_every_stream_instantiation_is_accounted_for: every row TABLE marks
   covered has been observed in this session with the stream bit.

3. The LDS tier's edges as streams: the widest beam of the tier (tier 0) and
   one past it (tier 1) at the class counts of test_lds_tier_exactly_full, and
   the four shapes of test_two_wave_layout_fallback, where the helper a stream
   chooses at open must be the one the one-shot call falls back to.

4. Without a GPU (unmarked): every schedule has properties (a) to (d); the
   oracle decodes every compared prefix of every cell, kind and edge shape
   without an error (an error on both sides must not stand in for a
   comparison); in the -inf kind every item's live rows contain -inf.

5. test_stream_bigram_table_kinds: the bigram cells again under the table
   kinds of tests/scorer_tables.py (test_gpu_kernel_matrix.table_kind_case,
   three items): grid entries with half-grid logits (equal totals: the tie
   order must survive the image) and forbidden bigrams with -inf logits, as two
   streams that take turns on the cell's schedule, with the comparisons, row
   and counter checks of 1; the forbidden stream's one-shot call must have
   taken literal frames.  At the run-time-W cells (C from 9000 to 31400, every
   seventh row of the table written) the second stream is grid_forbidden: grid
   entries with 30% -inf on the written rows under half-grid logits, so the
   stream builds of those four kernels copy and meet -inf table entries on the
   fast path (no frame of it may be a non-finite replay).  The forbidden
   pairing's -inf logits send their frames down the literal path, seconds a
   frame at these class counts with the scorer, in the stream and again in the
   one-shot call: measured, those four ids took 6.6, 8.0, 9.7 and 23.5 s, each
   longer than the slowest id its cell had (4.6, 5.6, 3.5 and 9.9 s), and the
   literal path under a forbidden table is what the fourteen smaller cells run.

The references are computed once per (cell, kind) and shared, read-only,
between the census and the GPU tests of a session.
"""
import contextlib
import functools
import zlib

import numpy as np
import pytest

import ctcext_amd
from ctcext_amd import _lib
from parity_util import compare
import oracle
import scorer_tables
from test_gpu_kernel_matrix import (BASE_KINDS, BIGRAM_CELLS, CELLS, KINDS, TABLE, _bigram_table, _stat_row,
                                    table_kind_case)
import test_gpu_stream as stream_tests
from test_gpu_stream import _inputs

gpu = pytest.mark.gpu

B = 3
F32, F64 = "f32", "f64"
NP = {F32: np.float32, F64: np.float64}
CODE = {F32: _lib.CTCEXT_F32, F64: _lib.CTCEXT_F64}
COUNTERS = ("literal_frames", "literal_nonfinite", "literal_fill", "duplicate_frames")

# (cell or edge id, kind) -> a suffix of the seed's name, where the inputs of
# crc32("<id>/<kind>") miss a condition of the census (part 4): the seed
# changes, never the condition
# (eight classes, a forbidden root row and -inf logits: the first frame must leave every item three leaves)
RESEED = {("gstate_f32_bigram", "table/forbidden"): "/b"}


def schedule(T):
    """(pushes, check): pushes[k][b] frames of item b's own utterance in push
    k, and the pushes compared with the oracle.  Item 0 gets all T frames,
    item 1 T - 3 (all four at T = 4), item 2 two."""
    if T < 8:
        # item 0 passes through push 1 and resumes in push 2 with two frames;
        # item 1 passes through push 2 and resumes in push 3; item 2 comes
        # from the header in pushes 2 and 3
        assert T == 4
        return ((1, 1, 1), (0, 2, 1), (2, 0, 0), (1, 1, 0)), (0, 1, 2, 3)
    ones = 3 if T >= 20 else 0   # a few one-frame pushes, as test_gpu_stream.PUSHES
    pushes = [(1, 1, 1), (1, 0, 1), (2, 2, 0)] + [(1, 1, 0)] * ones
    pushes.append((T - 4 - ones, T - 3 - 3 - ones, 0))
    return tuple(pushes), (0, 1, 2, len(pushes) - 1)


# three pushes with (a), (b), (c): item 1 passes through push 1 and resumes in
# push 2; item 2 ends after three frames and comes from the header once
EDGE_T = 6
EDGE_PUSHES = ((1, 1, 1), (2, 0, 2), (3, 3, 0))
EDGE_CHECK = (0, 1, 2)
EDGE_KINDS = ("normal", "ties")
EDGE_CLASSES = [(F32, 20000), (F32, 30000), (F32, 35000), (F32, 38000), (F64, 29), (F64, 5000), (F64, 10000), (F64, 15000)]
FALLBACK = [(30000, 100, 3), (31000, 100, 0), (24000, 200, 2), (24900, 200, 0)]


def _properties(pushes):
    """(a), (b), (c), (d) of the module docstring, for one schedule."""
    nb = len(pushes[0])
    a = max(pushes[0]) == 1
    b = any(max(n) >= 2 for n in pushes)
    c = d = False
    for i in range(nb):
        col = [n[i] for n in pushes]
        for k in range(1, len(col)):
            if col[k] == 0 and sum(col[:k]) > 0 and sum(col[k + 1:]) > 0:
                c = True
        if sum(col) > 0 and len(col) >= 3 and col[-1] == 0 and col[-2] == 0:
            d = True
    return a, b, c, d


def _frames_after(pushes):
    out, f = [], [0] * len(pushes[0])
    for n in pushes:
        f = [p + q for p, q in zip(f, n)]
        out.append(list(f))
    return out


def _rng(ident, kind):
    return np.random.default_rng(zlib.crc32(("%s/%s%s" % (ident, kind, RESEED.get((ident, kind), ""))).encode()))


def _kw(kind, C):
    kw = dict(KINDS[kind])
    if kw["blank_index"] is None:
        kw["blank_index"] = C // 2
    return kw


@functools.lru_cache(maxsize=1)   # (up to 3.9 GB of address space, a seventh of it written)
def _table(name, C, dtype):
    tab = _bigram_table(np.random.default_rng(zlib.crc32(("%s/table" % name).encode())), C, dtype)
    tab.setflags(write=False)
    return tab


def _case(ident, kind, T, C, W, P, dtype, tab, pushes, check, want_ref=True):
    """(x [T, B, C] read-only, the decode attributes, {push: the oracle's
    outputs for the frames given up to and including it}).  An oracle error
    is the test's failure, wherever this runs."""
    x = _inputs(_rng(ident, kind), kind, T, B, C, NP[dtype])
    x.setflags(write=False)
    kw = _kw(kind, C)
    refs = {}
    if want_ref:
        after = _frames_after(pushes)
        for k in check:
            f = after[k]
            try:
                refs[k] = oracle.decode(x[:max(f)], np.array(f, np.int32), W, P, scorer_table=tab, **kw)
            except oracle.OracleError as e:
                raise AssertionError("%s %s: the oracle fails after push %d (frames %s): %s" % (ident, kind, k, f, e))
    return x, kw, refs


def _cell_shapes(name):
    row, shapes, helper_env, flags, own_kinds = CELLS[name]
    return row, shapes, helper_env, flags, tuple(own_kinds or BASE_KINDS)


@functools.lru_cache(maxsize=None)
def _cell_case(name, si, kind):
    row, shapes, _, _, _ = _cell_shapes(name)
    T, C, W, P = shapes[si]
    tab = _table(name, C, row[1]) if row[2] == "bigram" else None
    pushes, check = schedule(T)
    return _case(name, kind, T, C, W, P, row[1], tab, pushes, check)


@functools.lru_cache(maxsize=None)
def _edge_case(ident, kind, C, W, dtype):
    return _case(ident, kind, EDGE_T, C, W, 2, dtype, None, EDGE_PUSHES, EDGE_CHECK)


def _live_has_neg_inf(x, frames):
    return [bool(np.isneginf(x[:n, b]).any()) for b, n in enumerate(frames)]


def _stream_table_kinds(name):
    """grid and forbidden; at the run-time-W cells grid and grid_forbidden, the
    kind test_gpu_kernel_matrix gives them (5 of the module docstring)."""
    return ("grid", "forbidden") if CELLS[name][1][0][1] <= 5000 else ("grid", "grid_forbidden")


_neg_inf_share = {}   # (cell, table kind) -> the share of -inf among the table's written rows, for the census


@functools.lru_cache(maxsize=2)   # (one cell's two kinds: a table is up to 3.9 GB of address space, a seventh of it written)
def _drawn(name, tkind):
    case = table_kind_case(name, tkind, B=B, reseed=RESEED.get((name, "table/" + tkind), ""))
    case[0].setflags(write=False)
    case[5].setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _table_kind_case(name, tkind):
    """(x read-only, attributes, {push: the oracle's outputs}) of a bigram cell
    under a table kind, on the cell's schedule.  The table is not kept with
    them: _kind_table has it from _drawn, or draws it again."""
    x, _, W, P, kw, tab = _drawn(name, tkind)
    written = tab if tab.shape[1] <= scorer_tables.SPARSE_ABOVE else tab[::scorer_tables.SPARSE_STEP]
    _neg_inf_share[name, tkind] = float(np.isneginf(written).mean())
    pushes, check = schedule(x.shape[0])
    after = _frames_after(pushes)
    refs = {}
    for k in check:
        f = after[k]
        try:
            refs[k] = oracle.decode(x[:max(f)], np.array(f, np.int32), W, P, scorer_table=tab, **kw)
        except oracle.OracleError as e:
            raise AssertionError("%s %s: the oracle fails after push %d (frames %s): %s" % (name, tkind, k, f, e))
    return x, kw, refs


def _kind_table(name, tkind):
    return _drawn(name, tkind)[5]


# ---- 4. the census, without a GPU

def test_schedules_have_the_four_properties():
    lengths = sorted({s[0] for c in CELLS.values() for s in c[1]})
    assert lengths[0] == 4 and lengths[-1] >= 20
    for T in lengths:
        pushes, check = schedule(T)
        assert _properties(pushes) == (True, True, True, True), (T, pushes)
        assert _frames_after(pushes)[-1] == [T, T if T == 4 else T - 3, 2], (T, pushes)
        assert all(max(n) >= 1 for n in pushes)
        # compared: after (a), after every pass-through push of (c), after the resume, after the last
        assert 0 in check and len(pushes) - 1 in check
        for b in range(B):
            col = [n[b] for n in pushes]
            for k in range(1, len(col) - 1):
                if col[k] == 0 and sum(col[:k]) > 0 and col[k + 1] > 0:
                    assert k in check and k + 1 in check, (T, b, k)
        if T >= 20:
            assert sum(1 for n in pushes if max(n) == 1) >= 4 and len(check) < len(pushes)
    assert _properties(EDGE_PUSHES)[:3] == (True, True, True)
    assert _frames_after(EDGE_PUSHES)[-1] == [EDGE_T, EDGE_T - 2, 3]


@pytest.mark.parametrize("name", sorted(CELLS))
def test_census_cell(name):
    row, shapes, _, _, kinds = _cell_shapes(name)
    for si, (T, C, W, P) in enumerate(shapes):
        pushes, check = schedule(T)
        for kind in kinds:
            x, kw, refs = _cell_case(name, si, kind)
            assert sorted(refs) == sorted(check)
            if kind == "neg_inf":
                assert all(_live_has_neg_inf(x, _frames_after(pushes)[-1])), (name, kind)


def _edge_shapes(dtype, C):
    W = int(_lib.load().ctcext_max_beam_width(C, CODE[dtype]))
    assert W >= 2
    return [("edge_%s_c%d_w%d" % (dtype, C, w), C, w, t) for w, t in ((W, 0), (W + 1, 1))]


@pytest.mark.parametrize("name", BIGRAM_CELLS)
def test_census_bigram_table_kinds(name):
    T = CELLS[name][1][0][0]
    pushes, check = schedule(T)
    for tkind in _stream_table_kinds(name):
        x, kw, refs = _table_kind_case(name, tkind)
        assert sorted(refs) == sorted(check)
        if tkind == "grid_forbidden":
            assert np.isfinite(x).all() and _neg_inf_share[name, tkind] > 0.2
        if tkind == "forbidden":
            assert all(_live_has_neg_inf(x, _frames_after(pushes)[-1])), name
            assert kw["merge_repeated"] is False and _neg_inf_share[name, tkind] > 0.3


@pytest.mark.parametrize("dtype,C", EDGE_CLASSES)
def test_census_lds_tier_edges(dtype, C):
    for ident, C_, W, _ in _edge_shapes(dtype, C):
        for kind in EDGE_KINDS:
            assert sorted(_edge_case(ident, kind, C_, W, dtype)[2]) == list(EDGE_CHECK)


@pytest.mark.parametrize("C,W,helper", FALLBACK)
def test_census_two_wave_layout_fallback(C, W, helper):
    for kind in EDGE_KINDS:
        assert sorted(_edge_case("fallback_c%d_w%d" % (C, W), kind, C, W, F32)[2]) == list(EDGE_CHECK)


@pytest.mark.parametrize("name", sorted(stream_tests.FAMILIES))
def test_census_stream_families_neg_inf(name):
    # the -inf kind of test_gpu_stream.test_family_chunked_matches_oracle: its
    # aligned pushes, the prefixes it compares
    (T, C, W, P), dtype, scorer, env, flags, row = stream_tests.FAMILIES[name]
    x, sl, kw, tab = stream_tests._family_case(name, "neg_inf")
    assert all(_live_has_neg_inf(x, sl)), name
    for i, (t1, _, _) in enumerate(stream_tests._aligned_chunks(x, sl, stream_tests.PUSHES)):
        if i in stream_tests.CHECK_AFTER:
            try:
                stream_tests._oracle_prefix(x, sl, t1, W, P, kw, tab)
            except oracle.OracleError as e:
                raise AssertionError("%s: the oracle fails on the first %d frames: %s" % (name, t1, e))


# ---- the stream runs

_observed = set()   # kernel rows seen with the stream bit in this session


def _set_helper(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    else:
        monkeypatch.setenv("CTCEXT_HELPER", env)


def _run_streams(jobs, pushes, check, W, P, dtype, tab, flags, row=None, tier=0):
    """Pushes the schedule through one stream per job (what, x, kw, refs), the
    streams taking turns push by push, and returns each stream's stats after
    its last push.  refs None: no comparison (the census of part 2).  A job
    with a fifth field brings its own scorer table.

    The streams of a call are the kinds of one shape: the same kernel and
    layout with other data and attributes.  LDS is not cleared between
    launches, so a lone stream could find a word its image missed still in
    place from its own previous push; with the turns, the launch before a
    resume left another stream's state there."""
    T, _, C = jobs[0][1].shape
    with contextlib.ExitStack() as stack:
        streams = [stack.enter_context(ctcext_amd.StreamDecoder(B, C, W, P, max_frames=T, dtype=NP[dtype],
                                                                scorer_table=job[4] if len(job) > 4 else tab,
                                                                flags=flags, **job[2])) for job in jobs]
        at = [[0] * B for _ in jobs]
        for k, n in enumerate(pushes):
            for s, f, (what, x, kw, refs) in zip(streams, at, (job[:4] for job in jobs)):
                chunk = np.zeros((max(n), B, C), NP[dtype])
                for b in range(B):
                    chunk[:n[b], b] = x[f[b]:f[b] + n[b], b]
                    f[b] += n[b]
                try:
                    out = s.push(chunk, np.array(n, np.int32), batch_first=False, results=k in check)
                except ctcext_amd.OpError as e:
                    raise AssertionError("%s push %d: %s" % (what, k, e))
                st = s.last_stats
                kst = st["kernel"]
                assert kst["launched"] and kst["stream"], (what, k, kst)
                if row is not None:
                    assert _stat_row(kst) == row, (what, k, kst)
                assert st["tier"] == tier and kst["tier"] == tier, (what, k, st)
                assert s.frames.tolist() == f, (what, k)
                _observed.add(_stat_row(kst))
                if k not in check:
                    assert out is None
                elif refs is not None:
                    try:
                        compare(out, refs[k], P, lp_exact=True)
                    except AssertionError as e:
                        raise AssertionError("%s after push %d (frames %s): %s" % (what, k, f, e))
        return [dict(s.last_stats) for s in streams]


def _run_cell(name, monkeypatch, kinds=None, want_ref=True):
    row, shapes, helper_env, flags, own_kinds = _cell_shapes(name)
    tier, dtype, scorer = row[:3]
    _set_helper(monkeypatch, helper_env)   # (read when the stream opens, and by the one-shot call)
    for si, (T, C, W, P) in enumerate(shapes):
        pushes, check = schedule(T)
        tab = _table(name, C, dtype) if scorer == "bigram" else None
        jobs = []
        for kind in kinds or own_kinds:
            if want_ref:
                x, kw, refs = _cell_case(name, si, kind)
            else:
                x, kw, refs = _case(name, kind, T, C, W, P, dtype, tab, pushes, check, want_ref=False)[:2] + (None,)
            jobs.append(("%s %s" % (name, kind), x, kw, refs))
        stats = _run_streams(jobs, pushes, check, W, P, dtype, tab, flags, row, tier)
        if not want_ref:
            continue
        lengths = np.array(_frames_after(pushes)[-1], np.int32)
        for (what, x, kw, _), st in zip(jobs, stats):
            ctcext_amd.ctc_ext_beam_search_decoder(x, lengths, W, P, flags=flags, scorer_table=tab, **kw)
            one = ctcext_amd.get_decoder(0).last_stats
            assert _stat_row(one["kernel"]) == row and not one["kernel"]["stream"], (what, one["kernel"])
            print("%s: one-shot %s, stream %s" % (what, {c: one[c] for c in COUNTERS}, {c: st[c] for c in COUNTERS}))
            if what.endswith(" neg_inf"):
                assert one["literal_frames"] > 0, (what, one)
            for c in COUNTERS:
                assert st[c] == one[c], (what, c, st[c], one[c])


@gpu
@pytest.mark.parametrize("name", sorted(CELLS))
def test_stream_instantiation_matches_oracle(name, monkeypatch):
    """1 of the module docstring.  The four counters of COUNTERS are compared
    with the one-shot call's in every cell and kind; none is left out."""
    _run_cell(name, monkeypatch)


@gpu
def test_every_stream_instantiation_is_accounted_for(monkeypatch):
    """The twin of test_gpu_kernel_matrix's census: of the 50 rows of TABLE
    the 42 marked covered have run as a stream build in this session (seen by
    the tests above, or by pushing the cell's first kind here without the
    oracle); the eight unreachable rows are the same (WC = 0 at C <= 64 below
    RN = 4), and no stream ran a row outside the table."""
    assert len(TABLE) == 50
    covered = [r for r, (mark, _) in TABLE.items() if mark == "covered"]
    unreachable = [r for r, (mark, _) in TABLE.items() if mark == "unreachable"]
    assert len(covered) == 42 and len(unreachable) == 8
    for (tier, dtype, scorer, RN, WC, BIG, helper) in unreachable:
        assert tier == 0 and WC == 0 and not BIG and RN in (1, 2) and helper == "none"
    for row in covered:
        cell = TABLE[row][1]
        assert CELLS[cell][0] == row
        if row not in _observed:
            _run_cell(cell, monkeypatch, kinds=_cell_shapes(cell)[4][:1], want_ref=False)
        assert row in _observed, cell
    assert _observed <= set(covered), sorted(_observed - set(covered))
    print("stream rows observed: %d" % len(_observed & set(covered)))


# ---- 5. the bigram cells under the other table kinds

@gpu
@pytest.mark.parametrize("name", BIGRAM_CELLS)
def test_stream_bigram_table_kinds(name, monkeypatch):
    """5 of the module docstring."""
    row, shapes, helper_env, flags, _ = _cell_shapes(name)
    tier, dtype = row[:2]
    _set_helper(monkeypatch, helper_env)
    (T, C, W, P), = shapes
    pushes, check = schedule(T)
    jobs = [("%s table %s" % (name, tkind),) + _table_kind_case(name, tkind) + (_kind_table(name, tkind),)
            for tkind in _stream_table_kinds(name)]
    stats = _run_streams(jobs, pushes, check, W, P, dtype, None, flags, row, tier)
    lengths = np.array(_frames_after(pushes)[-1], np.int32)
    for (what, x, kw, _, tab), st in zip(jobs, stats):
        ctcext_amd.ctc_ext_beam_search_decoder(x, lengths, W, P, flags=flags, scorer_table=tab, **kw)
        one = ctcext_amd.get_decoder(0).last_stats
        assert _stat_row(one["kernel"]) == row and not one["kernel"]["stream"], (what, one["kernel"])
        print("%s: one-shot %s, stream %s" % (what, {c: one[c] for c in COUNTERS}, {c: st[c] for c in COUNTERS}))
        if what.endswith(" table forbidden"):
            assert one["literal_frames"] > 0, (what, one)
        if what.endswith(" grid_forbidden"):   # (the fast path met the -inf entries)
            assert one["literal_nonfinite"] == 0, (what, one)
        for c in COUNTERS:
            assert st[c] == one[c], (what, c, st[c], one[c])


# ---- 3. the LDS tier's edges as streams

def _edge_stream(ident, C, W, dtype, tier):
    jobs = [("%s %s" % (ident, kind),) + _edge_case(ident, kind, C, W, dtype) for kind in EDGE_KINDS]
    stats = _run_streams(jobs, EDGE_PUSHES, EDGE_CHECK, W, 2, dtype, None, 0, None, tier)
    assert len({(st["helper"], st["kernel_raw"]) for st in stats}) == 1, stats   # (the same kernel for every kind)
    return stats[-1]


@gpu
@pytest.mark.parametrize("dtype,C", EDGE_CLASSES)
def test_lds_tier_exactly_full_as_stream(dtype, C, monkeypatch):
    # the widest beam the LDS tier takes: an image of (within bytes of) the
    # whole 160 KB; then one more: the global-state tier, no image at all
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    assert ctcext_amd.get_decoder(0).lib.ctcext_max_beam_width(C, CODE[dtype]) == _edge_shapes(dtype, C)[0][2]
    for ident, C_, W, tier in _edge_shapes(dtype, C):
        _edge_stream(ident, C_, W, dtype, tier)


@gpu
@pytest.mark.parametrize("C,W,helper", FALLBACK)
def test_two_wave_layout_fallback_as_stream(C, W, helper, monkeypatch):
    # the two-wave layout stops fitting before the one-wave one does: the
    # helper a stream chooses at open is the one-shot call's fallback
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    st = _edge_stream("fallback_c%d_w%d" % (C, W), C, W, F32, 0)
    assert st["helper"] == helper, st
    assert st["kernel"]["helper"] == {0: "none", 2: "HW", 3: "SQ"}[helper], st
