"""The frame boundary of the small-C scored two-wave float kernel (round 16):
the helper prefetches the next frame's row and normaliser into a second row
buffer, and with the beam full it scores the frame's first chunk from a bottom
of -inf beside wave 0's recursion (ctcx_decode.hip: kRowPrefetch,
kEarlyChunk0, recurse_wave0).  All seven outputs bit-exact against the oracle.

Every case first checks that the kernel under test ran (two-wave, scored,
small C, float, base scorer) without a re-decode, unless it says otherwise.

The closed-turn census (test_closed_turn_in_first_chunk_census).  A frame's
first chunk holds the offers of branches 0, 1 and (part of) 2.  Gathered at
-inf, the helper finds no turn closed, so wave 0 must find it closed at the
turn's start.  The census counts on the CPU, from the oracle's totals alone,
the frames in which that happens:
  * the frame-start totals of frame t are the oracle's log-probabilities of
    the prefix x[:t] with top_paths = W (descending: branch k's is lp_t[k]);
  * a branch's turn is closed iff its total is <= the bottom when its turn
    starts.  Every push of a later turn's child scores below that turn's
    branch total (x - norm < 0), and the bottom is at most the last pushed
    score, so "lp_t[k] <= the frame's final bottom lp_{t+1}[W-1]" holds iff no
    push happened from turn k on, that is iff the grow ended at a closed turn
    j <= k, with the bottom of that moment.
The census counts against the bottom at the turn's start, which is what wave
0 tests (against the bottom before branch 0's turn, the smallest recursed
leaf, no turn of branch 1 or 2 can be closed at all).

What it finds: for the grow to end by branch 2, the beam must hold W entries
at or above branch 2's total after at most two turns, and two turns push at
most 2 (C - 1) children.  On the N(0, 1) x 3.0 and x 8.0 inputs the count is 0
for every shape here (184 or 188 full-beam frames each, 172 at W = 17; closed
by branch 2: none), and for W = 100 / 128 at C = 29 it cannot be otherwise.
So the census asserts for those inputs that the early path runs at all (frames
that start with a full beam), and the non-zero count on an input built for
it: "peaked_flat" (x 8.0 on even frames, x 0.05 on odd ones: widely spread
totals, then a flat row whose 28 children of branch 0 all land above branch
1's total) at W = 16, C = 29, which test_shapes_and_inputs decodes too.  A
beam that never fills (W = 64, C = 2: at most T + 1 = 49 prefixes) has no
full-beam frame: the kernel's gather does not run there either, and the
census asserts that instead.
"""
import numpy as np
import pytest
import torch

import ctcext_amd
import oracle
import range_inputs
from ctcext_amd import _lib
from parity_util import compare

pytestmark = pytest.mark.gpu

B, T, P = 4, 48, 2
SHAPES = [(128, 29), (100, 29), (16, 29), (17, 3), (64, 2), (128, 64)]
KINDS = ["x0.25", "x3", "x8", "halves", "peaked_flat"]
SCALE = {"x0.25": 0.25, "x3": 3.0, "x8": 8.0}


def _stats():
    return ctcext_amd.get_decoder(0).last_stats


def _assert_scored_kernel(redecodes=0, st=None, stream=False):
    st = st or _stats()
    k = st["kernel"]
    assert st["helper"] == 3, st
    assert k["launched"] and k["helper"] == "SQ" and not k["BIG"] and k["RN"] == 1, k
    assert k["dtype"] == "f32" and k["scorer"] == "base" and k["tier"] == 0, k
    assert bool(k["stream"]) == stream, k
    assert st["helper_redecodes"] == redecodes, st


def _draw(W, C, kind, shape=(T, B)):
    rng = np.random.default_rng(16000 + 131 * W + 7 * C + KINDS.index(kind))
    x = rng.standard_normal(shape + (C,))
    if kind == "halves":
        x = np.round(x * 2) / 2
    elif kind == "peaked_flat":
        x[0::2] *= 8.0
        x[1::2] *= 0.05
    else:
        x = x * SCALE[kind]
    return x.astype(np.float32)


_CASES = {}


def _case(W, C, kind, blank):
    """(logits, lengths, oracle outputs), computed once per case and shared."""
    key = (W, C, kind, blank)
    if key not in _CASES:
        x = _draw(W, C, kind)
        x.setflags(write=False)
        sl = np.full(B, T, np.int32)
        _CASES[key] = (x, sl, oracle.decode(x, sl, W, P, True, blank))
    return _CASES[key]


# ---------------------------------------------------------------------------
# 1. shapes and inputs

@pytest.mark.parametrize("blank", ["first", "last"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,C", SHAPES)
def test_shapes_and_inputs(W, C, kind, blank):
    bi = 0 if blank == "first" else C - 1
    x, sl, ref = _case(W, C, kind, bi)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=bi)
    _assert_scored_kernel()
    compare(out, ref, P)


def _census(x, W, blank):
    """(frames that start with a full beam, those of them whose grow ended at
    a closed turn of branch 1 or 2), over the items of x: see the module
    docstring.  Oracle calls only."""
    full = closed = 0
    for b in range(x.shape[1]):
        lp = {}
        for t in range(1, x.shape[0] + 1):
            try:
                lp[t] = oracle.raw_decode(x[:t, b:b + 1], [t], W, W, True, blank)[2][0]
            except oracle.OracleError:      # fewer than W leaves: the beam is not full
                pass
        for t in sorted(lp):
            if t + 1 not in lp:
                continue
            start, end = lp[t], lp[t + 1]   # frame t (0-based) starts from `start`
            assert np.isfinite(start).all() and (np.diff(start) <= 0).all()
            full += 1
            closed += int(start[2] <= end[W - 1])   # (start[1] <= start[2]... descending: branch 2's test covers branch 1's)
    return full, closed


@pytest.mark.parametrize("blank", ["first", "last"])
@pytest.mark.parametrize("kind", ["x3", "x8", "peaked_flat"])
@pytest.mark.parametrize("W,C", SHAPES)
def test_closed_turn_in_first_chunk_census(W, C, kind, blank):
    """test_shapes_and_inputs is not vacuous: the early path runs (frames that
    start with a full beam), and on the input built for it the grow ends at a
    turn that starts inside the first chunk (a CPU count on the inputs;
    nothing of the product runs).  See the module docstring."""
    bi = 0 if blank == "first" else C - 1
    x, _, _ = _case(W, C, kind, bi)
    full, closed = _census(x, W, bi)
    print("census W=%d C=%d %s blank=%d: full-beam frames %d, closed in the first chunk %d" % (W, C, kind, bi, full, closed))
    if (W, C) == (64, 2):   # at most T + 1 prefixes over one label: never 64 leaves
        assert full == 0
    else:
        assert full > 0, (full, closed)
    if (W, C, kind) == (16, 29, "peaked_flat"):
        assert closed > 0, (full, closed)


# ---------------------------------------------------------------------------
# 2. ragged lengths, the rows past each length NaN

# literal_frames of this very call on the library of commit 50d534b (the
# parent of round 16), MI355X
RAGGED_LITERAL_FRAMES_PARENT = 2


def test_ragged_lengths_nan_past_the_end():
    # (top_paths = 1: the item without frames has one leaf, the root; with two
    # paths asked the op fails the call, as the reference does)
    W, C = 128, 29
    x = _draw(W, C, "x0.25").copy()
    sl = np.array([0, 1, 2, T], np.int32)
    for b, n in enumerate(sl):
        x[n:, b] = np.nan
    ref = oracle.decode(x, sl, W, 1, True, 0)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, 1, merge_repeated=True, blank_index=0)
    _assert_scored_kernel()
    st = _stats()
    print("ragged: literal_frames %d" % st["literal_frames"])
    compare(out, ref, 1)
    # a prefetch one row too far, or a stale buffer, reads a NaN row: a literal frame
    assert st["literal_frames"] == RAGGED_LITERAL_FRAMES_PARENT, st


# ---------------------------------------------------------------------------
# 3. strided device inputs, float32

def test_batch_major_view():
    W, C = 128, 29
    x, sl, ref = _case(W, C, "x3", 0)
    tm = torch.as_tensor(x.copy()).cuda()          # [T, B, C] storage
    view = tm.transpose(0, 1)                      # [B, T, C], time stride B * C
    assert not view.is_contiguous()
    out = ctcext_amd.decode_logits(view, sl, W, P, batch_first=True, merge_repeated=True, blank_index=0)
    _assert_scored_kernel()
    compare(out, ref, P)
    bm = tm.transpose(0, 1).contiguous()           # [B, T, C] storage
    out = ctcext_amd.decode_logits(bm, sl, W, P, batch_first=True, merge_repeated=True, blank_index=0)
    _assert_scored_kernel()
    compare(out, ref, P)


def test_time_window_of_a_nan_tensor():
    W, C = 128, 29
    x, _, _ = _case(W, C, "x3", 0)
    big = torch.full((T, B, C), float("nan"), dtype=torch.float32, device="cuda")
    big[5:37] = torch.as_tensor(x[5:37].copy()).cuda()
    win = big[5:37]
    sl = np.full(B, 32, np.int32)
    ref = oracle.decode(np.ascontiguousarray(x[5:37]), sl, W, P, True, 0)
    lit0 = None
    for view, bf in ((win, False), (win.transpose(0, 1), True)):
        out = ctcext_amd.decode_logits(view, sl, W, P, batch_first=bf, merge_repeated=True, blank_index=0)
        _assert_scored_kernel()
        compare(out, ref, P)
        # (a row read outside the window is NaN: a literal frame)
        clean = ctcext_amd.get_decoder(0).last_stats["literal_frames"]
        lit0 = clean if lit0 is None else lit0
        assert clean == lit0
    ctcext_amd.ctc_ext_beam_search_decoder(np.ascontiguousarray(x[5:37]), sl, W, P, merge_repeated=True, blank_index=0)
    assert _stats()["literal_frames"] == lit0


# ---------------------------------------------------------------------------
# 4. half inputs: the unchanged row stage

@pytest.mark.parametrize("half", ["float16", "bfloat16"])
def test_half_inputs(half):
    W, C = 128, 29
    xh = torch.as_tensor(_draw(W, C, "x3")).to(getattr(torch, half))
    wide = xh.float().numpy()
    sl = np.array([T, T - 1, 7, T], np.int32)
    ref = oracle.decode(wide, sl, W, P, True, 0)
    out = ctcext_amd.decode_logits(xh.cuda(), sl, W, P, batch_first=False, merge_repeated=True, blank_index=0)
    _assert_scored_kernel()
    compare(out, ref, P)


# ---------------------------------------------------------------------------
# 5. frames that leave the exact path mid-sequence

def _literal(x, sl, W, blank=0):
    ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=blank)
    return _stats()["literal_frames"]


def test_plus_inf_row_mid_sequence():
    """One +inf logit in frame 20 of item 1: the row test sends both waves to
    the literal path; its normaliser is NaN, so is every total of the item
    from then on, and each later frame of the item is literal as well (T - 20
    frames), on top of the frames the prefix has by itself.  The other items
    keep the exact path: the frames before and after run the early chunk."""
    W, C, t0 = 128, 29, 20
    x = _draw(W, C, "x0.25").copy()
    sl = np.full(B, T, np.int32)
    before = _literal(np.ascontiguousarray(x[:t0]), np.full(B, t0, np.int32), W)
    clean = _literal(x, sl, W)
    assert clean == before, (clean, before)      # (these inputs have no literal frame of their own after frame 20)
    x[t0, 1, C // 2] = np.inf
    ref = oracle.decode(x, sl, W, P, True, 0)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=0)
    _assert_scored_kernel()
    st = _stats()
    print("+inf: literal_frames %d (clean %d)" % (st["literal_frames"], clean))
    compare(out, ref, P)
    assert st["literal_frames"] == clean + (T - t0), st


def _huge_frame(x, t0, W, blank):
    """One row of the `huge` family per item for frame t0, such that the
    recursion of that frame gives a total of -inf although the row passes the
    row test (a condition on the inputs, established on the host): the row is
    finite with a finite normaliser; the blank overflows to -inf against it
    (every branch's blank-ending total is then -inf); and so does a label that
    a leaf of the beam after t0 frames ends in (the oracle's W best prefixes),
    whose label-ending total, and with it its total, is -inf too.  At least
    one label stays finite, so leaves survive."""
    C = x.shape[2]
    rows = range_inputs.family(range_inputs.rng_for("early_chunk/huge"), "huge", 512, 1, C, np.float32)[:, 0]
    norm = oracle.row_norm(rows)
    with np.errstate(over="ignore"):
        d = rows - norm[:, None]
    frame = np.empty((x.shape[1], C), np.float32)
    k = 0
    for b in range(x.shape[1]):
        dec = oracle.raw_decode(np.ascontiguousarray(x[:t0, b:b + 1]), [t0], W, W, True, blank)[0][0]
        assert len(dec) == W                      # the beam is full: the helper gathers this frame
        last = sorted({seq[-1] for seq in dec if seq})
        while True:
            assert k < len(rows), "no such row among 512 of the family"
            ok = np.isfinite(norm[k]) and np.isneginf(d[k, blank]) and np.isneginf(d[k, last]).any() \
                and np.isfinite(np.delete(d[k], blank)).any()
            k += 1
            if ok:
                frame[b] = rows[k - 1]
                break
    return frame


def test_nonfinite_total_after_the_recursion():
    """Frame 24 holds rows of the `huge` family (_huge_frame): finite, so the
    row test passes and the helper is already gathering when wave 0's
    recursion yields totals of -inf.  Wave 0 hands the frame to the literal
    path alone: one frame per item more that is literal for a non-finite
    value than the clean sequence has.  No other frame gains one: entries
    with a total of -inf are no leaves of the next frame, whose totals are
    finite again.  The frames after it run exact, from the leaves that
    survive (fewer than W at first, then a full beam again)."""
    W, C, t0 = 128, 29, 24
    x = _draw(W, C, "x0.25").copy()
    sl = np.full(B, T, np.int32)
    ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=0)
    clean = dict(_stats())
    x[t0] = _huge_frame(x, t0, W, 0)
    ref = oracle.decode(x, sl, W, P, True, 0)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=0)
    _assert_scored_kernel()
    st = _stats()
    print("huge: literal_frames %d nonfinite %d (clean %d, %d)" % (st["literal_frames"], st["literal_nonfinite"],
                                                                   clean["literal_frames"], clean["literal_nonfinite"]))
    compare(out, ref, P)
    assert st["literal_nonfinite"] == clean["literal_nonfinite"] + B, st
    assert st["literal_frames"] >= clean["literal_frames"] + B, st


# ---------------------------------------------------------------------------
# 6. streams

@pytest.mark.parametrize("W,C,kind", [(128, 29, "x3"), (100, 29, "halves")])
def test_stream_pushes(W, C, kind):
    x, sl, _ = _case(W, C, kind, 0)
    kw = dict(merge_repeated=True, blank_index=0)
    with ctcext_amd.StreamDecoder(B, C, W, P, T, **kw) as s:
        t0 = 0
        for n in (1, 2, 3, 7, None):
            t1 = T if n is None else t0 + n
            out = s.push(x[t0:t1], batch_first=False)
            _assert_scored_kernel(st=s.last_stats, stream=True)
            assert s.last_stats["kernel"]["stream"] == bool(_lib.CTCEXT_KERNEL_STREAM)
            ref = oracle.decode(np.ascontiguousarray(x[:t1]), np.full(B, t1, np.int32), W, P, **kw)
            compare(out, ref, P)
            t0 = t1


# ---------------------------------------------------------------------------
# 7. the helper starts out dead (the existing flag and path)

def test_helper_dead_redecodes():
    W, C = 128, 29
    x, sl, ref = _case(W, C, "x3", 0)
    with pytest.warns(RuntimeWarning, match="hand-over wait timed out"):
        out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=0,
                                                     flags=_lib.CTCEXT_FLAG_TEST_HELPER_DEAD)
    assert _stats()["helper_redecodes"] == 1, _stats()
    compare(out, ref, P)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, merge_repeated=True, blank_index=0)
    _assert_scored_kernel()
    compare(out, ref, P)
