"""Blank-frame skipping for streams on the GPU (StreamDecoder(skip_blank=) /
ctcext_stream_open_skip; include/ctcext.h, "Streaming: blank-frame skipping"):
after EVERY push, exact equality of all dense outputs, status, frames, the kept
counts, the mapped stable frames and the token times with the definition -- the
one-shot skipping decode (skip_util.expected over the CPU oracle) of everything
pushed to each item so far.

What a case exercises is asserted from the oracle-side plan before the
comparison (frames dropped, wholly dropped pushes, pushes that begin inside a
run), so a run that drops nothing cannot pass."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
import skip_util as su
import stream_skip_util as ssu
from ctcext_amd import _lib
from token_times_util import expected_from_rows, family

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = -7
GS = _lib.CTCEXT_FLAG_GLOBAL_STATE
DEAD = _lib.CTCEXT_FLAG_TEST_HELPER_DEAD
LENGTH, FEW, TIMEOUT, CAPACITY = (_lib.CTCEXT_ITEM_LENGTH, _lib.CTCEXT_ITEM_FEW_LEAVES,
                                  _lib.CTCEXT_ITEM_HELPER_TIMEOUT, _lib.CTCEXT_ITEM_CAPACITY)
HYP = ctcext_amd.StreamDense._fields[:5]
KW = dict(merge_repeated=True, blank_index=0, blank_label=-1)


def _i32(v):
    return torch.as_tensor(np.asarray(v, np.int32), device=DEV)


def _dev(c):
    return torch.as_tensor(np.array(c), device=DEV)


def _host(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def _stream_kw(kw):
    return {k: v for k, v in kw.items() if k != "scorer_table"}


class _Items:
    """What each item has received since its last reset, as the inputs of the
    one-shot call the definition compares with."""

    def __init__(self, B, C, dtype):
        self.rows = [np.zeros((0, C), dtype) for _ in range(B)]

    def take(self, b, frames):
        self.rows[b] = np.concatenate([self.rows[b], frames])

    def reset(self, b):
        self.rows[b] = self.rows[b][:0]

    @property
    def n(self):
        return [len(r) for r in self.rows]

    def expected(self, W, P, thr, kw):
        T = max(max(self.n), 1)
        x = np.zeros((T, len(self.rows)) + self.rows[0].shape[1:], self.rows[0].dtype)
        for b, r in enumerate(self.rows):
            x[:len(r), b] = r
        return su.expected(x, self.n, W, P, thr, **kw)


def _assert_push(got, tt, kept, e, n, F, kw, what, items=None, status=0):
    """One push's host arrays against the definition's outputs e for frames n."""
    B, P = got[0].shape[0], got[0].shape[1]
    sel = list(range(B)) if items is None else list(items)
    for name, g, w in zip(HYP, got[:5], su.to_dense(e, B, P, F, PAD)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g[sel], w[sel], err_msg="%s %s" % (what, name))
    np.testing.assert_array_equal(got[5][sel], status, err_msg=what + " status")
    assert got[6].dtype == np.int32 and got[6][sel].tolist() == [n[b] for b in sel], (what, got[6], n)
    assert kept.dtype == np.int32 and kept[sel].tolist() == e.kept[sel].tolist(), (what, kept, e.kept)
    if tt is not None:
        want = expected_from_rows(e.dec, e.ali, n, B, P, F, kw.get("blank_label", -1),
                                  bool(kw.get("merge_repeated", False)))
        for name, g, w in zip(ctcext_amd.TokenTimes._fields, tt, want):
            assert g.dtype == np.int32 and g.shape == w.shape, (what, name)
            np.testing.assert_array_equal(g[sel], w[sel], err_msg="%s %s" % (what, name))


def _mapped(e, r):
    """stable_frames on the original axis from the record-frame answers r."""
    return [0 if r[b] == 0 else e.kmaps[b][r[b] - 1] + 1 for b in range(len(r))]


def _drive(x, sl, sched, W, P, thr, kw=KW, *, F=None, dtype="float32", flags=0, to_dev=_dev, batch_major=False,
           width=None, what=""):
    """Feeds x / sl by the schedule to a skipping stream, nothing waited for
    until every push is enqueued; beside it a plain stream takes the frames the
    oracle-side plan keeps (the reference of the stable prefix in record
    frames).  Then compares every push.  Returns (check()'s stats, e of the end)."""
    T, B, C = x.shape
    F = int(max(sl)) if F is None else F
    skw = _stream_kw(kw)
    tab = kw.get("scorer_table")
    kmaps = su.plan(x, sl, thr, kw.get("blank_index", 0))
    items = _Items(B, C, x.dtype)
    pos = [0] * B
    rec = []
    with ctcext_amd.StreamDecoder(B, C, W, P, F, dtype=dtype, scorer_table=tab, flags=flags, device=DEV,
                                  skip_blank=thr, **skw) as s, \
            ctcext_amd.StreamDecoder(B, C, W, P, F, dtype=dtype, scorer_table=tab, flags=flags, device=DEV,
                                     **skw) as twin:
        for n in sched:
            c = ssu.chunk(x, pos, n, width)
            cd = to_dev(c)
            if batch_major:
                cd = cd.transpose(0, 1).contiguous()
            out = s.push_dense(cd, _i32(n), batch_first=batch_major, stable=True, pad_value=PAD)
            tt = s.token_times_dense()
            kept = s.kept_dense().clone()
            kn = [ssu.kept_between(kmaps[b], pos[b], pos[b] + n[b]) for b in range(B)]
            cc = np.zeros((max(max(map(len, kn)), 1), B, C), x.dtype)
            for b in range(B):
                cc[:len(kn[b]), b] = x[kn[b], b]
                items.take(b, x[pos[b]:pos[b] + n[b], b])
                pos[b] += n[b]
            tw = twin.push_dense(to_dev(cc), _i32([len(k) for k in kn]), batch_first=False, results=False, stable=True)
            rec.append((out, tt, kept, tw, list(pos), items.expected(W, P, thr, kw)))
        st = s.check()
        twin.check()
        assert st["kernel"]["launched"] and st["kernel"]["stream"], st
        prev = [0] * B
        for i, (out, tt, kept, tw, n, e) in enumerate(rec):
            w = "%s push %d" % (what, i)
            got, r = _host(out), _host(tw)
            assert [k[:len(m)] for k, m in zip(kmaps, e.kmaps)] == e.kmaps   # (a prefix's plan is a prefix of the plan)
            _assert_push(got, _host(tt), _host([kept])[0], e, n, F, kw, w)
            assert r[6].tolist() == e.kept.tolist(), w
            assert got[7].tolist() == r[7].tolist(), (w, got[7], r[7])
            assert got[8].dtype == np.int64 and got[8].tolist() == _mapped(e, r[8].tolist()), (w, got[8], r[8])
            assert all(a >= b for a, b in zip(got[8].tolist(), prev)), (w, got[8], prev)
            prev = got[8].tolist()
        # the synchronous queries, after the last push
        assert s.frames.tolist() == pos and s.kept_frames().tolist() == e.kept.tolist()
        last = _host(rec[-1][0])
        for q in (s.stable(), s._stable_reference()):
            assert q.decoded_length.tolist() == last[7].tolist() and q.frames.tolist() == last[8].tolist(), (what, q)
    return st, e


# ---- 1. the families, in pushes of 1, 3 and 7 frames and in one push

SHAPES = [(12, 6, 5, 8, 3), (40, 4, 29, 16, 3), (60, 3, 29, 128, 3)]
# the seed per (family, shape) at which every schedule below has a wholly
# dropped (item, push) pair and a push that begins inside a run (picked on the
# CPU with skip_util.plan; the test asserts it)
SEEDS = {"peaky": (1, 1, 1), "sticky": (3, 1, 0), "gaussian": (4, 2, 6)}
PUSHES = (1, 3, 7, None)
FAMILY_CASES = ([("peaky", s, m, p) for s in SHAPES for m in (False, True) for p in PUSHES]
                + [(k, s, True, p) for k in ("sticky", "gaussian") for s in SHAPES for p in PUSHES])


@functools.lru_cache(maxsize=None)
def _family_inputs(kind, shape, dtype="float32"):
    T, B, C, W, P = shape
    x = family(np.random.default_rng(SEEDS[kind][SHAPES.index(shape)]), kind, T, B, C, np.dtype(dtype))
    x.setflags(write=False)
    sl = su.lengths(T, B)
    thr = su.THR if kind == "peaky" else su.median_threshold(x, sl)
    return x, sl, thr


def _assert_exercised(x, sl, thr, sched, share=0.0, blank=0, whole_push=True):
    kmaps = su.plan(x, sl, thr, blank)
    dropped = 1 - sum(map(len, kmaps)) / float(np.maximum(sl, 0).sum())
    assert dropped > 0 and dropped >= share, dropped
    whole, straddle = ssu.exercised(kmaps, sched)
    if len(sched) > 1:
        assert (whole >= 1 or not whole_push) and straddle >= 1, (whole, straddle)
    return whole, straddle


@pytest.mark.parametrize("kind,shape,merge,push", FAMILY_CASES,
                         ids=["%s-%s-%s-%s" % (k, "x".join(map(str, s)), "merge" if m else "plain", p or "one")
                              for k, s, m, p in FAMILY_CASES])
def test_families_match_the_definition_after_every_push(kind, shape, merge, push, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = shape
    x, sl, thr = _family_inputs(kind, shape)
    sched = ssu.schedule(sl, push)
    _assert_exercised(x, sl, thr, sched, 0.25 if kind == "peaky" else 0.0)
    kw = dict(KW, merge_repeated=merge)
    _drive(np.array(x), sl, sched, W, P, thr, kw, what="%s %s %s" % (kind, shape, push))


# ---- 2. long rows: the tile carry and a long kmap

LONG = (600, 3, 29, 16, 2)


@functools.lru_cache(maxsize=None)
def _long_inputs():
    T, B, C, W, P = LONG
    x = family(np.random.default_rng(1), "peaky", T, B, C)
    x.setflags(write=False)
    return x, su.lengths(T, B)


@pytest.mark.parametrize("how", ["pushes_of_7", "300_and_300"])
def test_long_rows(how, monkeypatch):
    """600 frames per item: pushes of 7 frames (86 appends to kmap and cidx, 15
    wholly dropped pairs, about 120 that begin inside a run), and two pushes of
    300 (the plan's workgroup form: two tiles, the flag and the count carried
    from the first to the second)."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = LONG
    x, sl = _long_inputs()
    kept = [len(k) for k in su.plan(x, sl, su.THR)]
    assert all(280 <= k <= 340 for k in kept), kept
    if how == "pushes_of_7":
        sched = ssu.schedule(sl, 7)
        whole, straddle = _assert_exercised(x, sl, su.THR, sched, 0.25)
        assert whole >= 10 and straddle >= 100, (whole, straddle)
    else:
        sched = [[300] * B, [int(n) - 300 for n in sl]]
        _assert_exercised(x, sl, su.THR, sched, 0.25, whole_push=False)   # (both items begin push 2 inside a run)
    _drive(np.array(x), sl, sched, W, P, su.THR, what=how)


# ---- 3. ragged chunk lengths with empty pushes in between

def test_ragged_lengths_and_empty_pushes_carry_the_flag(monkeypatch):
    """Per-item chunk lengths of 0 .. 5 in chunks 5 frames wide; an item that
    gets no frame in a push keeps its flag: at least one such item stands inside
    a run (its next frame is dropped only if the flag survived the empty push)."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = SHAPES[1]
    T, B, C, W, P = shape
    x, sl, thr = _family_inputs("peaky", shape)
    rng = np.random.default_rng(9)
    sched, pos = [[1] * B], [1] * B
    while any(p < n for p, n in zip(pos, sl)):
        step = [min(int(rng.integers(0, 6)) * int(rng.random() < 0.7), int(n) - p) for p, n in zip(pos, sl)]
        sched.append(step)
        pos = [p + s for p, s in zip(pos, step)]
    kmaps = su.plan(x, sl, thr)
    pos, inside = [0] * B, 0
    for n in sched:
        for b in range(B):
            inside += n[b] == 0 and 0 < pos[b] < sl[b] and pos[b] not in kmaps[b]
            pos[b] += n[b]
    assert inside >= 3, inside
    _assert_exercised(x, sl, thr, sched, 0.25)
    _drive(np.array(x), sl, sched, W, P, thr, width=5, what="ragged")


# ---- 4. tiers, sizes, dtypes, layouts, labels, scorer

def test_global_state_tier(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = SHAPES[1]
    x, sl, thr = _family_inputs("peaky", SHAPES[1])
    sched = ssu.schedule(sl, 3)
    _assert_exercised(x, sl, thr, sched, 0.25)
    st, _ = _drive(np.array(x), sl, sched, W, P, thr, flags=GS, what="global state")
    assert st["tier"] == 1, st


def test_more_than_64_classes(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 2, 100, 16, 2
    x = family(np.random.default_rng(0), "peaky", T, B, C)
    sl = su.lengths(T, B)
    sched = ssu.schedule(sl, 3)
    _assert_exercised(x, sl, su.THR, sched, 0.25)
    st, _ = _drive(x, sl, sched, W, P, su.THR, what="C = 100")
    assert st["kernel"]["BIG"], st


def test_float64(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = SHAPES[1]
    x, sl, thr = _family_inputs("peaky", SHAPES[1], "float64")
    sched = ssu.schedule(sl, 3)
    _assert_exercised(x, sl, thr, sched, 0.25)
    st, e = _drive(np.array(x), sl, sched, W, P, thr, dtype="float64", what="float64")
    assert st["kernel"]["dtype"] == "f64" and e.log_prob.dtype == np.float64, st


@pytest.mark.parametrize("C", [29, 32], ids=["rows_of_single_elements", "rows_of_16_byte_pieces"])
@pytest.mark.parametrize("half", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_half_chunks(half, C, monkeypatch):
    """bf16 / f16 chunks, read in place by the plan and gathered as 2-byte
    elements or 16-byte pieces; the definition runs on the widened values."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, W, P = 40, 4, 16, 3
    x = torch.as_tensor(family(np.random.default_rng(1), "peaky", T, B, C)).to(half).float().numpy()
    sl = su.lengths(T, B)
    sched = ssu.schedule(sl, 3)
    _assert_exercised(x, sl, su.THR, sched, 0.25)
    _drive(x, sl, sched, W, P, su.THR, to_dev=lambda c: _dev(c).to(half), what=str(half))


def test_batch_major_chunk(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = SHAPES[1]
    x, sl, thr = _family_inputs("peaky", SHAPES[1])
    sched = ssu.schedule(sl, 7)
    _assert_exercised(x, sl, thr, sched, 0.25)
    _drive(np.array(x), sl, sched, W, P, thr, batch_major=True, what="batch-major")


def test_blank_index_2_with_blank_label_7(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 4, 5, 8, 3
    x = family(np.random.default_rng(1), "peaky", T, B, C, blank=2)
    sl = su.lengths(T, B)
    kw = dict(merge_repeated=True, blank_index=2, blank_label=7)
    sched = ssu.schedule(sl, 3)
    _assert_exercised(x, sl, su.THR, sched, 0.25, blank=2)
    assert su.plan(x, sl, su.THR, 0) != su.plan(x, sl, su.THR, 2)   # (the plan reads class 2)
    _, e = _drive(x, sl, sched, W, P, su.THR, kw, what="blank 2 / 7")
    assert any(7 in e.ali[b][p] for b in range(B) for p in range(P))


def test_bigram_scorer_table(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = SHAPES[1]
    x, sl, thr = _family_inputs("peaky", SHAPES[1])
    tab = (-np.abs(np.random.default_rng(84).standard_normal((C + 1, C))) * 2).astype(np.float32)
    sched = ssu.schedule(sl, 3)
    _assert_exercised(x, sl, thr, sched, 0.25)
    st, _ = _drive(np.array(x), sl, sched, W, P, thr, dict(KW, scorer_table=tab), what="bigram")
    assert st["kernel"]["scorer"] == "bigram", st


# ---- 5. threshold 0

def test_threshold_0_is_the_plain_stream_bit_for_bit(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = SHAPES[1]
    x, sl, _ = _family_inputs("peaky", SHAPES[1])
    pos, rec = [0] * B, []
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, skip_blank=0.0, **KW) as s, \
            ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, **KW) as plain:
        for n in ssu.schedule(sl, 3):
            c, ln = _dev(ssu.chunk(x, pos, n)), _i32(n)
            pos = [p + k for p, k in zip(pos, n)]
            a = s.push_dense(c, ln, batch_first=False, stable=True, pad_value=PAD)
            ta, ka = s.token_times_dense(), s.kept_dense().clone()
            b = plain.push_dense(c, ln, batch_first=False, stable=True, pad_value=PAD)
            rec.append((a, ta, ka, b, plain.token_times_dense(), list(pos)))
        s.check()
        plain.check()
        for i, (a, ta, ka, b, tb, n) in enumerate(rec):
            for name, g, w in zip(ctcext_amd.StreamDense._fields, _host(a), _host(b)):
                assert g.dtype == w.dtype
                np.testing.assert_array_equal(g, w, err_msg="push %d %s" % (i, name))
            for g, w in zip(_host(ta), _host(tb)):
                np.testing.assert_array_equal(g, w)
            assert _host([ka])[0].tolist() == n
        assert s.kept_frames().tolist() == s.frames.tolist() == plain.frames.tolist() == sl.tolist()
        assert plain.kept_frames().tolist() == sl.tolist()   # (without skipping: the frame counts)


# ---- 6. reset, status bits: hand-made runs

def _pattern(rows, C, seed, blank=0):
    """[T, B, C] float32 logits from one string per item: 'D' is a frame the
    blank dominates (+8 on it), any other character one with +8 on another
    class.  Asserted against the definition's own flags."""
    rng = np.random.default_rng(seed)
    T, B = max(map(len, rows)), len(rows)
    x = rng.standard_normal((T, B, C)).astype(np.float32)
    for b, r in enumerate(rows):
        for t, ch in enumerate(r):
            c = blank if ch == "D" else 1 + int(rng.integers(0, C - 1))
            x[t, b, c] += 8
    dom = su.logp_blank(x) > np.float32(su.THR)
    for b, r in enumerate(rows):
        assert [bool(v) for v in dom[:len(r), b]] == [ch == "D" for ch in r], (b, r)
    return x


ST = (20, 100, 5)   # C, W, P: the two-wave kernel, whose hand-over CTCEXT_FLAG_TEST_HELPER_DEAD fails


def _status_stream(rows, F, seed):
    C, W, P = ST
    x = _pattern(rows, C, seed)
    s = ctcext_amd.StreamDecoder(len(rows), C, W, P, F, device=DEV, skip_blank=su.THR, **KW)
    return s, x, _Items(len(rows), C, np.float32)


def _push(s, items, x, pos, n, length=None, take=None, **kw):
    """One push of frames pos[b] .. pos[b] + n[b] - 1 of x; `take` names the
    items expected to advance (all).  Returns the host arrays of the push."""
    B = x.shape[1]
    c = ssu.chunk(x, pos, n)
    out = s.push_dense(_dev(c), _i32(n if length is None else length), batch_first=False, pad_value=PAD, **kw)
    tt = s.token_times_dense()
    kept = s.kept_dense().clone()
    for b in (range(B) if take is None else take):
        items.take(b, x[pos[b]:pos[b] + n[b], b])
        pos[b] += n[b]
    return _host(out), _host(tt), _host([kept])[0]


@pytest.mark.parametrize("how", ["reset_argument", "reset_call"])
def test_reset_of_an_item_whose_last_frame_was_blank_dominant(how, monkeypatch):
    """Item 1 is reset standing in a run; its new utterance begins with
    blank-dominant frames: the first is frame 0 and kept (with the flag left
    over it would be dropped), the second is dropped.  The other items go on,
    item 0 through a run that straddles the push."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    C, W, P = ST
    F = 12
    s, x, items = _status_stream(["aDDDDaDDa", "aaDDD", "DDaDDDaDD"], F, 3)
    y = _pattern(["", "DDaDDa", ""], C, 4)
    pos = [0, 0, 0]
    got, tt, kept = _push(s, items, x, pos, [4, 5, 4])
    e = items.expected(W, P, su.THR, KW)
    assert e.kept.tolist() == [2, 3, 3]
    _assert_push(got, tt, kept, e, pos, F, KW, "before the reset")
    items.reset(1)
    ypos = [0, 0, 0]
    c = ssu.chunk(x, pos, [3, 0, 3])
    c[:3, 1] = y[:3, 1]
    if how == "reset_call":
        s.reset([1])
        assert s.frames.tolist() == [4, 0, 4] and s.kept_frames().tolist() == [2, 0, 3]
        out = s.push_dense(_dev(c), _i32([3, 3, 3]), batch_first=False, pad_value=PAD)
    else:
        out = s.push_dense(_dev(c), _i32([3, 3, 3]), reset=_i32([0, 1, 0]), batch_first=False, pad_value=PAD)
    tt, kept = s.token_times_dense(), s.kept_dense().clone()
    for b in (0, 2):
        items.take(b, x[pos[b]:pos[b] + 3, b])
        pos[b] += 3
    items.take(1, y[:3, 1])
    ypos[1] = 3
    e = items.expected(W, P, su.THR, KW)
    assert e.kmaps[1] == [0, 2] and e.kept.tolist() == [4, 2, 4]
    _assert_push(_host(out), _host(tt), _host([kept])[0], e, [7, 3, 7], F, KW, "the reset push")
    # a reset together with a status bit: the bit does not undo it
    out = s.push_dense(_dev(c), _i32([0, 9, 0]), reset=_i32([0, 1, 0]), batch_first=False, pad_value=PAD)
    got = _host(out)
    assert got[5].tolist() == [0, LENGTH, 0] and got[6].tolist() == [7, 0, 7]
    assert _host([s.kept_dense()])[0].tolist() == [4, 0, 4]
    with pytest.raises(ctcext_amd.FailedPreconditionError):
        s.check()
    items.reset(1)
    c = ssu.chunk(x, pos, [2, 0, 2])
    c[:2, 1] = y[:2, 1]
    out = s.push_dense(_dev(c), _i32([2, 2, 2]), batch_first=False, pad_value=PAD)
    tt, kept = s.token_times_dense(), s.kept_dense().clone()
    for b in (0, 2):
        items.take(b, x[pos[b]:pos[b] + 2, b])
    items.take(1, y[:2, 1])
    e = items.expected(W, P, su.THR, KW)
    assert e.kmaps[1] == [0]
    _assert_push(_host(out), _host(tt), _host([kept])[0], e, [9, 2, 9], F, KW, "after the reset")
    s.check()
    s.close()


def test_status_length_and_capacity_keep_n_kept_and_flag(monkeypatch):
    """max_frames = 12.  Item 1 (8 frames, 3 kept, standing in a run) is pushed
    5 more: 13 > 12 on the original axis though its 3 + 3 records would fit:
    CTCEXT_ITEM_CAPACITY, with the original-axis total in check()'s message.
    Then a length above the chunk's frames.  Both leave its n, kept count and
    flag: the frame it takes next is dropped, as the definition has it."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    C, W, P = ST
    F = 12
    s, x, items = _status_stream(["aDDaDDDaDDaa", "DDDaDDDDDaDDa", "aaDDDDaDDDDa"], F, 5)
    pos = [0, 0, 0]
    got, tt, kept = _push(s, items, x, pos, [4, 8, 4])
    e = items.expected(W, P, su.THR, KW)
    assert e.kept.tolist() == [3, 3, 3]
    _assert_push(got, tt, kept, e, pos, F, KW, "first")
    got, tt, kept = _push(s, items, x, pos, [5, 5, 5], take=[0, 2])
    e = items.expected(W, P, su.THR, KW)
    assert got[5].tolist() == [0, CAPACITY, 0]
    _assert_push(got, tt, kept, e, [9, 8, 9], F, KW, "capacity", items=[0, 2])
    assert got[6].tolist() == [9, 8, 9] and kept.tolist() == [e.kept[0], 3, e.kept[2]]
    assert (got[0][1] == PAD).all() and (got[3][1] == 0).all()
    with pytest.raises(ctcext_amd.InvalidArgumentError) as err:
        s.check()
    assert err.value.message == "stream capacity exceeded: item 1 would hold 13 frames of max_frames 12"
    assert s.frames.tolist() == [9, 8, 9] and s.kept_frames().tolist() == kept.tolist()
    got, tt, kept = _push(s, items, x, pos, [1, 2, 1], length=[1, 3, 1], take=[0, 2])
    assert got[5].tolist() == [0, LENGTH, 0] and got[6].tolist() == [10, 8, 10] and kept[1] == 3
    with pytest.raises(ctcext_amd.FailedPreconditionError) as err:
        s.check()
    assert err.value.message == "sequence_length(1) <= 2"
    # item 1 takes what it missed: frame 8 stands behind the blank-dominant frame 7 and is dropped
    got, tt, kept = _push(s, items, x, pos, [2, 4, 2])
    e = items.expected(W, P, su.THR, KW)
    assert 8 not in e.kmaps[1] and e.kmaps[1][-1] == 10 and pos == [12, 12, 12]
    _assert_push(got, tt, kept, e, pos, F, KW, "after the status bits")
    s.check()
    s.close()


def test_status_helper_timeout_keeps_n_kept_and_flag(monkeypatch):
    """A push whose hand-over fails commits nothing: not the records, and not n,
    the kept count or the flag its plan had ready.  Every item stands in a run
    when it fails and the failed chunk ends outside one, so the next frame is
    kept only if the flag was wrongly taken from the failed push."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    C, W, P = ST
    F = 12
    s, x, items = _status_stream(["aDDDDaDDaDDa", "DDDDDDaaDDDa", "aaDDDaDDDaDa"], F, 6)
    bad = _pattern(["aDa", "Daa", "DDa"], C, 7)
    pos = [0, 0, 0]
    got, tt, kept = _push(s, items, x, pos, [3, 3, 4])
    e = items.expected(W, P, su.THR, KW)
    _assert_push(got, tt, kept, e, pos, F, KW, "first")
    out = s.push_dense(_dev(bad), batch_first=False, pad_value=PAD, flags=DEAD)
    got, k2 = _host(out), _host([s.kept_dense().clone()])[0]
    assert got[5].tolist() == [TIMEOUT] * 3 and got[6].tolist() == pos and k2.tolist() == kept.tolist()
    assert (got[0] == PAD).all() and (got[1] == 0).all() and (got[3] == 0).all()
    with pytest.raises(ctcext_amd.InternalError):
        s.check()
    assert s.last_stats["kernel"]["helper"] == "SQ"
    assert s.frames.tolist() == pos and s.kept_frames().tolist() == kept.tolist()
    for n in ([2, 2, 1], [7, 7, 7]):
        got, tt, kept = _push(s, items, x, pos, n)
        e = items.expected(W, P, su.THR, KW)
        _assert_push(got, tt, kept, e, pos, F, KW, "after the timeout")
    assert all(3 not in e.kmaps[b] for b in (0, 1)) and 4 not in e.kmaps[2]   # (each stood in a run)
    s.check()
    s.close()


def test_too_few_leaves_is_judged_on_the_kept_frames(monkeypatch):
    """C = 3, top_paths = 4: one kept frame has 3 leaves.  The second frame is
    dropped, so the item still has too few after two frames (a plain stream has
    enough by then); the third is kept."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    B, C, W, P, F = 2, 3, 8, 4, 6
    x = _pattern(["DDaD", "DDDa"], C, 8)
    items = _Items(B, C, np.float32)
    with ctcext_amd.StreamDecoder(B, C, W, P, F, device=DEV, skip_blank=su.THR, **KW) as s, \
            ctcext_amd.StreamDecoder(B, C, W, P, F, device=DEV, **KW) as plain:
        pos = [0, 0]
        for i in range(2):
            got, _, kept = _push(s, items, x, pos, [1, 1])
            assert got[5].tolist() == [FEW, FEW] and got[6].tolist() == [i + 1] * 2 and kept.tolist() == [1, 1]
            assert (got[0] == PAD).all() and (got[1] == 0).all()
        for t in range(2):
            q = _host(plain.push_dense(_dev(x[t:t + 1]), batch_first=False))
        assert q[5].tolist() == [0, 0]
        with pytest.raises(ctcext_amd.InvalidArgumentError) as err:
            s.check()
        assert err.value.message == "Less leaves in the beam search than requested."
        got, tt, kept = _push(s, items, x, pos, [1, 1])
        assert got[5].tolist() == [0, FEW] and kept.tolist() == [2, 1] and got[6].tolist() == [3, 3]
        # (item 1, still short of leaves, cannot go through the oracle's batch: item 0 alone)
        one = su.expected(np.ascontiguousarray(x[:3, :1]), [3], W, P, su.THR, **KW)
        for name, g, w in zip(HYP, got[:5], su.to_dense(one, 1, P, F, PAD)):
            np.testing.assert_array_equal(g[:1], w, err_msg=name)
        with pytest.raises(ctcext_amd.InvalidArgumentError):
            s.check()
        got, tt, kept = _push(s, items, x, pos, [1, 1])
        e = items.expected(W, P, su.THR, KW)
        assert e.kmaps == [[0, 2, 3], [0, 3]]
        _assert_push(got, tt, kept, e, pos, F, KW, "fourth frame")
        s.check()


# ---- 7. the push only enqueues; graph capture; two streams; the synchronous push

@pytest.mark.parametrize("where", ["default_stream", "side_stream"])
def test_push_only_enqueues(where, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = LONG
    x, sl = _long_inputs()
    sched = [[300] * B, [int(n) - 300 for n in sl]]
    chunks = [(_dev(x[:300]), _i32(sched[0])), (_dev(x[300:]), _i32(sched[1]))]
    e = su.expected(np.array(x), sl, W, P, su.THR, **KW)
    stream = torch.cuda.Stream(device=DEV) if where == "side_stream" else torch.cuda.default_stream(DEV)

    def blocked(*a, **k):
        raise AssertionError("push_dense reached a host synchronisation")

    warm = ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, skip_blank=su.THR, **KW)
    s = ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, skip_blank=su.THR, **KW)
    with torch.cuda.stream(stream):
        if where == "default_stream":
            assert torch.cuda.current_stream(DEV).cuda_stream == 0
        warm.push_dense(chunks[0][0], chunks[0][1], batch_first=False, stable=True)   # loads the kernels
        warm.token_times_dense()
        s.reserve(300)
        kept = s.kept_dense()
        torch.cuda.synchronize()
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "synchronize", blocked)
            m.setattr(torch.cuda.Stream, "synchronize", blocked)
            m.setattr(torch.Tensor, "cpu", blocked)
            m.setattr(torch.Tensor, "item", blocked)
            for c, ln in chunks:
                out = s.push_dense(c, ln, batch_first=False, stable=True, pad_value=PAD)
                tt = s.token_times_dense()
        ev = torch.cuda.Event()
        ev.record()
        done_at_return = ev.query()
        ev.synchronize()
    assert not done_at_return, "the pushes had finished when push_dense returned: it did not only enqueue"
    _assert_push(_host(out), _host(tt), _host([kept])[0], e, sl.tolist(), T, KW, where)
    s.check()
    warm.close()
    s.close()


def test_graph_capture_and_replay(monkeypatch):
    """One push of 4 frames with its token times, captured after reserve(4)
    alone and replayed over successive chunks: ragged lengths, an empty push
    for an item, and the kept tensor, which the captured push keeps writing."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = SHAPES[1]
    F = T
    x, sl, thr = _family_inputs("peaky", SHAPES[1])
    side = torch.cuda.Stream(device=DEV)
    warm = ctcext_amd.StreamDecoder(B, C, W, P, F, device=DEV, skip_blank=thr, **KW)
    with torch.cuda.stream(side):
        warm.push_dense(torch.zeros((4, B, C), device=DEV), batch_first=False, stable=True)
        warm.token_times_dense()
    side.synchronize()
    s = ctcext_amd.StreamDecoder(B, C, W, P, F, device=DEV, skip_blank=thr, **KW)
    s.reserve(4)
    kept = s.kept_dense()
    xs = torch.zeros((4, B, C), device=DEV)
    lens = torch.zeros((B,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = s.push_dense(xs, lens, batch_first=False, stable=True, pad_value=PAD)
        tt = s.token_times_dense()
    items, pos = _Items(B, C, np.float32), [0] * B
    sched = [[4, 3, 2, 4], [4, 4, 0, 1], [1, 4, 4, 4], [4, 0, 3, 4], [2, 4, 4, 4], [4, 4, 1, 4], [3, 2, 4, 4],
             [4, 4, 4, 4]]
    kmaps = su.plan(x, sl, thr)
    assert ssu.exercised([k for k in kmaps], sched)[0] >= 1
    prev = [0] * B
    for i, n in enumerate(sched):
        n = [min(k, int(sl[b]) - pos[b]) for b, k in enumerate(n)]
        xs.copy_(torch.as_tensor(ssu.chunk(x, pos, n, 4)))
        lens.copy_(torch.as_tensor(np.asarray(n, np.int32)))
        for b in range(B):
            items.take(b, x[pos[b]:pos[b] + n[b], b])
            pos[b] += n[b]
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        e = items.expected(W, P, thr, KW)
        got = _host(out)
        _assert_push(got, _host(tt), _host([kept])[0], e, pos, F, KW, "replay %d" % i)
        assert all(a >= b for a, b in zip(got[8].tolist(), prev)) and all(a <= b for a, b in zip(got[8].tolist(), pos))
        prev = got[8].tolist()
    assert max(prev) > 0
    s.check()
    assert s.frames.tolist() == pos and s.kept_frames().tolist() == e.kept.tolist()
    s.close()
    warm.close()


def test_two_skipping_streams_of_one_decoder_in_flight(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    (Ta, Ba, Ca, Wa, Pa), (Tb, Bb, Cb, Wb, Pb) = SHAPES[0], SHAPES[1]
    xa, sla, tha = _family_inputs("peaky", SHAPES[0])
    xb, slb, thb = _family_inputs("sticky", SHAPES[1])
    ia, ib = _Items(Ba, Ca, np.float32), _Items(Bb, Cb, np.float32)
    pa, pb = [0] * Ba, [0] * Bb
    plan = []
    for na, nb in zip(ssu.schedule(sla, 3), ssu.schedule(slb, 7)):
        ca, cb = _dev(ssu.chunk(xa, pa, na)), _dev(ssu.chunk(xb, pb, nb))
        for it, x, pos, n in ((ia, xa, pa, na), (ib, xb, pb, nb)):
            for b in range(len(pos)):
                it.take(b, x[pos[b]:pos[b] + n[b], b])
                pos[b] += n[b]
        plan.append((ca, _i32(na), list(pa), ia.expected(Wa, Pa, tha, KW), cb, _i32(nb), list(pb),
                     ib.expected(Wb, Pb, thb, KW)))
    assert len(plan) >= 4
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    outs = []
    with ctcext_amd.StreamDecoder(Ba, Ca, Wa, Pa, Ta, device=DEV, skip_blank=tha, **KW) as sa, \
            ctcext_amd.StreamDecoder(Bb, Cb, Wb, Pb, Tb, device=DEV, skip_blank=thb, **KW) as sb:
        for ca, la, _, _, cb, lb, _, _ in plan:
            with torch.cuda.stream(s1):
                oa = sa.push_dense(ca, la, batch_first=False, pad_value=PAD)
                ta, ka = sa.token_times_dense(), sa.kept_dense().clone()
            with torch.cuda.stream(s2):
                ob = sb.push_dense(cb, lb, batch_first=False, pad_value=PAD)
                tb, kb = sb.token_times_dense(), sb.kept_dense().clone()
            outs.append((oa, ta, ka, ob, tb, kb))
        assert sa.dec is sb.dec
        sa.check()
        sb.check()
        torch.cuda.synchronize()
        for i, ((oa, ta, ka, ob, tb, kb), (_, _, na, ea, _, _, nb, eb)) in enumerate(zip(outs, plan)):
            _assert_push(_host(oa), _host(ta), _host([ka])[0], ea, na, Ta, KW, "stream a push %d" % i)
            _assert_push(_host(ob), _host(tb), _host([kb])[0], eb, nb, Tb, KW, "stream b push %d" % i)


def test_synchronous_push_is_unimplemented_and_leaves_the_stream_usable(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = SHAPES[0]
    x, sl, thr = _family_inputs("peaky", SHAPES[0])
    items, pos = _Items(B, C, np.float32), [0] * B
    sched = ssu.schedule(sl, 7)
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device=DEV, skip_blank=thr, **KW) as s:
        got, tt, kept = _push(s, items, x, pos, sched[0])
        for chunk in (_dev(x[7:9]), np.array(x[7:9])):
            with pytest.raises(ctcext_amd.UnimplementedError):
                s.push(chunk, batch_first=False)
        # ... and the library's own answer, behind the C ABI
        c = _lib.Chunk()
        cd = _dev(x[7:9])
        c.chunk_time, c.inputs = 2, cd.data_ptr()
        sizes = (_lib.PathSizes * P)()
        assert s.lib.ctcext_stream_push(s.handle, ctypes.byref(c), sizes) == _lib.CTCEXT_UNIMPLEMENTED
        assert "synchronous push" in s.lib.ctcext_last_error().decode()
        assert s.frames.tolist() == pos and s.kept_frames().tolist() == kept.tolist()
        got, tt, kept = _push(s, items, x, pos, sched[1])
        e = items.expected(W, P, thr, KW)
        _assert_push(got, tt, kept, e, pos, T, KW, "after the refused push")
        s.check()
    # host chunks cannot open a skipping stream at all
    with ctcext_amd.StreamDecoder(B, C, W, P, T, skip_blank=thr, **KW) as h:
        with pytest.raises(ValueError):
            h.push_dense(np.array(x[:2]), batch_first=False)
