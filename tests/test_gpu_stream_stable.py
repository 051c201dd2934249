"""StreamDecoder.stable(): how much of a stream's decoded output is final.

Inputs.  Random Gaussian logits are useless here: at beam widths of 100 and
more the common prefix of all hypotheses stays 0 for tens of frames, and a
kernel that always answers 0 would pass.  The tests use a two-hot recipe with a
decaying margin (``_recipe``): per frame one class at 0, a second at
-8 * 0.85**t, the rest near -40.  On the CPU oracle with top_paths = beam_width
the common prefix of all leaves is then monotone, trails the hypothesis by
roughly log2(W) plus a few labels and ends at or above T / 3 for every item
(36/27/33 of 47 labels at W = 100, 14/14/14 of 25 at (T, C, W) = (30, 8, 40)).
The oracle refuses top_paths = W only while the beam is not full (t <= 2), so
the first compared boundary is t = 3.

Pushes.  3, 1, 1, 5, 7 frames and then the rest.  With the rest in one push
the expected trajectory has three distinct values per item (0 until t = 10,
one value at t = 17, one at T), fewer than the five the non-vacuity check asks
for, so the rest is pushed four frames at a time: every boundary of the plain
schedule is still compared (t = 3, 4, 5, 10, 17, T) and the ones in between as
well.

One family per record format and beam range, the stream kernel-matrix rows of
tests/test_gpu_stream.py at these T; the kernel that ran is asserted from
last_stats as there."""
import functools

import numpy as np
import pytest

import ctcext_amd
from ctcext_amd import _lib
import oracle

pytestmark = pytest.mark.gpu

GS = _lib.CTCEXT_FLAG_GLOBAL_STATE
NP = {"f32": np.float32, "f64": np.float64}
B = 3

# id -> ((T, C, W), dtype, CTCEXT_HELPER or None, flags, record bytes,
#        the kernel that must run: (tier, dtype, scorer, RN, WC, BIG, helper))
FAMILIES = {
    "sq_small": ((48, 20, 100), "f32", None, 0, 4, (0, "f32", "base", 1, 128, False, "SQ")),
    "hw_small": ((48, 20, 100), "f32", "1", 0, 4, (0, "f32", "base", 1, 128, False, "HW")),
    "onewave_rn2": ((48, 20, 200), "f32", None, 0, 8, (0, "f32", "base", 2, 256, False, "none")),
    "onewave_rn4": ((48, 20, 400), "f32", None, 0, 8, (0, "f32", "base", 4, 0, False, "none")),
    "sq_big": ((40, 300, 100), "f32", None, 0, 8, (0, "f32", "base", 1, 128, True, "SQ")),
    "gather_big": ((40, 300, 200), "f32", None, 0, 8, (0, "f32", "base", 2, 256, True, "HW")),
    "f64": ((48, 20, 100), "f64", None, 0, 8, (0, "f64", "base", 1, 128, False, "none")),
    "gstate_f32": ((30, 8, 40), "f32", None, GS, 16, (1, "f32", "base", 1, 0, False, "none")),
}
HEAD = (3, 1, 1, 5, 7)   # then the rest, REST frames at a time
REST = 4
MERGES = {False: dict(merge_repeated=False, blank_index=0), True: dict(merge_repeated=True, blank_index=None)}


def _kw(merge, C):
    kw = dict(MERGES[merge])
    if kw["blank_index"] is None:
        kw["blank_index"] = C // 2
    return kw


def _boundaries(T, head=HEAD, rest=REST):
    """Frames pushed after each push."""
    out, t = [], 0
    for n in head:
        t += n
        out.append(t)
    assert t < T
    while t < T:
        t = min(t + rest, T)
        out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def _recipe(T, C, dtype):
    rng = np.random.default_rng(11)
    x = -40 + rng.standard_normal((T, B, C))
    for t in range(T):
        for b in range(B):
            h = rng.choice(C, size=2, replace=False)
            x[t, b, h[0]] = 0
            x[t, b, h[1]] = -8 * 0.85 ** t
    x = x.astype(NP[dtype])
    x.setflags(write=False)
    return x


def _lcp(seqs):
    n = min(len(s) for s in seqs)
    for i in range(n):
        if any(s[i] != seqs[0][i] for s in seqs):
            return i
    return n


@functools.lru_cache(maxsize=None)
def _expected(name, merge):
    """The oracle's trajectory, computed once per (family, merge): per boundary
    t and item, the longest common prefix of all W decoded sequences of the
    one-shot decode of x[:t] with top_paths = W.  A refusal is an error."""
    (T, C, W), dtype = FAMILIES[name][0], FAMILIES[name][1]
    x = _recipe(T, C, dtype)
    rows = []
    for t in _boundaries(T):
        dec, _, _, _ = oracle.raw_decode(x[:t], [t] * B, W, W, **_kw(merge, C))
        rows.append(tuple(_lcp(dec[b]) for b in range(B)))
    return tuple(rows)


def _set_helper(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    else:
        monkeypatch.setenv("CTCEXT_HELPER", env)


def _stat_row(k):
    return (k["tier"], k["dtype"], k["scorer"], k["RN"], k["WC"], k["BIG"], k["helper"])


def _open(name, merge, P, monkeypatch, max_frames=None):
    (T, C, W), dtype, env, flags, rbytes, row = FAMILIES[name]
    _set_helper(monkeypatch, env)
    return ctcext_amd.StreamDecoder(B, C, W, P, max_frames or T, dtype=NP[dtype], flags=flags, **_kw(merge, C))


def _assert_kernel(s, name):
    rbytes, row = FAMILIES[name][4], FAMILIES[name][5]
    k = s.last_stats["kernel"]
    assert k["launched"] and k["stream"] and _stat_row(k) == row, (name, k)
    assert s.last_stats["record_bytes"] == rbytes, (name, s.last_stats["record_bytes"])


def _pushes(x, bounds):
    t0 = 0
    for t1 in bounds:
        yield t1, x[t0:t1]
        t0 = t1


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_exact_against_oracle(name, monkeypatch):
    """1. merge_repeated=False: after every push decoded_length[b] is the
    longest common prefix of all W sequences the oracle decodes for the
    frames pushed so far; the expected trajectory is not vacuous."""
    (T, C, W) = FAMILIES[name][0]
    exp = _expected(name, False)
    for b in range(B):
        assert exp[-1][b] * 3 >= T, (name, b, exp[-1])
        assert len({row[b] for row in exp}) >= 5, (name, b, exp)
    x = _recipe(T, C, FAMILIES[name][1])
    got = []
    with _open(name, False, 5, monkeypatch) as s:
        for i, (t1, chunk) in enumerate(_pushes(x, _boundaries(T))):
            assert s.push(chunk, batch_first=False, results=False) is None
            _assert_kernel(s, name)
            r = s.stable()
            got.append(tuple(r.decoded_length.tolist()))
            assert (r.frames <= t1).all() and (r.frames >= 0).all()
    print(name, "expected", exp, "got", tuple(got))
    assert tuple(got) == exp


@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merge"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_kernel_against_host_reference(name, merge, monkeypatch):
    """2. Both merge settings, after every push: stable() equals the naive
    host walk in both fields.  With merge_repeated the count is at most the
    common prefix of the oracle's merged sequences (merging can only lengthen
    agreement)."""
    (T, C, W) = FAMILIES[name][0]
    exp = _expected(name, merge)
    x = _recipe(T, C, FAMILIES[name][1])
    seen = set()
    with _open(name, merge, 5, monkeypatch) as s:
        for i, (t1, chunk) in enumerate(_pushes(x, _boundaries(T))):
            s.push(chunk, batch_first=False, results=False)
            _assert_kernel(s, name)
            r, ref = s.stable(), s._stable_reference()
            assert r.decoded_length.tolist() == ref.decoded_length.tolist(), (name, merge, t1)
            assert r.frames.tolist() == ref.frames.tolist(), (name, merge, t1)
            if merge:
                assert (r.decoded_length <= np.array(exp[i])).all(), (name, t1, r.decoded_length, exp[i])
            else:
                assert r.decoded_length.tolist() == list(exp[i]), (name, t1)
            seen.update(r.decoded_length.tolist())
        assert (r.frames > 0).all() and (r.decoded_length > 0).all()
    assert len(seen) >= 5, (name, merge, seen)


def test_beam_past_the_lds_variant(monkeypatch):
    """2, for a beam whose frame of records does not fit the query kernel's LDS
    segment (1600 16-byte records): the variant that reads the records in
    place and keeps its position flags in global memory.  Against the host
    reference after every push, and against the oracle's common prefix from
    t = 17 on (before that the beam is not full and the oracle refuses
    top_paths = W); the oracle's trajectory moves (0 ... 6 ... 9)."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, C, W = 30, 8, 1600
    x = _recipe(T, C, "f32")
    kw = _kw(False, C)
    exp = {}
    for t in _boundaries(T):
        if t >= 17:
            dec, _, _, _ = oracle.raw_decode(x[:t], [t] * B, W, W, **kw)
            exp[t] = [_lcp(dec[b]) for b in range(B)]
    assert min(exp[T]) >= 8 and len({tuple(v) for v in exp.values()}) >= 4, exp
    with ctcext_amd.StreamDecoder(B, C, W, 5, T, flags=GS, **kw) as s:
        prev = None
        for t1, chunk in _pushes(x, _boundaries(T)):
            s.push(chunk, batch_first=False, results=False)
            assert s.last_stats["tier"] == 1 and s.last_stats["record_bytes"] == 16
            (r, walked), ref = s.stable(walked=True), s._stable_reference()
            assert r.decoded_length.tolist() == ref.decoded_length.tolist(), t1
            assert r.frames.tolist() == ref.frames.tolist(), t1
            if t1 in exp:
                assert r.decoded_length.tolist() == exp[t1], t1
            if prev is not None:
                assert (walked <= t1 - prev.frames + 1).all()
            prev = r


def _rows(out, P):
    """decoded rows [b][p] -> list of labels, from the SparseTensor components."""
    rows = [[[] for _ in range(P)] for _ in range(B)]
    for p in range(P):
        idx = np.asarray(out.decoded_indices[p])
        val = np.asarray(out.decoded_values[p])
        for (b, _), v in zip(idx.tolist(), val.tolist()):
            rows[b][p].append(v)
    return rows


def _soundness(s, x, bounds, P, lengths=None):
    """Every path of every later push starts with the labels a push declared
    final (the first decoded_length labels of its path 0)."""
    claims = [[] for _ in range(B)]   # per item: label prefixes declared final
    nonzero = 0
    t0 = 0
    for t1 in bounds:
        ln = None if lengths is None else (np.minimum(lengths, t1) - np.minimum(lengths, t0)).astype(np.int32)
        out = s.push(x[t0:t1], ln, batch_first=False, outputs="host")
        rows = _rows(out, P)
        r = s.stable()
        for b in range(B):
            n = int(r.decoded_length[b])
            assert n <= len(rows[b][0]), (t1, b, n, rows[b][0])
            for pre in claims[b]:
                for p in range(P):
                    assert rows[b][p][:len(pre)] == pre, (t1, b, p, pre, rows[b][p])
            for p in range(P):   # ... and this push's own paths agree on it
                assert rows[b][p][:n] == rows[b][0][:n], (t1, b, p, n)
            claims[b].append(rows[b][0][:n])
            nonzero += n > 0
        t0 = t1
    return nonzero


@pytest.mark.parametrize("merge", [False, True], ids=["plain", "merge"])
@pytest.mark.parametrize("name", ["sq_small", "onewave_rn4", "sq_big", "gstate_f32"])
def test_soundness_on_the_recipe(name, merge, monkeypatch):
    """3. What a push declared final stays: every path of every later push."""
    (T, C, W) = FAMILIES[name][0]
    x = _recipe(T, C, FAMILIES[name][1])
    P = 16
    with _open(name, merge, P, monkeypatch) as s:
        assert _soundness(s, x, _boundaries(T), P) >= B * 3


@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("name", ["sq_small", "gather_big", "gstate_f32"])
def test_soundness_on_flat_inputs(name, kind, monkeypatch):
    """3. Plain Gaussian logits and rounded ones with ties (the inputs of
    tests/test_gpu_stream.py): the answer is mostly 0 there and must not be
    wrong."""
    (T, C, W), dtype = FAMILIES[name][0], FAMILIES[name][1]
    rng = np.random.default_rng(1000 + sorted(FAMILIES).index(name))
    x = rng.standard_normal((T, B, C))
    if kind == "ties":
        x = np.round(x * 2) / 2
    x = x.astype(NP[dtype])
    P = 16
    with _open(name, kind == "ties", P, monkeypatch) as s:
        _soundness(s, x, _boundaries(T), P)
        r, ref = s.stable(), s._stable_reference()
        assert r.decoded_length.tolist() == ref.decoded_length.tolist()
        assert r.frames.tolist() == ref.frames.tolist()


@pytest.mark.parametrize("name", ["sq_small", "onewave_rn2", "gstate_f32"])
def test_cache(name, monkeypatch):
    """4. Querying after every push and only after the last give the same
    answer; frames and decoded_length never decrease; a query after the first
    walks at most the frames above the last answer's frontier."""
    (T, C, W) = FAMILIES[name][0]
    x = _recipe(T, C, FAMILIES[name][1])
    bounds = _boundaries(T)
    with _open(name, True, 5, monkeypatch) as s, _open(name, True, 5, monkeypatch) as once:
        prev = None
        total = 0
        for i, (t1, chunk) in enumerate(_pushes(x, bounds)):
            s.push(chunk, batch_first=False, results=False)
            once.push(chunk, batch_first=False, results=False)
            r, walked = s.stable(walked=True)
            assert s.frames.tolist() == [t1] * B
            if prev is not None:
                assert (r.frames >= prev.frames).all() and (r.decoded_length >= prev.decoded_length).all()
                assert (walked <= t1 - prev.frames + 1).all(), (t1, walked, prev.frames)
            assert (walked >= 0).all()
            total += int(walked.sum())
            prev = r
        last, w_once = once.stable(walked=True)
        assert last.decoded_length.tolist() == prev.decoded_length.tolist()
        assert last.frames.tolist() == prev.frames.tolist()
        # the one query walked from the newest frame to where the chains met
        assert (w_once >= T - 1 - last.frames).all() and (w_once <= T).all()
        # ... and asking again walks only what lies above its own frontier
        again, w_again = once.stable(walked=True)
        assert again.decoded_length.tolist() == last.decoded_length.tolist()
        assert again.frames.tolist() == last.frames.tolist()
        assert (w_again <= T - last.frames + 1).all()
        assert total > 0


def test_ragged_and_reset(monkeypatch):
    """5. Lengths [T, T - 3, T // 2]: an item that stops receiving frames
    keeps its answer; reset([1]) zeroes item 1 alone; item 1 pushed the recipe
    again equals a fresh stream; a stream before its first push answers
    zeros."""
    name = "sq_small"
    (T, C, W) = FAMILIES[name][0]
    x = _recipe(T, C, "f32")
    sl = np.array([T, T - 3, T // 2], np.int32)
    bounds = _boundaries(T)
    with _open(name, False, 5, monkeypatch, max_frames=2 * T) as s:
        z = s.stable()
        assert z.decoded_length.tolist() == [0] * B and z.frames.tolist() == [0] * B
        held = None
        t0 = 0
        for t1 in bounds:
            ln = (np.minimum(sl, t1) - np.minimum(sl, t0)).astype(np.int32)
            s.push(x[t0:t1], ln, batch_first=False, results=False)
            r, ref = s.stable(), s._stable_reference()
            assert r.decoded_length.tolist() == ref.decoded_length.tolist()
            assert r.frames.tolist() == ref.frames.tolist()
            assert (r.frames <= np.minimum(sl, t1)).all()
            if t0 >= sl[2]:   # item 2 got no frame in this push
                assert (r.decoded_length[2], r.frames[2]) == held
            held = (r.decoded_length[2], r.frames[2])
            t0 = t1
        # each item's answer is that of its own frames alone
        exp = _expected(name, False)
        assert r.decoded_length[0] == exp[-1][0]
        assert (r.decoded_length > 0).all()
        before = r
        s.reset([1])
        r = s.stable()
        assert (r.decoded_length[1], r.frames[1]) == (0, 0)
        assert (r.decoded_length[0], r.frames[0]) == (before.decoded_length[0], before.frames[0])
        assert (r.decoded_length[2], r.frames[2]) == (before.decoded_length[2], before.frames[2])
        # item 1 again, from frame 0, against a fresh stream pushed the same frames
        with _open(name, False, 5, monkeypatch) as fresh:
            for t1, chunk in _pushes(x, bounds):
                n = chunk.shape[0]
                s.push(chunk, np.array([0, n, 0], np.int32), batch_first=False, results=False)
                fresh.push(chunk, batch_first=False, results=False)
                r, fr = s.stable(), fresh.stable()
                assert (r.decoded_length[1], r.frames[1]) == (fr.decoded_length[1], fr.frames[1]), t1
                assert (r.decoded_length[0], r.frames[0]) == (before.decoded_length[0], before.frames[0])
            assert r.decoded_length[1] == exp[-1][1]


def test_batch_of_one(monkeypatch):
    """5. B = 1."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, C, W = FAMILIES["sq_small"][0]
    x = np.ascontiguousarray(_recipe(T, C, "f32")[:, 1:2])
    exp = _expected("sq_small", False)
    with ctcext_amd.StreamDecoder(1, C, W, 5, T, **_kw(False, C)) as s:
        for i, (t1, chunk) in enumerate(_pushes(x, _boundaries(T))):
            s.push(chunk, batch_first=False, results=False)
            r = s.stable()
            assert r.decoded_length.shape == (1,) and r.frames.shape == (1,)
            assert int(r.decoded_length[0]) == exp[i][1], t1
            assert r.frames.tolist() == s._stable_reference().frames.tolist()


def test_two_streams_on_one_decoder(monkeypatch):
    """6. Two streams on one decoder keep separate caches."""
    na, nb = "sq_small", "gstate_f32"
    (Ta, Ca, Wa), (Tb, Cb, Wb) = FAMILIES[na][0], FAMILIES[nb][0]
    xa, xb = _recipe(Ta, Ca, "f32"), _recipe(Tb, Cb, "f32")
    ea, eb = _expected(na, False), _expected(nb, False)
    ba, bb = _boundaries(Ta), _boundaries(Tb)
    with _open(na, False, 5, monkeypatch) as sa, _open(nb, False, 5, monkeypatch) as sb:
        pa, pb = list(_pushes(xa, ba)), list(_pushes(xb, bb))
        for i in range(max(len(pa), len(pb))):
            if i < len(pa):
                sa.push(pa[i][1], batch_first=False, results=False)
            if i < len(pb):
                sb.push(pb[i][1], batch_first=False, results=False)
            ra, rb = sa.stable(), sb.stable()
            assert ra.decoded_length.tolist() == list(ea[min(i, len(pa) - 1)]), i
            assert rb.decoded_length.tolist() == list(eb[min(i, len(pb) - 1)]), i
        assert sa.dec is sb.dec
