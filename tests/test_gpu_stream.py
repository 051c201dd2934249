"""Streaming decode against the oracle: a stream that has been pushed frames
[0, t) returns exactly what the oracle returns for the one-shot decode of
x[:t] -- for every kernel family's stream build, across chunk boundaries that
carry duplicate entries and literal frames, for ragged and empty chunks, the
input formats, resets, interleaved streams and failed pushes.

The shapes are the kernel matrix's smallest (tests/test_gpu_kernel_matrix.py,
SMALL) with three items; every comparison is parity_util.compare with the
log-probabilities bit-exact."""
import zlib

import numpy as np
import pytest
import torch

import ctcext_amd
from ctcext_amd import _lib
from parity_util import compare, oracle_or_error
import oracle
import range_inputs

pytestmark = pytest.mark.gpu

GS = _lib.CTCEXT_FLAG_GLOBAL_STATE
LITERAL = _lib.CTCEXT_FLAG_FORCE_LITERAL
DEAD = _lib.CTCEXT_FLAG_TEST_HELPER_DEAD
NP = {"f32": np.float32, "f64": np.float64}
KINDS = {"normal": dict(merge_repeated=False, blank_index=0),
         "ties": dict(merge_repeated=True, blank_index=None),   # (None: C // 2, a non-zero blank)
         # -inf logits: literal and duplicate frames on both sides of a push (the
         # census of test_gpu_stream_matrix.py holds the oracle to decoding
         # every compared prefix of these inputs without an error)
         "neg_inf": dict(merge_repeated=True, blank_index=0)}
# the whole float range (tests/range_inputs.py), test_family_chunked_numeric_range
RANGE_KINDS = {"logsoftmax": dict(merge_repeated=True, blank_index=None),
               "edges": dict(merge_repeated=False, blank_index=0)}
M_LEAVES = "Less leaves in the beam search than requested."

# id -> ((T, C, W, P), dtype, scorer, CTCEXT_HELPER or None, flags,
#        the kernel that must run: (tier, dtype, scorer, RN, WC, BIG, helper))
FAMILIES = {
    "sq_small": ((30, 20, 100, 5), "f32", "base", None, 0, (0, "f32", "base", 1, 128, False, "SQ")),
    "hw_small": ((30, 20, 100, 5), "f32", "base", "1", 0, (0, "f32", "base", 1, 128, False, "HW")),
    "onewave_rn1": ((30, 20, 100, 5), "f32", "base", "0", 0, (0, "f32", "base", 1, 128, False, "none")),
    "onewave_rn2": ((30, 20, 200, 5), "f32", "base", None, 0, (0, "f32", "base", 2, 256, False, "none")),
    "onewave_rn4": ((30, 20, 400, 5), "f32", "base", None, 0, (0, "f32", "base", 4, 0, False, "none")),
    "sq_big": ((20, 300, 100, 5), "f32", "base", None, 0, (0, "f32", "base", 1, 128, True, "SQ")),
    "hw_big": ((20, 300, 100, 5), "f32", "base", "1", 0, (0, "f32", "base", 1, 128, True, "HW")),
    "gather_big": ((20, 300, 200, 5), "f32", "base", None, 0, (0, "f32", "base", 2, 256, True, "HW")),
    "f64": ((30, 20, 100, 5), "f64", "base", None, 0, (0, "f64", "base", 1, 128, False, "none")),
    "bigram": ((30, 20, 100, 5), "f32", "bigram", None, 0, (0, "f32", "bigram", 1, 128, False, "none")),
    "gstate_f32": ((10, 8, 40, 3), "f32", "base", None, GS, (1, "f32", "base", 1, 0, False, "none")),
    "gstate_f64": ((10, 8, 40, 3), "f64", "base", None, GS, (1, "f64", "base", 1, 0, False, "none")),
}
PUSHES = (1, 1, 1, 1, 5, None)   # frames per push; None: the rest
CHECK_AFTER = (0, 3, 4, 5)       # the 1st, 4th, 5th and last push


def _stat_row(k):
    return (k["tier"], k["dtype"], k["scorer"], k["RN"], k["WC"], k["BIG"], k["helper"])


def _inputs(rng, kind, T, B, C, dtype=np.float32):
    if kind in RANGE_KINDS:
        return range_inputs.family(rng, kind, T, B, C, dtype)
    x = rng.standard_normal((T, B, C))
    if kind == "ties":
        x = np.round(x * 2) / 2
    elif kind == "neg_inf":
        x[rng.random(x.shape) < 0.15] = -np.inf
    return x.astype(dtype)


def _kw(kind, C):
    kw = dict(KINDS[kind] if kind in KINDS else RANGE_KINDS[kind])
    if kw["blank_index"] is None:
        kw["blank_index"] = C // 2
    return kw


def _oracle_prefix(x, sl, t, W, P, kw, tab=None):
    return oracle.decode(x[:t], np.minimum(sl, t).astype(np.int32), W, P, scorer_table=tab, **kw)


def _set_helper(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    else:
        monkeypatch.setenv("CTCEXT_HELPER", env)


def _aligned_chunks(x, sl, pushes):
    """(t1, chunk [t, B, C], lengths) per push of a batch whose items all start
    at frame 0: the chunk is x[t0:t1], item b has min(sl_b, t1) - min(sl_b, t0)
    frames in it."""
    T = x.shape[0]
    t0 = 0
    for n in pushes:
        t1 = T if n is None else t0 + n
        yield t1, x[t0:t1], (np.minimum(sl, t1) - np.minimum(sl, t0)).astype(np.int32)
        t0 = t1


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_family_chunked_matches_oracle(name, kind, monkeypatch):
    """1. Every kernel family's stream build: pushes of 1, 1, 1, 1, 5 and the
    rest; after the 1st, 4th, 5th and last the result is the oracle's of the
    prefix, and the kernel that ran is the family's, as a stream build.  The
    kinds: N(0,1) logits, logits on a grid of halves (ties), and N(0,1) with
    15% of the logits -inf."""
    _chunked_family(name, kind, monkeypatch)


@pytest.mark.parametrize("kind", sorted(RANGE_KINDS))
@pytest.mark.parametrize("name", ["sq_small", "sq_big", "f64", "gstate_f32"])
def test_family_chunked_numeric_range(name, kind, monkeypatch):
    """1, on log_softmax outputs and on terms at expf's / exp's underflow bound
    and in the subnormal band: the state saved between pushes carries totals
    of that range, and the last push's result is the one-shot decode's."""
    _chunked_family(name, kind, monkeypatch)


def _family_case(name, kind):
    """(x [T, 3, C], the items' lengths, the decode attributes, the bigram
    table or None) of one family and kind."""
    (T, C, W, P), dtype, scorer, env, flags, row = FAMILIES[name]
    rng = np.random.default_rng(zlib.crc32(("%s/%s" % (name, kind)).encode()))
    x = _inputs(rng, kind, T, 3, C, NP[dtype])
    sl = np.array([T, T - 3, T // 2], np.int32)
    tab = (-np.abs(rng.standard_normal((C + 1, C))) * 2).astype(NP[dtype]) if scorer == "bigram" else None
    return x, sl, _kw(kind, C), tab


def _chunked_family(name, kind, monkeypatch):
    (T, C, W, P), dtype, scorer, env, flags, row = FAMILIES[name]
    _set_helper(monkeypatch, env)
    B = 3
    x, sl, kw, tab = _family_case(name, kind)
    if kind in RANGE_KINDS:
        range_inputs.assert_census(kind, np.concatenate([x[:n, b] for b, n in enumerate(sl)]))
    with ctcext_amd.StreamDecoder(B, C, W, P, T, dtype=NP[dtype], scorer_table=tab, flags=flags, **kw) as s:
        for i, (t1, chunk, ln) in enumerate(_aligned_chunks(x, sl, PUSHES)):
            check = i in CHECK_AFTER
            out = s.push(chunk, ln, batch_first=False, results=check)
            k = s.last_stats["kernel"]
            assert k["launched"] and k["stream"] and _stat_row(k) == row, (name, kind, i, k)
            assert s.last_stats["tier"] == row[0]
            assert s.frames.tolist() == np.minimum(sl, t1).tolist()
            if check:
                compare(out, _oracle_prefix(x, sl, t1, W, P, kw, tab), P, lp_exact=True)
            else:
                assert out is None


@pytest.mark.parametrize("name", ["bigram", "sq_big", "hw_big", "gather_big", "f64", "onewave_rn4", "gstate_f32",
                                  "gstate_f64"])
def test_family_device_chunks_match_oracle(name, monkeypatch):
    """1, with the chunks where a model leaves them: GPU tensors, batch-major
    vocabulary-slice views read in place through their strides, the lengths a
    GPU tensor too (the bigram table stays a host array).  The large-C,
    double, bigram and global-state stream builds; compared after every push."""
    (T, C, W, P), dtype, scorer, env, flags, row = FAMILIES[name]
    _set_helper(monkeypatch, env)
    rng = np.random.default_rng(zlib.crc32(("dev/" + name).encode()))
    B = 3
    x = _inputs(rng, "ties", T, B, C, NP[dtype])
    sl = np.array([T, T - 3, T // 2], np.int32)
    kw = _kw("ties", C)
    tab = (-np.abs(rng.standard_normal((C + 1, C))) * 2).astype(NP[dtype]) if scorer == "bigram" else None
    big = torch.zeros((B, T, C + 5), dtype=torch.float32 if dtype == "f32" else torch.float64, device="cuda:0")
    xv = big[:, :, 3:3 + C]
    xv.copy_(torch.as_tensor(np.ascontiguousarray(x.transpose(1, 0, 2))))
    assert not xv.is_contiguous()
    with ctcext_amd.StreamDecoder(B, C, W, P, T, dtype=NP[dtype], scorer_table=tab, flags=flags, device="cuda:0",
                                  **kw) as s:
        t0 = 0
        for n in (1, 2, 4, None):
            t1 = T if n is None else t0 + n
            ln = torch.as_tensor(np.minimum(sl, t1) - np.minimum(sl, t0), dtype=torch.int32, device="cuda:0")
            out = s.push(xv[:, t0:t1], ln)
            k = s.last_stats["kernel"]
            assert k["launched"] and k["stream"] and _stat_row(k) == row, (name, t1, k)
            assert s.on_device and out.log_probability.is_cuda
            compare(out, _oracle_prefix(x, sl, t1, W, P, kw, tab), P, lp_exact=True)
            t0 = t1
        assert s.frames.tolist() == sl.tolist()


@pytest.mark.parametrize("name", ["sq_small", "sq_big"])
def test_one_push_is_one_shot(name, monkeypatch):
    """2. A single push of the whole tensor."""
    (T, C, W, P), dtype, scorer, env, flags, row = FAMILIES[name]
    _set_helper(monkeypatch, env)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    x = _inputs(rng, "normal", T, 3, C)
    sl = np.array([T, T - 3, T // 2], np.int32)
    kw = _kw("normal", C)
    with ctcext_amd.StreamDecoder(3, C, W, P, T, **kw) as s:
        out = s.push(x, sl, batch_first=False)
        assert _stat_row(s.last_stats["kernel"]) == row and s.last_stats["kernel"]["stream"]
    compare(out, oracle.decode(x, sl, W, P, **kw), P, lp_exact=True)


# 3. -inf logits: the seed is chosen so that the one-shot decode of these
# inputs meets duplicate entries and literal frames (asserted below on the
# one-shot call: a condition on the inputs, not on the stream)
NEG_INF_SEED = 116   # (the only seed below 200 that does: one duplicate frame, nine literal ones)


@pytest.mark.parametrize("flags", [0, LITERAL], ids=["fast", "force_literal"])
def test_state_crosses_every_boundary(flags, monkeypatch):
    """One frame per push over inputs whose beam holds entries twice and takes
    literal frames: the duplicate flag, the aliases and the counters travel in
    the saved state."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, C, W, P, B = 12, 6, 8, 3, 3
    rng = np.random.default_rng(NEG_INF_SEED)
    x = _inputs(rng, "neg_inf", T, B, C)
    sl = np.array([T, T - 3, T // 2], np.int32)
    kw = dict(merge_repeated=True, blank_index=0)
    ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, **kw)
    one = ctcext_amd.get_decoder(0).last_stats
    assert one["duplicate_frames"] > 0 and one["literal_frames"] > 0, one
    with ctcext_amd.StreamDecoder(B, C, W, P, T, flags=flags, **kw) as s:
        for t1, chunk, ln in _aligned_chunks(x, sl, (1,) * T):
            out = s.push(chunk, ln, batch_first=False)
            compare(out, _oracle_prefix(x, sl, t1, W, P, kw), P, lp_exact=True)
        if not flags:   # the counters after the last push are the one-shot call's
            for key in ("duplicate_frames", "literal_frames", "literal_nonfinite", "literal_fill"):
                assert s.last_stats[key] == one[key], key


class _Ragged:
    """Items with utterances of their own: push() hands item b its next n_b
    frames (in a chunk as long as the longest), ref() is the oracle over what
    each item has been given so far."""

    def __init__(self, utts, W, P, kw):
        self.utts, self.W, self.P, self.kw = utts, W, P, kw
        self.B, self.C = len(utts), utts[0].shape[1]
        self.at = [0] * self.B          # next frame of each utterance
        self.start = [0] * self.B       # where the item's current utterance began (reset)

    def chunk(self, n, chunk_time=None):
        t = max(n) if chunk_time is None else chunk_time
        c = np.zeros((self.B, t, self.C), np.float32)
        for b in range(self.B):
            c[b, :n[b]] = self.utts[b][self.at[b]:self.at[b] + n[b]]
            self.at[b] += n[b]
        return c

    def frames(self):
        return [a - s for a, s in zip(self.at, self.start)]

    def reset(self, b):
        self.start[b] = self.at[b]

    def ref(self):
        fr = self.frames()
        x = np.zeros((max(max(fr), 1), self.B, self.C), np.float32)
        for b in range(self.B):
            x[:fr[b], b] = self.utts[b][self.start[b]:self.at[b]]
        return oracle.decode(x, np.array(fr, np.int32), self.W, self.P, **self.kw)


def _utts(rng, B, T, C):
    return [_inputs(rng, "normal", T, 1, C)[:, 0] for _ in range(B)]


def test_ragged_chunks(monkeypatch):
    """4. An item without frames in a middle chunk and in the last one, a push
    of no frames at all, lengths=None: compared after every push."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    C, W, P = 6, 8, 3
    kw = dict(merge_repeated=True, blank_index=1)
    r = _Ragged(_utts(np.random.default_rng(11), 3, 16, C), W, P, kw)
    with ctcext_amd.StreamDecoder(3, C, W, P, 16, **kw) as s:
        for n, ct in (([2, 2, 2], None), ([3, 0, 1], None), ([0, 0, 0], 0), ([1, 2, 0], 4), ([2, 2, 2], None),
                      ([4, 1, 0], None)):
            c = r.chunk(n, ct)
            out = s.push(c, None if n == [2, 2, 2] else n)
            assert s.frames.tolist() == r.frames()
            compare(out, r.ref(), P, lp_exact=True)


def test_item_without_any_frame_and_batch_of_one(monkeypatch):
    """4. An item that never gets a frame still reports its (empty) hypothesis;
    B = 1."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    C, W, P = 6, 8, 1
    kw = dict(merge_repeated=False, blank_index=0)
    r = _Ragged(_utts(np.random.default_rng(12), 3, 8, C), W, P, kw)
    with ctcext_amd.StreamDecoder(3, C, W, P, 8, **kw) as s:
        for n in ([2, 0, 1], [1, 0, 0], [3, 0, 2]):
            out = s.push(r.chunk(n), n)
            compare(out, r.ref(), P, lp_exact=True)
        assert s.frames.tolist() == [6, 0, 3]
    r1 = _Ragged(_utts(np.random.default_rng(13), 1, 9, C), W, 3, kw)
    with ctcext_amd.StreamDecoder(1, C, W, 3, 9, **kw) as s:
        for n in ([2], [0], [4], [3]):
            out = s.push(r1.chunk(n, max(n[0], 1)), n)
            compare(out, r1.ref(), 3, lp_exact=True)


def test_too_few_leaves_counts_as_pushed(monkeypatch):
    """5. After one frame of three classes the beam has fewer leaves than the
    four paths asked for: the reference's error, as for the one-shot decode of
    that prefix; the chunk is pushed all the same and the stream goes on."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, C, W, P, B = 4, 3, 8, 4, 3
    x = _inputs(np.random.default_rng(5), "normal", T, B, C)
    sl = np.full((B,), T, np.int32)
    kw = dict(merge_repeated=False, blank_index=0)
    ref, err = oracle_or_error(x[:1], np.minimum(sl, 1), W, P, kw)
    assert ref is None and err == M_LEAVES
    with ctcext_amd.StreamDecoder(B, C, W, P, T, **kw) as s:
        with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
            s.push(x[:1], batch_first=False)
        assert e.value.message == M_LEAVES
        assert s.frames.tolist() == [1, 1, 1]
        out = s.push(x[1:2], batch_first=False)
        compare(out, _oracle_prefix(x, sl, 2, W, P, kw), P, lp_exact=True)
        out = s.push(x[2:], batch_first=False)
        compare(out, oracle.decode(x, sl, W, P, **kw), P, lp_exact=True)


def test_input_formats(monkeypatch):
    """6. bfloat16 batch-major vocabulary-slice views on the GPU, float16 numpy
    on the host: the final result is decode_logits' of the whole tensor and
    the oracle's of its float widening."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    B, T, C, W, P = 3, 14, 20, 100, 5
    sl = np.array([T, T - 3, T // 2], np.int32)
    kw = dict(merge_repeated=True, blank_index=2)
    g = torch.Generator().manual_seed(7)
    big = torch.randn(B, T, C + 11, generator=g).to(torch.bfloat16).cuda()
    xv = big[:, :, 4:4 + C]
    assert not xv.is_contiguous()
    xt = xv.float().cpu().numpy().transpose(1, 0, 2)   # [T, B, C] float32
    with ctcext_amd.StreamDecoder(B, C, W, P, T, **kw) as s:
        for t0, t1 in ((0, 1), (1, 6), (6, T)):
            ln = np.minimum(sl, t1) - np.minimum(sl, t0)
            out = s.push(xv[:, t0:t1], torch.as_tensor(ln.astype(np.int32)).cuda())
        assert s.last_stats["kernel"]["stream"]
    assert out.log_probability.is_cuda and out.log_probability.dtype == torch.float32
    compare(out, ctcext_amd.decode_logits(xv, sl, W, P, outputs="host", **kw), P, lp_exact=True)
    compare(out, oracle.decode(np.ascontiguousarray(xt), sl, W, P, **kw), P, lp_exact=True)

    h = np.random.default_rng(8).standard_normal((B, T, C)).astype(np.float16)
    ht = np.ascontiguousarray(h.astype(np.float32).transpose(1, 0, 2))
    with ctcext_amd.StreamDecoder(B, C, W, P, T, **kw) as s:
        for t0, t1 in ((0, 3), (3, 4), (4, T)):
            out = s.push(h[:, t0:t1], np.minimum(sl, t1) - np.minimum(sl, t0))
    assert isinstance(out.log_probability, np.ndarray) and out.log_probability.dtype == np.float32
    compare(out, ctcext_amd.decode_logits(h, sl, W, P, **kw), P, lp_exact=True)
    compare(out, oracle.decode(ht, sl, W, P, **kw), P, lp_exact=True)


def test_reset_one_item(monkeypatch):
    """7. Item 1 starts a new utterance mid-stream while items 0 and 2 go on:
    each item equals the oracle of its own frames."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    C, W, P = 20, 100, 5
    kw = dict(merge_repeated=False, blank_index=0)
    r = _Ragged(_utts(np.random.default_rng(21), 3, 24, C), W, P, kw)
    with ctcext_amd.StreamDecoder(3, C, W, P, 16, **kw) as s:
        for n in ([3, 3, 3], [4, 5, 2]):
            compare(s.push(r.chunk(n), n), r.ref(), P, lp_exact=True)
        s.reset([1])
        r.reset(1)
        assert s.frames.tolist() == r.frames() == [7, 0, 5]
        for n in ([2, 3, 2], [3, 5, 0], [1, 1, 1]):
            compare(s.push(r.chunk(n), n), r.ref(), P, lp_exact=True)
        assert s.frames.tolist() == [13, 9, 8]
        s.reset()
        for b in range(3):
            r.reset(b)
        compare(s.push(r.chunk([2, 2, 2])), r.ref(), P, lp_exact=True)


def test_two_streams_on_one_decoder(monkeypatch):
    """7. Two streams interleaved on one decoder are independent; only the
    fetch state is the decoder's."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    kw = dict(merge_repeated=True, blank_index=0)
    ra = _Ragged(_utts(np.random.default_rng(31), 3, 12, 20), 100, 5, kw)
    rb = _Ragged(_utts(np.random.default_rng(32), 3, 12, 6), 8, 3, kw)
    with ctcext_amd.StreamDecoder(3, 20, 100, 5, 12, **kw) as sa, ctcext_amd.StreamDecoder(3, 6, 8, 3, 12, **kw) as sb:
        for na, nb in (([1, 1, 1], [2, 2, 1]), ([4, 3, 2], [1, 0, 3]), ([3, 3, 3], [5, 5, 5])):
            oa = sa.push(ra.chunk(na), na)
            # (a one-shot decode on the same decoder in between leaves both streams alone)
            xo = _inputs(np.random.default_rng(33), "normal", 7, 2, 9)
            compare(ctcext_amd.ctc_ext_beam_search_decoder(xo, [7, 4], 16, 2), oracle.decode(xo, [7, 4], 16, 2), 2)
            ob = sb.push(rb.chunk(nb), nb)
            compare(oa, ra.ref(), 5, lp_exact=True)
            compare(ob, rb.ref(), 3, lp_exact=True)
        assert sa.dec is sb.dec


def test_multi_device_handle_is_unimplemented():
    """One device per stream: a sharded handle (the same device twice) answers
    CTCEXT_UNIMPLEMENTED at open."""
    import ctypes
    dec = ctcext_amd.Decoder((0, 0))
    try:
        a = _lib.StreamArgs()
        a.dtype, a.on_device = _lib.CTCEXT_F32, 1
        a.batch_size, a.num_classes, a.max_frames = 3, 6, 8
        a.beam_width, a.top_paths, a.blank_label = 8, 2, -1
        h = ctypes.c_void_p()
        rc = dec.lib.ctcext_stream_open(dec.handle, ctypes.byref(a), ctypes.byref(h))
        assert rc == _lib.CTCEXT_UNIMPLEMENTED and not h.value
        assert dec.lib.ctcext_last_error().decode() == "a stream needs a one-device decoder handle"
    finally:
        dec.close()


def test_failed_push_leaves_the_stream_intact(monkeypatch):
    """8. A push whose helper wave is dead fails with InternalError and one
    past the capacity with the capacity message; either way the frames are as
    before and the following pushes complete the utterance."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, C, W, P, B = 12, 20, 100, 5, 3
    x = _inputs(np.random.default_rng(41), "normal", T, B, C)
    sl = np.array([T, T - 3, T // 2], np.int32)
    kw = dict(merge_repeated=False, blank_index=0)
    s = ctcext_amd.StreamDecoder(B, C, W, P, T, **kw)
    compare(s.push(x[:4], batch_first=False), _oracle_prefix(x, sl, 4, W, P, kw), P, lp_exact=True)
    assert s.last_stats["kernel"]["helper"] == "SQ"
    with pytest.raises(ctcext_amd.InternalError) as e:
        s.push(x[4:7], batch_first=False, flags=DEAD)
    assert e.value.message == "decode kernel: a helper-wave hand-over wait timed out"
    assert s.frames.tolist() == [4, 4, 4]
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        s.push(np.zeros((T - 3, B, C), np.float32), batch_first=False)
    assert e.value.message == "stream capacity exceeded: item 0 would hold %d frames of max_frames %d" % (T + 1, T)
    assert s.frames.tolist() == [4, 4, 4]
    for t0, t1 in ((4, 7), (7, T)):
        ln = np.minimum(sl, t1) - np.minimum(sl, t0)
        out = s.push(x[t0:t1], ln, batch_first=False)
        compare(out, _oracle_prefix(x, sl, t1, W, P, kw), P, lp_exact=True)
    assert s.frames.tolist() == sl.tolist()
    s.close()
    with pytest.raises(ctcext_amd.OpError):
        s.push(x[:1], batch_first=False)
    with pytest.raises(ctcext_amd.OpError):
        s.frames
