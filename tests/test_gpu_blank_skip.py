"""Blank-frame skipping on the GPU (skip_blank= of ctc_ext_beam_search_decoder,
decode_logits and decode_dense; ctcext_decode_skip / ctcext_decode_dense_skip):
exact equality of every output with the definition of include/ctcext.h,
restated in skip_util over the CPU oracle -- the oracle's decode of the kept
frames, with the alignment put back on the original time axis."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import ctcext_amd
import oracle
import skip_util as su
from ctcext_amd import _lib, ops
from parity_util import compare
from token_times_util import expected_from_rows, family

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MSG = "blank skip threshold must be a log-probability (<= 0)"
FEW, LENGTH = _lib.CTCEXT_ITEM_FEW_LEAVES, _lib.CTCEXT_ITEM_LENGTH
PAD = -7


def _i32(v):
    return torch.as_tensor(np.asarray(v, np.int32), device=DEV)


def _host(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in ts]


def _assert_dense(out, e, B, P, T, items=None, status=0, pad=PAD):
    """out (DenseDecode) equals the definition bit for bit on `items` (all), whose status is `status`."""
    got = _host(out)
    sel = slice(None) if items is None else list(items)
    for name, g, w in zip(ctcext_amd.DenseDecode._fields, got[:5], su.to_dense(e, B, P, T, pad)):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g[sel], w[sel], err_msg=name)
    np.testing.assert_array_equal(got[5][sel], status, err_msg="status")


def _assert_times(tt, e, sl, B, P, T, kw, what=""):
    """Token times after a skipping call: the definition on the expanded rows, with the original lengths."""
    want = expected_from_rows(e.dec, e.ali, np.maximum(sl, 0), B, P, T, kw.get("blank_label", -1),
                              bool(kw.get("merge_repeated", False)))
    for name, g, w in zip(ctcext_amd.TokenTimes._fields, _host(tt), want):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, name))


def _check(x, sl, W, P, thr, e, kw, x_dev=None, batch_first=False, sync=True, scorer_table=None, what=""):
    """x / sl through decode_logits (all seven outputs, kept_frames, token_times)
    and through decode_dense (all dense tensors, status, kept_frames,
    dense_token_times) against e.  x_dev: the tensor the calls get (x itself)."""
    T, B, C = x.shape
    xd = torch.as_tensor(x, device=DEV) if x_dev is None else x_dev
    tab = None if scorer_table is None else torch.as_tensor(scorer_table, device=DEV)
    if sync:
        out = ctcext_amd.decode_logits(xd, _i32(sl), W, P, batch_first=batch_first, skip_blank=thr, scorer_table=tab, **kw)
        compare(out, e.sparse, P)
        kept = ctcext_amd.kept_frames()
        assert isinstance(kept, np.ndarray) and kept.dtype == np.int32 and kept.tolist() == e.kept.tolist(), what
        _assert_times(ctcext_amd.token_times(), e, sl, B, P, T, kw, what + " token_times")
    dense = ctcext_amd.decode_dense(xd, _i32(sl), W, P, batch_first=batch_first, skip_blank=thr, pad_value=PAD,
                                    scorer_table=tab, **kw)
    kept = ctcext_amd.kept_frames()
    assert torch.is_tensor(kept) and kept.is_cuda and kept.dtype == torch.int32
    tt = ctcext_amd.dense_token_times()
    _assert_dense(dense, e, B, P, T)
    assert _host([kept])[0].tolist() == e.kept.tolist(), what
    _assert_times(tt, e, sl, B, P, T, kw, what + " dense_token_times")
    return ctcext_amd.dense_check()


# ---- 1. the families

SHAPES = [(12, 6, 5, 8, 3), (40, 4, 29, 16, 3), (60, 3, 29, 128, 3)]
# log 0.9 with and without merge_repeated; and the median of the case's blank
# log-probabilities, at which the sticky and Gaussian rows drop frames too
# (at log 0.9 most of them drop none: tests/test_cpu_blank_skip.py counts them)
FAMILY_CASES = ([(k, s, m, su.THR) for k in ("peaky", "sticky", "gaussian") for s in SHAPES for m in (False, True)]
                + [(k, s, True, "median") for k in ("peaky", "sticky", "gaussian") for s in SHAPES])
NOTHING_DROPPED = {("gaussian", s) for s in SHAPES} | {("sticky", s) for s in SHAPES[1:]}


@functools.lru_cache(maxsize=None)
def _family_case(kind, shape, merge, thr, dtype="float32"):
    T, B, C, W, P = shape
    x = family(np.random.default_rng(sum(kind.encode()) + T), kind, T, B, C, np.dtype(dtype))
    x.setflags(write=False)
    sl = su.lengths(T, B)
    if thr == "median":
        thr = su.median_threshold(x, sl)
    kw = dict(merge_repeated=merge, blank_index=0, blank_label=-1)
    return x, sl, thr, kw, su.expected(x, sl, W, P, thr, **kw)


@pytest.mark.parametrize("kind,shape,merge,thr", FAMILY_CASES,
                         ids=["%s-%s-%s-%s" % (k, "x".join(map(str, s)), "merge" if m else "plain",
                                               t if t == "median" else "log0.9") for k, s, m, t in FAMILY_CASES])
def test_families_match_the_definition(kind, shape, merge, thr, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = shape
    named = thr
    x, sl, thr, kw, e = _family_case(kind, shape, merge, thr)
    dropped = int(sl.sum() - e.kept.sum())
    if named != "median" and (kind, shape) in NOTHING_DROPPED:
        assert dropped == 0
    else:
        assert dropped >= 1
    if kind == "peaky" and named != "median":
        assert su.dropped_share(e, sl) >= 0.25
    if (kind, shape, named) == ("peaky", SHAPES[0], su.THR):
        assert sl[0] == 12 and e.kept[0] == 1   # an item that keeps exactly 1 of its 12 frames
    st = _check(np.array(x), sl, W, P, thr, e, kw, what="%s %s" % (kind, shape))
    assert st["kernel"]["launched"], st


# ---- 2. long rows, large C, dtypes, layouts

@pytest.mark.parametrize("empty_item", [False, True], ids=["all_live", "one_item_of_length_0"])
def test_rows_longer_than_the_kernel_tiles(empty_item, monkeypatch):
    """T = 700: the plan's flag and count carries and the expansion's tiles
    cross several tiles of 256, in the items and in the kept rows (381, 377 and
    364 frames).  An item of length 0 has fewer leaves than top_paths: it is
    left out of the oracle's batch and its status says so."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 700, 3, 5, 8, 3
    x = family(np.random.default_rng(sum(b"peaky") + T), "peaky", T, B, C)
    sl = su.lengths(T, B)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    if not empty_item:
        e = su.expected(x, sl, W, P, su.THR, **kw)
        assert e.kept.tolist() == [381, 377, 364] and su.dropped_share(e, sl) >= 0.25
        _check(x, sl, W, P, su.THR, e, kw, what="T = 700")
        return
    sl[2] = 0
    live = [0, 1]
    e = su.expected(x[:, live], sl[live], W, P, su.THR, **kw)
    assert e.kept.tolist() == [381, 377]
    out = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), _i32(sl), W, P, batch_first=False, skip_blank=su.THR,
                                  pad_value=PAD, **kw)
    kept = ctcext_amd.kept_frames()
    tt = ctcext_amd.dense_token_times()
    got = _host(out)
    for name, g, w in zip(ctcext_amd.DenseDecode._fields, got[:5], su.to_dense(e, 2, P, T, PAD)):
        np.testing.assert_array_equal(g[live], w, err_msg=name)
    assert got[5].tolist() == [0, 0, FEW] and _host([kept])[0].tolist() == [381, 377, 0]
    assert (got[1][2] == 0).all() and (got[3][2] == 0).all() and (got[2][2] == PAD).all()
    want = expected_from_rows(e.dec, e.ali, sl[live], 2, P, T, -1, True)
    for g, w in zip(_host(tt), want):
        np.testing.assert_array_equal(g[live], w)
    with pytest.raises(ctcext_amd.InvalidArgumentError):
        ctcext_amd.dense_check()


def test_more_than_64_classes(monkeypatch):
    """C = 100: the normaliser without a pre-pass record in front of the plan,
    the large-C pre-pass and kernels behind it."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 300, 2, 100, 16, 2
    x = family(np.random.default_rng(sum(b"peaky") + T), "peaky", T, B, C)
    sl = su.lengths(T, B)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    e = su.expected(x, sl, W, P, su.THR, **kw)
    assert e.kept.tolist() == [207, 211] and su.dropped_share(e, sl) >= 0.25
    st = _check(x, sl, W, P, su.THR, e, kw, what="C = 100")
    assert st["kernel"]["BIG"] and st["kernel"]["prepass"] not in ("none", "norm_only"), st


def test_float64(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (40, 4, 29, 16, 3)
    T, B, C, W, P = shape
    x, sl, thr, kw, e = _family_case("peaky", shape, True, su.THR, "float64")
    assert e.log_prob.dtype == np.float64 and sl.sum() - e.kept.sum() >= 1
    _check(np.array(x), sl, W, P, thr, e, kw, what="float64")
    assert ctcext_amd.get_decoder(0).last_stats["kernel"]["dtype"] == "f64"


@pytest.mark.parametrize("C", [29, 32], ids=["rows_of_single_elements", "rows_of_16_byte_pieces"])
@pytest.mark.parametrize("half", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_half_inputs_stay_two_bytes(half, C, monkeypatch):
    """bf16 / f16 logits, read in place and gathered as 2-byte elements (C = 29)
    or 16-byte pieces (C = 32); the definition runs on the widened values."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, W, P = 40, 4, 16, 3
    xh = torch.as_tensor(family(np.random.default_rng(77 + C), "peaky", T, B, C), device=DEV).to(half)
    x = xh.float().cpu().numpy()
    sl = su.lengths(T, B)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    e = su.expected(x, sl, W, P, su.THR, **kw)
    assert su.dropped_share(e, sl) >= 0.25
    _check(x, sl, W, P, su.THR, e, kw, x_dev=xh, what=str(half))


@pytest.mark.parametrize("C", [29, 32, 6], ids=["f32_elements", "f32_pieces", "f64_pieces"])
def test_float_rows_of_pieces_and_elements(C, monkeypatch):
    """float32 rows of 16-byte pieces (C = 32) and of single elements (C = 29); float64 pieces (C = 6)."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, W, P = 40, 4, 16, 3
    x = family(np.random.default_rng(78 + C), "peaky", T, B, C, np.float64 if C == 6 else np.float32)
    sl = su.lengths(T, B)
    kw = dict(merge_repeated=False, blank_index=0, blank_label=-1)
    e = su.expected(x, sl, W, P, su.THR, **kw)
    assert su.dropped_share(e, sl) >= 0.25
    _check(x, sl, W, P, su.THR, e, kw, what="C = %d" % C)


def test_batch_major_tensor_and_vocabulary_slice_in_place(monkeypatch):
    """A batch-major [B, T, C] tensor, and a bf16 vocabulary slice with gaps in
    both dimensions (rows that start off 16-byte boundaries), read in place."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 4, 29, 16, 3
    x = family(np.random.default_rng(81), "peaky", T, B, C)
    sl = su.lengths(T, B)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    e = su.expected(x, sl, W, P, su.THR, **kw)
    assert su.dropped_share(e, sl) >= 0.25
    bm = torch.as_tensor(x, device=DEV).transpose(0, 1).contiguous()   # [B, T, C]
    _check(x, sl, W, P, su.THR, e, kw, x_dev=bm, batch_first=True, what="batch-major")
    full = torch.zeros((B, T, C + 6), device=DEV, dtype=torch.bfloat16)
    full[:, :, 3:3 + C] = bm.to(torch.bfloat16)
    view = full[:, :, 3:3 + C]
    assert not view.is_contiguous()
    xs = view.float().transpose(0, 1).contiguous().cpu().numpy()
    es = su.expected(xs, sl, W, P, su.THR, **kw)
    assert su.dropped_share(es, sl) >= 0.25
    _check(xs, sl, W, P, su.THR, es, kw, x_dev=view, batch_first=True, what="vocabulary slice")


def test_host_inputs(monkeypatch):
    """numpy logits: staged on the device, kept counts and outputs come back as numpy."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (40, 4, 29, 16, 3)
    T, B, C, W, P = shape
    x, sl, thr, kw, e = _family_case("peaky", shape, True, su.THR)
    out = ctcext_amd.ctc_ext_beam_search_decoder(np.array(x), sl, W, P, skip_blank=thr, **kw)
    assert isinstance(out.log_probability, np.ndarray)
    compare(out, e.sparse, P)
    assert ctcext_amd.kept_frames().tolist() == e.kept.tolist()
    tt = ctcext_amd.token_times()
    assert isinstance(tt.start, np.ndarray)
    _assert_times(tt, e, sl, B, P, T, kw, "host")
    # batch-major numpy, through its strides
    out = ctcext_amd.decode_logits(np.ascontiguousarray(np.array(x).transpose(1, 0, 2)), sl, W, P, skip_blank=thr, **kw)
    compare(out, e.sparse, P)


def test_blank_index_2_with_blank_label_7(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 4, 5, 8, 3
    x = family(np.random.default_rng(83), "peaky", T, B, C, blank=2)
    sl = su.lengths(T, B)
    kw = dict(merge_repeated=True, blank_index=2, blank_label=7)
    e = su.expected(x, sl, W, P, su.THR, **kw)
    assert su.dropped_share(e, sl) >= 0.25
    assert any(7 in e.ali[b][p] for b in range(B) for p in range(P))
    # (the plan reads class 2: with class 0 as the blank it keeps other frames)
    assert su.plan(x, sl, su.THR, 0) != e.kmaps
    _check(x, sl, W, P, su.THR, e, kw, what="blank 2 / 7")


def test_bigram_scorer_table(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 4, 29, 16, 3
    rng = np.random.default_rng(84)
    x = family(rng, "peaky", T, B, C)
    tab = (-np.abs(rng.standard_normal((C + 1, C))) * 2).astype(np.float32)
    sl = su.lengths(T, B)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    e = su.expected(x, sl, W, P, su.THR, scorer_table=tab, **kw)
    assert su.dropped_share(e, sl) >= 0.25
    st = _check(x, sl, W, P, su.THR, e, kw, scorer_table=tab, what="bigram")
    assert st["kernel"]["scorer"] == "bigram", st


# ---- 3. thresholds and rows the rule keeps

def test_threshold_0_is_the_plain_call_bit_for_bit(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (40, 4, 29, 16, 3)
    T, B, C, W, P = shape
    x, sl, _, kw, _ = _family_case("peaky", shape, True, su.THR)
    xd, sld = torch.as_tensor(np.array(x), device=DEV), _i32(sl)
    plain = ctcext_amd.decode_logits(xd, sld, W, P, batch_first=False, **kw)
    with pytest.raises(ctcext_amd.FailedPreconditionError):
        ctcext_amd.kept_frames()   # the plain call keeps no counts
    skip = ctcext_amd.decode_logits(xd, sld, W, P, batch_first=False, skip_blank=0.0, **kw)
    assert ctcext_amd.kept_frames().tolist() == sl.tolist()
    compare(skip, ops.CTCExtBeamSearchDecoder(*[[t.cpu().numpy() for t in f] if isinstance(f, list) else f.cpu().numpy()
                                                for f in plain]), P)
    dp = ctcext_amd.decode_dense(xd, sld, W, P, batch_first=False, **kw)
    ds = ctcext_amd.decode_dense(xd, sld, W, P, batch_first=False, skip_blank=0.0, **kw)
    for name, a, b in zip(ctcext_amd.DenseDecode._fields, _host(dp), _host(ds)):
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert _host([ctcext_amd.kept_frames()])[0].tolist() == sl.tolist()
    ctcext_amd.dense_check()


def test_threshold_above_0_raises_before_any_launch(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    x = torch.zeros((4, 1, 3), device=DEV)
    torch.cuda.synchronize()

    def launched(*a, **k):
        raise AssertionError("the call went on to the library's decode")

    dec = ctcext_amd.get_decoder(0)
    for thr in (1e-6, float("nan")):
        with monkeypatch.context() as m:
            m.setattr(dec, "decode", launched)
            for f in (lambda: ctcext_amd.decode_logits(x, [4], 2, 1, batch_first=False, skip_blank=thr),
                      lambda: ctcext_amd.ctc_ext_beam_search_decoder(x, [4], 2, 1, skip_blank=thr),
                      lambda: ctcext_amd.decode_dense(x, [4], 2, 1, batch_first=False, skip_blank=thr)):
                with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
                    f()
                assert e.value.message == MSG and e.value.error_code == _lib.CTCEXT_INVALID_ARGUMENT
    # ... and behind the C ABI itself
    k = _lib.SkipArgs()
    k.logp_threshold = 0.5
    a = ops._args(x.data_ptr(), (4, 1, 3), _lib.CTCEXT_F32, True, _i32([4]).data_ptr(), (1,), 2, 1, False, 0, -1, 0, None)
    sizes = (_lib.PathSizes * 1)()
    assert dec.lib.ctcext_decode_skip(dec.handle, ctypes.byref(a), ctypes.byref(k), sizes) == _lib.CTCEXT_INVALID_ARGUMENT
    assert dec.lib.ctcext_last_error().decode() == MSG
    assert dec.lib.ctcext_dense_reserve_skip(dec.handle, ctypes.byref(a), ctypes.byref(k)) == _lib.CTCEXT_INVALID_ARGUMENT


def test_nan_row_and_minus_inf_blank_are_kept(monkeypatch):
    """Inside runs of blank-dominant frames: a row of NaN, and a row whose blank
    is -inf.  A comparison with NaN is false, so both stay and end their runs."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 24, 2, 5, 8, 2
    x = np.random.default_rng(85).standard_normal((T, B, C)).astype(np.float32)
    x[:, :, 0] += 9   # every frame blank-dominant
    x[7, 0, :] = np.nan
    x[15, 1, 0] = -np.inf
    sl = np.array([T, T - 1], np.int32)
    kw = dict(merge_repeated=False, blank_index=0, blank_label=-1)
    e = su.expected(x, sl, W, P, su.THR, **kw)
    assert e.kmaps == [[0, 7, 8], [0, 15, 16]]
    _check(x, sl, W, P, su.THR, e, kw, what="NaN / -inf")


# ---- 4. the dense form only enqueues; graph capture

@functools.lru_cache(maxsize=None)
def _async_case():
    T, B, C, W, P = 600, 2, 29, 128, 3
    x = family(np.random.default_rng(600), "peaky", T, B, C)
    sl = np.array([T, T - 50], np.int32)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    return (T, B, C, W, P), x, sl, kw, su.expected(x, sl, W, P, su.THR, **kw)


@pytest.mark.parametrize("where", ["default_stream", "side_stream"])
def test_dense_call_only_enqueues(where, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    (T, B, C, W, P), x, sl, kw, e = _async_case()
    xd, sld = torch.as_tensor(x, device=DEV), _i32(sl)
    stream = torch.cuda.Stream(device=DEV) if where == "side_stream" else torch.cuda.default_stream(DEV)

    def blocked(*a, **k):
        raise AssertionError("decode_dense(skip_blank=) reached a host synchronisation")

    with torch.cuda.stream(stream):
        ctcext_amd.decode_dense(xd, sld, W, P, batch_first=False, skip_blank=su.THR, **kw)   # warm-up: workspace, kernels
        ctcext_amd.dense_token_times()
        torch.cuda.synchronize()
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "synchronize", blocked)
            m.setattr(torch.cuda.Stream, "synchronize", blocked)
            m.setattr(torch.Tensor, "cpu", blocked)
            m.setattr(torch.Tensor, "item", blocked)
            out = ctcext_amd.decode_dense(xd, sld, W, P, batch_first=False, skip_blank=su.THR, pad_value=PAD, **kw)
            kept = ctcext_amd.kept_frames()
            tt = ctcext_amd.dense_token_times()
        ev = torch.cuda.Event()
        ev.record()
        done_at_return = ev.query()
        ev.synchronize()
    assert not done_at_return, "the work had finished when the calls returned: they did not only enqueue"
    _assert_dense(out, e, B, P, T)
    assert _host([kept])[0].tolist() == e.kept.tolist()
    _assert_times(tt, e, sl, B, P, T, kw, where)
    ctcext_amd.dense_check()


def test_graph_capture_and_replay(monkeypatch):
    """decode_dense(skip_blank=) and dense_token_times captured into one graph
    on a side stream and replayed on new logits and lengths; the workspace of
    the captured shape comes from ctcext_dense_reserve_skip alone, so a call
    that allocated from HIP, freed or blocked would fail the capture."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 3, 20, 100, 3
    rng = np.random.default_rng(406)
    side = torch.cuda.Stream(device=DEV)
    kw = dict(batch_first=False, merge_repeated=True, pad_value=PAD, skip_blank=su.THR)
    with torch.cuda.stream(side):
        ctcext_amd.decode_dense(torch.zeros((4, 1, C), device=DEV), torch.full((1,), 4, dtype=torch.int32, device=DEV),
                                W, P, **kw)
        ctcext_amd.dense_token_times()   # loads the kernels
    side.synchronize()
    xs = torch.zeros((T, B, C), device=DEV)
    sls = torch.zeros((B,), dtype=torch.int32, device=DEV)
    dec = ctcext_amd.get_decoder(0)
    a = ops._args(xs.data_ptr(), (T, B, C), _lib.CTCEXT_F32, True, sls.data_ptr(), (B,), W, P, True, 0, -1, 0, None)
    k = _lib.SkipArgs()
    k.logp_threshold = su.THR
    assert dec.lib.ctcext_dense_reserve_skip(dec.handle, ctypes.byref(a), ctypes.byref(k)) == _lib.CTCEXT_OK
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = ctcext_amd.decode_dense(xs, sls, W, P, **kw)
        kept = ctcext_amd.kept_frames()
        tt = ctcext_amd.dense_token_times()
    okw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    for sl in ([T, T - 7, 9], [11, T, T - 1]):
        x = family(rng, "peaky", T, B, C)
        sl = np.asarray(sl, np.int32)
        xs.copy_(torch.as_tensor(x))
        sls.copy_(torch.as_tensor(sl))
        torch.cuda.synchronize()
        g.replay()
        e = su.expected(x, sl, W, P, su.THR, **okw)
        assert su.dropped_share(e, sl) >= 0.25
        _assert_dense(out, e, B, P, T)
        assert _host([kept])[0].tolist() == e.kept.tolist()
        _assert_times(tt, e, sl, B, P, T, okw, "replay %s" % (sl,))
        assert ctcext_amd.dense_check()["records_written"] > 0


# ---- 5. status, handles, the re-decode

def test_item_with_a_length_error_leaves_the_others_untouched(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (12, 6, 5, 8, 3)
    T, B, C, W, P = shape
    x, sl, thr, kw, e = _family_case("peaky", shape, False, su.THR)
    bad = np.array(sl)
    bad[1] = T + 1
    others = [0, 2, 3, 4, 5]
    out = ctcext_amd.decode_dense(torch.as_tensor(np.array(x), device=DEV), _i32(bad), W, P, batch_first=False,
                                  skip_blank=thr, pad_value=PAD, **kw)
    kept = ctcext_amd.kept_frames()
    tt = ctcext_amd.dense_token_times()
    _assert_dense(out, e, B, P, T, items=others)
    got = _host(out)
    assert got[5].tolist() == [0, LENGTH, 0, 0, 0, 0]
    assert (got[0][1] == PAD).all() and (got[2][1] == PAD).all() and (got[1][1] == 0).all() and (got[3][1] == 0).all()
    want_kept = e.kept.tolist()
    want_kept[1] = 0
    assert _host([kept])[0].tolist() == want_kept
    want = expected_from_rows(e.dec, e.ali, sl, B, P, T, -1, False)
    for g, w in zip(_host(tt), want):
        np.testing.assert_array_equal(g[others], w[others])
    assert (_host(tt)[0][1] == -1).all()
    with pytest.raises(ctcext_amd.FailedPreconditionError) as err:
        ctcext_amd.dense_check()
    assert err.value.message == "sequence_length(1) <= %d" % T   # (the original max_time)
    # the synchronous call fails as a whole, as it does without skipping
    with pytest.raises(ctcext_amd.FailedPreconditionError) as err:
        ctcext_amd.decode_logits(torch.as_tensor(np.array(x), device=DEV), _i32(bad), W, P, batch_first=False,
                                 skip_blank=thr, **kw)
    assert err.value.message == "sequence_length(1) <= %d" % T


def test_few_leaves_is_judged_on_the_compacted_item(monkeypatch):
    """Four blank-dominant frames compact to one: with three classes that is
    three leaves, fewer than the four paths the four frames themselves give."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 4, 1, 3, 8, 4
    x = np.random.default_rng(86).standard_normal((T, B, C)).astype(np.float32)
    x[:, :, 0] += 9
    ctcext_amd.decode_logits(torch.as_tensor(x, device=DEV), [T], W, P, batch_first=False)   # the plain call decodes
    with pytest.raises(oracle.OracleError, match="Less leaves"):
        su.expected(x, [T], W, P, su.THR)
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.decode_logits(torch.as_tensor(x, device=DEV), [T], W, P, batch_first=False, skip_blank=su.THR)
    assert e.value.message == "Less leaves in the beam search than requested."
    out = ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), [T], W, P, batch_first=False, skip_blank=su.THR)
    assert [v.tolist() for v in _host([out.status, ctcext_amd.kept_frames()])] == [[FEW], [1]]


def test_more_than_one_device_is_unimplemented(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    x = np.random.default_rng(87).standard_normal((10, 2, 5)).astype(np.float32)
    ctcext_amd.ctc_ext_beam_search_decoder(x, [10, 10], 4, 1, devices=[0, 0])   # (without skipping it decodes)
    for xin in (x, torch.as_tensor(x, device=DEV)):
        with pytest.raises(ctcext_amd.UnimplementedError) as e:
            ctcext_amd.ctc_ext_beam_search_decoder(xin, [10, 10], 4, 1, devices=[0, 0], skip_blank=su.THR)
        assert e.value.error_code == _lib.CTCEXT_UNIMPLEMENTED


def test_helper_dead_redecode_keeps_the_compaction(monkeypatch):
    """CTCEXT_FLAG_TEST_HELPER_DEAD: the two-wave kernel's helper starts out
    timed out, the call is decoded again by the one-wave kernels over the same
    kept rows, and the alignments are expanded again."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (60, 3, 29, 128, 3)
    T, B, C, W, P = shape
    x, sl, thr, kw, e = _family_case("peaky", shape, True, su.THR)
    xd = torch.as_tensor(np.array(x), device=DEV)
    with pytest.warns(RuntimeWarning, match="hand-over wait timed out"):
        out = ctcext_amd.decode_logits(xd, _i32(sl), W, P, batch_first=False, skip_blank=thr,
                                       flags=_lib.CTCEXT_FLAG_TEST_HELPER_DEAD, **kw)
    assert ctcext_amd.get_decoder(0).last_stats["helper_redecodes"] == 1
    compare(out, e.sparse, P)
    assert ctcext_amd.kept_frames().tolist() == e.kept.tolist()
    _assert_times(ctcext_amd.token_times(), e, sl, B, P, T, kw, "re-decode")
