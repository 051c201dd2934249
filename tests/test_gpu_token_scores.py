"""Token scores on the GPU (ctcext_dense_token_scores / _fetch_token_scores
behind dense_token_scores and token_scores): NaN mask, then exact equality with
the definition of include/ctcext.h, restated in token_scores_util.token_scores
and applied to the CPU oracle's rows, their token times and the oracle's
normaliser.  Shapes are (T, B, C, W, P)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
import range_inputs
import skip_util
from ctcext_amd import _lib, ops
from test_gpu_dense import ASYNC_SHAPE, _async_case
from token_scores_util import (FAMILY_CASES, SKIP_SHAPE, TILED, expected, expected_from_rows_and_times, family_case,
                               lengths, nan_cells_inside_decoded_length, skip_case, skip_properties, tile_properties,
                               tiled_case)
from token_times_util import expected_from_rows, family

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MSG = "token times need a blank_label that is no class label"
NO_OPT_IN = "token scores need a decode with token_scores=True"


def _host(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in ts]


def _assert_scores(sc, want, items=None, what=""):
    got = _host(sc)
    sel = slice(None) if items is None else list(items)
    for name, g, w in zip(ctcext_amd.TokenScores._fields, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        g, w = g[sel], w[sel]
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg="%s %s: NaN mask" % (what, name))
        np.testing.assert_array_equal(g[~np.isnan(g)], w[~np.isnan(w)], err_msg="%s %s" % (what, name))


def _dense(x, sl, W, P, batch_first=False, **kw):
    """decode_dense with the opt-in, its token times and its scores."""
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), device=DEV)
    out = ctcext_amd.decode_dense(x, torch.as_tensor(np.asarray(sl, np.int32), device=DEV), W, P,
                                  batch_first=batch_first, token_scores=True, **kw)
    tt = ctcext_amd.dense_token_times()
    return out, tt, ctcext_amd.dense_token_scores(tt)


# ---- 1. the dense form over the families

@pytest.mark.parametrize("kind,shape,merge", FAMILY_CASES,
                         ids=["%s-%s-%s" % (k, "x".join(map(str, s)), "merge" if m else "plain") for k, s, m in FAMILY_CASES])
def test_dense_matches_definition(kind, shape, merge, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = shape
    x, sl, kw, (dec, ali, times, want) = family_case(kind, shape, merge)
    if kind == "neg_inf":
        assert nan_cells_inside_decoded_length(dec, want) >= 1   # on the expected values: untimed tokens
    out, tt, sc = _dense(np.array(x), sl, W, P, **kw)
    assert tuple(sc.logp_sum.shape) == (B, P, T) and sc.logp_sum.is_cuda and sc.logp_sum.dtype == torch.float32
    _assert_scores(sc, want, what="%s %s" % (kind, shape))
    assert _host([out.status])[0].tolist() == [0] * B
    ctcext_amd.dense_check()


def test_times_default_to_the_decodes_own(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (12, 6, 5, 8, 3)
    T, B, C, W, P = shape
    x, sl, kw, (dec, ali, times, want) = family_case("peaky", shape, True)
    ctcext_amd.decode_dense(torch.as_tensor(np.array(x), device=DEV), torch.as_tensor(sl, device=DEV), W, P,
                            batch_first=False, token_scores=True, **kw)
    _assert_scores(ctcext_amd.dense_token_scores(), want, what="times=None")


# ---- 2. rows of several tiles; the order of the sum

TILE_CASES = [(TILED[0], False), (TILED[1], False), (TILED[0], True)]


@pytest.mark.parametrize("shape,soft", TILE_CASES,
                         ids=["x".join(map(str, s)) + ("-soft" if f else "") for s, f in TILE_CASES])
def test_rows_longer_than_the_kernel_tile(shape, soft, monkeypatch):
    """Scored spans lie across a multiple of the kernel's tile: the carry of the
    sum and the minimum.  The issue's two sticky cases have sums that are exact
    in float32 whatever the order (token_scores_util.tiled_case says why; 0 of
    their 516 and 242 timed tokens differ), so the soft case is there for the
    order: on it the expected sums of tile-crossing tokens differ from their
    terms added in descending order, and a kernel that adds in another order
    fails."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = shape
    case = tiled_case(shape, soft)
    x, sl, kw, live, dec, ali, times, want = case
    crossing, differ = tile_properties(case, _lib.load().ctcext_token_scores_tile())
    assert crossing >= 1, crossing
    if soft:
        assert differ >= 1, differ
    out, tt, sc = _dense(np.array(x), sl, W, P, **kw)
    _assert_scores(sc, want, what="%s soft=%s" % (shape, soft))
    assert _host([out.status])[0].tolist() == [0 if b in live else _lib.CTCEXT_ITEM_FEW_LEAVES for b in range(B)]


# ---- 3. routes: the large-C pre-pass's normaliser, float64, halves in place, the float range

def test_large_c_normaliser(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 20, 2, 80, 8, 2
    x = family(np.random.default_rng(80), "peaky", T, B, C)
    sl = lengths(T, B)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    want = expected(x, sl, W, P, T, **kw)[3]
    assert (~np.isnan(want[0])).any()
    out, tt, sc = _dense(x, sl, W, P, **kw)
    _assert_scores(sc, want, what="C = 80")


def test_float64(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (12, 6, 5, 8, 3)
    T, B, C, W, P = shape
    x, sl, kw, (dec, ali, times, want) = family_case("gaussian", shape, True, "float64")
    out, tt, sc = _dense(np.array(x), sl, W, P, **kw)
    assert sc.logp_sum.dtype == torch.float64 and sc.logp_min.dtype == torch.float64
    _assert_scores(sc, want, what="float64")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_half_vocabulary_slice_read_in_place(dtype, monkeypatch):
    """A batch-major half view with gaps in both dimensions: the kernel gathers
    from the caller's tensor through the remembered format and strides."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 24, 3, 29, 16, 2
    rng = np.random.default_rng(40)
    full = torch.as_tensor(family(rng, "sticky", T, B, 40).transpose(1, 0, 2).copy(), device=DEV).to(dtype)   # [B, T, 40]
    view = full[:, :, 5:5 + C]
    assert not view.is_contiguous() and view.stride(-1) == 1
    x = view.float().transpose(0, 1).contiguous().cpu().numpy()   # the widened slice, [T, B, C]
    sl = np.array([T, T - 3, T // 2], np.int32)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    want = expected(x, sl, W, P, T, **kw)[3]
    assert (~np.isnan(want[0])).any()
    out, tt, sc = _dense(view, sl, W, P, batch_first=True, **kw)
    assert ctcext_amd.get_decoder(0)._scores_keep.data_ptr() == view.data_ptr()   # nothing was copied
    assert sc.logp_sum.dtype == torch.float32
    _assert_scores(sc, want, what=str(dtype))


@pytest.mark.parametrize("kind", ["edges", "huge"])
def test_float_range(kind, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 12, 3, 5, 8, 2
    x = range_inputs.family(range_inputs.rng_for("token scores " + kind), kind, T, B, C, np.float32)
    range_inputs.assert_census(kind, x)
    sl = np.array([T, T - 1, T - 5], np.int32)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    want = expected(x, sl, W, P, T, **kw)[3]
    out, tt, sc = _dense(x, sl, W, P, **kw)
    _assert_scores(sc, want, what=kind)


# ---- 4. after a skipping decode: the original time axis

def test_after_a_skipping_decode(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = SKIP_SHAPE
    case = skip_case()
    x, sl, kw, e, times, want = case
    spans, fewer, dominant = skip_properties(case)
    assert spans >= 1 and fewer >= 1 and dominant >= 3   # on the expected values: a scored span holds a dropped frame
    assert (e.kept < sl).all()
    out, tt, sc = _dense(np.array(x), sl, W, P, skip_blank=skip_util.THR, **kw)
    np.testing.assert_array_equal(_host([ctcext_amd.kept_frames()])[0], e.kept)
    _assert_scores(sc, want, what="dense, skipping")
    ctcext_amd.dense_check()
    # the synchronous form, host inputs: the staged rows and the plan's normaliser
    ctcext_amd.decode_logits(np.array(x), sl, W, P, batch_first=False, skip_blank=skip_util.THR, token_scores=True, **kw)
    th = ctcext_amd.token_scores()
    assert isinstance(th.logp_sum, np.ndarray)
    _assert_scores(th, want, what="synchronous, skipping")


# ---- 5. status and preconditions

def test_item_with_a_status_bit_is_nan_and_alone(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (12, 6, 5, 8, 3)
    T, B, C, W, P = shape
    x, sl, kw, (dec, ali, times, want) = family_case("peaky", shape, False)
    bad = np.array(sl)
    bad[1] = T + 1
    out, tt, sc = _dense(np.array(x), bad, W, P, **kw)
    got = _host(sc)
    assert np.isnan(got[0][1]).all() and np.isnan(got[1][1]).all()
    _assert_scores(sc, want, items=[0, 2, 3, 4, 5], what="neighbours")
    assert _host([out.status])[0].tolist() == [0, _lib.CTCEXT_ITEM_LENGTH, 0, 0, 0, 0]
    with pytest.raises(ctcext_amd.FailedPreconditionError):
        ctcext_amd.dense_check()


def test_without_the_opt_in_the_score_calls_fail_precondition(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    x = family(np.random.default_rng(7), "gaussian", 6, 2, 4)
    xd = torch.as_tensor(x, device=DEV)
    ctcext_amd.decode_dense(xd, [6, 6], 8, 1, batch_first=False)
    assert ctcext_amd.get_decoder(0)._scores_keep is None
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.dense_token_scores()
    assert e.value.message == NO_OPT_IN and e.value.error_code == _lib.CTCEXT_FAILED_PRECONDITION
    ctcext_amd.dense_check()
    ctcext_amd.decode_logits(xd, [6, 6], 8, 1, batch_first=False)
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.token_scores()
    assert e.value.message == NO_OPT_IN


def test_without_a_dense_decode_fails_precondition(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C = 6, 2, 4
    x = family(np.random.default_rng(7), "gaussian", T, B, C)
    ctcext_amd.decode_logits(torch.as_tensor(x, device=DEV), [T, T], 8, 1, batch_first=False,
                             token_scores=True)   # ends any dense call
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.dense_token_scores()
    assert e.value.error_code == _lib.CTCEXT_FAILED_PRECONDITION
    # ... and behind the Python layer's own bookkeeping, the library's answer
    d = ctcext_amd.get_decoder(0)
    start = torch.zeros((B, 1, T), dtype=torch.int32, device=DEV)
    t, o = _lib.TokenTimesOut(), _lib.TokenScoresOut()
    t.start = t.end = start.data_ptr()
    o.logp_sum = torch.zeros((B, 1, T), device=DEV).data_ptr()
    assert d.lib.ctcext_dense_token_scores(d.handle, ctypes.byref(t), ctypes.byref(o)) == _lib.CTCEXT_FAILED_PRECONDITION
    assert d.lib.ctcext_last_error().decode() == "ctcext_dense_token_scores without a ctcext_decode_dense"
    # a dense call in turn leaves nothing for the synchronous form
    ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), [T, T], 8, 1, batch_first=False, token_scores=True)
    with pytest.raises(ctcext_amd.FailedPreconditionError):
        ctcext_amd.token_scores()
    assert d.lib.ctcext_fetch_token_scores(d.handle, ctypes.byref(o), 1) == _lib.CTCEXT_FAILED_PRECONDITION
    ctcext_amd.dense_check()


def test_blank_label_that_is_a_class_label_is_refused(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 12, 2, 5, 8, 1
    x = family(np.random.default_rng(6), "gaussian", T, B, C)
    ctcext_amd.decode_dense(torch.as_tensor(x, device=DEV), [T, T], W, P, batch_first=False, blank_label=3,
                            token_scores=True)
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.dense_token_scores()
    assert e.value.message == MSG
    # the scores' own check, with times it is handed
    tt = ctcext_amd.TokenTimes(torch.full((B, P, T), -1, dtype=torch.int32, device=DEV),
                               torch.full((B, P, T), -1, dtype=torch.int32, device=DEV), None)
    with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
        ctcext_amd.dense_token_scores(tt)
    assert e.value.message == MSG and e.value.error_code == _lib.CTCEXT_INVALID_ARGUMENT
    ctcext_amd.dense_check()


# ---- 6. defensive reads: the kernel trusts nothing in start / end

I32_MAX = 2 ** 31 - 1


def test_out_of_range_spans_are_refused(monkeypatch):
    """Plain out-of-range integers in start / end, through the C ABI: every cell
    is a NaN and the call completes normally.  Then either output alone."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    shape = (12, 6, 5, 8, 3)
    T, B, C, W, P = shape
    x, sl, kw, (dec, ali, times, want) = family_case("sticky", shape, True)
    out, tt, sc = _dense(np.array(x), sl, W, P, **kw)
    d = ctcext_amd.get_decoder(0)

    def call(start, end, lsum, lmin):
        t, o = _lib.TokenTimesOut(), _lib.TokenScoresOut()
        t.start, t.end = start.data_ptr(), end.data_ptr()
        o.logp_sum, o.logp_min = [None if v is None else v.data_ptr() for v in (lsum, lmin)]
        return d.lib.ctcext_dense_token_scores(d.handle, ctypes.byref(t), ctypes.byref(o))

    def filled(v):
        return torch.full((B, P, T), v, dtype=torch.int32, device=DEV)

    for s, e in ((-7, -7), (T, T), (5, 2), (I32_MAX, I32_MAX), (-7, 3), (0, T), (0, I32_MAX), (I32_MAX, 0)):
        lsum, lmin = torch.zeros((B, P, T), device=DEV), torch.zeros((B, P, T), device=DEV)
        assert call(filled(s), filled(e), lsum, lmin) == _lib.CTCEXT_OK, (s, e)
        got = _host([lsum, lmin])
        assert np.isnan(got[0]).all() and np.isnan(got[1]).all(), (s, e)
    # either output may be NULL, not both; the other is not touched
    lsum, lmin = torch.full((B, P, T), 77.0, device=DEV), torch.full((B, P, T), 77.0, device=DEV)
    assert call(tt.start, tt.end, lsum, None) == _lib.CTCEXT_OK
    _assert_scores([lsum], want[:1], what="logp_sum alone")
    assert (lmin == 77).all().item()
    lsum.fill_(77.0)
    assert call(tt.start, tt.end, None, lmin) == _lib.CTCEXT_OK
    got = _host([lmin])[0]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want[1]))
    np.testing.assert_array_equal(got[~np.isnan(got)], want[1][~np.isnan(want[1])])
    assert (lsum == 77).all().item()
    assert call(tt.start, tt.end, None, None) == _lib.CTCEXT_INVALID_ARGUMENT
    ctcext_amd.dense_check()


# ---- 7. the call only enqueues; graph capture

@functools.lru_cache(maxsize=None)
def _async_scores():
    T, B, C, W, P = ASYNC_SHAPE
    x, sl, dense = _async_case()
    dec, dl, ali, al = dense[:4]
    rows = [[ali[b, p, :al[b, p]].tolist() for p in range(P)] for b in range(B)]
    decs = [[dec[b, p, :dl[b, p]].tolist() for p in range(P)] for b in range(B)]
    start, end, _ = expected_from_rows(decs, rows, sl, B, P, T, -1, True)
    return expected_from_rows_and_times(x, rows, sl, start, end, dl, B, P, T, 0, -1)


@pytest.mark.parametrize("where", ["default_stream", "side_stream"])
def test_call_only_enqueues(where, monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = ASYNC_SHAPE
    x, sl, _ = _async_case()
    want = _async_scores()
    xd, sld = torch.as_tensor(x, device=DEV), torch.as_tensor(sl, device=DEV)
    stream = torch.cuda.Stream(device=DEV) if where == "side_stream" else torch.cuda.default_stream(DEV)
    kw = dict(batch_first=False, merge_repeated=True, token_scores=True)

    def blocked(*a, **k):
        raise AssertionError("dense_token_scores reached a host synchronisation")

    with torch.cuda.stream(stream):
        ctcext_amd.decode_dense(xd, sld, W, P, **kw)   # warm-up: workspace, kernels
        ctcext_amd.dense_token_scores()
        torch.cuda.synchronize()
        with monkeypatch.context() as m:
            m.setattr(torch.cuda, "synchronize", blocked)
            m.setattr(torch.cuda.Stream, "synchronize", blocked)
            m.setattr(torch.Tensor, "cpu", blocked)
            m.setattr(torch.Tensor, "item", blocked)
            ctcext_amd.decode_dense(xd, sld, W, P, **kw)
            sc = ctcext_amd.dense_token_scores()
        ev = torch.cuda.Event()
        ev.record()
        done_at_return = ev.query()
        ev.synchronize()
    assert not done_at_return, "the work had finished when dense_token_scores returned: it did not only enqueue"
    _assert_scores(sc, want, what=where)
    ctcext_amd.dense_check()


def test_graph_capture_and_replay(monkeypatch):
    """decode_dense, dense_token_times and dense_token_scores captured together
    on a side stream and replayed on new logits copied into the static input,
    which is what the captured scores kernel reads; the workspace of the
    captured shape comes from ctcext_dense_reserve alone."""
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 3, 20, 100, 3
    rng = np.random.default_rng(406)
    side = torch.cuda.Stream(device=DEV)
    kw = dict(batch_first=False, merge_repeated=True, pad_value=-7, token_scores=True)
    with torch.cuda.stream(side):
        ctcext_amd.decode_dense(torch.zeros((4, 1, C), device=DEV), torch.full((1,), 4, dtype=torch.int32, device=DEV),
                                W, P, **kw)
        ctcext_amd.dense_token_scores()   # loads the kernels
    side.synchronize()
    xs = torch.zeros((T, B, C), device=DEV)
    sls = torch.zeros((B,), dtype=torch.int32, device=DEV)
    dec = ctcext_amd.get_decoder(0)
    a = ops._args(xs.data_ptr(), (T, B, C), _lib.CTCEXT_F32, True, sls.data_ptr(), (B,), W, P, True, 0, -1, 0, None)
    assert dec.lib.ctcext_dense_reserve(dec.handle, ctypes.byref(a)) == _lib.CTCEXT_OK
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctcext_amd.decode_dense(xs, sls, W, P, **kw)
        tt = ctcext_amd.dense_token_times()
        sc = ctcext_amd.dense_token_scores(tt)
    for sl in ([T, T - 7, 3], [5, T, T - 1]):
        x = family(rng, "sticky", T, B, C)
        xs.copy_(torch.as_tensor(x))
        sls.copy_(torch.as_tensor(np.asarray(sl, np.int32)))
        torch.cuda.synchronize()
        g.replay()
        _assert_scores(sc, expected(x, sl, W, P, T, merge_repeated=True)[3], what="replay %s" % (sl,))
        assert ctcext_amd.dense_check()["records_written"] > 0


# ---- 8. the synchronous form

def test_token_scores_after_decode_logits_equals_the_dense_form(monkeypatch):
    monkeypatch.delenv("CTCEXT_HELPER", raising=False)
    T, B, C, W, P = 40, 3, 29, 128, 3
    x = family(np.random.default_rng(9), "sticky", T, B, C)
    sl = lengths(T, B)
    kw = dict(merge_repeated=True, blank_index=0, blank_label=-1)
    want = expected(x, sl, W, P, T, **kw)[3]
    out, tt, sd = _dense(x, sl, W, P, **kw)
    dense = _host(sd)
    _assert_scores(dense, want, what="dense form")
    # device inputs: the caller's tensor is read again; CUDA tensors out
    ctcext_amd.decode_logits(torch.as_tensor(x, device=DEV), torch.as_tensor(sl, device=DEV), W, P, batch_first=False,
                             token_scores=True, **kw)
    ts = ctcext_amd.token_scores()
    assert ts.logp_sum.is_cuda and tuple(ts.logp_sum.shape) == (B, P, T)
    _assert_scores(ts, dense, what="device inputs")
    # host inputs, batch-major: the staged copy in the workspace; numpy out
    ctcext_amd.decode_logits(np.ascontiguousarray(x.transpose(1, 0, 2)), sl, W, P, token_scores=True, **kw)
    th = ctcext_amd.token_scores()
    assert isinstance(th.logp_sum, np.ndarray) and th.logp_sum.dtype == np.float32
    _assert_scores(th, dense, what="host inputs")
    ctcext_amd.ctc_ext_beam_search_decoder(x, sl, W, P, token_scores=True, **kw)
    _assert_scores(ctcext_amd.token_scores(), dense, what="host inputs, the drop-in call")
