"""The greedy decode on the GPU (decode_greedy): all six outputs equal the numpy
restatement of the definition (test_cpu_greedy.greedy over oracle.row_norm)
exactly: values, NaN cells, and the sign bit of every float that is no NaN
(same_bits says why a created NaN's sign is left out)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctcext_amd
import oracle
import range_inputs
from ctcext_amd import _lib
from test_cpu_greedy import greedy, quantised, same_bits, special, sticky

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def ranged(kind, bad=True):
    """A family of range_inputs (finite, over the whole float range), with NaN and infinite cells on top if bad."""
    def make(rng, T, B, C, dtype=np.float32):
        x = range_inputs.family(rng, kind, T, B, C, dtype)
        cells = special(rng, T, B, C, dtype)
        return np.where(np.isfinite(cells), x, cells) if bad else x
    return make


def ragged(rng, T, B):
    """Lengths 0, T, a negative one, and items 0..69 of under 10 frames: with B = 130, waves of 64 (t, b) rows lie
    wholly and partly past their items."""
    sl = rng.integers(0, T + 1, size=B).astype(np.int32)
    sl[:70] = rng.integers(0, min(10, T + 1), size=70)[:min(B, 70)]
    sl[B - 1], sl[B // 2], sl[0] = T, -3, 0
    return sl


# name: (family, [T, B, C] time-major, dtype of the tensor); C = 33 is one past the LDS tile, T = 600 past two
# 256-frame tiles
CASES = {
    "quantised-7x3x5": (quantised, (7, 3, 5), "float32"), "range-7x3x5": (ranged("edges"), (7, 3, 5), "float32"),
    "quantised-1x1x1": (quantised, (1, 1, 1), "float32"),
    "quantised-70x130x29": (quantised, (70, 130, 29), "float32"),
    "range-70x130x29": (ranged("huge"), (70, 130, 29), "float32"),
    "quantised-600x2x33": (quantised, (600, 2, 33), "float32"), "sticky-600x2x33": (sticky, (600, 2, 33), "float32"),
    "range-600x2x33": (ranged("logsoftmax"), (600, 2, 33), "float32"),
    "quantised-40x2x300": (quantised, (40, 2, 300), "float32"), "range-40x2x300": (ranged("edges", False), (40, 2, 300), "float32"),
    "sticky-600x2x33-f64": (sticky, (600, 2, 33), "float64"), "range-600x2x33-f64": (ranged("logsoftmax", False), (600, 2, 33), "float64"),
    "sticky-70x130x29-bf16": (sticky, (70, 130, 29), "bfloat16"), "quantised-70x130x29-f16": (quantised, (70, 130, 29), "float16"),
}


def expected(x, sl, merge, blank=0, blank_label=-1, pad=-1):
    """The DenseDecode of x [T, B, C] (the widened values) as numpy arrays."""
    T, B, _ = x.shape
    dec, ali = np.full((B, 1, T), pad, np.int64), np.full((B, 1, T), pad, np.int64)
    dlen, alen = np.zeros((B, 1), np.int32), np.zeros((B, 1), np.int32)
    logp, status = np.zeros((B, 1), x.dtype), np.zeros((B,), np.int32)
    for b in range(B):
        if sl[b] > T:
            status[b], logp[b, 0] = _lib.CTCEXT_ITEM_LENGTH, -np.inf
            continue
        n = max(int(sl[b]), 0)
        xb = np.ascontiguousarray(x[:n, b])
        d, a, logp[b, 0] = greedy(xb, oracle.row_norm(xb) if n else [], n, blank, blank_label, merge)
        dec[b, 0, :len(d)], ali[b, 0, :n], dlen[b, 0], alen[b, 0] = d, a, len(d), n
    return ctcext_amd.DenseDecode(dec, dlen, ali, alen, logp, status)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case (computed once): the tensor's values, their widened form, the lengths."""
    fam, (T, B, C), dt = CASES[name]
    rng = range_inputs.rng_for(name)
    t = torch.as_tensor(fam(rng, T, B, C, np.float64 if dt == "float64" else np.float32)).to(getattr(torch, dt))
    wide = t.numpy() if dt == "float64" else t.float().numpy()
    sl = ragged(rng, T, B) if B > 3 else np.array([T, T - 2, 0][:B], np.int32)
    return t, wide, sl


@functools.lru_cache(maxsize=None)
def want(name, merge):
    _, wide, sl = case(name)
    return expected(wide, sl, merge)


def on_device(name):
    """The case's tensor on the GPU, time-major; a half tensor as a batch-major view with gaps in both dimensions."""
    t, _, sl = case(name)
    T, B, C = t.shape
    kw = dict(batch_first=False)
    x = t.to(DEV)
    if t.dtype in (torch.float16, torch.bfloat16):
        full = torch.zeros((B, T + 3, 40), dtype=t.dtype, device=DEV)
        full[:, 1:1 + T, 5:5 + C] = x.transpose(0, 1)
        x, kw = full[:, 1:1 + T, 5:5 + C], dict(batch_first=True)
    return x, torch.as_tensor(sl, device=DEV), kw


def check(got, exp, what):
    torch.cuda.synchronize()
    for field, g, w in zip(exp._fields, got, exp):
        same_bits(g.cpu().numpy(), w, (what, field))


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_definition(name, merge):
    x, sl, kw = on_device(name)
    check(ctcext_amd.decode_greedy(x, sl, merge_repeated=merge, **kw), want(name, merge), name)
    st = ctcext_amd.dense_check()
    assert st["tier"] == 0 and not st["kernel"]["launched"] and st["literal_frames"] == st["records_written"] == 0
    if name.startswith("sticky"):
        assert not np.array_equal(want(name, True).decoded, want(name, False).decoded)   # A blank A is in there


def test_item_above_max_time_is_empty_and_alone():
    name = "quantised-7x3x5"
    x, _, kw = on_device(name)
    sl = np.array([7, 8, 5], np.int32)
    exp = expected(case(name)[1], sl, True)
    assert exp.status.tolist() == [0, _lib.CTCEXT_ITEM_LENGTH, 0] and exp.decoded_lengths[1, 0] == 0
    check(ctcext_amd.decode_greedy(x, sl, merge_repeated=True, **kw), exp, "length")
    with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
        ctcext_amd.dense_check()
    assert e.value.message == "sequence_length(1) <= 7"


def test_token_times_and_scores_follow():
    name = "sticky-600x2x33"
    x, sl, kw = on_device(name)
    out = ctcext_amd.decode_greedy(x, sl, merge_repeated=True, token_scores=True, **kw)
    tt = ctcext_amd.dense_token_times()
    ts = ctcext_amd.dense_token_scores(tt)
    exp, (_, wide, lens) = want(name, True), case(name)
    check(out, exp, name)
    for b, n in enumerate(np.maximum(lens, 0)):
        m, xb = int(exp.decoded_lengths[b, 0]), np.ascontiguousarray(wide[:n, b])
        d, a = exp.decoded[b, 0, :m], exp.alignment[b, 0, :n]
        s, e, trail = ctcext_amd.token_times_row(d, a, n, -1, merge_repeated=True)
        assert m > 2 and (s >= 0).all()
        same_bits(tt.start[b, 0, :m].cpu().numpy(), s, "start")
        same_bits(tt.end[b, 0, :m].cpu().numpy(), e, "end")
        assert int(tt.trailing_blank[b, 0]) == trail
        lsum, lmin = ctcext_amd.token_scores_row(xb, oracle.row_norm(xb), a, n, s, e, 0, -1)
        same_bits(ts.logp_sum[b, 0, :m].cpu().numpy(), lsum, "logp_sum")
        same_bits(ts.logp_min[b, 0, :m].cpu().numpy(), lmin, "logp_min")


def test_refused_before_anything_is_enqueued():
    x, sl, _ = on_device("quantised-7x3x5")
    with pytest.raises(ValueError):
        ctcext_amd.decode_greedy(x.cpu(), sl)
    d = ctcext_amd.get_decoder(0)
    out = ctcext_amd.decode_greedy(x, sl, batch_first=False)
    o = _lib.DenseOutputs()
    o.decoded, o.decoded_length, o.alignment, o.alignment_length, o.log_probability, o.status = [t.data_ptr() for t in out]
    tab = torch.zeros((6, 5), device=DEV)
    for change, message in ((dict(top_paths=2), "top_paths must be 1"), (dict(scorer=1, scorer_table=tab.data_ptr()), "no beam scorer"),
                            (dict(flags=_lib.CTCEXT_FLAG_NO_RING), "flags may hold only")):
        a = ctcext_amd.ops._args(x.data_ptr(), (7, 3, 5), _lib.CTCEXT_F32, True, sl.data_ptr(), (3,), 4, 1, False, 0, -1, 0, None)
        for k, v in change.items():
            setattr(a, k, v)
        for rc in (d.lib.ctcext_greedy_validate(ctypes.byref(a), ctypes.byref(o)),
                   d.lib.ctcext_decode_greedy(d.handle, ctypes.byref(a), ctypes.byref(o))):
            assert rc == _lib.CTCEXT_INVALID_ARGUMENT and message in d.lib.ctcext_last_error().decode()


def test_graph_capture_and_replay():
    """After a warm-up call of the shape, one capture of decode_greedy (a linear chain of three kernels) replayed over
    new contents of the static input."""
    name = "sticky-600x2x33"
    _, wide, lens = case(name)
    side = torch.cuda.Stream(device=DEV)
    xs, sls = torch.zeros(wide.shape, device=DEV), torch.as_tensor(lens, device=DEV)
    with torch.cuda.stream(side):
        ctcext_amd.decode_greedy(xs, sls, batch_first=False, merge_repeated=True)
    side.synchronize()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = ctcext_amd.decode_greedy(xs, sls, batch_first=False, merge_repeated=True)
    for x, exp in ((wide, want(name, True)), (wide[::-1].copy(), None), (wide, want(name, True))):
        xs.copy_(torch.as_tensor(x))
        torch.cuda.synchronize()
        g.replay()
        check(out, exp or expected(x, lens, True), "replay")
