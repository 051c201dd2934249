"""decode_logits: half-precision (float16 / bfloat16) and batch-major or
strided logits decoded in place.  Widening is exact, so every case demands
all seven outputs bit-exact against the oracle run on the widened time-major
float32 array (compare(..., lp_exact=True)).  The inputs are drawn in float32,
rounded to the half type once, and the same rounded values go to both sides.
Needs an MI355X."""
import numpy as np
import pytest
import torch

import ctcext_amd
from ctcext_amd import _lib
from parity_util import compare, to_numpy
import oracle
import range_inputs

pytestmark = pytest.mark.gpu

HALVES = {"fp16": torch.float16, "bf16": torch.bfloat16}
KW = dict(merge_repeated=True, blank_index=0, blank_label=-1)

# name: (C, W, P, T, B, flags) -- the smallest shapes that reach each decode
# kernel and each load path of the row stage and the pre-pass
CASES = {
    "score_table_ring": (29, 128, 3, 40, 3, 0),                  # two-wave score-table kernel, default ring
    "score_table_ring_min": (29, 128, 3, 40, 3, _lib.CTCEXT_FLAG_RING_MIN),
    "one_wave_small": (5, 7, 2, 20, 3, 0),                       # odd C, scalar loads
    "two_classes": (2, 4, 2, 20, 3, 0),
    "one_class": (1, 3, 1, 20, 3, 0),                            # the literal path
    "c64": (64, 16, 2, 16, 3, 0),                                # last C of the small kernels
    "c65": (65, 16, 2, 16, 3, 0),                                # first of the big ones, odd
    "c72_vector": (72, 32, 2, 16, 3, 0),                         # rows of whole 16-byte pieces
    "c70_unaligned_rows": (70, 32, 2, 16, 3, 0),                 # 140-byte rows
    "c1001_odd": (1001, 64, 2, 12, 2, 0),
    "c1000_facts": (1000, 64, 2, 12, 2, 0),                      # cfg4's fused facts kernel
    "c5000": (5000, 256, 2, 6, 2, 0),                            # cfg5's kernels
    "c33000_dynamic": (33000, 100, 2, 6, 2, 0),                  # 66-KB rows: the run-time-W layout, the global-row pre-pass
    "gather_queue": (29, 200, 3, 16, 3, 0),
    "one_wave_wide": (29, 300, 3, 16, 3, 0),
    "global_state": (29, 8, 2, 16, 3, _lib.CTCEXT_FLAG_GLOBAL_STATE),   # widened into workspace
}

_cache = {}


def _lengths(T, B):
    return np.array([T, max(T // 2, 1), max(T - 3, 1), T, T - 1][:B], np.int32)


def _draw(name, half, scale=1.0):
    """The case's rounded logits (time-major half tensor on the host), their
    widened float32 array, the lengths and the oracle's outputs: computed once
    per (case shape, half type) and shared."""
    C, W, P, T, B, _ = CASES[name]
    key = (C, W, P, T, B, half)
    if key not in _cache:
        rng = np.random.default_rng(sum(map(ord, name)) * 131 + C)
        x32 = (rng.standard_normal((T, B, C)) * scale).astype(np.float32)
        xh = torch.from_numpy(x32).to(HALVES[half])
        wide = xh.float().numpy()
        sl = _lengths(T, B)
        _cache[key] = (xh, wide, sl, oracle.decode(wide, sl, W, P, **KW))
    return _cache[key]


def _host(o):
    """A decoder result with every field as numpy (compare's reference side)."""
    return type(o)(*[[to_numpy(t) for t in f] for f in o[:6]], to_numpy(o.log_probability))


def _assert_device_f32(out):
    assert out.log_probability.is_cuda and out.log_probability.dtype == torch.float32


@pytest.mark.parametrize("batch_first", [False, True], ids=["time_major", "batch_major"])
@pytest.mark.parametrize("half", sorted(HALVES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_half_logits_match_oracle(name, half, batch_first):
    C, W, P, T, B, flags = CASES[name]
    xh, wide, sl, ref = _draw(name, half)
    logits = xh.cuda()
    if batch_first:
        logits = logits.transpose(0, 1).contiguous()
    out = ctcext_amd.decode_logits(logits, torch.as_tensor(sl, device="cuda"), W, P, batch_first=batch_first,
                                   flags=flags, **KW)
    _assert_device_f32(out)
    compare(out, ref, P, lp_exact=True)
    st = ctcext_amd.get_decoder(0).last_stats
    assert st["tier"] == (1 if flags & _lib.CTCEXT_FLAG_GLOBAL_STATE else 0)
    if name.startswith("score_table_ring"):
        assert st["ring_frames"] > 0


# ---------------------------------------------------------------------------
# strided views, decoded in place

@pytest.mark.parametrize("half", sorted(HALVES))
@pytest.mark.parametrize("name,pad", [("score_table_ring", 11), ("c72_vector", 11), ("c72_vector", 16),
                                      ("c1000_facts", 24)])
def test_vocabulary_slice(name, pad, half):
    # [B, T, C] at the front of a [B, T, C + pad] buffer: C + 11 leaves odd
    # row starts (scalar loads); + 16 / + 24 keep every row 16-byte aligned
    C, W, P, T, B, flags = CASES[name]
    xh, wide, sl, ref = _draw(name, half)
    big = torch.full((B, T, C + pad), 7.0, dtype=HALVES[half], device="cuda")   # (a wrong read would win the beam)
    big[:, :, :C] = xh.cuda().transpose(0, 1)
    view = big[:, :, :C]
    assert not view.is_contiguous() and view.data_ptr() == big.data_ptr()
    out = ctcext_amd.decode_logits(view, sl, W, P, flags=flags, **KW)
    compare(out, ref, P, lp_exact=True)


@pytest.mark.parametrize("half", sorted(HALVES))
@pytest.mark.parametrize("name", ["one_wave_small", "c72_vector"])
def test_transpose_views(name, half):
    C, W, P, T, B, flags = CASES[name]
    xh, wide, sl, ref = _draw(name, half)
    tm = xh.cuda()                                # [T, B, C] storage
    bm = tm.transpose(0, 1).contiguous()          # [B, T, C] storage
    for view, batch_first in ((tm.transpose(0, 1), True), (bm.transpose(0, 1), False)):
        assert not view.is_contiguous()
        out = ctcext_amd.decode_logits(view, sl, W, P, batch_first=batch_first, **KW)
        compare(out, ref, P, lp_exact=True)


@pytest.mark.parametrize("half", sorted(HALVES))
@pytest.mark.parametrize("name", ["c72_vector", "c1000_facts", "score_table_ring"])
def test_base_two_byte_aligned(name, half):
    # the storage starts one element into a flat buffer: C would allow the
    # 16-byte loads, the base address does not
    C, W, P, T, B, flags = CASES[name]
    xh, wide, sl, ref = _draw(name, half)
    flat = torch.zeros(1 + B * T * C, dtype=HALVES[half], device="cuda")
    view = flat[1:].view(B, T, C)
    view.copy_(xh.cuda().transpose(0, 1))
    assert view.data_ptr() % 4 == 2
    out = ctcext_amd.decode_logits(view, sl, W, P, **KW)
    compare(out, ref, P, lp_exact=True)


# ---------------------------------------------------------------------------
# special values

def _special(kind, half, C):
    rng = np.random.default_rng(900 + C + len(kind))
    T, B = 16, 4
    x = rng.standard_normal((T, B, C)).astype(np.float32)
    if kind == "nonfinite":
        x[rng.random(x.shape) < 0.12] = -np.inf        # everywhere
        x[3, 1, C // 2] = np.inf                       # item 1: a +inf
        x[5, 2, C - 1] = np.nan                        # item 2: a NaN
        x[7, 3, :] = -np.inf                           # item 3: a row of -inf only
    elif kind == "tiny":
        # fp16 subnormals (below 2^-14) and bf16 values below 2^-126 (float32
        # subnormals): both widen to nonzero float32
        tiny = 2.0 ** -20 if half == "fp16" else 2.0 ** -130
        x = (np.sign(x) * rng.integers(1, 8, size=x.shape) * tiny).astype(np.float32)
    elif kind == "ties":
        x = (np.round(x * 2) / 2).astype(np.float32)   # a 0.5 grid: exact in both formats, heavy ties
    elif kind in ("logsoftmax", "edges"):
        # the whole float range, rounded to the half type (bf16's grid
        # straddles expf's underflow bound at -103.5 / -104; fp16 turns the
        # family's -1e30 into -inf)
        x = range_inputs.family(range_inputs.rng_for("layouts/%s/%d" % (kind, C)), kind, T, B, C, np.float32)
    xh = torch.from_numpy(x).to(HALVES[half])
    wide = xh.float().numpy()
    if kind == "tiny":
        assert (wide != 0).all() and (np.abs(wide) < (2.0 ** -14 if half == "fp16" else 2.0 ** -126)).all()
    if kind in ("logsoftmax", "edges"):   # finite terms below the bound survive the rounding
        assert range_inputs.census(wide)["below"] >= 1
    return xh, wide, np.array([T, T - 1, T, T - 5], np.int32)


@pytest.mark.parametrize("half", sorted(HALVES))
@pytest.mark.parametrize("C,W", [(6, 8), (72, 16), (1000, 16)])
@pytest.mark.parametrize("kind", ["nonfinite", "tiny", "ties", "logsoftmax", "edges"])
def test_special_values(kind, C, W, half):
    """Against the oracle and against this library's own float32 decode of the
    widened tensor: the same literal-path decisions, the same outputs."""
    xh, wide, sl = _special(kind, half, C)
    P = 2
    try:
        ref, rerr = oracle.decode(wide, sl, W, P, **KW), None
    except oracle.OracleError as e:
        ref, rerr = None, str(e)
    if kind in ("logsoftmax", "edges"):
        assert rerr is None, rerr   # (an error on both sides would stand in for a comparison)
    dec = ctcext_amd.get_decoder(0)

    def run(fn):
        try:
            out = fn()
            return out, None, {k: dec.last_stats[k] for k in ("literal_frames", "literal_nonfinite",
                                                               "literal_fill", "duplicate_frames")}
        except ctcext_amd.OpError as e:
            return None, e.message, None
    f32, ferr, fst = run(lambda: ctcext_amd.ctc_ext_beam_search_decoder(
        torch.from_numpy(wide).cuda(), torch.as_tensor(sl, device="cuda"), W, P, **KW))
    assert ferr == rerr
    for batch_first in (False, True):
        logits = xh.cuda()
        if batch_first:
            logits = logits.transpose(0, 1).contiguous()
        out, err, st = run(lambda: ctcext_amd.decode_logits(logits, sl, W, P, batch_first=batch_first, **KW))
        assert err == rerr
        if ref is None:
            continue
        compare(out, ref, P, lp_exact=True)
        compare(out, _host(f32), P, lp_exact=True)
        assert st == fst


# ---------------------------------------------------------------------------
# float32 / float64 through decode_logits: layout alone changes nothing

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("C,W", [(29, 16), (72, 16), (70, 16)])
def test_native_dtypes_batch_major(dtype, C, W):
    rng = np.random.default_rng(77 + C)
    T, B, P = 16, 3, 2
    x = rng.standard_normal((T, B, C)).astype(dtype)
    sl = _lengths(T, B)
    tm = torch.from_numpy(x).cuda()
    drop = ctcext_amd.ctc_ext_beam_search_decoder(tm, sl, W, P, **KW)
    ref = oracle.decode(x, sl, W, P, **KW)
    bm = tm.transpose(0, 1).contiguous()
    for logits, batch_first in ((bm, True), (tm, False), (tm.transpose(0, 1), True)):
        out = ctcext_amd.decode_logits(logits, sl, W, P, batch_first=batch_first, **KW)
        assert out.log_probability.dtype == tm.dtype
        compare(out, ref, P, lp_exact=True)
        compare(out, _host(drop), P, lp_exact=True)


# ---------------------------------------------------------------------------
# sharding: the non-root shard is copied, dense, from either layout

@pytest.mark.parametrize("layout", ["time_major", "batch_major", "vocabulary_slice", "host_batch_major"])
@pytest.mark.parametrize("C,W", [(29, 16), (72, 16)])
def test_sharded_bf16(layout, C, W):
    rng = np.random.default_rng(310 + C)
    T, B, P = 20, 5, 2
    xh = torch.from_numpy(rng.standard_normal((T, B, C)).astype(np.float32)).to(torch.bfloat16)
    wide = xh.float().numpy()
    sl = _lengths(T, B)
    ref = oracle.decode(wide, sl, W, P, **KW)
    if layout == "time_major":
        logits, batch_first = xh.cuda(), False
    elif layout == "batch_major":
        logits, batch_first = xh.cuda().transpose(0, 1).contiguous(), True
    elif layout == "host_batch_major":
        logits, batch_first = xh.transpose(0, 1).contiguous(), True
    else:
        big = torch.full((B, T, C + 11), 7.0, dtype=torch.bfloat16, device="cuda")
        big[:, :, :C] = xh.cuda().transpose(0, 1)
        logits, batch_first = big[:, :, :C], True
    out = ctcext_amd.decode_logits(logits, sl, W, P, batch_first=batch_first, devices=[0, 0], **KW)
    assert ctcext_amd.get_decoder((0, 0)).last_stats["n_devices"] == 2
    compare(out, ref, P, lp_exact=True)


# ---------------------------------------------------------------------------
# host inputs: copied to the device as 2-byte elements, outputs numpy

@pytest.mark.parametrize("name", ["score_table_ring", "c72_vector"])
def test_host_inputs(name):
    C, W, P, T, B, flags = CASES[name]
    xh, wide, sl, ref = _draw(name, "bf16")
    out = ctcext_amd.decode_logits(xh.transpose(0, 1).contiguous(), sl, W, P, **KW)   # a CPU torch bf16 tensor
    assert isinstance(out.log_probability, np.ndarray) and out.log_probability.dtype == np.float32
    assert isinstance(out.decoded_values[0], np.ndarray)
    compare(out, ref, P, lp_exact=True)
    xh, wide, sl, ref = _draw(name, "fp16")
    x16 = np.ascontiguousarray(wide.astype(np.float16).transpose(1, 0, 2))           # a numpy float16 array
    assert (x16.astype(np.float32).transpose(1, 0, 2) == wide).all()
    out = ctcext_amd.decode_logits(x16, sl, W, P, **KW)
    assert isinstance(out.log_probability, np.ndarray) and out.log_probability.dtype == np.float32
    compare(out, ref, P, lp_exact=True)
    # ... and a host view that is not contiguous, read through its strides
    pad = np.full((B, T, C + 3), 7, np.float16)
    pad[:, :, :C] = x16
    compare(ctcext_amd.decode_logits(pad[:, :, :C], sl, W, P, **KW), ref, P, lp_exact=True)


# ---------------------------------------------------------------------------
# edge cases

@pytest.mark.parametrize("half", sorted(HALVES))
def test_zero_length_item_and_empty_batch(half):
    rng = np.random.default_rng(4)
    T, B, C = 5, 3, 4
    xh = torch.from_numpy(rng.standard_normal((T, B, C)).astype(np.float32)).to(HALVES[half])
    sl = np.array([5, 0, 3], np.int32)
    ref = oracle.decode(xh.float().numpy(), sl, 4, 1, **KW)   # a zero-length item has one leaf: top_paths 1
    for batch_first in (False, True):
        logits = xh.cuda().transpose(0, 1).contiguous() if batch_first else xh.cuda()
        compare(ctcext_amd.decode_logits(logits, sl, 4, 1, batch_first=batch_first, **KW), ref, 1, lp_exact=True)
    empty = torch.zeros((0, T, C), dtype=HALVES[half], device="cuda")
    out = ctcext_amd.decode_logits(empty, np.zeros(0, np.int32), 4, 2, **KW)
    drop = ctcext_amd.ctc_ext_beam_search_decoder(torch.zeros((T, 0, C), device="cuda"), np.zeros(0, np.int32),
                                                  4, 2, **KW)
    _assert_device_f32(out)
    assert tuple(out.log_probability.shape) == (0, 2)
    compare(out, _host(drop), 2, lp_exact=True)
