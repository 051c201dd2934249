"""Every kernel route against recorded outputs of the REFERENCE decoder.

tests/golden/reference_cases.json (tests/golden/make_reference_fixtures.py)
holds what the reference's own headers computed for each case of groups A
(one per kernel route) and B (semantics a restatement could misread).  This
file reads only that JSON, neither the reference tree nor a build of it, and
compares all seven outputs of the op with it, log-probabilities bit for bit,
through each route a case's shape reaches:

  default          the default dispatch
  helper0/1/4      CTCEXT_HELPER=0 (one wave), =1 (score table / gather queue,
                   where the shape has one), =4 at every beam of 129..256 (the
                   scored queue for float at C > 64; one wave for the rest)
  literal          CTCEXT_FLAG_FORCE_LITERAL
  gstate           CTCEXT_FLAG_GLOBAL_STATE
  ring_min         CTCEXT_FLAG_RING_MIN: an 8-frame ring must have run, behind
                   the default dispatch's kernel (every shape but the one the
                   ring does not fit beside, _ring_fits)
  stream           StreamDecoder in three ragged pushes, compared after the last
  dense            decode_dense (test_gpu_dense.to_dense)
  bf16 / fp16      decode_logits on batch-major half-precision tensors, for
                   the float32 half-grid cases (exact in both formats)

Each test asserts from last_stats (tier, helper, kernel) that its route ran:
a fallback cannot stand in for the kernel.  A case the reference ended with an
error must raise that message.

tests/golden/reference_scorer_cases.json (group S) holds what the reference
decoder computed with a bigram table scorer in its scorer hook
(oracle/ref/ref_driver.cpp), for tables of every kind of
tests/scorer_tables.py.  test_bigram_route_matches_reference runs those cases
with the table through the same routes (helper0 left out; helper1 and helper4
ask for a two-wave kernel that a table must refuse: helper none), the stream
with the table on the host, decode_dense with it as a CUDA tensor, and

  sharded          devices=[0, 0]: two shards, each with its own copy of the
                   table; n_devices == 2 and the root shard's kernel row

and asserts on each that the kernel row's scorer is bigram.  A shape the
scorer's state arrays put past the LDS tier, or leave no room for the ring
(_scored_layout, from decode_lds_bytes), runs the routes it still reaches.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import ctcext_amd
import oracle
from ctcext_amd import _lib
from parity_util import compare
from test_gpu_dense import to_dense

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_reference_fixtures as gen  # noqa: E402  (inputs(): the cases' random streams)

CASES = json.load(open(os.path.join(GOLDEN, "reference_cases.json")))["cases"]
S_CASES = json.load(open(os.path.join(GOLDEN, "reference_scorer_cases.json")))["cases"]
assert not set(CASES) & set(S_CASES)
ALL = dict(CASES, **S_CASES)
DEV = "cuda:0"
NP = {"f32": np.float32, "f64": np.float64}
PAD = -7
FLAGS = {"literal": _lib.CTCEXT_FLAG_FORCE_LITERAL, "gstate": _lib.CTCEXT_FLAG_GLOBAL_STATE,
         "ring_min": _lib.CTCEXT_FLAG_RING_MIN}
HELPER_ENV = {"helper0": "0", "helper1": "1", "helper4": "4"}


def _helper(c, mode):
    """ctcx::helper_kind as ctcext_stats.kernel names it, for CTCEXT_HELPER
    unset (None), "0", "1" or "4": the scored queue SQ (float, the base
    scorer, beams <= 128; with "4" also beams <= 256 at C > 64), else the score
    table (C <= 64, beams <= 128) or the gather queue (C > 64, beams <= 256),
    both HW, else the one-wave kernel."""
    C, W = c["C"], c["beam_width"]
    if mode == "0" or c["dtype"] != "f32" or C < 2 or c.get("table") is not None:
        return "none"   # (a table keeps the one-wave bigram kernel whatever CTCEXT_HELPER says)
    if mode in (None, "4") and (W <= 128 or (mode == "4" and W <= 256 and C > 64)):
        return "SQ"
    if C <= 64:
        return "HW" if W <= 128 else "none"
    return "HW" if W <= 256 else "none"


def _a16(v):
    return (v + 15) & ~15


def _decode_lds_bytes(W, C, tsize, scored):
    """decode_lds_bytes of ctcx_kernels.h, line by line: the bytes of the decode
    kernel's LDS layout for a beam capacity W."""
    enc = 3 * W + 2
    nbuf = 1 if C > 64 else 2
    htab = 16
    while htab < 2 * W:
        htab <<= 1
    s = nbuf * _a16(5 * W * tsize) + nbuf * _a16(3 * W * 4) + _a16(4 * W * 4) + _a16(5 * enc * tsize) + _a16(5 * enc * 4)
    s += _a16((W + 1) * 4) * 2 + _a16(W * 4) * 2 + 64 + 32 * 8 + nbuf * 2 * W * 8 + _a16(4 * htab) + _a16(8 * W)
    s += ((W if W > 256 else 256 if W > 128 else 128) + 2 + 64) * (16 if tsize == 8 else 8)
    if scored:
        s += _a16((nbuf * W + enc) * tsize)
    s += _a16(C * tsize) + _a16(((C + 63) // 64) * tsize)
    if C > 64:
        nw = (C - 1 + 63) // 64
        s += 64 * 4 + 8 * nw + 8 * ((nw + 63) // 64) + 64 * 8
    return s


LDS_BYTES = 160 * 1024
assert _decode_lds_bytes(400, 20, 4, False) == 110768 and _decode_lds_bytes(400, 300, 8, False) == 130496 \
    and _decode_lds_bytes(400, 20, 8, False) == 154608   # (the figures of _ring_fits' docstring)
# with the scorer's states, (2 W + 3 W + 2) values more at C <= 64: 8016 bytes in float at 400 beams, 16016 in
# double, which is past the LDS; 380 beams in double stay inside (test_gpu_kernel_matrix's cell runs in tier 0)
assert _decode_lds_bytes(400, 20, 4, True) == 118784 and _decode_lds_bytes(400, 20, 8, True) == 170624 > LDS_BYTES \
    and _decode_lds_bytes(380, 20, 8, True) <= LDS_BYTES and _decode_lds_bytes(400, 300, 8, True) == 143312


def _scored_layout(c):
    """(whether a scored decode of the case's shape stays in the LDS tier, and
    there whether an 8-frame ring fits beside its layout): max_beam_width and
    ring_frames of the library, for two items (the whole LDS is the budget).
    The scorer's state arrays put (30, 20, 400) in double past the LDS tier
    (test_gpu_kernel_matrix decodes that cell at 380 beams for the same
    reason), and leave the ring no room at 400 beams in double at C = 300."""
    W, C, ts = c["beam_width"], c["C"], 8 if c["dtype"] == "f64" else 4
    if _decode_lds_bytes(W, C, ts, True) > LDS_BYTES:
        return False, False
    cap = 128 if W <= 128 else 256 if W <= 256 else W   # (C <= 300: the compile-time layouts fit)
    ring = _a16(8 * W * 8) + _a16(4 * 8) + 2 * _a16(4 * W) + _a16(8 * W)
    return True, _a16(_decode_lds_bytes(cap, C, ts, True)) + ring <= LDS_BYTES


def _ring_fits(c):
    """Whether the 8-frame record ring (32032 bytes at W = 400, ring_lds_bytes)
    fits the 160 KB LDS beside the decode layout (decode_lds_bytes,
    ctcx_kernels.h; two items: the whole LDS is the budget).  Beams up to 256
    leave it room at every class count here.  At W = 400 the layout takes
    110768 bytes (float, C = 20), less at C = 300 (one branch buffer),
    130496 (double, C = 300) and 154608 (double, C = 20: two branch buffers of
    8-byte values): only the last leaves less than the ring needs, and has no
    ring_min route."""
    if c.get("table") is not None:
        return _scored_layout(c)[1]
    return not (c["beam_width"] > 256 and c["dtype"] == "f64" and c["C"] <= 64)


def _scored_routes(c):
    """The routes of a group-S case: as _routes, with helper1 / helper4 asking
    for a two-wave kernel that a table must refuse, and the sharded handle
    (two shards on device 0, each with its own copy of the table)."""
    W = c["beam_width"]
    if not _scored_layout(c)[0]:     # past the LDS tier: every route is the global-state bigram kernel
        return ["default", "gstate", "stream", "dense", "sharded"]
    routes = ["default", "helper1"]
    if 129 <= W <= 256:
        routes.append("helper4")
    routes += ["literal", "gstate", "stream", "dense", "sharded"]
    if _ring_fits(c):
        routes.append("ring_min")
    if c["dtype"] == "f32" and c["table"] == "grid" and c["gen"] == "ties":
        routes += ["bf16", "fp16"]
    return routes


def _routes(c):
    """The routes the case's shape reaches."""
    if c.get("table") is not None:
        return _scored_routes(c)
    C, W = c["C"], c["beam_width"]
    routes = ["default", "helper0"]
    if _helper(c, "1") == "HW":
        routes.append("helper1")
    if 129 <= W <= 256:   # (the scored queue for float at C > 64; any other shape must stay on one wave)
        routes.append("helper4")
    routes += ["literal", "gstate", "stream", "dense"]
    if _ring_fits(c):
        routes.append("ring_min")
    if c["dtype"] == "f32" and c["gen"] == "ties":
        routes += ["bf16", "fp16"]
    return routes


PARAMS = [(name, route) for name in sorted(CASES) for route in _routes(CASES[name]["case"])]
S_PARAMS = [(name, route) for name in sorted(S_CASES) for route in _routes(S_CASES[name]["case"])]


@functools.lru_cache(maxsize=None)
def _table(name):
    fx = S_CASES[name]
    tab = gen.scorer_table(fx["case"])
    assert gen.sha(tab) == fx["table_sha256"], "table stream changed"
    tab.setflags(write=False)
    return tab


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, seq_len, the recorded outputs as the op's seven fields or None, the recorded error)."""
    fx = ALL[name]
    c = fx["case"]
    x, sl = gen.inputs(c)
    assert gen.sha(x) == fx["sha256"], "input stream changed"
    x.setflags(write=False)
    if fx["error"] is not None:
        return x, sl, None, fx["error"]
    B, P = c["B"], c["top_paths"]
    di, dv, ds = oracle.pack_sparse(fx["decoded"], B, P)
    ai, av, ash = oracle.pack_sparse(fx["alignment"], B, P)
    lp = np.asarray([[float.fromhex(h) for h in row] for row in fx["log_probability_hex"]], NP[c["dtype"]])
    return x, sl, oracle.OracleOutput(di, dv, ds, ai, av, ash, lp), None


def _kernel_row(c, helper, tier=0):
    W = c["beam_width"]
    scorer = "base" if c.get("table") is None else "bigram"
    if tier == 1:
        return (1, c["dtype"], scorer, 1, 0, False, "none")
    # (every shape here fits the compile-time layouts: C <= 300)
    return (0, c["dtype"], scorer, 1 if W <= 128 else 2 if W <= 256 else 4,
            128 if W <= 128 else 256 if W <= 256 else 0, c["C"] > 64, helper)


def _stat_row(k):
    return (k["tier"], k["dtype"], k["scorer"], k["RN"], k["WC"], k["BIG"], k["helper"])


def _assert_route(st, c, route, sl, stream=False):
    k = st["kernel"]
    frames = int(np.maximum(sl, 0).sum())
    if frames == 0 and not k["launched"]:
        return
    assert k["launched"], (route, st)
    assert k["stream"] == stream, (route, k)
    assert k["scorer"] == ("base" if c.get("table") is None else "bigram"), (route, k)
    if route == "gstate" or (c.get("table") is not None and not _scored_layout(c)[0]):
        assert st["tier"] == 1 and _stat_row(k) == _kernel_row(c, "none", tier=1), (route, st)
        return
    assert st["tier"] == 0, (route, st)
    if route == "ring_min":
        assert st["ring_frames"] == 8, (route, st)
    helper = _helper(c, HELPER_ENV.get(route))
    assert _stat_row(k) == _kernel_row(c, helper), (route, k)
    assert st["helper"] == {"none": 0, "SQ": 3, "HW": 1 if c["C"] <= 64 else 2}[helper], (route, st)
    if route == "literal" and not stream:
        assert st["literal_frames"] == frames, (route, st["literal_frames"], frames)


def _one_shot(x, sl, c, flags, tab=None, devices=None):
    return ctcext_amd.ctc_ext_beam_search_decoder(x, sl, c["beam_width"], c["top_paths"], flags=flags, scorer_table=tab,
                                                  devices=devices, **gen.attrs(c))


def _stream(x, sl, c, tab=None):
    T, B, C = x.shape
    cuts = [0, -(-T // 3), -(-2 * T // 3), T]
    x = np.ascontiguousarray(x)
    with ctcext_amd.StreamDecoder(B, C, c["beam_width"], c["top_paths"], T, dtype=NP[c["dtype"]], scorer_table=tab,
                                  **gen.attrs(c)) as s:
        for i in range(3):
            t0, t1 = cuts[i], cuts[i + 1]
            n = (np.minimum(sl, t1) - np.minimum(sl, t0)).astype(np.int32)
            out = s.push(x[t0:t1], n, batch_first=False, results=i == 2)
            if i == 0:   # (the first push always has frames; with T = 1 the later ones have none)
                st = s.last_stats
        assert s.frames.tolist() == np.maximum(sl, 0).tolist()
        return out, st


def _dense(x, sl, c, tab=None):
    out = ctcext_amd.decode_dense(torch.as_tensor(np.array(x), device=DEV), torch.as_tensor(sl, device=DEV),
                                  c["beam_width"], c["top_paths"], batch_first=False, pad_value=PAD,
                                  scorer_table=None if tab is None else torch.as_tensor(np.array(tab), device=DEV),
                                  **gen.attrs(c))
    st = ctcext_amd.dense_check()   # (waits; raises what the synchronous call would have raised)
    return out, st


@pytest.mark.parametrize("name,route", S_PARAMS)
def test_bigram_route_matches_reference(name, route, monkeypatch):
    """The group-S cases (the reference under the driver's table scorer)
    through every route a table reaches.  _assert_route holds the kernel row to
    scorer bigram on each; helper1 / helper4 must have stayed on one wave; the
    sharded handle must have split the batch over its two shards and give what
    the recorded reference gave."""
    _check_route(name, route, monkeypatch, _table(name))


@pytest.mark.parametrize("name,route", PARAMS)
def test_route_matches_reference(name, route, monkeypatch):
    _check_route(name, route, monkeypatch, None)


def _check_route(name, route, monkeypatch, tab):
    c = ALL[name]["case"]
    x, sl, want, error = _case(name)
    P = c["top_paths"]
    if route in HELPER_ENV:
        monkeypatch.setenv("CTCEXT_HELPER", HELPER_ENV[route])
    else:
        monkeypatch.delenv("CTCEXT_HELPER", raising=False)

    def run():
        if route == "stream":
            return _stream(x, sl, c, tab)
        if route == "dense":
            return _dense(x, sl, c, tab)
        if route == "sharded":
            out = _one_shot(x, sl, c, 0, tab, devices=[0, 0])
            st = ctcext_amd.get_decoder((0, 0)).last_stats
            assert st["n_devices"] == 2, st
            return out, st
        if route in ("bf16", "fp16"):
            half = torch.bfloat16 if route == "bf16" else torch.float16
            logits = torch.from_numpy(np.array(x)).transpose(0, 1).contiguous().to(half)
            assert (logits.float().transpose(0, 1).numpy() == x).all(), "the half grid is exact in the format"
            out = ctcext_amd.decode_logits(logits.to(DEV), sl, c["beam_width"], P, batch_first=True, scorer_table=tab,
                                           **gen.attrs(c))
        else:
            out = _one_shot(x, sl, c, FLAGS.get(route, 0), tab)
        return out, ctcext_amd.get_decoder(0).last_stats

    if error is not None:
        with pytest.raises(ctcext_amd.OpError) as e:
            run()
        assert e.value.message == error
        return
    out, st = run()
    _assert_route(st, c, route, sl, stream=route == "stream")
    if route == "dense":
        got = [t.cpu().numpy() for t in out]
        for field, g, w in zip(ctcext_amd.DenseDecode._fields, got[:5], to_dense(want, c["B"], P, c["T"], PAD)):
            assert g.dtype == w.dtype, (field, g.dtype, w.dtype)
            np.testing.assert_array_equal(g, w, err_msg=field)
        assert (got[5] == 0).all(), got[5]
    else:
        compare(out, want, P, lp_exact=True)
