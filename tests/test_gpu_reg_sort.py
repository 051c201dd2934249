"""The register-resident std::sort of the one-node float decode kernels
(reg_sort_extract in csrc/ctcx_decode.hip over csrc/ctcx_regsort.h): the
Extract() of a frame whose beam no push changed, or whose beam is not full
yet.

1. The unit programme (tools/reg_sort_unit.hip, built with the library): one
   launch, every wave sorts its own array with the register form and with the
   literal lit_sort; the host compares both with std::sort over every length
   1..128 and the input families of test_cpu_reg_sort.py, the depth-limit
   input included.  0 mismatches.

2. End to end, bit-exact against the oracle on all seven outputs: 6 frames of
   logits quantised to halves (equal totals), then 14 "quiet" frames -- blank
   at +16, every label N(0,1) - 16, so a child scores about 32 below its
   parent and cannot beat the bottom of a full beam: those frames accept no
   push and their Extract() is std::sort over the beam in branch order with
   the minimum in front.  Beam widths: insertion sort only (2, 16), the first
   partition level (17, 33), 64 and the second register coming into use (65),
   a partial second register (100), the bench width (128).  One-shot, the
   stream build in two pushes (7 + 13 frames), and decode_dense.

   The coverage the cases rely on is checked with the oracle alone
   (test_cases_have_quiet_frames_and_ties, no GPU): decoding x[:t] with
   top_paths = W for consecutive t, a frame that leaves the set of W label
   sequences unchanged accepted no push; every item of every case has at
   least 8 such frames, and in at least one of them two of the W
   log-probabilities are bit-equal.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from parity_util import compare

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
UNIT = os.path.join(ROOT, "tools", "reg_sort_unit.bin")

B, T, T_TIES = 3, 20, 6
CS = [5, 29]
WS = [2, 16, 17, 33, 64, 65, 100, 128]
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _logits(C, W):
    rng = np.random.default_rng(9000 + 1000 * C + W)
    x = rng.standard_normal((T, B, C)).astype(np.float32)
    x[:T_TIES] = (np.round(x[:T_TIES] * 2) / 2).astype(np.float32)   # parity_util.random_case, ties=True
    x[T_TIES:] -= np.float32(16.0)
    x[T_TIES:, :, 0] = np.float32(16.0)   # blank_index 0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(C, W, merge):
    sl = np.full(B, T, np.int32)
    return oracle.decode(_logits(C, W), sl, W, min(3, W), merge)


def _quiet_frames(C, W):
    """Per item: the frames t whose beam (the set of W label sequences after
    x[:t]) equals the one after x[:t - 1], and whether two of the W
    log-probabilities are bit-equal in one of them."""
    x = _logits(C, W)
    prev = [None] * B
    quiet = [0] * B
    tied = [False] * B
    for t in range(1, T + 1):
        try:
            dec, _, lp, _ = oracle.raw_decode(x, np.full(B, t, np.int32), W, W, False)
        except oracle.OracleError:   # fewer than W leaves yet: the beam is not full
            prev = [None] * B
            continue
        for b in range(B):
            cur = frozenset(tuple(int(v) for v in dec[b][p]) for p in range(W))
            assert len(cur) == W
            if prev[b] is not None and cur == prev[b]:
                quiet[b] += 1
                bits = np.asarray(lp[b], np.float32).view(np.uint32)
                tied[b] |= len(set(bits.tolist())) < W
            prev[b] = cur
    return quiet, tied


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("C", CS)
def test_cases_have_quiet_frames_and_ties(C, W):
    quiet, tied = _quiet_frames(C, W)
    assert min(quiet) >= 8, (C, W, quiet)
    assert any(tied), (C, W, tied)


@pytest.mark.gpu
def test_unit_programme_matches_std_sort():
    assert os.path.exists(UNIT), "tools/reg_sort_unit.bin is missing: build() makes it with the library"
    r = subprocess.run(["timeout", "-k", "10", "120", UNIT], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("reg_sort_unit: 0/"), r.stdout
    assert "register sort gave up 1 (cases that gave up: 1, want 1)" in r.stdout, r.stdout


def _assert_one_node_float(st):
    k = st["kernel"]
    assert k["launched"] and k["RN"] == 1 and k["dtype"] == "f32" and k["tier"] == 0, k
    assert st["helper_redecodes"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("C", CS)
def test_one_shot(C, W, merge):
    import ctcext_amd
    P = min(3, W)
    x = _logits(C, W)
    out = ctcext_amd.ctc_ext_beam_search_decoder(x, np.full(B, T, np.int32), W, P, merge_repeated=merge)
    _assert_one_node_float(ctcext_amd.get_decoder(0).last_stats)
    compare(out, _reference(C, W, merge), P)


@pytest.mark.gpu
@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("C", CS)
def test_stream_two_pushes(C, W, merge):
    import ctcext_amd
    P = min(3, W)
    x = np.ascontiguousarray(_logits(C, W))
    with ctcext_amd.StreamDecoder(B, C, W, P, T, merge_repeated=merge) as s:
        s.push(x[:7], batch_first=False, results=False)
        out = s.push(x[7:], batch_first=False)
        _assert_one_node_float(s.last_stats)
    compare(out, _reference(C, W, merge), P)


@pytest.mark.gpu
@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("C", CS)
def test_dense(C, W, merge):
    import torch

    import ctcext_amd
    from test_gpu_dense import PAD, _assert_dense, to_dense
    P = min(3, W)
    x = _logits(C, W)
    sl = np.full(B, T, np.int32)
    out = ctcext_amd.decode_dense(torch.as_tensor(np.ascontiguousarray(x), device=DEV), torch.as_tensor(sl, device=DEV),
                                  W, P, batch_first=False, pad_value=PAD, merge_repeated=merge)
    _assert_dense(out, to_dense(_reference(C, W, merge), B, P, T, PAD))
    st = ctcext_amd.dense_check()
    k = st["kernel"]
    assert k["launched"] and k["RN"] == 1 and k["dtype"] == "f32" and k["tier"] == 0, k
