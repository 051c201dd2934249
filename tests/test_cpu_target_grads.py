"""Target gradients without a GPU: the symbols and the header's macros, and the
host definition (target_grad_row) against the numpy definition in longdouble
and float64 autograd through torch's ctc_loss."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ctcext_amd
import tgrad_util
from ctcext_amd import _lib

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
# The largest |target_grad_row - autograd through ctc_loss(log_softmax(x))| over the finite rows of ROWS, both in
# float64, measured here: 2.22e-15 ("aa" with blank 0; the other normaliser is most of it); the bound is 4 times that.
BOUND = 4 * 2.23e-15
T, C = 6, 7
ROWS = {"empty": (), "one": (3,), "aa": (2, 2), "full": (1, 2, 3, 4, 6, 1), "infeasible": (2, 2, 2, 2)}


def test_symbols_are_exported_and_the_header_says_so(tmp_path):
    lib = _lib.load()
    for s in _lib.TARGET_GRADS_SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    (tmp_path / "abi.c").write_text('#include "ctcext.h"\nint main(void) { return (CTCEXT_HAS_TARGET_GRADS - 1) | '
                                    '(CTCEXT_ABI_VERSION - 8) | (CTCEXT_TARGET_GRADS_TILE_F32 - 16) | '
                                    '(CTCEXT_TARGET_GRADS_TILE_F64 - 8); }\n')
    subprocess.check_call(["gcc", "-I", INCLUDE, str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")])
    subprocess.check_call([str(tmp_path / "abi")])


@pytest.mark.parametrize("blank", [0, 5])
@pytest.mark.parametrize("row", list(ROWS))
def test_row_matches_numpy_longdouble_and_autograd(row, blank):
    x = np.random.default_rng(11).normal(size=(T, C)) * 2
    norm = np.logaddexp.reduce(x, axis=1)
    y = list(ROWS[row])   # (no 0 and no 5: ctc_loss takes no blank in a target)
    logp, g = ctcext_amd.target_grad_row(x, norm, y, T, blank)
    want_logp, want = tgrad_util.target_grad(x, norm, y, T, blank)
    assert g.dtype == np.float64 and g.shape == (T, C)
    if row == "infeasible":
        assert np.isneginf(logp) and np.isneginf(want_logp) and not g.any() and not want.any()
        return
    assert abs(logp - want_logp) <= BOUND * max(1, abs(want_logp))
    assert np.abs(g - want).max() <= BOUND
    xt = torch.tensor(x, requires_grad=True)
    loss = torch.nn.functional.ctc_loss(torch.log_softmax(xt, 1)[:, None], torch.tensor([y], dtype=torch.long).reshape(1, -1),
                                        torch.tensor([T]), torch.tensor([len(y)]), blank=blank, reduction="sum")
    loss.backward()
    err = np.abs(g + xt.grad.numpy()).max()
    print(row, blank, "against autograd %.3g" % err)
    assert err <= BOUND and abs(logp + loss.item()) <= BOUND * max(1, abs(logp))


def test_row_conventions():
    x = (np.random.default_rng(3).normal(size=(4, 3)) * 2).astype(np.float32)
    norm = np.logaddexp.reduce(x.astype(np.float64), axis=1).astype(np.float32)
    logp, g = ctcext_amd.target_grad_row(x, norm, (), 0, 1)   # frames == 0
    assert logp == 0 and g.shape == (0, 3) and g.dtype == np.float32
    logp, g = ctcext_amd.target_grad_row(x, norm, (3,), 4, 1)   # a label outside [0, C)
    assert np.isnan(logp) and not g.any()
    x[2, 0] = -np.inf   # a masked logit under a feasible target: zeros in its column, never NaN
    norm = np.logaddexp.reduce(x.astype(np.float64), axis=1).astype(np.float32)
    logp, g = ctcext_amd.target_grad_row(x, norm, (0,), 4, 1)
    assert np.isfinite(logp) and np.isfinite(g).all() and g[2, 0] == 0
    with pytest.raises(ctcext_amd.InvalidArgumentError):
        ctcext_amd.target_grad_row(x, norm, (), 4, 3)
