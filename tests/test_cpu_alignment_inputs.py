"""The inputs of test_gpu_alignment_ties and of the new target-scores cases do
what they exist for -- conditions on the inputs and on the definition's own
values, checked without a GPU, never on the code under test: every tie case
ties, in the band and at the label states its name promises, and tells each of
the three single-comparison mutants of the definition (>= for >) from the
definition itself; the masked cases keep their planted row feasible and walk
past -inf states; the nonfinite cases are NaN exactly where the definition
says.  Prints the counts per case."""
import numpy as np
import pytest

import oracle
import path_alignments_util as pau
import path_scores_util as psu
import test_gpu_alignment_ties as ties
import test_gpu_target_scores as tgs
import tie_inputs


@pytest.mark.parametrize("kind", ["flat", "grid_hot", "onehot", "sticky", "masked"])
def test_align_variant_is_the_definition(kind):
    """With all three comparisons strict, align_variant is path_alignments_util.align, alignment and bits."""
    c = ties.case("forced-seg-L15-" + kind) if kind in tie_inputs.TIE_FAMILIES else \
        ties.case("forced-blank5-sticky" if kind == "sticky" else "forced-masked-L15")
    rows = 0
    for b, fr in enumerate(c["sl"]):
        xb = np.ascontiguousarray(c["x"][:fr, b])
        norm = oracle.row_norm(xb) if fr else np.zeros((0,), xb.dtype)
        for i in range(c["n"].shape[1]):
            if 0 <= c["n"][b, i] <= c["y"].shape[2]:
                row = [int(v) for v in c["y"][b, i, :c["n"][b, i]]]
                a, logp = pau.align(xb, norm, row, int(fr), c["blank"], -1)
                a2, logp2, _ = tie_inputs.align_variant(xb, norm, row, int(fr), c["blank"])
                assert a == a2 and np.array([logp]).tobytes() == np.array([logp2]).tobytes()
                rows += 1
    assert rows > 20


@pytest.mark.parametrize("name", list(ties.TIE_CASES))
def test_tie_case_ties_where_it_says_and_separates_the_mutants(name):
    c = ties.case(name)   # (asserts an aligned and an unaligned row)
    cs = tie_inputs.census(c["x"], c["sl"], c["y"], c["n"], c["blank"])
    meant = ties.MEANT_FOR.get(name, tuple(tie_inputs.MUTANTS))
    print("%s: %d aligned rows, %d finite in-band ties, %d end-state ties, rows changed by >= in %s" % (
        name, cs["aligned"], cs["ties"], cs["end_ties"], ", ".join("%s: %d" % kv for kv in cs["separates"].items())))
    for k in meant:
        assert cs["separates"][k] >= 1, (name, k, cs["separates"])
    missing = [j for j in c["edges"] if j not in cs["labels"]]
    assert not missing, (name, "no finite in-band tie at the label states of", missing)


@pytest.mark.parametrize("name", [k for k in ties.PLANTED if "masked" in k] + ["both-masked-L63"])
def test_masked_case_walks_past_minus_infinity(name):
    c = ties.case(name) if name in ties.PLANTED else dict(tie_inputs.planted_case(name, "masked", 63, 12))
    if "want" not in c:
        c["want"] = ties.expected(c["x"], c["sl"], c["y"], c["n"])
    logp = c["want"]["logp"]
    assert np.isfinite(logp[:, -1]).all(), name                       # the planted rows are aligned
    fits = (c["n"][:, :-1] >= 0) & (c["n"][:, :-1] <= np.minimum(c["sl"][:, None], c["y"].shape[2]))
    assert (np.isneginf(logp[:, :-1]) & fits).any(), name             # a row of the lists whose every alignment passes a -inf
    siblings = 0
    for b, fr in enumerate(c["sl"]):
        xb, info = np.ascontiguousarray(c["x"][:fr, b]), {}
        tie_inputs.align_variant(xb, oracle.row_norm(xb), c["planted"][b], int(fr), c["blank"], maps=info)
        siblings += len(info["sibling"])
    print("%s: %d walked states beside a -inf source, %d -inf and %d aligned rows" % (
        name, siblings, np.isneginf(logp).sum(), np.isfinite(logp).sum()))
    assert siblings >= 1, name


@pytest.mark.parametrize("name", [k for k in ties.PLANTED if "nonfinite" in k])
def test_nonfinite_case_is_nan_where_the_definition_says(name):
    c = ties.case(name)
    logp, x = c["want"]["logp"], c["x"]
    assert np.isfinite(logp[0, -1]) and np.isfinite(x[:, 0]).all()    # item 0 is clean
    # The marked frame's normaliser is NaN and with it every lp of the frame.  From the middle or the last frame that NaN
    # reaches every state the band holds, and logp is NaN.  At frame 0 only states 0 and 1 get it: a comparison with a NaN
    # is false, so no later state ever takes a value from them, and a row of one label or more ends at -inf.
    edge = "edges" in name
    assert all(len(row) >= 1 for row in c["planted"])
    assert np.isnan(logp[2, -1]) and (np.isneginf if edge else np.isnan)(logp[[1, 3], -1]).all(), (name, logp[:, -1])
    assert np.isnan(x[:, 1]).sum() == 1 and np.isposinf(x[:, 2]).sum() == 1 and np.isneginf(x[:, 3]).all(axis=1).sum() == 1
    for b in (1, 2, 3):
        fr = int(c["sl"][b])
        f = int(np.nonzero(~np.isfinite(x[:fr, b]).all(axis=1))[0][0])
        assert f == ((0, fr - 1, 0)[b - 1] if edge else fr // 2), (name, b, f)
    print("%s: %d NaN, %d -inf and %d aligned rows" % (name, np.isnan(logp).sum(), np.isneginf(logp).sum(),
                                                       np.isfinite(logp).sum()))


def test_new_target_score_cases_and_their_error_constant():
    """E_NEW is the largest |definition in the compute dtype with numpy's logaddexp - the same in longdouble| over
    the finite cells of the new target-scores cases, held from both sides; the masked ones hold a -inf row that fits
    its frames, the nonfinite ones NaN items."""
    worst = {np.float32: (0.0, None), np.float64: (0.0, None)}
    for name in tgs.NEW_CASES:
        c = tgs.new_case(name)
        want, ft = c["want"], c["x"].dtype.type
        plain = tgs.expected(c["x"], c["sl"], c["y"], c["n"], ftype=ft, blank=c["blank"])
        for mask in (np.isnan, np.isneginf, np.isposinf):
            np.testing.assert_array_equal(mask(plain), mask(want), err_msg=name)
        fin = np.isfinite(want)
        err = float(np.abs(plain[fin].astype(np.longdouble) - want[fin]).max())
        if err > worst[ft][0]:
            worst[ft] = (err, name)
        if "masked" in name:
            fits = (c["n"] >= 0) & (c["n"] <= np.minimum(c["sl"][:, None], c["y"].shape[2]))
            assert (np.isneginf(want) & fits).any() and np.isfinite(want[:, -1]).all(), name
        if "nonfinite" in name:
            assert np.isnan(want[1:]).all() and np.isfinite(want[0, -1]), name
    for ft, (err, name) in worst.items():
        print("E_NEW %s: %.5g on %s (constant %.5g)" % (ft.__name__, err, name, tgs.E_NEW[ft]))
        assert 0.98 * tgs.E_NEW[ft] <= err <= tgs.E_NEW[ft], (ft, err, name)
