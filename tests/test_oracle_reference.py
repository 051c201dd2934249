"""Pins the CPU oracle to the REFERENCE decoder itself, not to a reading of it.

tests/golden/reference_cases.json holds outputs of the reference's own headers
(compiled by oracle/ref into oracle/_ref/libctc_ref.so where the reference
tree is present; tests/golden/make_reference_fixtures.py recorded them).  Here,
without the library: the oracle reproduces every recorded case in both of its
modes (labels equal, log-probabilities bit-equal, the same error messages and
no-label counts); a census, computed with the oracle alone, holds the cases to
what they exist for; and the fixtures the GPU tests trust (full_length.json,
large_vocab.json, the paper example) carry the reference's verdict, with
their stored outputs re-hashed against what the reference gave.

With the library: the reference runs its own test vector through its own
code, and a fixed-seed sweep compares the oracle with it live, item by item.
The sweep skips only where neither the library nor the reference tree exists;
a tree without the library is a failed build.

The bigram scorer is pinned the same way.  tests/golden/reference_scorer_cases.json
(group S) holds what the reference decoder gave with the driver's TableScorer
in its scorer hook (oracle/ref/ref_driver.cpp: a scorer over the reference's
default EmptyBeamState that keeps its value in a side table keyed by the state
object's address), for tables of every kind of tests/scorer_tables.py.  Both
oracle modes reproduce every case; a census holds the recorded data to what
the cases exist for, from the JSON and the regenerated tables; and with the
library a second live sweep runs random items under random tables, asserting
on every call that the side table's argument held (no lookup without a stored
value, no address re-expanded to another value), that the decoder never calls
the end hooks and that it initialises the state once per Reset.

Scope: gtl::TopN (the stand-in is the same restatement as the oracle's), the
op's validation and the SparseTensor packing stay pinned by reading
(ctc_oracle.cpp, "Pinning").
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import oracle
import reference
from parity_util import random_case
import range_inputs
import scorer_tables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_reference_fixtures as gen  # noqa: E402

FX = json.load(open(os.path.join(GOLDEN, "reference_cases.json")))
CASES = FX["cases"]
S_PATH = os.path.join(GOLDEN, "reference_scorer_cases.json")
SFX = json.load(open(S_PATH))
S_CASES = SFX["cases"]
LESS = "Less leaves in the beam search than requested."
MORE = "requested more paths than the beam width."


@functools.lru_cache(maxsize=None)
def _inputs(name):
    x, sl = gen.inputs(CASES[name]["case"])
    x.setflags(write=False)
    return x, sl


def _oracle(name, mode="shared", stats=None, **over):
    c = CASES[name]["case"]
    x, sl = _inputs(name)
    return oracle.raw_decode(x, sl, over.get("W", c["beam_width"]), over.get("P", c["top_paths"]), mode=mode,
                             stats=stats, **gen.attrs(c))


def test_fixture_is_the_generators():
    """The recorded cases are the generator's list, under the size of the
    largest fixture committed before it."""
    assert set(CASES) == set(gen.CASES)
    for name, c in gen.CASES.items():
        assert CASES[name]["case"] == json.loads(json.dumps(c)), name
    assert set(FX["reference_headers_sha256"]) == set(reference.HEADERS)
    assert os.path.getsize(os.path.join(GOLDEN, "reference_cases.json")) < \
        os.path.getsize(os.path.join(GOLDEN, "full_length.json"))
    groups = {c["case"]["group"] for c in CASES.values()}
    assert groups == {"A", "B"}
    for c in CASES.values():
        x = gen.inputs(c["case"])[0]
        assert not np.isnan(x).any() and not np.isposinf(x).any()


@pytest.mark.parametrize("mode", ["faithful", "shared"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_reproduces_reference(name, mode):
    fx = CASES[name]
    x, _ = _inputs(name)
    assert gen.sha(x) == fx["sha256"], "input stream changed"
    if fx["error"] is not None:
        with pytest.raises(oracle.OracleError) as e:
            _oracle(name, mode)
        assert str(e.value) == fx["error"]
        return
    dec, ali, lp, events = _oracle(name, mode)
    assert dec == fx["decoded"]
    assert ali == fx["alignment"]
    assert gen.hex_rows(lp) == fx["log_probability_hex"]
    assert events == fx["no_label"]


def _items(name):
    """(x of one item cut to its length, as a batch of one) per item."""
    x, sl = _inputs(name)
    return [np.ascontiguousarray(x[:max(int(n), 0), b:b + 1]) for b, n in enumerate(sl)]


def _tied_full_beam(name):
    """test_cases_have_quiet_frames_and_ties' method: some prefix of an item
    ends with W leaves of which two have bit-equal totals."""
    c = CASES[name]["case"]
    W = c["beam_width"]
    for xi in _items(name):
        for t in range(1, xi.shape[0] + 1):
            try:
                lp = oracle.raw_decode(xi[:t], [t], W, W, **gen.attrs(c))[2]
            except oracle.OracleError:   # fewer than W leaves yet
                continue
            bits = np.asarray(lp[0]).view(np.uint32 if lp.dtype == np.float32 else np.uint64)
            if len(set(bits.tolist())) < W:
                return True
    return False


def test_census():
    """Conditions on the recorded cases, computed with the oracle alone."""
    dup_items = no_label_items = 0
    for name, fx in CASES.items():
        c = fx["case"]
        if c["group"] != "B":
            continue
        for xi in _items(name):
            if xi.shape[0] == 0:
                xi = np.zeros((1, 1, c["C"]), xi.dtype)   # (max_time 0 is refused; length 0 of 1 is the item)
                n = 0
            else:
                n = xi.shape[0]
            st = {}
            try:
                events = oracle.raw_decode(xi, [n], c["beam_width"], c["top_paths"], stats=st, **gen.attrs(c))[3]
            except oracle.OracleError:
                continue
            dup_items += st["duplicate_frames"] > 0
            no_label_items += events > 0
    assert dup_items >= 10, dup_items
    assert no_label_items >= 3, no_label_items
    assert {fx["error"] for fx in CASES.values()} == {None, LESS, MORE}
    # every half-grid case the kernel routes decode at a beam above 16 (W = 40
    # to 400 at C = 8, 20 and 300, cfg3's 128 and 256) has a full beam with two
    # bit-equal totals: the kernels' tie paths get what the census says
    tied = {n: _tied_full_beam(n) for n, fx in CASES.items()
            if fx["case"]["group"] == "A" and fx["case"]["gen"] == "ties" and fx["case"]["beam_width"] > 16}
    print("tied full beams:", tied)
    assert len(tied) == 16 and all(tied.values()), tied
    # a beam that never fills: at no length does an item have W leaves
    for name in ("B_beam_never_fills", "B_beam_never_fills_ties"):
        c = CASES[name]["case"]
        for xi in _items(name):
            for t in range(1, xi.shape[0] + 1):
                with pytest.raises(oracle.OracleError, match=LESS):
                    oracle.raw_decode(xi[:t], [t], c["beam_width"], c["beam_width"], **gen.attrs(c))
    # and one that is full after its first frame
    for name in ("B_beam_fills_on_first_frame", "B_beam_fills_on_first_frame_ties"):
        c = CASES[name]["case"]
        for xi in _items(name):
            oracle.raw_decode(xi[:1], [1], c["beam_width"], c["beam_width"], **gen.attrs(c))


# ---- group C: the fixtures the GPU tests trust

def _sparse_to_lists(idx, val, B):
    out = [[] for _ in range(B)]
    for (b, _), v in zip(np.asarray(idx).reshape(-1, 2).tolist(), val):
        out[b].append(v)
    return out


def _stored_outputs(fixture, key):
    fx = json.load(open(os.path.join(GOLDEN, fixture)))[key]
    if fixture == "full_length.json":
        return fx["decoded"], fx["alignment"], fx["log_probability_hex"]
    B, P = fx["case"][2], fx["case"][5]
    per_path = [(_sparse_to_lists(fx["decoded_indices"][p], fx["decoded_values"][p], B),
                 _sparse_to_lists(fx["alignment_indices"][p], fx["alignment_values"][p], B)) for p in range(P)]
    dec = [[per_path[p][0][b] for p in range(P)] for b in range(B)]
    ali = [[per_path[p][1][b] for p in range(P)] for b in range(B)]
    return dec, ali, fx["log_probability_hex"]


def test_group_c_covers_the_trusted_fixtures():
    got = FX["group_c"]
    assert set(got) == set(gen.GROUP_C)
    full = json.load(open(os.path.join(GOLDEN, "full_length.json")))
    cfg3 = {"full_length/" + k for k in full if k.startswith("cfg3")}
    assert len(cfg3) == 2 and cfg3 <= set(got) and "paper_example" in got
    # every case of the oracle-made fixtures is verified or listed as skipped, with the reason
    import fnmatch
    for fixture in ("full_length", "large_vocab"):
        for key in json.load(open(os.path.join(GOLDEN, fixture + ".json"))):
            name = "%s/%s" % (fixture, key)
            assert name in got or any(fnmatch.fnmatch(name, pat) for pat in FX["group_c_skipped"]), name


@pytest.mark.parametrize("name", sorted(FX["group_c"]))
def test_group_c_fixture_is_the_references(name):
    """The reference gave, bit for bit, what the fixture stores (so
    test_full_length_golden compares the kernels with the reference), and the
    fixture still stores it."""
    v = FX["group_c"][name]
    assert v["matches_reference"] is True, v
    if v["fixture"] == "bench_digests.json":
        cfg = v["case"].split("_rank")[0]
        stored = json.load(open(os.path.join(GOLDEN, "bench_digests.json")))[cfg]["digests"]["0"]
        assert stored == v["reference_digest"]
    elif name != "paper_example":
        assert gen.outputs_sha256(*_stored_outputs(v["fixture"], v["case"])) == v["reference_outputs_sha256"]


# ---- group S: the reference under a table scorer

@functools.lru_cache(maxsize=None)
def _s_inputs(name):
    c = S_CASES[name]["case"]
    x, sl = gen.inputs(c)
    tab = gen.scorer_table(c)
    x.setflags(write=False)
    tab.setflags(write=False)
    return x, sl, tab


def test_scorer_fixture_is_the_generators():
    assert set(S_CASES) == set(gen.S_CASES)
    for name, c in gen.S_CASES.items():
        assert S_CASES[name]["case"] == json.loads(json.dumps(c)), name
        assert c["group"] == "S" and c["table"] in scorer_tables.KINDS + scorer_tables.SEMANTIC
    # recorded from the headers the first file was recorded from
    assert SFX["reference_headers_sha256"] == FX["reference_headers_sha256"]
    assert os.path.getsize(S_PATH) < 400 * 1000
    # the cases the file exists for: the SMALL shapes, both dtypes, the four
    # pairings; cfg3 at both beams under continuous and grid
    small = {(c["T"], c["C"], c["beam_width"], c["dtype"], c["table"], c["gen"])
             for n, c in gen.S_CASES.items() if n.startswith("S_T")}
    want = {(T, C, W, dt, tk, kind) for (T, C, W, _) in gen._SMALL for dt in ("f32", "f64")
            for tk, kind in (("continuous", "normal"), ("grid", "ties"), ("forbidden", "neg_inf"), ("extreme", "normal"))}
    assert small == want and len(want) == 56
    cfg3 = {(c["beam_width"], c["table"]) for n, c in gen.S_CASES.items() if n.startswith("S_cfg3")}
    assert cfg3 == {(W, tk) for W in (128, 256) for tk in ("continuous", "grid")}
    for n, c in gen.S_CASES.items():
        if n.startswith("S_cfg3"):
            assert (c["T"], c["C"]) == (200, 29)


@pytest.mark.parametrize("mode", ["faithful", "shared"])
@pytest.mark.parametrize("name", sorted(S_CASES))
def test_oracle_reproduces_reference_under_scorer(name, mode):
    fx = S_CASES[name]
    c = fx["case"]
    x, sl, tab = _s_inputs(name)
    assert gen.sha(x) == fx["sha256"], "input stream changed"
    assert gen.sha(tab) == fx["table_sha256"], "table stream changed"

    def run():
        return oracle.raw_decode(x, sl, c["beam_width"], c["top_paths"], mode=mode, scorer_table=tab, **gen.attrs(c))
    if fx["error"] is not None:
        with pytest.raises(oracle.OracleError) as e:
            run()
        assert str(e.value) == fx["error"]
        return
    dec, ali, lp, events = run()
    assert dec == fx["decoded"]
    assert ali == fx["alignment"]
    assert gen.hex_rows(lp) == fx["log_probability_hex"]
    assert events == fx["no_label"]


def _hooks_held(hs, inits):
    assert hs["lookups_without_state"] == 0, hs
    assert hs["reexpansions_differ"] == 0, hs
    assert hs["end_hook_calls"] == 0, hs
    assert hs["initialize_state"] == inits, (hs, inits)


def test_scorer_census():
    """Conditions on the recorded group-S data, from the JSON and the tables
    its seeds name (the duplicate-entry count alone needs the oracle)."""
    assert {fx["error"] for fx in S_CASES.values()} == {None, LESS, MORE}
    repeats = {}
    for name, fx in S_CASES.items():
        c = fx["case"]
        assert c["top_paths"] <= 50
        # the hook counters the reference reported while it recorded the case:
        # one InitializeState for the constructor's Reset and one per item
        # decoded (a failed TopPaths ends the call before its Reset)
        done = c["B"] if fx["error"] is None else None
        hs = fx["hook_stats"]
        if done is not None:
            _hooks_held(hs, done + 1)
        else:
            assert 1 <= hs["initialize_state"] <= c["B"] and hs["lookups_without_state"] == 0 \
                and hs["reexpansions_differ"] == 0 and hs["end_hook_calls"] == 0, hs
        if fx["error"] is not None:
            continue
        if c["table"] == "grid":
            # (a row of NaN, an item that -inf left no path, repeats nothing)
            rows = [[v for v in row if v != "nan"] for row in fx["log_probability_hex"]]
            repeats[name] = max(len(row) - len(set(row)) for row in rows)
        if c["table"] == "forbidden":
            assert c["merge_repeated"] is False, name
            tab = _s_inputs(name)[2]
            assert np.isneginf(tab).mean() > 0.3
            paths = [p for item in fx["decoded"] for p in item]
            assert scorer_tables.forbidden_pairs(tab, paths) == [], name
    print("grid cases, repeated log-probabilities in the fullest item:", repeats)
    assert len(repeats) >= 16 + 4 and all(n >= 1 for n in repeats.values()), repeats
    # an all-zero table is the base scorer: the recorded outputs of the group-A case
    for name, of in gen.S_ZERO_OF.items():
        a, z = CASES[of], S_CASES[name]
        assert z["sha256"] == a["sha256"] and a["error"] is None
        for k in ("decoded", "alignment", "log_probability_hex", "no_label"):
            assert z[k] == a[k], (name, k)
    # row 0 is the root's: with it all -inf only the empty path is left
    for name in ("S_root_forbidden_one_path", "S_root_forbidden_f64_blank_2"):
        fx = S_CASES[name]
        assert fx["decoded"] == [[[]]] * fx["case"]["B"], name
        assert fx["hook_stats"]["expand_state"] > 0 and fx["hook_stats"]["lookups"] > 0
    assert S_CASES["S_root_forbidden_two_paths"]["error"] == LESS
    assert S_CASES["S_root_forbidden_two_paths"]["case"]["top_paths"] == 2
    # one successor a label: every decoded path counts up modulo C, skipping
    # nothing (merge_repeated cannot hide a step: no label follows itself)
    for name in ("S_chain", "S_chain_f64_blank_3"):
        fx = S_CASES[name]
        C = fx["case"]["C"]
        for item in fx["decoded"]:
            for path in item:
                assert all(b == (a + 1) % C for a, b in zip(path, path[1:])), (name, path)
        assert any(len(path) >= 3 for item in fx["decoded"] for path in item), name
    assert any(fx["case"]["blank_index"] != 0 for fx in S_CASES.values())
    assert any(fx["case"]["beam_width"] == 1 for fx in S_CASES.values())
    assert any(fx["case"]["T"] == 1 for fx in S_CASES.values())
    assert any(0 in fx["case"]["seq_len"] for fx in S_CASES.values())
    # the duplicate-entry state under a grid table
    dup_items = 0
    for name, fx in S_CASES.items():
        c = fx["case"]
        if not name.startswith("S_duplicate_state"):
            continue
        assert c["table"] == "grid"
        x, sl, tab = _s_inputs(name)
        for b, n in enumerate(sl):
            st = {}
            oracle.raw_decode(np.ascontiguousarray(x[:n, b:b + 1]), [n], c["beam_width"], c["top_paths"], stats=st,
                              scorer_table=tab, **gen.attrs(c))
            dup_items += st["duplicate_frames"] > 0
    assert dup_items >= 4, dup_items


# ---- with the library: the reference live

def _need_reference():
    if reference.available():
        return
    if reference.tree() is None:
        pytest.skip("neither oracle/_ref/libctc_ref.so nor the reference tree is here")
    pytest.fail("the reference tree is present but oracle/_ref/libctc_ref.so is not: run build() (__graft_entry__.py)")


def test_reference_reproduces_its_own_test():
    """ctc_ext_beam_search_decoder_ops_test.py:20-100 through the reference's
    own decoder, with assertAllClose's default tolerances."""
    _need_reference()
    g = json.load(open(os.path.join(GOLDEN, "paper_example.json")))
    a = g["attrs"]
    for dtype in (np.float32, np.float64):
        x = np.log(np.asarray(g["probs"])).astype(dtype)
        dec, ali, lp, _ = reference.raw_decode(x, g["sequence_length"], a["beam_width"], a["top_paths"],
                                               a["merge_repeated"], a["blank_index"], a["blank_label"])
        for p in range(a["top_paths"]):
            assert dec[0][p] == g["decoded_values"][p]
            assert ali[0][p] == g["alignment_values"][p]
        np.testing.assert_allclose(lp, np.asarray(g["log_probability"]), rtol=1e-6, atol=1e-6)


def _both(x, sl, W, P, kw, mode, tab=None, hook_stats=None):
    res = []
    scored = {} if tab is None else dict(scorer_table=tab, hook_stats=hook_stats)
    for f in (lambda: oracle.raw_decode(x, sl, W, P, mode=mode, scorer_table=tab, **kw),
              lambda: reference.raw_decode(x, sl, W, P, **kw, **scored)):
        try:
            r = f()
            res.append((r[0], r[1], r[2].tobytes(), r[3]))
        except oracle.OracleError as e:
            res.append(str(e))
    return res


SWEEP = (("plain", {}), ("ties", dict(ties=True)), ("neg_inf", dict(neg_inf=True)),
         ("f64_ties", dict(ties=True, dtype=np.float64)), ("ties_neg_inf", dict(ties=True, neg_inf=True)),
         ("wide", dict(C_max=40, W_max=60, T_max=30)))


def test_live_sweep_oracle_against_reference():
    """About 3500 items of parity_util.random_case, one at a time so that an
    item that ends in an error hides no other: the oracle's faithful mode and
    the reference give the same labels, log-probability bits, no-label counts
    and error messages.  Then the shared mode on every range_inputs family and
    on a cfg3-shaped and a large-C item."""
    _need_reference()
    if reference.tree() is not None:
        assert reference.header_sha256() == FX["reference_headers_sha256"], \
            "the reference headers changed since reference_cases.json was recorded: rerun make_reference_fixtures.py"
    items = errors = dups = 0
    for i, (fam, kwf) in enumerate(SWEEP):
        rng = np.random.default_rng(9100 + i)
        for _ in range(300):
            x, sl, W, P, kw = random_case(rng, **kwf)
            for b in range(x.shape[1]):
                n = int(sl[b])
                xi = np.ascontiguousarray(x[:max(n, 1), b:b + 1])
                got, want = _both(xi, [n], W, P, kw, "faithful")
                assert got == want, (fam, xi.shape, W, P, kw, got, want)
                items += 1
                errors += isinstance(want, str)
                if not isinstance(want, str) and kwf.get("neg_inf"):
                    st = {}
                    oracle.raw_decode(xi, [n], W, P, stats=st, **kw)
                    dups += st["duplicate_frames"] > 0
    print("live sweep: %d items, %d ended in an error, %d reached the duplicate-entry state" % (items, errors, dups))
    assert items >= 3000 and errors >= 50 and dups >= 5, (items, errors, dups)
    for dtype in (np.float32, np.float64):
        for kind in range_inputs.FAMILIES:
            if kind == "banded" and dtype == np.float64:
                continue
            rng = range_inputs.rng_for("live/%s/%s" % (kind, np.dtype(dtype).name))
            x = range_inputs.family(rng, kind, 20, 2, 20, dtype)
            kw = dict(merge_repeated=kind in ("logsoftmax", "onehot", "huge", "peaked"), blank_index=10, blank_label=-1)
            got, want = _both(x, [20, 17], 30, 3, kw, "shared")
            assert got == want and not isinstance(want, str), (kind, dtype)
    rng = np.random.default_rng(9200)
    for (T, C, W, P) in ((400, 29, 128, 3), (40, 300, 200, 3)):
        x = rng.standard_normal((T, 1, C)).astype(np.float32)
        got, want = _both(x, [T], W, P, dict(merge_repeated=True, blank_index=0, blank_label=-1), "shared")
        assert got == want and not isinstance(want, str), (T, C, W)


def test_live_sweep_oracle_against_reference_under_scorer():
    """About 2400 items of parity_util.random_case: the families of the sweep
    above at 200 batches each to its 300, since drawing a table and looking
    up the side table make an item dearer and this sweep must take no longer
    than that one.  Each batch runs under a table of the next kind of
    scorer_tables.KINDS, its items decoded one at a time: the oracle's
    faithful mode and the reference with the
    driver's TableScorer give the same labels, log-probability bits, no-label
    counts and error messages.  On every call the hook counters show that the
    side table held: no lookup without a stored value, no address re-expanded
    to another value, no end-hook call, and one InitializeState for the
    constructor's Reset plus one per item decoded.  Then the shared mode on a
    short cfg3-shaped and a large-C item under each kind (the recorded group-S
    cases hold both modes to the full shapes)."""
    _need_reference()
    items = errors = dups = expands = 0
    by_kind = dict.fromkeys(scorer_tables.KINDS, 0)
    for i, (fam, kwf) in enumerate(SWEEP):
        rng = np.random.default_rng(9300 + i)
        for j in range(200):
            x, sl, W, P, kw = random_case(rng, **kwf)
            kind = scorer_tables.KINDS[(i + j) % 4]
            tab = scorer_tables.table(rng, kind, x.shape[2], x.dtype)
            for b in range(x.shape[1]):
                n = int(sl[b])
                xi = np.ascontiguousarray(x[:max(n, 1), b:b + 1])
                hs = {}
                got, want = _both(xi, [n], W, P, kw, "faithful", tab, hs)
                assert got == want, (fam, kind, xi.shape, W, P, kw, got, want)
                failed = isinstance(want, str)
                _hooks_held(hs, 1 if failed else 2)
                items += 1
                errors += failed
                expands += hs["expand_state"]
                by_kind[kind] += 1
                if not failed and kwf.get("neg_inf"):
                    st = {}
                    oracle.raw_decode(xi, [n], W, P, stats=st, scorer_table=tab, **kw)
                    dups += st["duplicate_frames"] > 0
    print("live scorer sweep: %d items %s, %d ended in an error, %d reached the duplicate-entry state, %d ExpandState calls"
          % (items, by_kind, errors, dups, expands))
    assert items >= 2000 and min(by_kind.values()) >= 400 and errors >= 50 and dups >= 5, (items, by_kind, errors, dups)
    rng = np.random.default_rng(9400)
    for (T, C, W, P) in ((60, 29, 128, 3), (10, 300, 100, 3)):
        for kind in scorer_tables.KINDS:
            x = rng.standard_normal((T, 1, C))
            if kind == "grid":
                x = np.round(x * 2) / 2
            x = x.astype(np.float32)
            tab = scorer_tables.table(rng, kind, C, np.float32)
            hs = {}
            got, want = _both(x, [T], W, P, dict(merge_repeated=kind != "forbidden", blank_index=0, blank_label=-1),
                              "shared", tab, hs)
            assert got == want and not isinstance(want, str), (T, C, W, kind)
            _hooks_held(hs, 2)
