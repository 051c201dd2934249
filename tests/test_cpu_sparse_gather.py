"""Host restatement of the small-C scored helper's gather (ctcx_decode.hip), as
two pure functions over the same inputs:

  gather_one_pass   gather_small_scored: every scanned offer is scored, then
                    the wanted ones are compacted into the chunk; the
                    turn-start lane comes from the step's lanes (b0, lbr, lpos)
  gather_two_pass   gather_small_sparse: pass 1 filters each 64-offer step and
                    stages (branch, child, label) words, pass 2 scores the
                    staged entries once per chunk; the turn-start lane comes
                    from a ballot of run starts over the staged entries

Both walk the frame's offers from (i0, li0) as the helper's chunk loop does
(help_gather_scored: chunk after chunk until an empty chunk or a closed turn;
one_step: the frame's first chunk is one dense scan step, in either form) and
must return the same chunks: entries, order, turn-start lanes, span start,
resume point and gstop.  The lanes of a step are simulated one by one, with
the ballots, ranks and broadcasts of the kernel.
"""
import functools

import numpy as np
import pytest

NI = np.float32(-np.inf)


def _lanes(nb, Cm1, blank, i0, li0):
    """The 64 lanes of one scan step: (v, i, li, l) per lane."""
    out = []
    for lane in range(64):
        x = li0 + lane
        q = x // Cm1
        iv = i0 + q
        v = iv < nb
        i = iv if v else i0
        li = x - q * Cm1 if v else 0
        out.append((v, i, li, li + (1 if li >= blank else 0)))
    return out


def _score(st, i, l):
    p = st["row"][l]
    return np.float32(p + (st["bob"][i] if l == st["lab"][i] else st["bt"][i]))


def _filter_step(st, bottom, i0, li0, cqn, cov):
    """What both forms share per step: the lanes, the wanted mask after the
    closed-turn and chunk-fills rules, the offers passed over, gstop."""
    nb, Cm1, blank = st["nb"], st["C"] - 1, st["blank"]
    lanes = _lanes(nb, Cm1, blank, i0, li0)
    s = [_score(st, i, l) for (v, i, li, l) in lanes]
    cw = [st["child"].get((i, l), -1) if v else -1 for (v, i, li, l) in lanes]
    brk = [v and li == 0 and not (st["bt"][i] > bottom) for (v, i, li, l) in lanes]
    kb = brk.index(True) if any(brk) else 64
    want = [lanes[k][0] and (bool(s[k] > bottom) or cw[k] >= 0) and k < kb for k in range(64)]
    rank = [sum(want[:k]) for k in range(64)]
    room = 64 - cqn
    gstop = False
    if sum(want) > room:
        want = [want[k] and rank[k] < room for k in range(64)]
        adv = max(k for k in range(64) if want[k]) + 1
        cov.add("fills mid-step")
    else:
        adv = kb
        if kb < 64:
            gstop = True
            cov.add("gstop lane 0" if kb == 0 else "gstop mid-step")
        if sum(want) == room:
            cov.add("fills exactly")
    for k in range(64):
        if want[k] and cw[k] >= 0 and not s[k] > bottom:
            cov.add("re-offer below bottom")
    return lanes, s, cw, want, rank, adv, gstop


def _advance(Cm1, i0, li0, adv):
    xa = li0 + adv
    return i0 + xa // Cm1, xa % Cm1


def _chunk_one_pass(st, bottom, i0, li0, one_step, cov):
    nb, Cm1 = st["nb"], st["C"] - 1
    sp_i0, sp_mid = i0, li0 != 0
    ent, gstop = [], False
    lbr, lpos = -1, 0
    while len(ent) < 64 and i0 < nb:
        cqn = len(ent)
        lanes, s, cw, want, rank, adv, gstop = _filter_step(st, bottom, i0, li0, cqn, cov)
        cov.add("steps")
        tls = []
        for k, (v, i, li, l) in enumerate(lanes):
            b0 = k - li if k > li else 0
            tl = lpos if i == lbr else cqn + sum(want[:b0])
            tls.append(tl)
            if want[k]:
                assert cqn + rank[k] == len(ent)
                ent.append((i, cw[k], l, s[k], st["bt"][i], -1 if (sp_mid and i == sp_i0) else tl))
        if any(want):
            last = max(k for k in range(64) if want[k])
            lbr, lpos = lanes[last][1], tls[last]
        i0, li0 = _advance(Cm1, i0, li0, adv)
        if gstop or (one_step and ent):
            break
    return ent, gstop, i0, li0


def _chunk_two_pass(st, bottom, i0, li0, cov):
    nb, Cm1 = st["nb"], st["C"] - 1
    sp_i0, sp_mid = i0, li0 != 0
    staged, gstop = [], False   # pass 1: (branch, child, label) words
    while len(staged) < 64 and i0 < nb:
        lanes, s, cw, want, rank, adv, gstop = _filter_step(st, bottom, i0, li0, len(staged), cov)
        base = len(staged)
        for k, (v, i, li, l) in enumerate(lanes):
            if want[k]:
                assert base + rank[k] == len(staged)
                staged.append((i, cw[k], l))
        i0, li0 = _advance(Cm1, i0, li0, adv)
        if gstop:
            break
    # pass 2: lane r scores the r-th staged entry; run starts by ballot
    start = [r == 0 or staged[r - 1][0] != staged[r][0] for r in range(len(staged))]
    ent = []
    for r, (i, cw, l) in enumerate(staged):
        tl = max(k for k in range(r + 1) if start[k])
        ent.append((i, cw, l, _score(st, i, l), st["bt"][i], -1 if (sp_mid and i == sp_i0) else tl))
    return ent, gstop, i0, li0


def _gather(st, bottom, i0, li0, one_step, two_pass, cov):
    chunks = []
    for c in range(10 ** 6):
        s_i0, s_l0 = i0, li0
        if two_pass and not (one_step and c == 0):
            ent, gstop, i0, li0 = _chunk_two_pass(st, bottom, i0, li0, cov)
        else:
            ent, gstop, i0, li0 = _chunk_one_pass(st, bottom, i0, li0, one_step and c == 0, cov)
        chunks.append(dict(entries=ent, span=(s_i0, s_l0), resume=(i0, li0), gstop=gstop))
        if not ent or gstop:
            break
    return chunks


def gather_one_pass(st, bottom, i0, li0, one_step, cov=None):
    return _gather(st, bottom, i0, li0, one_step, False, set() if cov is None else cov)


def gather_two_pass(st, bottom, i0, li0, one_step, cov=None):
    return _gather(st, bottom, i0, li0, one_step, True, set() if cov is None else cov)


def _state(rng, Cm1, blank_at, nb):
    C = Cm1 + 1
    blank = {"first": 0, "middle": C // 2, "last": C - 1}[blank_at]
    row = rng.standard_normal(C).astype(np.float32)
    row = (row - np.float32(np.log(np.exp(row.astype(np.float64)).sum()))).astype(np.float32)
    bt = -np.sort(np.abs(rng.standard_normal(nb)) * 3).astype(np.float32)   # the beam in descending order
    bob = (bt - np.abs(rng.standard_normal(nb)).astype(np.float32)).astype(np.float32)
    bob[rng.random(nb) < 0.2] = NI
    labels = [l for l in range(C) if l != blank]
    lab = np.asarray([labels[int(rng.integers(len(labels)))] if rng.random() < 0.9 else -1 for _ in range(nb)])
    child = {}
    for i in range(nb):
        for l in labels:
            if rng.random() < 0.06:
                child[(i, l)] = int(rng.integers(nb))
    return dict(nb=nb, C=C, blank=blank, row=row, bt=bt, bob=bob, lab=lab, child=child)


def _bottom(st, density):
    if density >= 1.0:
        return NI
    s = [_score(st, i, l) for i in range(st["nb"]) for l in range(st["C"]) if l != st["blank"]]
    return np.float32(np.quantile(np.asarray(s, np.float64), 1.0 - density))


DENSITIES = [0.02, 0.1, 0.3, 0.6, 1.0]
CM1 = [1, 2, 28, 63]
BLANKS = ["first", "middle", "last"]


@functools.lru_cache(maxsize=None)
def _run_cases(Cm1, blank_at):
    """Runs the seeded cases of one (alphabet, blank position), asserting the
    two forms equal on each; returns the edges they reached (run once, shared)."""
    rng = np.random.default_rng(4100 + 10 * Cm1 + BLANKS.index(blank_at))
    cov = set()
    for density in DENSITIES:
        for rep in range(3):
            nb = int(rng.integers(2, 129)) if rep else 128
            st = _state(rng, Cm1, blank_at, nb)
            bottom = _bottom(st, density)
            starts = [(0, 0), (int(rng.integers(nb)), 0)]
            if Cm1 > 1:
                starts.append((int(rng.integers(nb)), int(rng.integers(1, Cm1))))
                cov.add("span starts mid-branch")
            # a closed turn on lane 0: a span that starts at the first closed branch
            closed = [i for i in range(nb) if not st["bt"][i] > bottom]
            if closed:
                starts.append((closed[0], 0))
            for (i0, li0) in starts:
                for one_step in (False, True):
                    c1, c2 = set(), set()
                    a = gather_one_pass(st, bottom, i0, li0, one_step, c1)
                    b = gather_two_pass(st, bottom, i0, li0, one_step, c2)
                    assert len(a) == len(b), (density, nb, i0, li0, one_step)
                    for k, (ca, cb) in enumerate(zip(a, b)):
                        assert ca["entries"] == cb["entries"], (density, nb, i0, li0, one_step, k)
                        assert ca["span"] == cb["span"] and ca["resume"] == cb["resume"], (k, ca, cb)
                        assert ca["gstop"] == cb["gstop"], (k, ca, cb)
                    cov |= c1
                    # the measured density of the scan (wanted per scanned offer)
                    taken = sum(len(c["entries"]) for c in a)
                    scanned = (a[-1]["resume"][0] - i0) * Cm1 + a[-1]["resume"][1] - li0
                    if scanned >= 64:
                        d = taken / scanned
                        cov.add("sparse" if d <= 0.05 else "dense" if d >= 0.99 else "between")
    return frozenset(cov)


@pytest.mark.parametrize("blank_at", BLANKS)
@pytest.mark.parametrize("Cm1", CM1)
def test_two_pass_equals_one_pass(Cm1, blank_at):
    _run_cases(Cm1, blank_at)


def test_cases_cover_the_edges():
    """The seeded cases reach every edge the two forms could differ at."""
    COVERED = {(Cm1, b): _run_cases(Cm1, b) for Cm1 in CM1 for b in BLANKS}
    everything = set().union(*COVERED.values())
    for edge in ("fills exactly", "fills mid-step", "gstop lane 0", "gstop mid-step", "span starts mid-branch",
                 "re-offer below bottom", "sparse", "dense", "between"):
        assert edge in everything, (edge, sorted(everything))
    # ... and each alphabet size on its own reaches the fill and stop rules
    for Cm1 in CM1:
        got = set().union(*(COVERED[(Cm1, b)] for b in BLANKS))
        for edge in ("fills mid-step", "gstop mid-step", "re-offer below bottom"):
            assert edge in got, (Cm1, edge, sorted(got))


def test_turn_start_lane_by_hand():
    # C - 1 = 2, three branches, everything wanted: entries (0,l1) (0,l2) (1,l1) ...
    st = dict(nb=3, C=3, blank=0, row=np.zeros(3, np.float32), bt=np.asarray([0, -1, -2], np.float32),
              bob=np.full(3, NI), lab=np.asarray([-1, -1, -1]), child={})
    for f in (gather_one_pass, gather_two_pass):
        (c,) = f(st, NI, 0, 1, False)[:1]
        # the span starts mid-branch: branch 0's offer has no turn start in this chunk
        assert [(e[0], e[2], e[5]) for e in c["entries"]] == [(0, 2, -1), (1, 1, 1), (1, 2, 1), (2, 1, 3), (2, 2, 3)]
        # (no turn closed: the step passes over all 64 of its offers, beyond the last branch)
        assert c["span"] == (0, 1) and c["resume"] == (32, 1) and not c["gstop"]
