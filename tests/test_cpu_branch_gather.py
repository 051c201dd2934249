"""Host restatement of the small-C scored helper's branch-per-lane filter
(ctcx_decode.hip gather_small_branch, CTCX_SPARSE_BRANCH), as a third pure
function beside the two of test_cpu_sparse_gather.py:

  gather_branch     pass 1 with one branch per lane: lane b of window w holds
                    branch 64 * w + b and builds the mask of its wanted label
                    indices; popcounts and a prefix over the lanes place the
                    wanted offers in the chunk; the resume point comes from the
                    linear offer index.  Pass 2 is gather_two_pass's.

It must return the same chunks as gather_two_pass (entries, order, turn-start
lanes, span start, resume point and gstop), which test_cpu_sparse_gather.py
ties to the one-pass form.  The lanes of a window are simulated one by one,
with the kernel's ballots, prefix, takes and resume arithmetic.
"""
import functools

import numpy as np
import pytest

from test_cpu_sparse_gather import NI, _bottom, _chunk_one_pass, _score, _state, gather_two_pass


def _lowmask(n):
    return 0 if n <= 0 else (1 << 64) - 1 if n >= 64 else (1 << n) - 1


def _frame_state(st):
    """sq_br_load: what a lane holds per branch for the whole frame."""
    C, blank = st["C"], st["blank"]
    out = []
    for i in range(st["nb"]):
        bl = int(st["lab"][i])
        own = 0 <= bl < C and bl != blank
        cm = 0
        for (pi, l) in st["child"]:
            if pi == i:
                cm |= 1 << (l - (1 if l > blank else 0))
        out.append(dict(bt=st["bt"][i], li=bl - (1 if bl > blank else 0) if own else -1,
                        sl=np.float32(st["row"][bl if own else 0] + st["bob"][i]), cm=cm))
    return out


def _window(st, fs, w, bottom, i0, li0):
    """sq_br_window: the 64 lanes' wanted masks, the span's start and the first
    closed turn applied; kbr its lane (64: none)."""
    nb, Cm1, blank = st["nb"], st["C"] - 1, st["blank"]
    M, closed = [], []
    for lane in range(64):
        i = 64 * w + lane
        v = i0 <= i < nb
        m = 0
        if v:
            b = fs[i]
            for li in range(Cm1):
                l = li + (1 if li >= blank else 0)
                if np.float32(st["row"][l] + b["bt"]) > bottom:
                    m |= 1 << li
            if b["li"] >= 0:
                m = (m & ~(1 << b["li"])) | ((1 << b["li"]) if b["sl"] > bottom else 0)
            m |= b["cm"]
            if i == i0:
                m &= ~_lowmask(li0)
        M.append(m)
        closed.append(v and not (fs[i]["bt"] > bottom) and (i > i0 or li0 == 0))
    kbr = closed.index(True) if any(closed) else 64
    return [0 if lane >= kbr else M[lane] for lane in range(64)], kbr


def _chunk_branch(st, fs, bottom, i0, li0, cov):
    nb, Cm1, blank = st["nb"], st["C"] - 1, st["blank"]
    sp_i0, sp_mid = i0, li0 != 0
    staged, gstop = {}, False
    cqn = 0
    if i0 < nb:
        xend = (nb - i0) * Cm1
        w = i0 >> 6
        while True:
            if w > (i0 >> 6):
                cov.add("second window")
            R, kbr = _window(st, fs, w, bottom, i0, li0)
            xs = [(64 * w + lane - i0) * Cm1 for lane in range(64)]
            cnt = [bin(m).count("1") for m in R]
            inc = list(np.cumsum(cnt))
            tot, room = int(inc[63]), 64 - cqn
            last = [0] * 64
            take = [0] * 64
            for lane in range(64):
                pos = cqn + int(inc[lane]) - cnt[lane]
                t = min(max(room - (int(inc[lane]) - cnt[lane]), 0), cnt[lane])
                take[lane] = t
                i = 64 * w + lane
                for _ in range(t):
                    li = (R[lane] & -R[lane]).bit_length() - 1
                    l = li + (1 if li >= blank else 0)
                    cw = st["child"].get((i, l), -1) if (fs[i]["cm"] >> li) & 1 else -1
                    assert pos not in staged and pos < 64
                    staged[pos] = (i, cw, l)
                    R[lane] &= R[lane] - 1
                    last[lane] = li
                    pos += 1
            if tot >= room:
                L = max(lane for lane in range(64) if take[lane] > 0)
                x64 = xs[L] + last[L]
                hi = li0 + ((x64 - li0) & ~63) + 64
                more = any(R[lane] & _lowmask(hi - xs[lane]) for lane in range(64))
                xstop = xs[kbr] if kbr < 64 else hi
                if not more and kbr == 64 and 64 * (w + 1) < nb and (64 * (w + 1) - i0) * Cm1 < hi:
                    cov.add("step runs into the next window")
                    R2, kbr2 = _window(st, fs, w + 1, bottom, i0, li0)
                    more = any(R2[lane] & _lowmask(hi - (xs[lane] + 64 * Cm1)) for lane in range(64))
                    if kbr2 < 64:
                        xstop = xs[kbr2] + 64 * Cm1
                xstop = min(xstop, hi)
                cqn = 64
                if more:
                    xres = x64 + 1
                else:
                    xres, gstop = xstop, xstop < hi
                break
            cqn += tot
            if kbr < 64:
                xres, gstop = xs[kbr], True
                break
            if 64 * (w + 1) >= nb:
                xres = li0 + ((xend - li0 + 63) & ~63)
                break
            w += 1
        i0, li0 = i0 + xres // Cm1, xres % Cm1
    staged = [staged[r] for r in range(cqn)]
    # pass 2, as gather_two_pass: lane r scores the r-th staged entry; run starts by ballot
    start = [r == 0 or staged[r - 1][0] != staged[r][0] for r in range(len(staged))]
    ent = []
    for r, (i, cw, l) in enumerate(staged):
        tl = max(k for k in range(r + 1) if start[k])
        ent.append((i, cw, l, _score(st, i, l), st["bt"][i], -1 if (sp_mid and i == sp_i0) else tl))
    return ent, gstop, i0, li0


def gather_branch(st, bottom, i0, li0, one_step, cov=None):
    cov = set() if cov is None else cov
    fs = _frame_state(st)
    chunks = []
    for c in range(10 ** 6):
        s_i0, s_l0 = i0, li0
        if one_step and c == 0:   # the frame's first dense step stays the one-pass form
            ent, gstop, i0, li0 = _chunk_one_pass(st, bottom, i0, li0, True, set())
        else:
            ent, gstop, i0, li0 = _chunk_branch(st, fs, bottom, i0, li0, cov)
        chunks.append(dict(entries=ent, span=(s_i0, s_l0), resume=(i0, li0), gstop=gstop))
        if not ent or gstop:
            break
    return chunks


CM1 = [1, 2, 28, 63]
NB = [1, 63, 64, 65, 127, 128]
BLANKS = ["first", "middle", "last"]
DENSITIES = [0.02, 0.1, 0.6]


def _bottoms(st, rng):
    """From -inf to above every total: the quantiles of the frame's scores, a
    branch total itself (the closed-turn test at equality), and past the top."""
    with np.errstate(invalid="ignore"):   # (scores of -inf among the quantile's inputs)
        out = [NI] + [_bottom(st, d) for d in DENSITIES]
    out.append(np.float32(st["bt"][int(rng.integers(st["nb"]))]))
    out.append(np.float32(max(float(st["bt"].max()), float(st["row"].max() + st["bt"].max())) + 1.0))
    return out


@functools.lru_cache(maxsize=None)
def _run_cases(Cm1, blank_at):
    """The seeded cases of one (alphabet, blank position) over every beam size,
    asserting the branch form equal to the two-pass form on each; returns the
    edges reached (run once, shared)."""
    rng = np.random.default_rng(1900 + 10 * Cm1 + BLANKS.index(blank_at))
    cov = set()
    for nb in NB:
        st = _state(rng, Cm1, blank_at, nb)
        # equal totals: runs of neighbours share one (the beam stays in descending order)
        for k in range(1, nb):
            if rng.random() < 0.15:
                st["bt"][k] = st["bt"][k - 1]
        for bottom in _bottoms(st, rng):
            starts = [(0, 0), (int(rng.integers(nb)), 0)]
            if Cm1 > 1:
                starts.append((int(rng.integers(nb)), int(rng.integers(1, Cm1))))
                starts.append((0, Cm1 - 1))
                cov.add("span starts mid-branch")
            closed = [i for i in range(nb) if not st["bt"][i] > bottom]
            if closed:
                starts.append((closed[0], 0))
            for k, (i0, li0) in enumerate(starts):
                for one_step in ((False, True) if k == 0 else (False,)):
                    c2 = set()
                    a = gather_two_pass(st, bottom, i0, li0, one_step, c2)
                    b = gather_branch(st, bottom, i0, li0, one_step, cov)
                    what = (Cm1, blank_at, nb, float(bottom), i0, li0, one_step)
                    assert len(a) == len(b), what
                    for c, (ca, cb) in enumerate(zip(a, b)):
                        assert ca["entries"] == cb["entries"], (what, c)
                        assert ca["span"] == cb["span"] and ca["resume"] == cb["resume"], (what, c, ca["resume"], cb["resume"])
                        assert ca["gstop"] == cb["gstop"], (what, c)
                    cov |= c2
                    taken = sum(len(c["entries"]) for c in a)
                    scanned = (a[-1]["resume"][0] - i0) * Cm1 + a[-1]["resume"][1] - li0
                    if scanned >= 64:
                        d = taken / scanned
                        cov.add("sparse" if d <= 0.05 else "dense" if d >= 0.99 else "between")
    return frozenset(cov)


@pytest.mark.parametrize("blank_at", BLANKS)
@pytest.mark.parametrize("Cm1", CM1)
def test_branch_form_equals_two_pass(Cm1, blank_at):
    _run_cases(Cm1, blank_at)


EDGES = ("fills exactly", "fills mid-step", "gstop lane 0", "gstop mid-step", "span starts mid-branch",
         "re-offer below bottom", "sparse", "dense", "between", "second window", "step runs into the next window")


def test_cases_cover_the_edges():
    """Every edge test_cpu_sparse_gather.py collects, and the two of the window
    form: a chunk that goes on into the second window, and a chunk that fills
    in a scan step whose rest lies in the next window."""
    covered = {(Cm1, b): _run_cases(Cm1, b) for Cm1 in CM1 for b in BLANKS}
    everything = set().union(*covered.values())
    for edge in EDGES:
        assert edge in everything, (edge, sorted(everything))
    for Cm1 in CM1:
        got = set().union(*(covered[(Cm1, b)] for b in BLANKS))
        for edge in ("fills mid-step", "gstop mid-step", "re-offer below bottom", "second window"):
            assert edge in got, (Cm1, edge, sorted(got))


def test_resume_point_by_hand():
    # C - 1 = 2, three branches, everything wanted, the span starting mid-branch:
    # one scan step passes over 64 offers from (0, 1), beyond the last branch
    st = dict(nb=3, C=3, blank=0, row=np.zeros(3, np.float32), bt=np.asarray([0, -1, -2], np.float32),
              bob=np.full(3, NI), lab=np.asarray([-1, -1, -1]), child={})
    (c,) = gather_branch(st, NI, 0, 1, False)[:1]
    assert [(e[0], e[2], e[5]) for e in c["entries"]] == [(0, 2, -1), (1, 1, 1), (1, 2, 1), (2, 1, 3), (2, 2, 3)]
    assert c["span"] == (0, 1) and c["resume"] == (32, 1) and not c["gstop"]
    # branch 1 closed at a bottom between the totals: the grow ends before it
    (c,) = gather_branch(st, np.float32(-0.5), 0, 0, False)
    assert [(e[0], e[2]) for e in c["entries"]] == [(0, 1), (0, 2)]
    assert c["resume"] == (1, 0) and c["gstop"]
