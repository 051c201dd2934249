"""Shared by the token-times tests: the definition restated in Python
(include/ctcext.h, "Token times"), the input families, and the expected
tensors from the oracle's rows."""
import numpy as np

import oracle


# neg_inf inputs: the seed per (T, B, C, W, P) at which the oracle's rows, with
# merge_repeated, hold an alignment shorter than its item and an untimed token
# (picked on the CPU; test_cpu_token_times asserts it)
NEG_INF_SEEDS = {(12, 6, 5, 8, 3): 5, (30, 6, 6, 16, 3): 9}


def token_times(dec, ali, frames, blank_label, merge):
    """The normative definition, verbatim."""
    m, L, base = len(dec), len(ali), frames - len(ali)
    start, end, runs, i = [-1] * m, [-1] * m, [], 0
    while i < L:
        j = i
        while j + 1 < L and ali[j + 1] == ali[i]: j += 1
        if ali[i] != blank_label: runs.append((ali[i], base + i, base + j))
        i = j + 1
    trailing = 0
    while trailing < L and ali[L - 1 - trailing] == blank_label: trailing += 1
    j, opened = m - 1, False
    for lab, s, e in reversed(runs):
        if j < 0: break
        if opened and merge and lab == dec[j]:     # an earlier run of the same merged token
            start[j] = s; continue
        if opened: j -= 1; opened = False
        if j < 0 or lab != dec[j]: break           # first mismatch: every earlier token stays -1
        start[j] = s; end[j] = e; opened = True
    return start, end, trailing


def runs_of(ali, frames, blank_label):
    """The non-blank runs of an alignment row as (label, first frame, last frame)."""
    out, i, L, base = [], 0, len(ali), frames - len(ali)
    while i < L:
        j = i
        while j + 1 < L and ali[j + 1] == ali[i]: j += 1
        if ali[i] != blank_label: out.append((ali[i], base + i, base + j))
        i = j + 1
    return out


def family(rng, kind, T, B, C, dtype=np.float32, blank=0):
    """[T, B, C] logits.
    gaussian  standard normal;
    peaky     +8 on one class per row, the blank with p = 0.7;
    sticky    a held class gets +5 for 2..7 frames, then another;
    neg_inf   each logit -inf with p = 0.6, the blank additionally with
              p = 0.5, one finite value forced per row."""
    x = rng.standard_normal((T, B, C))
    if kind == "peaky":
        for t in range(T):
            for b in range(B):
                if rng.random() < 0.7 or C == 1:
                    c = blank
                else:
                    c = int(rng.integers(0, C - 1))
                    c += c >= blank
                x[t, b, c] += 8
    elif kind == "sticky":
        for b in range(B):
            t = 0
            while t < T:
                c, n = int(rng.integers(0, C)), int(rng.integers(2, 8))
                x[t:t + n, b, c] += 5
                t += n
    elif kind == "neg_inf":
        keep = x.copy()
        x[rng.random(x.shape) < 0.6] = -np.inf
        x[rng.random((T, B)) < 0.5, blank] = -np.inf
        forced = rng.integers(0, C, size=(T, B))
        for t in range(T):
            for b in range(B):
                x[t, b, forced[t, b]] = keep[t, b, forced[t, b]]
    elif kind != "gaussian":
        raise ValueError(kind)
    return x.astype(dtype)


def expected_from_rows(dec, ali, frames, B, P, width, blank_label, merge):
    """TokenTimes as numpy from rows dec[b][p] / ali[b][p] (lists) and
    frames[b]: (start [B, P, width], end, trailing_blank [B, P])."""
    start = np.full((B, P, width), -1, np.int32)
    end = np.full((B, P, width), -1, np.int32)
    trail = np.zeros((B, P), np.int32)
    for b in range(B):
        for p in range(P):
            s, e, t = token_times(dec[b][p], ali[b][p], int(frames[b]), blank_label, merge)
            start[b, p, :len(s)] = s
            end[b, p, :len(e)] = e
            trail[b, p] = t
    return start, end, trail


def expected(x, sl, W, P, width, **kw):
    """The oracle's rows of x / sl and their token times: (dec, ali, (start, end, trailing_blank))."""
    sl = np.asarray(sl, np.int32)
    dec, ali, _, _ = oracle.raw_decode(x, sl, W, P, **kw)
    frames = np.maximum(sl, 0)
    return dec, ali, expected_from_rows(dec, ali, frames, x.shape[1], P, width, kw.get("blank_label", -1),
                                        bool(kw.get("merge_repeated", False)))
