"""Shared by the blank-frame-skipping tests: the definition restated in Python
(include/ctcext.h, "Blank-frame skipping") over the oracle -- skip_plan on
oracle.row_norm, the compaction, oracle.raw_decode of the kept frames,
skip_expand, oracle.pack_sparse -- and the expected outputs in the shapes the
entry points return them."""
import collections
import math

import numpy as np

import oracle

THR = math.log(0.9)


def skip_plan(logp_blank, n, thr):
    """The normative definition, verbatim."""
    dom = [logp_blank[t] > thr for t in range(n)]
    return [t for t in range(n) if not (t > 0 and dom[t] and dom[t - 1])]


def skip_expand(ali_c, kmap, n, blank_label):
    """The normative definition, verbatim."""
    L = len(ali_c)
    if L == 0: return []
    k = kmap[len(kmap) - L:]
    row = [blank_label] * (n - k[0])
    for v, f in zip(ali_c, k): row[f - k[0]] = v
    return row


def logp_blank(x, blank_index=0):
    """x[t, b, blank_index] - norm[t, b] in x's dtype, norm the oracle's normaliser: [T, B]."""
    T, B, C = x.shape
    norm = oracle.row_norm(x.reshape(T * B, C)).reshape(T, B)
    with np.errstate(invalid="ignore"):
        lp = x[:, :, blank_index] - norm
    assert lp.dtype == x.dtype
    return lp


def median_threshold(x, sl, blank_index=0):
    """The median of the blank's log-probability over the items' frames: a
    threshold at which about half the frames of any input are blank-dominant,
    so that runs of them exist whatever the family."""
    lp = logp_blank(x, blank_index)
    return float(np.median(np.concatenate([lp[:max(int(n), 0), b] for b, n in enumerate(sl)])))


def plan(x, sl, thr, blank_index=0):
    """kmap per item (lists) of float32 / float64 logits x [T, B, C] and lengths sl."""
    lp = logp_blank(x, blank_index)
    t = x.dtype.type(thr)   # converted once to the compute dtype
    return [skip_plan(lp[:, b], max(int(sl[b]), 0), t) for b in range(x.shape[1])]


def compact(x, kmaps):
    """The tensor that holds item b's frames kmap_b, and their counts."""
    xc = np.zeros_like(x)
    for b, k in enumerate(kmaps):
        xc[:len(k), b] = x[k, b]
    return xc, np.array([len(k) for k in kmaps], np.int32)


Expected = collections.namedtuple("Expected", ["kmaps", "kept", "dec", "ali", "log_prob", "sparse"])


def expected(x, sl, W, P, thr, **kw):
    """The definition's outputs for x / sl: the kept frames, the rows dec[b][p]
    and (expanded) ali[b][p], log_probability and the seven sparse outputs."""
    sl = np.asarray(sl, np.int32)
    B = x.shape[1]
    kmaps = plan(x, sl, thr, kw.get("blank_index", 0))
    xc, slc = compact(x, kmaps)
    dec, ali_c, lp, _ = oracle.raw_decode(xc, slc, W, P, **kw)
    bl = kw.get("blank_label", -1)
    ali = [[skip_expand(ali_c[b][p], kmaps[b], max(int(sl[b]), 0), bl) for p in range(P)] for b in range(B)]
    di, dv, ds = oracle.pack_sparse(dec, B, P)
    ai, av, ash = oracle.pack_sparse(ali, B, P)
    return Expected(kmaps, slc, dec, ali, lp, oracle.OracleOutput(di, dv, ds, ai, av, ash, lp))


def to_dense(e, B, P, T, pad):
    """Expected as the padded tensors of DenseDecode (without status)."""
    dec = np.full((B, P, T), pad, np.int64)
    ali = np.full((B, P, T), pad, np.int64)
    dl = np.zeros((B, P), np.int32)
    al = np.zeros((B, P), np.int32)
    for b in range(B):
        for p in range(P):
            d, a = e.dec[b][p], e.ali[b][p]
            dec[b, p, :len(d)] = d
            ali[b, p, :len(a)] = a
            dl[b, p], al[b, p] = len(d), len(a)
    return dec, dl, ali, al, np.asarray(e.log_prob)


def lengths(T, B):
    """Ragged lengths, as the token-times tests'."""
    return np.array([T] + [max(T - 1 - 2 * b, 0) for b in range(1, B)], np.int32)


def dropped_share(e, sl):
    frames = int(np.maximum(np.asarray(sl), 0).sum())
    return (frames - int(e.kept.sum())) / max(frames, 1)
