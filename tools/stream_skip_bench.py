#!/usr/bin/env python3
"""What blank-frame skipping does to a stream: one cfg3 batch (B=256, T=1500,
C=29, W=128, P=3) pushed through StreamDecoder.push_dense in three schedules --
150 x 10 and 15 x 100 frames with hypothesis outputs on the last push alone,
150 x 10 with them on every push -- each as

    (a) a plain stream,
    (b) a stream opened with skip_blank=0 (the whole skipping pipeline, no frame dropped),
    (c) a stream opened with skip_blank=log 0.9,

alternating, --runs times each, medians.  (b) - (a) is what the skipping
pipeline costs (normaliser of the caller's rows, chunk plan, gather, finish,
expansion); (c) / (a) is what dropping the frames buys on that input.  Inputs:
"peaky" (the bench's noise with 8.0 added to one class per (t, b) row, the
blank with probability 0.7) and "gaussian" (the bench's noise: no frame is
blank-dominant at log 0.9).

wall_ms is the time from the first call to the last outputs complete, nothing
waited for in between.  The phase columns come from a run of its own with
CTCEXT_FLAG_PROFILE (HIP events around prologue + pre-pass + skipping front,
decode, commit, the rest), summed over the pushes; that run checks after every
push to read the events, so its wall time is not reported.

    python tools/stream_skip_bench.py [--runs 5] [--inputs peaky,gaussian] [--out FILE]

Prints one table and one JSON line.  It is a report, not a check, and it does
not touch bench.py.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ctc-beam-search-op_amd"))

import numpy as np   # noqa: E402
import torch         # noqa: E402

import ctcext_amd    # noqa: E402
from ctcext_amd import _lib   # noqa: E402

B, T, C, W, P = 256, 1500, 29, 128, 3
KW = dict(merge_repeated=True, blank_index=0)
THR = math.log(0.9)
SCHEDULES = (("150x10 last", 10, False), ("15x100 last", 100, False), ("150x10 every", 10, True))
VARIANTS = (("plain", None), ("skip=0", 0.0), ("skip=log0.9", THR))


def inputs(kind):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((T, B, C)).astype(np.float32)
    if kind == "peaky":
        blank = rng.random((T, B)) < 0.7
        cls = np.where(blank, 0, rng.integers(1, C, size=(T, B)))
        np.add.at(x, (np.arange(T)[:, None], np.arange(B)[None, :], cls), 8.0)
    elif kind != "gaussian":
        raise ValueError(kind)
    return torch.as_tensor(x, device="cuda:0")


def run(x, chunk, every, thr, profile=False):
    """One pass over x: (wall ms, kept frames in total, phase sums in ms or None)."""
    flags = _lib.CTCEXT_FLAG_PROFILE if profile else 0
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device="cuda:0", skip_blank=thr, **KW) as s:
        s.reserve(chunk)   # opens the stream: its allocations are not timed
        phases = dict(front=0.0, decode=0.0, commit=0.0, rest=0.0) if profile else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a in range(0, T, chunk):
            b = min(a + chunk, T)
            s.push_dense(x[a:b], batch_first=False, results=every or b == T, flags=flags)
            if profile:
                st = s.check()
                phases["front"] += st["norm_kernel_ms"]
                phases["decode"] += st["decode_kernel_ms"]
                phases["commit"] += s.commit_ms()
                phases["rest"] += st["traceback_ms"]
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        s.check()
        kept = int(s.kept_frames().sum())
    return wall, kept, phases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inputs", default="peaky,gaussian")
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for kind in a.inputs.split(","):
        x = inputs(kind)
        for name, chunk, every in SCHEDULES:
            for _, thr in VARIANTS:   # warm-up: kernels loaded, allocator filled
                run(x, chunk, every, thr)
            walls = {v: [] for v, _ in VARIANTS}
            kept = {}
            for _ in range(a.runs):
                for v, thr in VARIANTS:
                    w, k, _ = run(x, chunk, every, thr)
                    walls[v].append(w)
                    kept[v] = k
            med = {v: statistics.median(w) for v, w in walls.items()}
            for v, thr in VARIANTS:
                _, _, ph = run(x, chunk, every, thr, profile=True)
                rows.append(dict(input=kind, schedule=name, variant=v, wall_ms=round(med[v], 2),
                                 wall_min=round(min(walls[v]), 2), wall_max=round(max(walls[v]), 2),
                                 kept_share=round(kept[v] / float(B * T), 4),
                                 overhead_ms=round(med[v] - med["plain"], 2), ratio=round(med[v] / med["plain"], 3),
                                 **{k: round(val, 2) for k, val in ph.items()}))
    head = ("input", "schedule", "variant", "wall_ms", "wall_min", "wall_max", "kept_share", "overhead_ms", "ratio",
            "front", "decode", "commit", "rest")
    lines = ["  ".join("%-12s" % h for h in head)]
    for r in rows:
        lines.append("  ".join("%-12s" % r[h] for h in head))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(shape=[B, T, C, W, P], runs=a.runs, rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(dict(shape=[B, T, C, W, P], runs=a.runs, rows=rows)) + "\n")


if __name__ == "__main__":
    main()
