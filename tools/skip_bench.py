#!/usr/bin/env python3
"""What blank-frame skipping costs and saves at the cfg3 shape (B=256, T=1500,
C=29, W=128, P=3), on Gaussian and on peaky inputs (+8 on one class per row,
the blank with p = 0.7), on one box in one session.  Three forms of
decode_dense alternate, --runs times each, and the medians are reported:

  (a) the plain call;
  (b) skip_blank=0: nothing is dropped, so (b) - (a) is the overhead of the
      normaliser, plan, gather and expansion;
  (c) skip_blank=log 0.9.

Per form: the whole call (a torch.cuda.Event pair around it) and, from runs
with CTCEXT_FLAG_PROFILE, the HIP-event times of the pre-pass, the decode
kernel, the traceback and the pack, and for (b) and (c) of what runs in front
of the pipeline (normaliser + plan + gather) and of the expansion; the share of
frames kept, as mean and maximum over items; and the share of items whose top
path's labels equal the plain decode's.

    python tools/skip_bench.py [--runs 5] [--out FILE]

Prints one table per input family and one JSON line.  It is a report, not a
check (it does stop if (b) differs from (a) anywhere), and it does not touch
bench.py.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ctc-beam-search-op_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch         # noqa: E402

import ctcext_amd    # noqa: E402
from ctcext_amd import _lib   # noqa: E402
from dense_bench import stat, times_inputs   # noqa: E402

SHAPE = (256, 1500, 29, 128, 3)
KW = dict(merge_repeated=True, blank_index=0)
FORMS = (("(a) plain", None), ("(b) skip_blank=0", 0.0), ("(c) skip_blank=log 0.9", math.log(0.9)))


def call(x, sl, W, P, thr, flags=0):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, flags=flags, skip_blank=thr, **KW)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the tables and the JSON line here")
    args = ap.parse_args()
    B, T, C, W, P = SHAPE
    dec = ctcext_amd.get_decoder(0)
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    res = {"runs": args.runs, "shape": list(SHAPE), "inputs": {}}
    lines = []
    for kind in ("gaussian", "peaky"):
        x = times_inputs(kind, T, B, C)
        outs, kept = {}, {}
        for name, thr in FORMS:   # warm-up: workspace, kernels; the outputs compared below
            _, outs[name] = call(x, sl, W, P, thr)
            kept[name] = None if thr is None else ctcext_amd.kept_frames().cpu().numpy()
            ctcext_amd.dense_check()
        for f, a, b in zip(ctcext_amd.DenseDecode._fields, outs[FORMS[0][0]], outs[FORMS[1][0]]):
            if not torch.equal(a, b):
                raise SystemExit("%s: skip_blank=0 differs from the plain call in %s" % (kind, f))
        whole = {name: [] for name, _ in FORMS}
        kern = {name: {k: [] for k in ("prepass", "decode", "traceback", "pack", "front", "expand")} for name, _ in FORMS}
        for _ in range(args.runs):   # alternating
            for name, thr in FORMS:
                whole[name].append(call(x, sl, W, P, thr)[0])
        for _ in range(args.runs):
            for name, thr in FORMS:
                call(x, sl, W, P, thr, flags=_lib.CTCEXT_FLAG_PROFILE)
                st = ctcext_amd.dense_check()
                ms, ms2 = ctypes.c_double(), ctypes.c_double()
                if dec.lib.ctcext_dense_pack_ms(dec.handle, ctypes.byref(ms)) != _lib.CTCEXT_OK:
                    raise SystemExit(dec.lib.ctcext_last_error().decode())
                k = kern[name]
                k["prepass"].append(st["norm_kernel_ms"])
                k["decode"].append(st["decode_kernel_ms"])
                k["traceback"].append(st["traceback_ms"])
                pack = ms.value
                if thr is not None:
                    if dec.lib.ctcext_dense_skip_ms(dec.handle, ctypes.byref(ms), ctypes.byref(ms2)) != _lib.CTCEXT_OK:
                        raise SystemExit(dec.lib.ctcext_last_error().decode())
                    k["front"].append(ms.value)
                    k["expand"].append(ms2.value)
                    pack -= ms2.value   # (the pack interval starts at the traceback's end)
                k["pack"].append(pack)
        plain = outs[FORMS[0][0]]
        lines.append("%-24s %9s %9s %9s %9s %9s %9s %9s %11s %10s   (%s; median of %d, ms; B=%d T=%d C=%d W=%d P=%d)"
                     % ("", "call", "front", "prepass", "decode", "traceback", "expand", "pack", "kept mean/max",
                        "top1 same", kind, args.runs, B, T, C, W, P))
        r = res["inputs"][kind] = {}
        for name, thr in FORMS:
            o = outs[name]
            n = plain.decoded_lengths[:, 0].long()
            same = (o.decoded_lengths[:, 0] == plain.decoded_lengths[:, 0])
            cols = torch.arange(T, device=n.device)[None, :] < n[:, None]
            same &= ((o.decoded[:, 0] == plain.decoded[:, 0]) | ~cols).all(dim=1)
            share = 1.0 if kept[name] is None else kept[name] / float(T)
            mean, mx = (1.0, 1.0) if kept[name] is None else (float(share.mean()), float(share.max()))
            k = kern[name]
            med = {q: (statistics.median(v) if v else 0.0) for q, v in k.items()}
            lines.append("%-24s %9.3f %9.3f %9.3f %9.3f %9.3f %9.3f %9.3f %5.3f/%5.3f %10.4f"
                         % (name, statistics.median(whole[name]), med["front"], med["prepass"], med["decode"],
                            med["traceback"], med["expand"], med["pack"], mean, mx, float(same.float().mean())))
            r[name] = {"call": stat(whole[name]), "kernels_ms": {q: round(v, 4) for q, v in med.items()},
                       "kept_mean": round(mean, 4), "kept_max": round(mx, 4),
                       "top1_same": round(float(same.float().mean()), 4)}
        lines.append("")
    text = "\n".join(lines) + "\n" + json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
