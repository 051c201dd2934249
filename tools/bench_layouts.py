#!/usr/bin/env python3
"""What decode_logits buys: batch-major bfloat16 device logits decoded

  (a) in place, by decode_logits, against
  (b) logits.float().transpose(0, 1).contiguous() followed by the drop-in
      ctc_ext_beam_search_decoder, the conversion inside the timed call,

at bench.py's cfg3 (B=256, T=1500, C=29, W=128) and cfg4 shard (B=128,
T=2000, C=1000, W=64) shapes, N(0,1) logits drawn on the device, every item
at full length.  Whole calls are timed with torch.cuda.Event pairs (both
functions return synchronised), the two ways alternating, after warm-up calls
of both; the medians, (a)/(b), and the pre-pass / decode kernel times of one
CTCEXT_FLAG_PROFILE call of each are printed as one JSON line per shape.
The outputs of (a) and (b) are compared once per shape.

    python tools/bench_layouts.py [--reps 7] [--warmup 2] [--shapes cfg3,cfg4]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ctc-beam-search-op_amd"))

SHAPES = {   # name: (B, T, C, beam_width, top_paths, merge_repeated): bench.py's CONFIGS
    "cfg3": (256, 1500, 29, 128, 3, True),
    "cfg4": (128, 2000, 1000, 64, 1, False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="cfg3,cfg4")
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float16"])
    args = ap.parse_args()
    import torch

    import ctcext_amd
    from ctcext_amd import _lib
    if not torch.cuda.is_available():
        sys.exit("bench_layouts: no GPU (this measures device time; there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    dec = ctcext_amd.get_decoder(0)
    for name in args.shapes.split(","):
        B, T, C, W, P, merge = SHAPES[name]
        g = torch.Generator(device=dev)
        g.manual_seed(20251015)
        logits = torch.randn((B, T, C), generator=g, device=dev, dtype=torch.float32).to(getattr(torch, args.dtype))
        sl = torch.full((B,), T, dtype=torch.int32, device=dev)
        kw = dict(merge_repeated=merge)

        def in_place(flags=0):
            return ctcext_amd.decode_logits(logits, sl, W, P, flags=flags, **kw)

        def converted(flags=0):
            return ctcext_amd.ctc_ext_beam_search_decoder(logits.float().transpose(0, 1).contiguous(), sl, W, P,
                                                          flags=flags, **kw)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(args.warmup):
            a, b = in_place(), converted()
        same = all(torch.equal(u, v) for fa, fb in zip(a[:6], b[:6]) for u, v in zip(fa, fb)) and \
            torch.equal(a.log_probability, b.log_probability)
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(in_place))
            tb.append(timed(converted))
        prof = {}
        for key, fn in (("in_place", in_place), ("converted", converted)):
            fn(_lib.CTCEXT_FLAG_PROFILE)
            st = dec.last_stats
            prof[key] = {"prepass_ms": round(st["norm_kernel_ms"], 3), "decode_ms": round(st["decode_kernel_ms"], 3),
                         "traceback_ms": round(st["traceback_ms"], 3)}
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(json.dumps({"shape": name, "B": B, "T": T, "C": C, "beam_width": W, "dtype": args.dtype,
                          "reps": args.reps, "in_place_ms": round(ma, 3), "converted_ms": round(mb, 3),
                          "in_place_over_converted": round(ma / mb, 4),
                          "in_place_ms_all": [round(v, 2) for v in ta],
                          "converted_ms_all": [round(v, 2) for v in tb],
                          "profile": prof, "outputs_equal": bool(same)}), flush=True)
        del logits, a, b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
