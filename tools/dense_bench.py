#!/usr/bin/env python3
"""What the dense, enqueue-only decode costs and saves, at two shapes on one
box in one session: cfg3 (B=256, T=1500, C=29, W=128, P=3) and a latency
shape (B=8, T=200, same C, W, P).  Dense and synchronous calls alternate.

Per shape:
  (i)   the host time inside decode_dense (perf_counter around the call; the
        device idle before it, nothing waited for after it);
  (ii)  the time from the call to its outputs being complete: a
        torch.cuda.Event pair around the call, and the wall time from the
        call to that event's completion;
  (iii) the wall time of decode_logits(..., outputs="device"), synchronised
        before and after -- with the library given by --parent-lib (the
        parent commit's build), and with this tree's;
  (iv)  the pack kernel's own time (CTCEXT_FLAG_PROFILE runs of their own).

    python tools/dense_bench.py [--runs 5] [--parent-lib PATH] [--out FILE]

With --times, instead: the token-times kernel (dense_token_times) at cfg3, on
Gaussian and on peaky inputs (+8 on one class per row, the blank with p = 0.7):
its HIP-event time under CTCEXT_FLAG_PROFILE beside the pack kernel's of the
same run and the whole call's (events around decode_dense + dense_token_times).

With --scores, instead: the token-scores kernel (dense_token_scores) on the
same two inputs, beside the token-times and the pack kernels' of the same run.

Prints one table per shape and one JSON line.  It is a report, not a check
(it does stop if the dense outputs differ from the synchronous ones), and it
does not touch bench.py.
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ctc-beam-search-op_amd", "ctcext_amd")
sys.path.insert(0, os.path.join(ROOT, "ctc-beam-search-op_amd"))

import numpy as np   # noqa: E402
import torch         # noqa: E402

import ctcext_amd    # noqa: E402
from ctcext_amd import _lib   # noqa: E402

SHAPES = {"cfg3": (256, 1500, 29, 128, 3), "latency": (8, 200, 29, 128, 3)}
KW = dict(merge_repeated=True, blank_index=0)


def load_package_with(lib_path, name="ctcext_amd_parent"):
    """A second copy of the package bound to another libctcext.so (the
    library path is read when the package's _lib module is imported)."""
    old = os.environ.get("CTCEXT_LIB_PATH")
    os.environ["CTCEXT_LIB_PATH"] = lib_path
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "__init__.py"),
                                                      submodule_search_locations=[PKG])
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    finally:
        if old is None:
            del os.environ["CTCEXT_LIB_PATH"]
        else:
            os.environ["CTCEXT_LIB_PATH"] = old
    return mod


def sync_call(pkg, x, sl, W, P):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = pkg.decode_logits(x, sl, W, P, batch_first=False, outputs="device", **KW)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def dense_call(x, sl, W, P, flags=0):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, flags=flags, **KW)
    t1 = time.perf_counter()
    e1.record()
    e1.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, e0.elapsed_time(e1), (t2 - t0) * 1e3, out


def same(dense, ref, P):
    """The padded rows against the SparseTensor components of the synchronous call."""
    for p in range(P):
        for rows, lens, idx, val in ((dense.decoded, dense.decoded_lengths, ref.decoded_indices[p], ref.decoded_values[p]),
                                     (dense.alignment, dense.alignment_lengths, ref.alignment_indices[p],
                                      ref.alignment_values[p])):
            if int(lens[:, p].sum()) != val.numel():
                return False
            if not torch.equal(rows[idx[:, 0], p, idx[:, 1]], val):
                return False
    return torch.equal(dense.log_probability, ref.log_probability) and not bool(dense.status.any())


def times_inputs(kind, T, B, C):
    rng = np.random.default_rng(20261020)
    x = rng.standard_normal((T, B, C), dtype=np.float32)
    if kind == "peaky":
        c = np.where(rng.random((T, B)) < 0.7, 0, rng.integers(1, C, size=(T, B)))
        np.put_along_axis(x, c[..., None], np.take_along_axis(x, c[..., None], 2) + 8, 2)
    return torch.as_tensor(x, device="cuda:0")


def times_report(args):
    """--times: one row per input family at cfg3."""
    B, T, C, W, P = SHAPES["cfg3"]
    dec = ctcext_amd.get_decoder(0)
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    lines = ["%-10s %14s %14s %14s %10s   (median of %d, ms; cfg3 B=%d T=%d C=%d W=%d P=%d)"
             % ("inputs", "token times", "pack kernel", "whole call", "timed/tok", args.runs, B, T, C, W, P)]
    res = {"runs": args.runs, "shape": [B, T, C, W, P], "times": {}}
    for kind in ("gaussian", "peaky"):
        x = times_inputs(kind, T, B, C)
        ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, **KW)   # warm-up: workspace, kernels
        ctcext_amd.dense_token_times()
        ctcext_amd.dense_check()
        tt_ms, pack_ms, call_ms = [], [], []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, **KW)
            tt = ctcext_amd.dense_token_times()
            e1.record()
            e1.synchronize()
            ctcext_amd.dense_check()
            ms = ctypes.c_double()
            for fn, acc in ((dec.lib.ctcext_dense_token_times_ms, tt_ms), (dec.lib.ctcext_dense_pack_ms, pack_ms)):
                if fn(dec.handle, ctypes.byref(ms)) != _lib.CTCEXT_OK:
                    raise SystemExit(dec.lib.ctcext_last_error().decode())
                acc.append(ms.value)
            call_ms.append(e0.elapsed_time(e1))
        tokens = int(out.decoded_lengths.sum())
        timed = int((tt.start >= 0).sum())
        lines.append("%-10s %14.4f %14.4f %14.3f %5d/%-5d" % (kind, statistics.median(tt_ms), statistics.median(pack_ms),
                                                            statistics.median(call_ms), timed, tokens))
        res["times"][kind] = {"token_times": stat(tt_ms), "pack": stat(pack_ms), "call": stat(call_ms),
                              "tokens": tokens, "timed": timed, "trailing_blank_max": int(tt.trailing_blank.max())}
    return lines, res


def scores_report(args):
    """--scores: one row per input family at cfg3."""
    B, T, C, W, P = SHAPES["cfg3"]
    dec = ctcext_amd.get_decoder(0)
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    lines = ["%-10s %14s %14s %14s %14s %8s %11s   (median of %d, ms; cfg3 B=%d T=%d C=%d W=%d P=%d)"
             % ("inputs", "token scores", "token times", "pack kernel", "whole call", "sc/tt", "scored/tok", args.runs,
                B, T, C, W, P)]
    res = {"runs": args.runs, "shape": [B, T, C, W, P], "scores": {}}
    for kind in ("gaussian", "peaky"):
        x = times_inputs(kind, T, B, C)
        ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, token_scores=True, **KW)   # warm-up: workspace, kernels
        ctcext_amd.dense_token_scores()
        ctcext_amd.dense_check()
        sc_ms, tt_ms, pack_ms, call_ms = [], [], [], []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE,
                                          token_scores=True, **KW)
            tt = ctcext_amd.dense_token_times()
            sc = ctcext_amd.dense_token_scores(tt)
            e1.record()
            e1.synchronize()
            ctcext_amd.dense_check()
            ms = ctypes.c_double()
            for fn, acc in ((dec.lib.ctcext_dense_token_scores_ms, sc_ms), (dec.lib.ctcext_dense_token_times_ms, tt_ms),
                            (dec.lib.ctcext_dense_pack_ms, pack_ms)):
                if fn(dec.handle, ctypes.byref(ms)) != _lib.CTCEXT_OK:
                    raise SystemExit(dec.lib.ctcext_last_error().decode())
                acc.append(ms.value)
            call_ms.append(e0.elapsed_time(e1))
        tokens = int(out.decoded_lengths.sum())
        scored = int((~torch.isnan(sc.logp_sum)).sum())
        frames = int(((tt.end - tt.start + 1) * (tt.start >= 0)).sum())
        ratio = statistics.median(sc_ms) / statistics.median(tt_ms)
        lines.append("%-10s %14.4f %14.4f %14.4f %14.3f %8.2f %5d/%-5d"
                     % (kind, statistics.median(sc_ms), statistics.median(tt_ms), statistics.median(pack_ms),
                        statistics.median(call_ms), ratio, scored, tokens))
        res["scores"][kind] = {"token_scores": stat(sc_ms), "token_times": stat(tt_ms), "pack": stat(pack_ms),
                               "call": stat(call_ms), "scores_over_times": round(ratio, 3), "tokens": tokens,
                               "scored": scored, "span_frames": frames}
    return lines, res


def stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libctcext.so of the parent commit, for (iii)")
    ap.add_argument("--out", default=None, help="also write the tables and the JSON line here")
    ap.add_argument("--times", action="store_true", help="the token-times kernel's cost at cfg3 instead")
    ap.add_argument("--scores", action="store_true",
                    help="the token-scores kernel's cost at cfg3, beside the token-times and pack kernels' of the same run")
    args = ap.parse_args()
    if args.times or args.scores:
        lines, res = scores_report(args) if args.scores else times_report(args)
        text = "\n".join(lines) + "\n" + json.dumps(res)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    parent = load_package_with(os.path.abspath(args.parent_lib)) if args.parent_lib else None
    res = {"runs": args.runs, "parent_lib": bool(parent), "shapes": {}}
    lines = []
    for name, (B, T, C, W, P) in SHAPES.items():
        rng = np.random.default_rng(20261019)
        x = torch.as_tensor(rng.standard_normal((T, B, C), dtype=np.float32), device="cuda:0")
        sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
        pkgs = {"sync, this tree": ctcext_amd}
        if parent:
            pkgs["sync, parent lib"] = parent
        ref = None
        for pkg in pkgs.values():   # warm-up: workspace, kernels
            _, ref = sync_call(pkg, x, sl, W, P)
        *_, out = dense_call(x, sl, W, P)
        ctcext_amd.dense_check()
        if not same(out, ref, P):
            raise SystemExit("%s: the dense outputs differ from the synchronous ones" % name)
        rows = {k: [] for k in list(pkgs) + ["dense (i) host", "dense (ii) events", "dense (ii) wall"]}
        for _ in range(args.runs):   # alternating
            for k, pkg in pkgs.items():
                rows[k].append(sync_call(pkg, x, sl, W, P)[0])
            host, ev, wall, _ = dense_call(x, sl, W, P)
            rows["dense (i) host"].append(host)
            rows["dense (ii) events"].append(ev)
            rows["dense (ii) wall"].append(wall)
        rows["dense_check after completion"] = []
        rows["pack kernel (iv)"] = []
        kern = {"norm": [], "decode": [], "traceback": []}
        dec = ctcext_amd.get_decoder(0)
        for _ in range(args.runs):
            dense_call(x, sl, W, P, flags=_lib.CTCEXT_FLAG_PROFILE)
            t0 = time.perf_counter()
            st = ctcext_amd.dense_check()
            rows["dense_check after completion"].append((time.perf_counter() - t0) * 1e3)
            ms = ctypes.c_double()
            if dec.lib.ctcext_dense_pack_ms(dec.handle, ctypes.byref(ms)) != _lib.CTCEXT_OK:
                raise SystemExit(dec.lib.ctcext_last_error().decode())
            rows["pack kernel (iv)"].append(ms.value)
            kern["norm"].append(st["norm_kernel_ms"])
            kern["decode"].append(st["decode_kernel_ms"])
            kern["traceback"].append(st["traceback_ms"])
        base_key = "sync, parent lib" if parent else "sync, this tree"
        base = rows[base_key]
        spread = max(base) - min(base)
        lines.append("%-32s %10s %10s %10s" % ("%s B=%d T=%d C=%d W=%d P=%d" % (name, B, T, C, W, P), "median ms", "min",
                                                "max"))
        r = res["shapes"][name] = {"shape": [B, T, C, W, P], "rows": {}}
        for k, v in rows.items():
            lines.append("%-32s %10.3f %10.3f %10.3f" % (k, statistics.median(v), min(v), max(v)))
            r["rows"][k] = stat(v)
        r["kernels_ms"] = {k: round(statistics.median(v), 4) for k, v in kern.items()}
        r["sync_spread_ms"] = round(spread, 4)
        r["ii_minus_iii_ms"] = round(statistics.median(rows["dense (ii) events"]) - statistics.median(base), 4)
        lines.append("(iii) is '%s': spread max - min %.3f ms; (ii) events - (iii) medians %+.3f ms; kernels "
                     "(PROFILE runs, median ms) norm %.3f decode %.3f traceback %.3f"
                     % (base_key, spread, r["ii_minus_iii_ms"], r["kernels_ms"]["norm"], r["kernels_ms"]["decode"],
                        r["kernels_ms"]["traceback"]))
        lines.append("")
    text = "\n".join(lines) + "\n" + json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
