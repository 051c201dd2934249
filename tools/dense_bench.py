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

With --paths, instead: the path-scores kernels (dense_path_scores) on the same
two inputs, beside the decode kernel, the whole call, and the token-scores and
pack kernels of the same run.

With --align, instead: the path-alignment kernels (dense_path_alignments with
times and scores) on the same two inputs: the forward, walk back, emit,
token-times and token-scores launches, beside the path-scores kernels of the
same run and inputs, the decode kernel and the whole call.

With --greedy, instead: the greedy decode (decode_greedy) on the same two
inputs: its per-row kernel and its collapse under CTCEXT_FLAG_PROFILE and the
whole call (events around it), beside the beam call of the same run
(decode_dense, W and P of cfg3): its normaliser kernel -- the same read and the
same class-order chain as the per-row kernel -- and its whole call.

With --talign, instead: the target-alignments kernel (dense_target_alignments)
at cfg3 on Gaussian and peaky logits, with the times alone and with scores and
alignment rows, beside the target-scores kernel on the same targets and its own
gathered route, in alternating rounds.

With --transcripts, instead: the transcript-alignments kernel
(dense_transcript_alignments) at cfg3 on Gaussian and peaky logits, each item's
target its own greedy-decoded row, with the times alone and with scores and
alignment rows, beside dense_path_alignments(times=True, scores=True) on the
same rows (its five launches together), in alternating rounds; then the
Gaussian rows cut to 255, 511 and 1023 labels, so that every K is timed.

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


def paths_report(args):
    """--paths: one row per input family at cfg3."""
    B, T, C, W, P = SHAPES["cfg3"]
    dec = ctcext_amd.get_decoder(0)
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    lines = ["%-10s %12s %12s %12s %12s %12s %8s %11s   (median of %d, ms; cfg3 B=%d T=%d C=%d W=%d P=%d)"
             % ("inputs", "path scores", "token scores", "pack kernel", "decode", "whole call", "ps/dec", "labels/row",
                args.runs, B, T, C, W, P)]
    res = {"runs": args.runs, "shape": [B, T, C, W, P], "paths": {}}
    for kind in ("gaussian", "peaky"):
        x = times_inputs(kind, T, B, C)
        ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, token_scores=True, **KW)   # warm-up: workspace, kernels
        ctcext_amd.dense_token_scores()
        ctcext_amd.dense_path_scores()
        ctcext_amd.dense_check()
        ps_ms, sc_ms, pack_ms, dec_ms, call_ms = [], [], [], [], []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE,
                                          token_scores=True, **KW)
            ctcext_amd.dense_token_scores()
            ps = ctcext_amd.dense_path_scores()
            e1.record()
            e1.synchronize()
            dec_ms.append(ctcext_amd.dense_check()["decode_kernel_ms"])
            ms = ctypes.c_double()
            for fn, acc in ((dec.lib.ctcext_dense_path_scores_ms, ps_ms), (dec.lib.ctcext_dense_token_scores_ms, sc_ms),
                            (dec.lib.ctcext_dense_pack_ms, pack_ms)):
                if fn(dec.handle, ctypes.byref(ms)) != _lib.CTCEXT_OK:
                    raise SystemExit(dec.lib.ctcext_last_error().decode())
                acc.append(ms.value)
            call_ms.append(e0.elapsed_time(e1))
        lens = out.decoded_lengths.float()
        ratio = statistics.median(ps_ms) / statistics.median(dec_ms)
        lines.append("%-10s %12.4f %12.4f %12.4f %12.3f %12.3f %8.4f %5d..%-5d"
                     % (kind, statistics.median(ps_ms), statistics.median(sc_ms), statistics.median(pack_ms),
                        statistics.median(dec_ms), statistics.median(call_ms), ratio, int(lens.min()), int(lens.max())))
        res["paths"][kind] = {"path_scores": stat(ps_ms), "token_scores": stat(sc_ms), "pack": stat(pack_ms),
                              "decode": stat(dec_ms), "call": stat(call_ms), "paths_over_decode": round(ratio, 4),
                              "labels_min": int(lens.min()), "labels_max": int(lens.max()),
                              "finite": int(torch.isfinite(ps).sum()), "rows": B * P}
    return lines, res


def align_report(args):
    """--align: one row per input family at cfg3."""
    B, T, C, W, P = SHAPES["cfg3"]
    dec = ctcext_amd.get_decoder(0)
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    names = ("forward", "walk_back", "emit", "token_times", "token_scores")
    lines = ["%-10s %9s %9s %9s %9s %9s %11s %10s %11s %8s   (median of %d, ms; cfg3 B=%d T=%d C=%d W=%d P=%d)"
             % (("inputs",) + tuple(n[:9] for n in names) + ("path scores", "decode", "whole call", "all/call", args.runs,
                                                             B, T, C, W, P))]
    res = {"runs": args.runs, "shape": [B, T, C, W, P],
           "workspace_row_bytes": int(dec.lib.ctcext_path_alignments_row_bytes(T)), "align": {}}
    for kind in ("gaussian", "peaky"):
        x = times_inputs(kind, T, B, C)
        ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, token_scores=True, **KW)   # warm-up: workspaces, kernels
        ctcext_amd.dense_path_scores()
        ctcext_amd.dense_path_alignments(scores=True)
        ctcext_amd.dense_check()
        parts, ps_ms, dec_ms, call_ms = [[] for _ in names], [], [], []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True, **KW)
            ctcext_amd.dense_path_scores()
            pa = ctcext_amd.dense_path_alignments(scores=True)
            e1.record()
            e1.synchronize()
            dec_ms.append(ctcext_amd.dense_check()["decode_kernel_ms"])
            ms, five = ctypes.c_double(), (ctypes.c_double * 5)()
            if dec.lib.ctcext_dense_path_scores_ms(dec.handle, ctypes.byref(ms)) != _lib.CTCEXT_OK or \
                    dec.lib.ctcext_dense_path_alignments_ms(dec.handle, five) != _lib.CTCEXT_OK:
                raise SystemExit(dec.lib.ctcext_last_error().decode())
            ps_ms.append(ms.value)
            for acc, v in zip(parts, five):
                acc.append(v)
            call_ms.append(e0.elapsed_time(e1))
        total = sum(statistics.median(v) for v in parts)
        share = total / statistics.median(call_ms)
        lines.append("%-10s %9.4f %9.4f %9.4f %9.4f %9.4f %11.4f %10.3f %11.3f %8.4f"
                     % ((kind,) + tuple(statistics.median(v) for v in parts)
                        + (statistics.median(ps_ms), statistics.median(dec_ms), statistics.median(call_ms), share)))
        res["align"][kind] = dict({n: stat(v) for n, v in zip(names, parts)}, path_scores=stat(ps_ms), decode=stat(dec_ms),
                                  call=stat(call_ms), all_over_call=round(share, 4),
                                  aligned=int((pa.alignment_lengths > 0).sum()), rows=B * P)
    return lines, res


def greedy_report(args):
    """--greedy: one row per input family at cfg3."""
    B, T, C, W, P = SHAPES["cfg3"]
    dec = ctcext_amd.get_decoder(0)
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    lines = ["%-10s %10s %10s %11s %10s %8s %9s %11s %10s   (median of %d, ms; cfg3 B=%d T=%d C=%d; beam W=%d P=%d)"
             % ("inputs", "frames", "collapse", "greedy call", "beam norm", "fr/norm", "read GB/s", "beam call", "labels/row",
                args.runs, B, T, C, W, P)]
    res = {"runs": args.runs, "shape": [B, T, C, W, P], "logit_bytes": 4 * B * T * C, "sum_chain_adds": T, "greedy": {}}

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for kind in ("gaussian", "peaky"):
        x = times_inputs(kind, T, B, C)
        ctcext_amd.decode_greedy(x, sl, batch_first=False, **KW)   # warm-up: workspaces, kernels
        ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, **KW)
        ctcext_amd.dense_check()
        fr_ms, co_ms, call_ms, norm_ms, beam_ms = [], [], [], [], []
        for _ in range(args.runs):   # alternating
            ms, out = timed(lambda: ctcext_amd.decode_greedy(x, sl, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, **KW))
            call_ms.append(ms)
            two = (ctypes.c_double * 2)()
            if dec.lib.ctcext_greedy_ms(dec.handle, two) != _lib.CTCEXT_OK:
                raise SystemExit(dec.lib.ctcext_last_error().decode())
            fr_ms.append(two[0])
            co_ms.append(two[1])
            ctcext_amd.dense_check()
            ms, _ = timed(lambda: ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, **KW))
            beam_ms.append(ms)
            norm_ms.append(ctcext_amd.dense_check()["norm_kernel_ms"])
        lens = out.decoded_lengths.float()
        ratio = statistics.median(fr_ms) / statistics.median(norm_ms)
        gbs = res["logit_bytes"] / statistics.median(fr_ms) / 1e6
        lines.append("%-10s %10.4f %10.4f %11.4f %10.4f %8.3f %9.1f %11.3f %4d..%-5d"
                     % (kind, statistics.median(fr_ms), statistics.median(co_ms), statistics.median(call_ms),
                        statistics.median(norm_ms), ratio, gbs, statistics.median(beam_ms), int(lens.min()), int(lens.max())))
        res["greedy"][kind] = {"frames": stat(fr_ms), "collapse": stat(co_ms), "call": stat(call_ms),
                               "beam_norm": stat(norm_ms), "beam_call": stat(beam_ms), "frames_over_norm": round(ratio, 3),
                               "read_gb_per_s": round(gbs, 1), "labels_min": int(lens.min()), "labels_max": int(lens.max())}
    return lines, res


def targets_report(args):
    """--targets: the packed route against the per-row route (CTCEXT_TARGETS=rows) of the same targets at cfg3,
    alternating pairs; the kernels' own time by device events (ctcext_dense_target_scores_ms)."""
    B, T, C, W, P = SHAPES["cfg3"]
    dec = ctcext_amd.get_decoder(0)
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    x = times_inputs("gaussian", T, B, C)
    rng = np.random.default_rng(20261126)
    lines = ["%-22s %6s %10s %10s %8s %12s %12s %9s   (median of %d alternating pairs, ms; cfg3 B=%d T=%d C=%d)"
             % ("targets", "route", "packed", "per-row", "gain", "greedy call", "whole call", "share", args.runs, B, T, C)]
    res = {"runs": args.runs, "shape": [B, T, C], "targets": {}}

    def once(y, n, rows):
        if rows:
            os.environ["CTCEXT_TARGETS"] = "rows"
        else:
            os.environ.pop("CTCEXT_TARGETS", None)
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        ctcext_amd.decode_greedy(x, sl, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True, **KW)
        e[1].record()
        out = ctcext_amd.dense_target_scores(y, n)
        e[2].record()
        e[2].synchronize()
        ms, route = ctypes.c_double(), ctypes.c_int32()
        if dec.lib.ctcext_dense_target_scores_ms(dec.handle, ctypes.byref(ms)) != _lib.CTCEXT_OK or \
                dec.lib.ctcext_dense_target_scores_route(dec.handle, ctypes.byref(route)) != _lib.CTCEXT_OK:
            raise SystemExit(dec.lib.ctcext_last_error().decode())
        return ms.value, route.value, e[0].elapsed_time(e[1]), e[0].elapsed_time(e[2]), out

    for name, N, lo, hi, shared in (("64 x 4..15", 64, 4, 15, False), ("64 x 4..15 shared", 64, 4, 15, True),
                                    ("8 x 200", 8, 200, 200, False)):
        shape = (N, hi) if shared else (B, N, hi)
        y = torch.as_tensor(rng.integers(1, C, size=shape), device="cuda:0")
        n = torch.as_tensor(rng.integers(lo, hi + 1, size=shape[:-1]).astype(np.int32), device="cuda:0")
        for rows in (False, True):   # warm-up: kernels
            once(y, n, rows)
        packed, per_row, gains, greedy, call = [], [], [], [], []
        for _ in range(args.runs):   # alternating pairs
            a, route, g, c, out_a = once(y, n, False)
            b, _, _, _, out_b = once(y, n, True)
            packed.append(a); per_row.append(b); gains.append(1 - a / b); greedy.append(g); call.append(c)
        os.environ.pop("CTCEXT_TARGETS", None)
        diff = float((out_a.double() - out_b.double()).abs().max())
        share = statistics.median(packed) / statistics.median(call)
        lines.append("%-22s %6d %10.4f %10.4f %7.1f%% %12.4f %12.4f %9.4f   gain per pair: %s; max |packed - per-row| %.3g"
                     % (name, route, statistics.median(packed), statistics.median(per_row), 100 * statistics.median(gains),
                        statistics.median(greedy), statistics.median(call), share,
                        " ".join("%.1f%%" % (100 * v) for v in gains), diff))
        res["targets"][name] = {"route": route, "packed": stat(packed), "per_row": stat(per_row),
                                "gain_per_pair": [round(v, 4) for v in gains], "greedy_call": stat(greedy),
                                "call": stat(call), "kernel_share_of_call": round(share, 4), "max_abs_diff": diff,
                                "finite": int(torch.isfinite(out_a).sum()), "rows": B * N}
    return lines, res


def talign_report(args):
    """--talign: the target-alignments kernel at cfg3 (times alone, and with scores and alignment rows) beside the
    target-scores kernel on the same targets, and against its own gathered route (CTCEXT_TARGETS=gathered), in
    alternating pairs; the kernels' own time by device events (ctcext_dense_target_*_ms).  The per-row route of the
    issue's pairs does not exist yet, so those pairs are not timed."""
    B, T, C, W, P = SHAPES["cfg3"]
    dec = ctcext_amd.get_decoder(0)
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    rng = np.random.default_rng(20261126)
    lines = ["%-10s %-12s %10s %10s %10s %10s %9s %9s   (median of %d alternating pairs, ms; cfg3 B=%d T=%d C=%d)"
             % ("inputs", "targets", "times", "all", "gathered", "scores-k", "t/scores", "t/gath", args.runs, B, T, C)]
    res = {"runs": args.runs, "shape": [B, T, C], "talign": {}}

    def once(x, y, n, what):
        os.environ.pop("CTCEXT_TARGETS", None)
        if what == "gathered":
            os.environ["CTCEXT_TARGETS"] = "gathered"
        torch.cuda.synchronize()
        ctcext_amd.decode_greedy(x, sl, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True, **KW)
        ms = ctypes.c_double()
        if what == "scores-k":
            out = ctcext_amd.dense_target_scores(y, n)
            rc = dec.lib.ctcext_dense_target_scores_ms(dec.handle, ctypes.byref(ms))
        else:
            out = ctcext_amd.dense_target_alignments(y, n, scores=what == "all", alignment=what == "all")
            rc = dec.lib.ctcext_dense_target_alignments_ms(dec.handle, ctypes.byref(ms))
        os.environ.pop("CTCEXT_TARGETS", None)
        if rc != _lib.CTCEXT_OK:
            raise SystemExit(dec.lib.ctcext_last_error().decode())
        return ms.value, out

    kinds = ("times", "all", "gathered", "scores-k")
    for inputs in ("gaussian", "peaky"):
        x = times_inputs(inputs, T, B, C)
        for name, N, lo, hi in (("16 x 4..15", 16, 4, 15), ("4 x 40..60", 4, 40, 60), ("64 x 4..15", 64, 4, 15)):
            y = torch.as_tensor(rng.integers(1, C, size=(B, N, hi)), device="cuda:0")
            n = torch.as_tensor(rng.integers(lo, hi + 1, size=(B, N)).astype(np.int32), device="cuda:0")
            for k in kinds:   # warm-up: kernels, the decision words
                once(x, y, n, k)
            t = {k: [] for k in kinds}
            outs = {}
            for _ in range(args.runs):   # alternating
                for k in kinds:
                    v, outs[k] = once(x, y, n, k)
                    t[k].append(v)
            a, g = outs["times"], outs["gathered"]
            same = bool(torch.equal(a.logp, g.logp) and torch.equal(a.times.start, g.times.start) and
                        torch.equal(a.times.end, g.times.end))
            med = {k: statistics.median(v) for k, v in t.items()}
            lines.append("%-10s %-12s %10.4f %10.4f %10.4f %10.4f %9.2f %9.2f   staged == gathered: %s; aligned %d of %d"
                         % (inputs, name, med["times"], med["all"], med["gathered"], med["scores-k"],
                            med["times"] / med["scores-k"], med["times"] / med["gathered"], same,
                            int((a.logp > -np.inf).sum()), B * N))
            res["talign"]["%s %s" % (inputs, name)] = dict({k: stat(v) for k, v in t.items()}, routes_identical=same,
                                                          workspace_bytes=int(dec.lib.ctcext_target_alignments_bytes(B, N, hi, T)))
    return lines, res


def transcripts_report(args):
    """--transcripts: the transcript-alignments kernel at cfg3, one target per item (its own greedy row), beside the
    path-alignment kernels on the same rows, in alternating rounds; the kernels' own time by device events
    (ctcext_dense_transcript_alignments_ms, ctcext_dense_path_alignments_ms).  Rows cut short have no yardstick:
    the path alignments take only the rows the decode returned."""
    B, T, C, W, P = SHAPES["cfg3"]
    dec = ctcext_amd.get_decoder(0)
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    lines = ["%-10s %-12s %3s %10s %10s %10s %8s %8s   (median of %d alternating rounds, ms; cfg3 B=%d T=%d C=%d, N=1)"
             % ("inputs", "labels", "K", "times", "all", "path-align", "t/path", "all/path", args.runs, B, T, C)]
    res = {"runs": args.runs, "shape": [B, T, C], "transcripts": {}}

    def once(x, y, n, what):
        torch.cuda.synchronize()
        ctcext_amd.decode_greedy(x, sl, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True)
        ms, five = ctypes.c_double(), (ctypes.c_double * 5)()
        if what == "path-align":
            out = ctcext_amd.dense_path_alignments(times=True, scores=True)
            rc = dec.lib.ctcext_dense_path_alignments_ms(dec.handle, five)
            ms.value = sum(five)
        else:
            out = ctcext_amd.dense_transcript_alignments(y, n, scores=what == "all", alignment=what == "all")
            rc = dec.lib.ctcext_dense_transcript_alignments_ms(dec.handle, ctypes.byref(ms))
        if rc != _lib.CTCEXT_OK:
            raise SystemExit(dec.lib.ctcext_last_error().decode())
        return ms.value, out

    for inputs, caps in (("gaussian", (None, 255, 511, 1023)), ("peaky", (None,))):
        x = times_inputs(inputs, T, B, C)
        g = ctcext_amd.decode_greedy(x, sl, batch_first=False, token_scores=True)
        torch.cuda.synchronize()
        for cap in caps:
            L = min(int(g.decoded_lengths.max()), cap or T)
            y, n = g.decoded[:, :, :L].contiguous(), g.decoded_lengths.clamp(max=L)
            kinds = ("times", "all") + (() if cap else ("path-align",))
            for k in kinds:   # warm-up: kernels, the decision words
                once(x, y, n, k)
            t, outs = {k: [] for k in kinds}, {}
            for _ in range(args.runs):   # alternating
                for k in kinds:
                    v, outs[k] = once(x, y, n, k)
                    t[k].append(v)
            med = {k: statistics.median(v) for k, v in t.items()}
            a, pa = outs["all"], outs.get("path-align")
            eq = lambda u, v: bool(torch.equal(u.isnan(), v.isnan()) and torch.equal(u.nan_to_num(), v.nan_to_num()))
            same = pa is None or (eq(a.logp, pa.logp) and torch.equal(a.times.start, pa.times.start[..., :L]) and
                                  torch.equal(a.times.end, pa.times.end[..., :L]) and
                                  eq(a.scores.logp_sum, pa.scores.logp_sum[..., :L]) and
                                  eq(a.scores.logp_min, pa.scores.logp_min[..., :L]))   # (cells past a row's labels are NaN)
            K = next(k for k in (1, 2, 4, 8) if 256 * k > L)
            yard = ("%10.4f %8.2f %8.2f" % (med["path-align"], med["times"] / med["path-align"], med["all"] / med["path-align"])
                    if pa is not None else "%10s %8s %8s" % ("-", "-", "-"))
            lines.append("%-10s %4d..%-6d %3d %10.4f %10.4f %s   equal to the path alignments: %s; aligned %d of %d"
                         % (inputs, int(n.min()), int(n.max()), K, med["times"], med["all"], yard,
                            same if pa is not None else "-", int((a.logp > -np.inf).sum()), B))
            res["transcripts"]["%s L=%d" % (inputs, L)] = dict(
                {k: stat(v) for k, v in t.items()}, K=K, equal=same,
                workspace_bytes=int(dec.lib.ctcext_transcript_alignments_bytes(B, 1, L, T)),
                path_alignments_workspace_bytes=int(dec.lib.ctcext_path_alignments_row_bytes(T)) * B)
    return lines, res


def prefixes_report(args):
    """--prefixes: the prefix scores' two kernels (device events: ctcext_dense_prefix_scores_ms) beside the whole
    score_prefixes call, 16 prefixes of 20 to 60 labels an item, at cfg3 and at B=32 T=750 C=5000, for both layouts
    (CTCEXT_PREFIX) and with the per-row forward (CTCEXT_TARGETS=rows); a sweep of class counts for the layouts' switch; and what a
    caller had before: dense_target_scores over the N * (C - 1) extended rows at the cfg3 shape."""
    dec = ctcext_amd.get_decoder(0)
    rng = np.random.default_rng(20261126)
    N, lo, hi = 16, 20, 60
    res = {"runs": args.runs, "prefixes": [N, lo, hi], "shapes": {}}
    lines = ["%-26s %7s %7s %10s %10s %12s   (median of %d runs, ms; %d prefixes of %d..%d labels an item)"
             % ("shape", "layout", "forward", "tails", "reduce", "whole call", args.runs, N, lo, hi)]

    def once(x, sl, y, n, layout=None, forward=None):
        for k, v in (("CTCEXT_PREFIX", layout), ("CTCEXT_TARGETS", forward)):
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        ctcext_amd.decode_greedy(x, sl, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True, **KW)
        out = ctcext_amd.dense_prefix_scores(y, n)
        e[1].record()
        e[1].synchronize()
        a, b = ctypes.c_double(), ctypes.c_double()
        if dec.lib.ctcext_dense_prefix_scores_ms(dec.handle, ctypes.byref(a), ctypes.byref(b)) != _lib.CTCEXT_OK:
            raise SystemExit(dec.lib.ctcext_last_error().decode())
        return a.value, b.value, e[0].elapsed_time(e[1]), out

    def inputs(B, T, C):
        x = times_inputs("gaussian", T, B, C)
        sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
        y = torch.as_tensor(rng.integers(1, C, size=(B, N, hi)), device="cuda:0")
        n = torch.as_tensor(rng.integers(lo, hi + 1, size=(B, N)).astype(np.int32), device="cuda:0")
        return x, sl, y, n

    def row(name, data, layout, forward=None):
        once(*data, layout, forward)   # warm-up
        runs = [once(*data, layout, forward)[:3] for _ in range(args.runs)]
        t, r, c = (statistics.median(v) for v in zip(*runs))
        lines.append("%-26s %7s %7s %10.4f %10.4f %12.4f" % (name, layout or "default", forward or "packed", t, r, c))
        return {"tails": stat([v[0] for v in runs]), "reduce": stat([v[1] for v in runs]), "call": stat([v[2] for v in runs])}

    B3, T3, C3 = SHAPES["cfg3"][:3]
    for name, (B, T, C) in (("cfg3", (B3, T3, C3)), ("B32-T750-C5000", (32, 750, 5000))):
        data = inputs(B, T, C)
        tag = "%s B=%d T=%d C=%d" % (name, B, T, C)
        res["shapes"][name] = {"default": row(tag, data, None), "rows": row(tag, data, None, "rows")}
        for layout in ("narrow", "wide"):
            res["shapes"][name][layout] = row(tag, data, layout)
        if name == "cfg3":   # the nearest thing before: every g.c as a whole transcript, N * (C - 1) rows of up to 61 labels
            x, sl, y, n = data
            ext = torch.zeros((B, N, C - 1, hi + 1), dtype=torch.int64, device="cuda:0")
            ext[:, :, :, :hi] = y[:, :, None, :]
            ext.scatter_(3, n.long()[:, :, None, None].expand(B, N, C - 1, 1),
                         torch.arange(1, C, device="cuda:0")[None, None, :, None].expand(B, N, C - 1, 1))
            ye, ne = ext.reshape(B, N * (C - 1), hi + 1), (n + 1)[:, :, None].expand(B, N, C - 1).reshape(B, -1).contiguous()
            ms, v = [], ctypes.c_double()
            for _ in range(args.runs + 1):
                ctcext_amd.decode_greedy(x, sl, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True, **KW)
                ctcext_amd.dense_target_scores(ye, ne)
                if dec.lib.ctcext_dense_target_scores_ms(dec.handle, ctypes.byref(v)) != _lib.CTCEXT_OK:
                    raise SystemExit(dec.lib.ctcext_last_error().decode())
                ms.append(v.value)
            lines.append("%-26s dense_target_scores over %d extended rows an item: %.4f ms" % (tag, N * (C - 1), statistics.median(ms[1:])))
            res["shapes"][name]["target_scores_extended"] = stat(ms[1:])
    for C in (29, 64, 96, 128, 192, 256, 512):   # the layouts' switch, at cfg3's batch and frames
        data = inputs(B3, T3, C)
        res["shapes"]["switch-C%d" % C] = {k: row("switch B=%d T=%d C=%d" % (B3, T3, C), data, k) for k in ("narrow", "wide")}
    for k in ("CTCEXT_PREFIX", "CTCEXT_TARGETS"):
        os.environ.pop(k, None)
    return lines, res


def tgrads_report(args):
    """--tgrads: the target gradients at cfg3 over the --targets workload (64 targets of 4 to 15 labels an item):
    the launches' time by device events (ctcext_dense_target_grads_ms), with smaller tiles (CTCEXT_TGRADS_TILE) and
    the forward alone (CTCEXT_TGRADS=forward); dense_target_scores on the same rows in the same session; and
    torch's own ctc_loss backward over the same (item, target) pairs flattened to a batch (another normaliser:
    informative only)."""
    B, T, C, W, P = SHAPES["cfg3"]
    N, lo, hi = 64, 4, 15
    dec = ctcext_amd.get_decoder(0)
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    x = times_inputs("gaussian", T, B, C)
    rng = np.random.default_rng(20261126)
    y = torch.as_tensor(rng.integers(1, C, size=(B, N, hi)), device="cuda:0")
    n = torch.as_tensor(rng.integers(lo, hi + 1, size=(B, N)).astype(np.int32), device="cuda:0")
    w = torch.as_tensor(rng.uniform(-1, 1, size=(B, N)).astype(np.float32), device="cuda:0")

    def once(env, scores_only=False):
        for k in ("CTCEXT_TGRADS", "CTCEXT_TGRADS_TILE"):
            os.environ.pop(k, None)
        os.environ.update(env)
        ctcext_amd.decode_greedy(x, sl, batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE, token_scores=True, **KW)
        ms = ctypes.c_double()
        if scores_only:
            ctcext_amd.dense_target_scores(y, n)
            rc = dec.lib.ctcext_dense_target_scores_ms(dec.handle, ctypes.byref(ms))
        else:
            ctcext_amd.dense_target_grads(y, n, w)
            rc = dec.lib.ctcext_dense_target_grads_ms(dec.handle, ctypes.byref(ms))
        if rc != _lib.CTCEXT_OK:
            raise SystemExit(dec.lib.ctcext_last_error().decode())
        return ms.value

    lines = ["%-34s %10s   (median of %d runs after a warm-up, ms; cfg3 B=%d T=%d C=%d, %d targets of %d..%d labels an item)"
             % ("what", "kernels", args.runs, B, T, C, N, lo, hi)]
    res = {"runs": args.runs, "shape": [B, T, C], "targets": [N, lo, hi], "rows": {}}
    for name, env, so in (("target gradients (tile 16)", {}, False), ("target gradients, tile 8", {"CTCEXT_TGRADS_TILE": "8"}, False),
                          ("target gradients, tile 4", {"CTCEXT_TGRADS_TILE": "4"}, False),
                          ("forward with checkpoints alone", {"CTCEXT_TGRADS": "forward"}, False),
                          ("dense_target_scores, same rows", {}, True)):
        once(env, so)
        runs = [once(env, so) for _ in range(args.runs)]
        lines.append("%-34s %10.4f" % (name, statistics.median(runs)))
        res["rows"][name] = stat(runs)
    for k in ("CTCEXT_TGRADS", "CTCEXT_TGRADS_TILE"):
        os.environ.pop(k, None)
    # what a caller had before: torch's loss over the B * N pairs as a batch, its backward timed by device events
    lp = torch.log_softmax(x, 2).repeat_interleave(N, dim=1).requires_grad_()
    runs = []
    for _ in range(args.runs + 1):
        loss = torch.nn.functional.ctc_loss(lp, y.reshape(B * N, hi), sl.long().repeat_interleave(N), n.reshape(-1).long(),
                                            blank=0, reduction="sum")
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        loss.backward()
        e[1].record()
        e[1].synchronize()
        runs.append(e[0].elapsed_time(e[1]))
        lp.grad = None
    lines.append("%-34s %10.4f" % ("torch ctc_loss backward, %d pairs" % (B * N), statistics.median(runs[1:])))
    res["rows"]["torch_ctc_loss_backward"] = stat(runs[1:])
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
    ap.add_argument("--paths", action="store_true",
                    help="the path-scores kernels' cost at cfg3, beside the decode, token-scores and pack kernels' of the same run")
    ap.add_argument("--greedy", action="store_true",
                    help="the greedy decode's two kernels at cfg3, beside the beam call's normaliser kernel of the same run")
    ap.add_argument("--align", action="store_true",
                    help="the path-alignment kernels' cost at cfg3, beside the path-scores kernels' of the same run")
    ap.add_argument("--targets", action="store_true",
                    help="the target-scores kernel at cfg3: the packed route against the per-row route of the same targets")
    ap.add_argument("--talign", action="store_true",
                    help="the target-alignments kernel at cfg3 beside the target-scores kernel and its own gathered route")
    ap.add_argument("--transcripts", action="store_true",
                    help="the transcript-alignments kernel at cfg3 beside the path-alignment kernels on the same rows")
    ap.add_argument("--prefixes", action="store_true",
                    help="the prefix-scores kernels at cfg3 and at B=32 T=750 C=5000: layouts, G, and the target scores of the extended rows")
    ap.add_argument("--tgrads", action="store_true",
                    help="the target-gradients kernel at cfg3 beside the target scores of the same rows and torch's ctc_loss backward")
    args = ap.parse_args()
    if args.tgrads or args.times or args.prefixes or args.scores or args.paths or args.align or args.greedy or args.targets or args.talign or args.transcripts:
        lines, res = tgrads_report(args) if args.tgrads else prefixes_report(args) if args.prefixes else transcripts_report(args) if args.transcripts else talign_report(args) if args.talign else targets_report(args) if args.targets else greedy_report(args) if args.greedy else align_report(args) if args.align else paths_report(args) if args.paths else scores_report(args) if args.scores else times_report(args)
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
