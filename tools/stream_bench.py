#!/usr/bin/env python3
"""What streaming costs: the summed time of the pushes of one cfg3 batch
(B=256, T=1500, C=29, W=128, P=3) at several chunk sizes, beside the one-shot
decode_logits of the same tensor on the same build and box.

Every push but the last runs with results=False (no traceback, no outputs);
the last one returns the hypotheses, as the one-shot call does.  The
difference to the one-shot time is the per-push cost: the pre-pass launch,
the state image's load and store, the host synchronisation.  The 1500-frame
row is one push: the stream build of the kernel (no record ring, image saved
once) against the default one; the one-shot call is timed with and without
its record ring, since a stream writes every record.

With --stable every multi-push row is run a second time with
StreamDecoder.stable() after every push (the query's time inside the push's),
in the same session, and the row records the frames its convergence walks
visited in total (walked, summed over items and pushes).  --input chooses the
logits: "gaussian", the bench's, whose chains may never meet (the worst case:
a query walks back to its last frontier, which stays at frame 0 while they do
not); "peaky": the same noise with 8.0 added to one class per (t, b) row, the
blank with probability 0.7 and a uniformly drawn label otherwise (a confident
model: every frame's winner has probability ~0.985); or "twohot": every class
near -40 but two per row, one at 0 and one at -0.5, so that each frame is a
near-even choice between two continuations and the beam's entries are the
variants of the last few frames.  A library without the query (an older build
through CTCEXT_LIB_PATH) prints the other rows only.

With --dense every schedule is also run through the enqueue-only
StreamDecoder.push_dense: with hypothesis outputs on the last push alone (as
the rows above), with them on every push, and (10-frame pushes) as two
captured pushes replayed from a graph.  Each reports the host time inside the
calls, the wall time from the first call to the last outputs complete (the
synchronous rows' summed push times are wall times too: every push waits), and
the commit kernel's summed time from a CTCEXT_FLAG_PROFILE run of its own.

With --dense --scores every schedule is also run through a stream with a score
store (StreamDecoder(token_scores=True)), alternating round by round with the
same schedule on a stream without one, in the same session: the wall times of
both; from a CTCEXT_FLAG_PROFILE run of their own the append kernel's time per
push beside the commit kernel's of the same pushes; and the token-scores
kernel's time over the store after the last push beside the one-shot
dense_token_scores over the caller's tensor for the same rows.  --score-store
chooses the store's element type (the chunks are converted to it beforehand).

    python tools/stream_bench.py [--runs 5] [--chunks 1500,100,10] [--stable] [--dense [--times] [--scores [--score-store bfloat16]]] [--input gaussian|peaky|twohot] [--out FILE]

Prints one table and one JSON line.  It is a report, not a check, and it does
not touch bench.py.
"""
import argparse
import json
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


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def one_shot(x, sl, flags=0):
    return ctcext_amd.decode_logits(x, sl, W, P, batch_first=False, outputs="device", flags=flags, **KW)


def streamed(x, chunk, stable=False, info=None):
    with ctcext_amd.StreamDecoder(B, C, W, P, T, **KW) as s:
        s.push(x[:0], batch_first=False, results=False)   # opens the stream: its allocations are not timed
        ms = 0.0
        out = None
        walked = 0
        last = None

        def step(t0, t1):
            nonlocal walked, last
            o = s.push(x[t0:t1], batch_first=False, results=t1 == T, outputs="device")
            if stable:
                last, w = s.stable(walked=True)
                walked += int(w.sum())
            return o
        for t0 in range(0, T, chunk):
            t1 = min(t0 + chunk, T)
            dt, out = _timed(lambda: step(t0, t1))
            ms += dt
        kernel = s.last_stats["kernel"]
        if info is not None and stable:
            info["walked"] = walked
            info["decoded_length_mean"] = float(last.decoded_length.mean())
            info["stable_frames_mean"] = float(last.frames.mean())
    return ms, out, kernel


def streamed_dense(x, chunk, every, profile=False, **stream_kw):
    """The same schedule through push_dense: (host ms inside the calls, wall ms
    from the first call to the last outputs complete, the last push's outputs,
    summed commit-kernel ms of a CTCEXT_FLAG_PROFILE run).  every: hypothesis
    outputs on every push instead of on the last one alone.  A profile run
    checks after each push to read that push's events: its wall time is not a
    measurement."""
    flags = _lib.CTCEXT_FLAG_PROFILE if profile else 0
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device="cuda:0", **KW, **stream_kw) as s:
        s.reserve(chunk)   # opens the stream: its allocations are not timed
        torch.cuda.synchronize()
        host = commit = 0.0
        out = None
        w0 = time.perf_counter()
        for t0 in range(0, T, chunk):
            t1 = min(t0 + chunk, T)
            h0 = time.perf_counter()
            out = s.push_dense(x[t0:t1], batch_first=False, results=every or t1 == T, flags=flags)
            host += time.perf_counter() - h0
            if profile:
                s.check()
                commit += s.commit_ms()
        torch.cuda.synchronize()
        wall = time.perf_counter() - w0
        s.check()
    return host * 1e3, wall * 1e3, out, commit


def streamed_graph(x, chunk):
    """The schedule as two captured pushes of `chunk` frames over static
    inputs, one without hypothesis outputs replayed for every chunk but the
    last and one with them for the last: (host ms, wall ms, outputs).  The
    chunk is copied into the static tensor on the replay stream before each
    replay, inside both times."""
    side = torch.cuda.Stream(device="cuda:0")
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device="cuda:0", **KW) as s:
        s.reserve(chunk)
        xs = torch.zeros((chunk, B, C), device="cuda:0")
        torch.cuda.synchronize()
        g0, g1 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=side):
            s.push_dense(xs, batch_first=False, results=False)
        with torch.cuda.graph(g1, stream=side):
            out = s.push_dense(xs, batch_first=False, results=True)
        torch.cuda.synchronize()
        host = 0.0
        w0 = time.perf_counter()
        with torch.cuda.stream(side):
            for t0 in range(0, T, chunk):
                xs.copy_(x[t0:t0 + chunk])
                h0 = time.perf_counter()
                (g1 if t0 + chunk >= T else g0).replay()
                host += time.perf_counter() - h0
        torch.cuda.synchronize()
        wall = time.perf_counter() - w0
        s.check()
    return host * 1e3, wall * 1e3, out


def streamed_times(x, chunk):
    """--times: the schedule through push_dense with hypothesis outputs and
    token_times_dense() on every push, under CTCEXT_FLAG_PROFILE, checked after
    each push to read its events.  Returns per push (token-times kernel ms,
    traceback + pack ms, the push's kernels' ms in all), and the last outputs."""
    per = []
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device="cuda:0", **KW) as s:
        s.reserve(chunk)
        for t0 in range(0, T, chunk):
            out = s.push_dense(x[t0:min(t0 + chunk, T)], batch_first=False, flags=_lib.CTCEXT_FLAG_PROFILE)
            tt = s.token_times_dense()
            st = s.check()
            rest = st["traceback_ms"]
            per.append((s.token_times_ms(), rest,
                        st["norm_kernel_ms"] + st["decode_kernel_ms"] + s.commit_ms() + rest))
    return per, out, tt


def streamed_scores_profile(x, chunk, store):
    """One CTCEXT_FLAG_PROFILE run of the schedule on a stream with a score
    store, checked after each push to read its events: per push (append kernel
    ms, commit kernel ms), and the token-scores kernel's ms over the store after
    the last push (rows of T frames)."""
    per = []
    with ctcext_amd.StreamDecoder(B, C, W, P, T, device="cuda:0", token_scores=True, score_store=store, **KW) as s:
        s.reserve(chunk)
        for t0 in range(0, T, chunk):
            t1 = min(t0 + chunk, T)
            s.push_dense(x[t0:t1], batch_first=False, results=t1 == T, flags=_lib.CTCEXT_FLAG_PROFILE)
            if t1 == T:
                s.token_scores_dense()
            s.check()
            append_ms, scores_ms = s.scores_ms()
            per.append((append_ms, s.commit_ms()))
    return per, scores_ms


def one_shot_scores_ms(x, sl):
    """The token-scores kernel's ms of the one-shot dense decode of the same rows."""
    import ctypes
    ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, token_scores=True, flags=_lib.CTCEXT_FLAG_PROFILE, **KW)
    ctcext_amd.dense_token_scores()
    ctcext_amd.dense_check()
    dec = ctcext_amd.get_decoder(0)
    ms = ctypes.c_double()
    if dec.lib.ctcext_dense_token_scores_ms(dec.handle, ctypes.byref(ms)) != _lib.CTCEXT_OK:
        raise SystemExit("ctcext_dense_token_scores_ms: %s" % dec.lib.ctcext_last_error().decode())
    return ms.value


def scores_rows(x, sl, chunks, runs, store):
    """--scores: per chunk size, the schedule with and without a score store in
    alternating rounds, and the kernels' times of a profile run per round."""
    xs = x if store is None else x.to(getattr(torch, store))
    ref = ctcext_amd.decode_dense(xs, sl, W, P, batch_first=False, **KW)
    torch.cuda.synchronize()
    med = statistics.median
    rows = {}
    for c in chunks:
        if c >= T:
            continue
        kw = dict(token_scores=True, score_store=store)
        for fn_kw in ({}, kw):   # warm-up, and the results are the one-shot decode's
            out = streamed_dense(xs, c, False, **fn_kw)[2]
            if not all(torch.equal(a, b) for a, b in zip(out[:5], ref[:5])):
                raise SystemExit("%d-frame pushes: the result differs from the one-shot decode_dense" % c)
        plain, with_store, append, commit, scores, dense = [], [], [], [], [], []
        for _ in range(runs):
            plain.append(streamed_dense(xs, c, False)[1])
            with_store.append(streamed_dense(xs, c, False, **kw)[1])
            per, sc_ms = streamed_scores_profile(xs, c, store)
            append.append(med(p[0] for p in per))
            commit.append(med(p[1] for p in per))
            scores.append(sc_ms)
            dense.append(one_shot_scores_ms(xs, sl))
        n = -(-T // c)
        rows["%d-frame pushes" % c] = {
            "pushes": n, "wall_ms": round(med(plain), 3), "wall_store_ms": round(med(with_store), 3),
            "wall_rounds_ms": [round(v, 3) for v in plain], "wall_store_rounds_ms": [round(v, 3) for v in with_store],
            "store_ms_per_push": round((med(with_store) - med(plain)) / n, 4),
            "append_kernel_ms_per_push": round(med(append), 4), "commit_kernel_ms_per_push": round(med(commit), 4),
            "append_over_commit": round(med(append) / med(commit), 3) if med(commit) > 0 else None,
            "scores_kernel_ms": round(med(scores), 4), "one_shot_scores_kernel_ms": round(med(dense), 4)}
    return rows


def times_row(x, chunk, runs):
    streamed_times(x, chunk)   # warm-up
    got = [streamed_times(x, chunk)[0] for _ in range(runs)]
    med = lambda k, sel: round(statistics.median(sel([g[k] for g in r]) for r in got), 4)   # noqa: E731
    last, mean = (lambda v: v[-1]), (lambda v: sum(v) / len(v))
    return {"pushes": len(got[0]),
            "last_push": {"token_times_ms": med(0, last), "traceback_pack_ms": med(1, last), "push_kernels_ms": med(2, last)},
            "mean_push": {"token_times_ms": med(0, mean), "traceback_pack_ms": med(1, mean), "push_kernels_ms": med(2, mean)}}


def dense_rows(x, sl, chunks, runs):
    """--dense: name -> {host_ms, wall_ms (medians, min, max), commit_ms}."""
    ref = ctcext_amd.decode_dense(x, sl, W, P, batch_first=False, **KW)
    torch.cuda.synchronize()

    def same(out):
        return all(torch.equal(a, b) for a, b in zip(out[:5], ref[:5]))
    rows = {}
    for c in chunks:
        variants = [("dense, %d-frame pushes" % c, lambda c=c: streamed_dense(x, c, False)[:3]),
                    ("dense, %d-frame pushes, results every push" % c, lambda c=c: streamed_dense(x, c, True)[:3])]
        if c == 10 and T % c == 0:
            variants.append(("dense, %d-frame pushes, captured graph" % c, lambda c=c: streamed_graph(x, c)))
        for name, fn in variants:
            if not same(fn()[2]):   # warm-up
                raise SystemExit("%s: the result differs from the one-shot decode_dense" % name)
            got = [fn()[:2] for _ in range(runs)]
            host, wall = [g[0] for g in got], [g[1] for g in got]
            rows[name] = {"pushes": -(-T // c), "host_ms": round(statistics.median(host), 3),
                          "wall_ms": round(statistics.median(wall), 3), "wall_min_ms": round(min(wall), 3),
                          "wall_max_ms": round(max(wall), 3)}
        commit = streamed_dense(x, c, False, profile=True)[3]
        rows["dense, %d-frame pushes" % c]["commit_kernel_ms"] = round(commit, 3)
        rows["dense, %d-frame pushes" % c]["commit_kernel_ms_per_push"] = round(commit / -(-T // c), 4)
    return rows


def make_input(kind):
    rng = np.random.default_rng(20251015)
    x = rng.standard_normal((T, B, C), dtype=np.float32)
    if kind == "peaky":
        cls = np.where(rng.random((T, B)) < 0.7, KW["blank_index"], rng.integers(1, C, size=(T, B)))
        np.put_along_axis(x, cls[..., None], np.take_along_axis(x, cls[..., None], 2) + 8.0, 2)
    elif kind == "twohot":
        x -= 40.0
        c0 = rng.integers(0, C, size=(T, B))
        c1 = (c0 + rng.integers(1, C, size=(T, B))) % C
        np.put_along_axis(x, c0[..., None], 0.0, 2)
        np.put_along_axis(x, c1[..., None], -0.5, 2)
    elif kind != "gaussian":
        raise SystemExit("--input must be gaussian, peaky or twohot")
    return torch.as_tensor(x, device="cuda:0")


def _same(a, b):
    for p in range(P):
        for name in ("decoded_indices", "decoded_values", "alignment_indices", "alignment_values"):
            if not torch.equal(getattr(a, name)[p], getattr(b, name)[p]):
                return False
    return torch.equal(a.log_probability, b.log_probability)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunks", default="1500,100,10")
    ap.add_argument("--stable", action="store_true", help="also run each multi-push row with stable() after every push")
    ap.add_argument("--dense", action="store_true", help="also run each schedule through the enqueue-only push_dense")
    ap.add_argument("--input", default="gaussian", help="gaussian (the bench's logits), peaky or twohot")
    ap.add_argument("--times", action="store_true",
                    help="with --dense: a row for token_times_dense() after every push of the smallest chunk size")
    ap.add_argument("--scores", action="store_true",
                    help="with --dense: each multi-push schedule with and without a score store, and its kernels' times")
    ap.add_argument("--score-store", default=None, help="with --scores: bfloat16 or float16 (default: the compute dtype)")
    ap.add_argument("--out", default=None, help="also write the table and the JSON line here")
    args = ap.parse_args()
    chunks = [int(c) for c in args.chunks.split(",")]
    if args.scores and not args.dense:
        raise SystemExit("--scores needs --dense: a stream with a score store has the enqueue-only push alone")
    if args.scores and not hasattr(_lib.load(), "ctcext_stream_open_scores"):
        raise SystemExit("--scores: this libctcext.so has no token scores for streams (CTCEXT_HAS_STREAM_SCORES)")
    if args.score_store and not args.scores:
        raise SystemExit("--score-store needs --scores")
    x = make_input(args.input)
    with_stable = args.stable and hasattr(_lib.load(), "ctcext_stream_stable")
    sl = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    ref = one_shot(x, sl)   # warm-up: workspace, kernels
    rows = {}
    rows["one-shot"] = [_timed(lambda: one_shot(x, sl))[0] for _ in range(args.runs)]
    rows["one-shot, no ring"] = [_timed(lambda: one_shot(x, sl, _lib.CTCEXT_FLAG_NO_RING))[0]
                                 for _ in range(args.runs)]
    kernel = None
    stable_info = {}
    for c in chunks:
        ms, out, kernel = streamed(x, c)   # warm-up
        if not _same(out, ref):
            raise SystemExit("chunk size %d: the streamed result differs from the one-shot one" % c)
        rows["stream, %d-frame pushes" % c] = [streamed(x, c)[0] for _ in range(args.runs)]
        if with_stable and c < T:
            # (alternating with the plain row would be fairer still; the two lists are taken back to back)
            name = "stream, %d-frame pushes + stable()" % c
            streamed(x, c, True)   # warm-up
            stable_info[name] = {}
            rows[name] = [streamed(x, c, True, stable_info[name])[0] for _ in range(args.runs)]
    base = statistics.median(rows["one-shot"])
    lines = ["%-40s %9s %9s %9s %8s %10s %9s" % ("B=256 T=1500 C=29 W=128 P=3, %s" % args.input, "median ms", "min", "max",
                                                  "vs 1-shot", "per push", "walked")]
    res = {"shape": [B, T, C, W, P], "input": args.input, "runs": args.runs, "stream_kernel": kernel, "rows": {}}
    for name, v in rows.items():
        med = statistics.median(v)
        n = 1
        if name.startswith("stream"):
            n = -(-T // int(name.split()[1].split("-")[0]))
        per = "" if n == 1 else "%+.3f ms" % ((med - base) / n)
        info = stable_info.get(name, {})
        lines.append("%-40s %9.2f %9.2f %9.2f %7.1f%% %10s %9s" % (name, med, min(v), max(v), 100 * (med / base - 1), per,
                                                                  info.get("walked", "")))
        res["rows"][name] = {"median_ms": round(med, 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                             "pushes": n}
        res["rows"][name].update(info)
        if info:   # what the query costs per push: against the same pushes without it
            plain = statistics.median(rows[name.replace(" + stable()", "")])
            res["rows"][name]["query_ms_per_push"] = round((med - plain) / n, 4)
    if args.dense and hasattr(_lib.load(), "ctcext_stream_push_dense"):
        # the sums above are the synchronous rows' wall times (each push waits): the yardstick of wall_ms below
        dense = dense_rows(x, sl, chunks, args.runs)
        lines.append("%-52s %9s %9s %9s %9s %12s" % ("push_dense (enqueue-only)", "host ms", "wall ms", "min", "max",
                                                      "commit ms"))
        for name, v in dense.items():
            lines.append("%-52s %9.2f %9.2f %9.2f %9.2f %12s" % (name, v["host_ms"], v["wall_ms"], v["wall_min_ms"],
                                                                v["wall_max_ms"], v.get("commit_kernel_ms", "")))
        res["dense_rows"] = dense
        if args.times and hasattr(_lib.load(), "ctcext_stream_token_times"):
            c = min(chunks)
            tr = times_row(x, c, args.runs)
            lines.append("token times, %d-frame pushes with results (PROFILE, median of %d runs; ms)  %12s %16s %14s"
                         % (c, args.runs, "token times", "traceback+pack", "push kernels"))
            for k in ("last_push", "mean_push"):
                lines.append("  %-83s %12.4f %16.4f %14.4f" % (k.replace("_", " ") + (" (rows of %d frames)" % T if k == "last_push" else ""),
                                                              tr[k]["token_times_ms"], tr[k]["traceback_pack_ms"],
                                                              tr[k]["push_kernels_ms"]))
            res["times_row"] = tr
        if args.scores and hasattr(_lib.load(), "ctcext_stream_open_scores"):
            sr = scores_rows(x, sl, chunks, args.runs, args.score_store)
            store = args.score_store or "native"
            lines.append("score store (%s, %.1f MB), %d alternating rounds; medians, ms"
                         % (store, B * T * (C * (2 if args.score_store else 4) + 4) / 1e6, args.runs))
            lines.append("  %-18s %9s %11s %10s %11s %11s %8s %12s %14s" % ("", "wall", "wall+store", "per push", "append/push",
                                                                         "commit/push", "ratio", "scores (T)", "one-shot scores"))
            for name, v in sr.items():
                lines.append("  %-18s %9.2f %11.2f %+10.4f %11.4f %11.4f %8s %12.4f %14.4f"
                             % (name, v["wall_ms"], v["wall_store_ms"], v["store_ms_per_push"], v["append_kernel_ms_per_push"],
                                v["commit_kernel_ms_per_push"], v["append_over_commit"], v["scores_kernel_ms"],
                                v["one_shot_scores_kernel_ms"]))
            res["scores_rows"] = {"store": store, "rows": sr}
    text = "\n".join(lines) + "\n" + json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
