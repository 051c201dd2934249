"""The greedy stream on the GPU (GreedyStream): after every push every output -- the hypothesis, the token times, the
token scores, status and frames -- equals the host definitions over the frames each item has taken so far
(test_cpu_greedy_stream.Model), exactly: values, NaN cells, and the sign bit of every float that is no NaN."""
import numpy as np
import pytest
import torch

import ctcext_amd
from ctcext_amd import _lib
from test_cpu_greedy import quantised, same_bits
from test_cpu_greedy_stream import CASES, Model, case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENGTH, CAPACITY = _lib.CTCEXT_ITEM_LENGTH, _lib.CTCEXT_ITEM_CAPACITY


def check(out, exp, what):
    torch.cuda.synchronize()
    got = dict(zip(out._fields[:7], out[:7]), **out.times._asdict(), **out.scores._asdict())
    for field, want in exp.items():
        same_bits(got[field].cpu().numpy(), want, (what, field))


def chunk_of(rows, lengths, t, dtype, batch_first, strided=False):
    """The chunk tensor of a push: item b's rows first, NaN behind them (no row past an item's length is read)."""
    B, C = len(rows), rows[0].shape[1]
    x = np.full((B, t, C), np.nan, rows[0].dtype)
    for b in range(B):
        x[b, :max(int(lengths[b]), 0)] = rows[b]
    x = torch.as_tensor(x).to(getattr(torch, dtype)).to(DEV)
    if strided:   # a view with gaps in both dimensions
        full = torch.zeros((B, t + 3, C + 11), dtype=x.dtype, device=DEV)
        full[:, 1:1 + t, 5:5 + C] = x
        x = full[:, 1:1 + t, 5:5 + C]
    return x if batch_first else x.transpose(0, 1).contiguous()


# the cases every row evaluator must hold, whatever the switch-over would choose: rows below one group of 64 classes,
# of many groups whole and not, float64, half chunks through strides, chunks of more than one step
BOTH = ["ranged-7x3x5-ragged", "ranged-10x3x1000-ragged", "quantised-9x2x1091-all", "ranged-600x2x33-f64-ragged",
        "sticky-70x130x29-bf16-all", "ranged-40x2x300-ragged", "sticky-600x2x33-ragged"]


@pytest.mark.parametrize("name, rows", [(n, None) for n in CASES] + [(n, r) for n in BOTH for r in ("lane", "wide")])
def test_every_push_equals_the_definition(name, rows, monkeypatch):
    if rows:
        monkeypatch.setenv("CTCEXT_GREEDY_ROWS", rows)   # (read when the stream opens, at its first push)
    (wide, pushes), (_, (T, B, C), dtype, _, merge) = case(name), CASES[name]
    model, at = Model(B, C, T, wide.dtype, merge), [0] * B
    half = dtype in ("bfloat16", "float16")
    with ctcext_amd.GreedyStream(B, C, T, dtype="float64" if dtype == "float64" else "float32", merge_repeated=merge,
                                 token_scores=True) as s:
        for i, (t, lengths) in enumerate(pushes):
            rows = [wide[at[b]:at[b] + max(int(n), 0), b] for b, n in enumerate(lengths)]
            for b in range(B):
                model.take(b, rows[b])
                at[b] += len(rows[b])
            out = s.push(chunk_of(rows, lengths, t, dtype, batch_first=bool(i % 2) or half, strided=half),
                         torch.as_tensor(lengths, device=DEV), batch_first=bool(i % 2) or half)
            check(out, model.expected([0] * B), (name, i))
        s.check()
        assert s.frames.tolist() == at and at[0] == T


@pytest.mark.parametrize("rows", ["lane", "wide"])
def test_status_reset_and_check(rows, monkeypatch):
    monkeypatch.setenv("CTCEXT_GREEDY_ROWS", rows)
    B, C, F = 3, 5, 12
    x = quantised(np.random.default_rng(5), 40, B, C)
    model, at = Model(B, C, F, np.float32, True), [0] * B

    def push(s, t, lengths, status, reset=None):
        rows = [x[at[b]:at[b] + (0 if status[b] else max(n, 0)), b] for b, n in enumerate(lengths)]
        for b in range(B):
            if reset is not None and reset[b]:
                model.reset(b)
            model.take(b, rows[b])
            at[b] += len(rows[b])
        # (an item with a bit gets the frames it would have taken, which must not be)
        fill = [x[at[b]:at[b] + min(n, t), b] if status[b] else rows[b] for b, n in enumerate(lengths)]
        out = s.push(chunk_of(fill, np.minimum(lengths, t), t, "float32", True),
                     torch.as_tensor(lengths, dtype=torch.int32, device=DEV),
                     reset=None if reset is None else torch.as_tensor(reset, dtype=torch.int32, device=DEV))
        check(out, model.expected(status), (t, lengths))

    with ctcext_amd.GreedyStream(B, C, F, merge_repeated=True, token_scores=True) as s:
        push(s, 5, [5, 6, 5], [0, LENGTH, 0])      # item 1 keeps its (empty) rows, the bit shows in this push only
        with pytest.raises(ctcext_amd.FailedPreconditionError) as e:
            s.check()
        assert e.value.message == "sequence_length(1) <= 5"
        push(s, 5, [5, 5, 5], [0, 0, 0])
        push(s, 5, [5, 5, 2], [CAPACITY, 0, 0])    # item 0 keeps the rows of its 10 frames
        with pytest.raises(ctcext_amd.InvalidArgumentError) as e:
            s.check()
        assert e.value.message == "stream capacity exceeded: item 0 would hold 15 frames of max_frames 12"
        s.check()                                  # (forgotten)
        push(s, 3, [3, 0, 0], [0, 0, 0], reset=[1, 0, 0])   # item 0 starts again with this chunk, the others go on
        assert s.frames.tolist() == [3, 10, 12]
        s.reset([2])                               # the host form: item 2's rows are padding again
        model.reset(2)
        push(s, 2, [2, 2, 2], [0, 0, 0])
        assert s.frames.tolist() == [5, 12, 2]


def test_graph_capture_and_replay():
    """One capture of a push (a single kernel node) replayed over three chunks copied into the captured input equals
    the uncaptured stream's definition."""
    name = "sticky-600x2x33-ragged"
    (wide, _), (_, (T, B, C), _, _, merge) = case(name), CASES[name]
    t, side, model = 70, torch.cuda.Stream(device=DEV), Model(B, C, T, np.float32, merge)
    static = torch.zeros((B, t, C), device=DEV)
    with ctcext_amd.GreedyStream(B, C, T, merge_repeated=merge, token_scores=True) as s:
        with torch.cuda.stream(side):
            s.push(static)      # (opens the stream: the one call that allocates)
        side.synchronize()
        s.reset()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = s.push(static)
        for i in range(3):
            rows = [wide[i * t:(i + 1) * t, b] for b in range(B)]
            static.copy_(chunk_of(rows, [t] * B, t, "float32", True))
            torch.cuda.synchronize()
            g.replay()
            for b in range(B):
                model.take(b, rows[b])
            check(out, model.expected([0] * B), ("replay", i))
