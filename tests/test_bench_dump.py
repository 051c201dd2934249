"""bench.py --dump-outputs: the writer alone, on host arrays (no GPU): names,
dtypes, the byte limit with its seeded row sample, and run-to-run identity."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from ctcext_amd.ops import CTCExtBeamSearchDecoder  # noqa: E402


def _outputs(n, P, B, fdt):
    rng = np.random.default_rng(3)
    idx = [rng.integers(0, 1 << 40, (n + p, 2), dtype=np.int64) for p in range(P)]
    val = [rng.integers(0, 29, (n + p,), dtype=np.int64) for p in range(P)]
    shp = [np.array([B, n], np.int64) for _ in range(P)]
    return CTCExtBeamSearchDecoder(idx, val, shp, [a + 1 for a in idx], [a + 1 for a in val], shp,
                                   rng.standard_normal((B, P)).astype(fdt))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole(tmp_path):
    out = _outputs(1000, 2, 4, np.float32)
    info = bench.dump_outputs(out, 2, str(tmp_path / "a"))
    got = _load(str(tmp_path / "a"))
    assert sorted(got) == sorted(["%s_%d" % (f, p) for f in out._fields[:6] for p in range(2)] + ["log_probability"])
    assert info["sampled_fraction"] == 1.0 and info["bytes"] == sum(a.nbytes for a in got.values())
    for p in range(2):
        # int64 components as float64, exactly
        assert got["decoded_indices_%d" % p].dtype == np.float64
        assert np.array_equal(got["decoded_indices_%d" % p].astype(np.int64), out.decoded_indices[p])
        assert np.array_equal(got["alignment_values_%d" % p].astype(np.int64), out.alignment_values[p])
    assert got["log_probability"].dtype == np.float32
    assert np.array_equal(got["log_probability"], out.log_probability)


def test_dump_sampled_is_bounded_and_repeatable(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    out = _outputs(5000, 1, 8, np.float64)
    info = bench.dump_outputs(out, 1, str(tmp_path / "a"))
    bench.dump_outputs(out, 1, str(tmp_path / "b"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert 0.0 < info["sampled_fraction"] < 1.0
    assert sum(v.nbytes for v in a.values()) <= (64 << 10) + 1024   # the small arrays stay whole
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # indices and values of one path keep the same rows; the rows come from the full arrays in order
    assert len(a["decoded_indices_0"]) == len(a["decoded_values_0"]) < 5000
    full = out.decoded_values[0].astype(np.float64)
    rows = np.sort(np.random.default_rng(0).choice(5000, size=len(a["decoded_values_0"]), replace=False))
    assert np.array_equal(a["decoded_values_0"], full[rows])
    assert np.array_equal(a["decoded_shape_0"], [8, 5000]) and a["log_probability"].dtype == np.float64
