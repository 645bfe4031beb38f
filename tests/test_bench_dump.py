"""CPU: bench.py's --dump-outputs writer (bench.dump_outputs): float64 .npy files that hold the arrays
exactly, and, past the size limit, the same seeded sample of rows every run within 64 MB in all."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _outputs(B, seed=5):
    g = np.random.default_rng(seed)
    return dict(tau=g.normal(size=(B, 12)), grf=g.normal(size=(B, 12)),
                status=g.integers(0, 4, B).astype(np.int32), iters=g.integers(0, 60, B).astype(np.int32))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_array_whole_in_float64(tmp_path):
    src = _outputs(4097)
    bench.dump_outputs(str(tmp_path / "a"), **src)
    got = _load(str(tmp_path / "a"))
    assert sorted(got) == sorted(src)
    for k, v in src.items():
        assert got[k].dtype == np.float64 and got[k].shape == v.shape
        assert np.array_equal(got[k], v)  # int32 status / iters are exact in float64


def test_dump_samples_the_same_rows_within_64_mb(tmp_path):
    """208 B per robot: 400 000 robots are 83 MB, past the limit.  Every array keeps the same fraction
    of its rows, in order, with their numbers beside it; a second run writes the same files."""
    B = 400_000
    src = _outputs(B)
    assert sum(np.asarray(v, np.float64).nbytes for v in src.values()) > 64 << 20
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), **src)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    assert sorted(a) == sorted(list(src) + ["rows_" + k for k in src])
    for k, v in src.items():
        rows = a["rows_" + k].astype(np.int64)
        assert a[k].dtype == np.float64 and len(rows) >= B // 2
        assert np.all(np.diff(rows) > 0) and 0 <= rows[0] and rows[-1] < B
        assert np.array_equal(a[k], v[rows])
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_dump_limit_is_a_threshold(tmp_path):
    src = _outputs(100)
    n = sum(np.asarray(v, np.float64).nbytes for v in src.values())
    bench.dump_outputs(str(tmp_path / "at"), limit=n, **src)
    bench.dump_outputs(str(tmp_path / "over"), limit=n - 1, **src)
    assert sorted(_load(str(tmp_path / "at"))) == sorted(src)
    over = _load(str(tmp_path / "over"))
    assert len(over["tau"]) == 99 and np.array_equal(over["tau"], src["tau"][over["rows_tau"].astype(np.int64)])
