"""bench.py without a GPU: what --dump-outputs writes (names, dtypes, the seeded sample that keeps a dump within 64 MB) and
what --steps means for every workload."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    import bench as mod
    return mod


def _dump_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole(bench, tmp_path):
    x = np.linspace(0.0, 1.0, 1000)
    bench.dump_outputs(str(tmp_path), {"x": x, "b": np.arange(10, dtype=np.int32), "h": np.ones(5, dtype=np.float32)})
    assert sorted(os.listdir(tmp_path)) == ["b.npy", "h.npy", "x.npy"]
    assert np.array_equal(np.load(tmp_path / "x.npy"), x)
    b = np.load(tmp_path / "b.npy")
    assert b.dtype == np.float64 and np.array_equal(b, np.arange(10))
    assert np.load(tmp_path / "h.npy").dtype == np.float32


def test_large_outputs_are_a_fixed_sample_within_64_mb(bench, tmp_path):
    n = 5 << 20
    x = np.arange(n, dtype=np.float64) * 0.5
    v = np.arange(3 * n // 2, dtype=np.float64).reshape(-1, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "velocity": v})
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == ["velocity.npy", "velocity_rows.npy", "x.npy", "x_rows.npy"]
    assert _dump_bytes(str(a)) <= 64 << 20
    for name in os.listdir(a):
        assert np.array_equal(np.load(a / name), np.load(b / name)), name
    rows = np.load(a / "x_rows.npy").astype(np.int64)
    assert len(rows) > 1 << 20 and np.all(np.diff(rows) > 0) and np.array_equal(np.load(a / "x.npy"), x[rows])
    vrows = np.load(a / "velocity_rows.npy").astype(np.int64)
    assert np.array_equal(np.load(a / "velocity.npy"), v[vrows])


def test_ranks_write_their_own_parts_within_64_mb_in_all(bench, tmp_path):
    x = np.ones(6 << 20)
    for r in range(4):
        bench.dump_outputs(str(tmp_path), {"x": x * r}, rank=r, world=4)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(["x_rank%d.npy" % r for r in range(4)] + ["x_rows_rank%d.npy" % r for r in range(4)])
    assert _dump_bytes(str(tmp_path)) <= 64 << 20


@pytest.mark.parametrize("argv,steps", [([], 20), (["--steps", "7"], 7), (["--workload", "th"], 10),
                                        (["--workload", "th", "--steps", "20"], 20), (["--workload", "p2", "--steps", "3"], 3)])
def test_steps_is_the_number_of_timed_steps(bench, monkeypatch, argv, steps):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    assert bench.parse().steps == steps


def test_no_timed_steps_is_refused_before_any_work():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, capture_output=True, timeout=120)
    assert p.returncode == 2 and b"--steps" in p.stderr
