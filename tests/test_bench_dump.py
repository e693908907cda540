"""`bench.py --dump-outputs DIR`: what the last timed step computed, as float64 .npy files, the same inputs on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench(monkeypatch):
    """bench.py, imported with the environment default it sets at import time undone after the test."""
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import bench
    return bench


def test_dump_writes_float64_and_samples_a_large_t2(bench, tmp_path):
    no, nv = 50, 200            # the headline workload: T2 is 800 MB, only a fixed sample of it is written
    rng = np.random.default_rng(0)
    t1 = rng.standard_normal((nv, no))
    t2 = np.arange(nv * nv * no * no, dtype=np.float64).reshape(nv, nv, no, no)
    shapes = bench.dump_outputs(str(tmp_path / "a"), (1.0, 2.0, 3.0, 4.0, 5.0), t1, t2)
    assert set(shapes) == {"step_result", "t1", "t2_sample"}
    total = 0
    for name in shapes:
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == np.float64 and list(a.shape) == shapes[name]
        total += os.path.getsize(tmp_path / "a" / (name + ".npy"))
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / "a" / "step_result.npy"), [1.0, 2.0, 3.0, 4.0, 5.0])
    assert np.array_equal(np.load(tmp_path / "a" / "t1.npy"), t1)
    s = np.load(tmp_path / "a" / "t2_sample.npy")          # t2 holds its own flat index: the sample shows where it came from
    assert len(s) > 0.95 * bench.DUMP_T2_SAMPLE and np.all(np.diff(s) > 0) and s[-1] < t2.size
    bench.dump_outputs(str(tmp_path / "b"), (1.0, 2.0, 3.0, 4.0, 5.0), t1, t2)
    assert np.array_equal(np.load(tmp_path / "b" / "t2_sample.npy"), s)       # the same indices on every run


def test_dump_writes_a_small_t2_whole(bench, tmp_path):
    t2 = np.random.default_rng(1).standard_normal((20, 20, 6, 6))
    shapes = bench.dump_outputs(str(tmp_path), np.zeros(5), np.zeros((20, 6)), t2)
    assert set(shapes) == {"step_result", "t1", "t2"}
    assert np.array_equal(np.load(tmp_path / "t2.npy"), t2)


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--stub-collectives"]])
def test_dump_refused_off_the_single_rank_path(tmp_path, extra):
    """Refused before anything touches the GPU (or starts rank processes)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(tmp_path)] + extra, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--dump-outputs needs the single-rank path" in r.stderr and not r.stdout.strip()


@pytest.mark.gpu
def test_bench_dump_is_reproducible(tmp_path):
    """Two runs with the same arguments: the same number of timed steps in the line, and the same outputs."""
    lines = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                            "--nocc", "20", "--nvirt", "80", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / run)],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    for line in lines:
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert set(line["dump_outputs"]["arrays"]) == {"step_result", "t1", "t2"}
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("step_result", "t1", "t2")}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in ("step_result", "t1", "t2")}
    assert a["t2"].shape == (80, 80, 20, 20) and a["t1"].shape == (80, 20)
    assert np.all(np.isfinite(a["t2"])) and np.abs(a["t2"]).max() > 0
    assert a["step_result"][0] + a["step_result"][1] + a["step_result"][2] == pytest.approx(lines[0]["iteration"]["last_energy"],
                                                                                           abs=1e-12)
    for n in a:
        np.testing.assert_allclose(a[n], b[n], rtol=0, atol=1e-12)
