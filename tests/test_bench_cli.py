"""bench.py's command line: a plain run times the headline only (--full adds the other legs), --dump-outputs writes the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _plans(K, N=8, Ms=(5, 6, 7)):
    from swarm_simulator_amd.types import PlanResult
    rng = np.random.default_rng(7)
    plans = []
    for k in range(K):
        M = Ms[k % len(Ms)]
        p = PlanResult(rng.standard_normal((N, M + 1, 3)).astype(np.float32), np.arange(M + 1, dtype=np.float64))
        for name in ("sfc_box", "sfc_time", "rsfc_normal", "rsfc_time", "coef", "ctrl"):
            a = getattr(p, name)
            a[...] = rng.standard_normal(a.shape).astype(a.dtype)
        p.sfc_count[:] = 1 + k % M
        p.total_cost, p.time_scale = float(k) + 0.5, 1.0 + k / 100
        plans.append(p)
    return plans


def test_dump_outputs_is_float_seeded_and_bounded(tmp_path):
    plans = _plans(40)
    status = [0] * 39 + [3]
    names = bench.dump_outputs(str(tmp_path / "a"), plans, status)
    files = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in names) <= bench.DUMP_LIMIT_BYTES
    np.testing.assert_array_equal(files["status"], np.array(status, np.float64))
    np.testing.assert_array_equal(files["total_cost"], [p.total_cost for p in plans])
    np.testing.assert_array_equal(files["sfc_count"], np.stack([p.sfc_count for p in plans]))
    sample = files["sample_missions"].astype(int)
    assert len(sample) == bench.DUMP_SAMPLE_MISSIONS and len(set(sample)) == len(sample)
    for k in sample:
        np.testing.assert_array_equal(files[f"ctrl_k{k:04d}"], plans[k].ctrl)
        np.testing.assert_array_equal(files[f"rsfc_normal_k{k:04d}"], plans[k].rsfc_normal)
        assert files[f"rsfc_normal_k{k:04d}"].dtype == np.float32
    # the same missions are sampled on every run
    assert bench.dump_outputs(str(tmp_path / "b"), plans, status) == names


def test_dump_outputs_stays_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40_000)
    names = bench.dump_outputs(str(tmp_path), _plans(40), [0] * 40)
    total = sum(np.load(tmp_path / (n + ".npy")).nbytes for n in names)
    assert total <= 40_000
    assert 0 < len(np.load(tmp_path / "sample_missions.npy")) < bench.DUMP_SAMPLE_MISSIONS


def test_command_line_has_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """a plain run: the headline line with ms_per_step over exactly --steps steps, none of the --full legs, and the outputs of the last
    step on disk (every mission solved: status 0, a finite cost)."""
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--missions-per-gpu", "50", "--steps", "2",
                          "--warmup", "1", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in res
    for k in ("cpu_baseline", "latency_ms_single_mission", "single_sweep", "roofline_joint"):
        assert k not in res
    assert np.all(np.load(d / "status.npy") == 0)
    cost = np.load(d / "total_cost.npy")
    assert cost.shape == (50,) and np.all(np.isfinite(cost))
    for k in np.load(d / "sample_missions.npy").astype(int):
        assert np.all(np.isfinite(np.load(d / f"ctrl_k{k:04d}.npy")))
