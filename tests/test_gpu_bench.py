"""GPU: bench.py's output contract - ONE JSON line on stdout (libraries' chatter goes to stderr), the keys the driver reads, the
roofline object of the dominant kernel class, the workload named; a short run of the real script as a child process."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_keys():
    env = dict(os.environ)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-decode",
                          "--no-other-modes"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, f"stdout must carry the JSON line alone, got {len(lines)} lines"
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and d["unit"] == "audio-frames/s"
    assert "configs[1]" in d["config"]["workload"] and d["config"]["parallelism"] == "dp1"
    assert d["value"] > 0 and abs(d["value"] - 32 * 998 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]     # frames of the batch per step time
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == pytest.approx(2500.0 / 6)
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"]) and 0 < r["frac"] < 1
    assert r["launches_per_step"] > 100 and r["algorithmic_gflop_per_step"] > 1000


def _plain_run(dump):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                          "--dump-outputs", str(dump)], cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, f"stdout must carry the JSON line alone, got {len(lines)} lines"
    return json.loads(lines[0])


def test_plain_bench_times_the_step_only_and_dumps_the_same_outputs_every_run(tmp_path):
    """Without --full the line carries the headline alone (no roofline, other modes, CPU baselines or decode); --steps sets the
    timed steps; --dump-outputs writes the last timed step's results (its loss is the line's) as float32 arrays under 64 MB, and
    two runs with the same arguments write the same arrays to within the rounding of one step (split-K float atomics), not the
    drift of chained steps (~1e-3 of the weights): the dumped step starts from the seeded state."""
    import numpy as np
    d = _plain_run(tmp_path / "a")
    assert d["steps"] == 4 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["unit"] == "audio-frames/s" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 32 * 998 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["decode"] is None
    assert not [k for k in d if k.startswith("dtype_")]
    e = _plain_run(tmp_path / "b")
    files = {p.name: (np.load(p), np.load(tmp_path / "b" / p.name)) for p in (tmp_path / "a").iterdir()}
    assert set(files) == {"loss.npy", "acc.npy", "params_sample.npy", "grads_sample.npy"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a, _ in files.values())
    assert sum(a.nbytes for a, _ in files.values()) <= 64 << 20
    assert files["params_sample.npy"][0].shape == files["grads_sample.npy"][0].shape == (1 << 22,)
    assert np.abs(files["grads_sample.npy"][0]).max() > 0 and 0 <= float(files["acc.npy"][0][0]) <= 1
    assert float(files["loss.npy"][0][0]) == d["loss"] and float(files["loss.npy"][1][0]) == e["loss"]
    for name, (a, b) in files.items():
        assert np.abs(a.astype(np.float64) - b).max() <= 1e-5 * np.abs(a).max(), name
