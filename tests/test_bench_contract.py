"""bench.py contract (task statement): one JSON line with the agreed keys, measured on the GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--full",
                        "--cpu-sample", "1", "--extra-file", str(tmp_path / "bench_extra_test.json")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and r.stdout.rstrip().splitlines()[-1] == lines[0]  # the JSON object is the LAST stdout line
    assert len(lines[0]) < 4096, len(lines[0])  # round 5's 22 KB line was not parsed by the driver: the long form goes to extra_file + stderr
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1 and j["higher_is_better"] is True and j["scaling"] == "weak"
    assert j["dtype"].startswith("f32") and j["data"] == "synthetic" and j["vs_baseline"] is None and "workload" in j["config"]
    assert j["value"] > 0 and abs(j["value"] - 2 * 1e3 / j["ms_per_step"]) < 1e-6 * j["value"]
    ro = j["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in ro, k
    # "valu": the fp16-piece pair kernel is bound by vector issue, not by a matrix pipe; its frac stays the f32-equivalent figure
    assert ro["bound"] in ("hbm", "mfma", "valu") and abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-9
    assert "kernel" in ro and ro["avg_launch_ms"] > 0 and "roofline_second" in j
    assert not any(isinstance(v, str) and len(v) > 200 for v in ro.values())
    extra = j["extra_file"]
    extra = extra if os.path.isabs(extra) else os.path.join(ROOT, extra)
    with open(extra) as f:
        long_form = json.load(f)
    assert long_form["headline"]["roofline"]["kernel"].startswith(ro["kernel"]) and "extra" in long_form
    cb = j["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_its_last_step(tmp_path):
    """A plain run (no --full): nothing measured beside the headline and no side file; --steps sets the number of timed steps (the step
    time agrees between 205 and 5 steps, and the 200 extra steps show in the wall time of the run).  --dump-outputs writes matched1 /
    matched2 of the last timed step (float32; a fixed sample of 16 of the 1024 frame-pairs), and since every step computes from the same
    inputs, both runs write the same arrays."""
    import time

    import numpy as np
    runs = []
    for steps in (205, 5):  # the long run first: a slower (cold) start can only widen the gap checked below
        d = tmp_path / ("outputs%d" % steps)
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3",
                            "--dump-outputs", str(d), "--extra-file", str(tmp_path / "bench_extra.json")],
                           capture_output=True, text=True, cwd=ROOT, timeout=600)
        wall = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-2000:]
        j = json.loads(r.stdout.rstrip().splitlines()[-1])
        assert j["steps"] == steps and j["warmup"] == 3 and j["config"]["frame_pairs_per_step_per_gpu"] == 1024
        assert abs(j["value"] - 1024 * 1e3 / j["ms_per_step"]) < 1e-6 * j["value"]
        assert j["cpu_baseline"] is None and j["selfcheck_max_abs"] is None and j["extra_file"] is None
        assert not (tmp_path / "bench_extra.json").exists()
        assert sorted(os.listdir(d)) == ["matched1.npy", "matched2.npy"]
        m1, m2 = np.load(d / "matched1.npy"), np.load(d / "matched2.npy")
        assert m1.dtype == np.float32 and m1.shape == (16, 500, 502) and m2.dtype == np.float32 and m2.shape == (16, 502, 500)
        assert m1.nbytes + m2.nbytes <= 64 << 20
        # matched1: softmax over each row's N + 2 columns; matched2: over each column's N + 2 rows
        assert np.abs(m1.sum(2) - 1).max() < 1e-4 and np.abs(m2.sum(1) - 1).max() < 1e-4
        runs.append((j["ms_per_step"], wall, m1, m2))
    (ms_long, wall_long, m1_long, m2_long), (ms_short, wall_short, m1_short, m2_short) = runs
    assert 0.5 < ms_long / ms_short < 2, (ms_long, ms_short)
    assert wall_long - wall_short > 0.5 * 200 * ms_long / 1e3, (wall_long, wall_short, ms_long)
    assert np.array_equal(m1_long, m1_short) and np.array_equal(m2_long, m2_short)
