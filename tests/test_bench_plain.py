"""bench.py without --full: set-up, warm-up, the timed headline steps, the dump if asked for, and the result line -- nothing else."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_only_relaxations_needs_full():
    """the leg selectors of the full run are refused in a plain run, before anything touches a GPU"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--only-relaxations"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--full" in out.stderr, out.stderr[-1500:]


@pytest.mark.gpu
def test_plain_run_times_only_the_headline(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--lp-size", "500",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "simplex pivots/sec" and line["unit"] == "pivots/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - 657) < 1e-6 * 657  # the reference's 657 pivots per solve at n = 500
    assert line["roofline"]["units"] > 0
    for leg in ("sustained", "cycle_check_on", "resident_health", "phase1_instance", "streaming_instance", "relaxations", "dropin_js",
                "cpu_baseline", "speedup_vs_cpu_baseline"):
        assert leg not in line, leg
    assert "pivot_digest" not in line["config"]
    assert line["dumped_outputs"]["of"] == "the last timed step"
    for name in line["dumped_outputs"]["arrays"]:
        assert os.path.exists(str(tmp_path / (name + ".npy"))), name
    import numpy as np
    from jslpsolver_amd._capi import SimplexResult
    res = dict(zip([f for f, _ in SimplexResult._fields_], np.load(str(tmp_path / "simplex_result.npy")).tolist()))
    assert res["feasible"] == 1 and res["optimal"] == 1 and res["pivots_phase1"] + max(res["pivots_phase2"], 0) == 657, res
