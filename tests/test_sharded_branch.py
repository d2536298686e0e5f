"""The branch-record exchange (sharding.evaluate_nodes_sharded_branch, Solve(..., group=...) with JSLP_SHARD_BRANCH=1): whole solves and node
batches -- ragged and empty ones included -- against the reference's goldens, on the CPU over gloo with oracle engines at world 2, 4 and 8, and
on the GPU with 4 virtual shards and with one RCCL rank."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(engine, nproc, port, backend="gloo", models=None):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", JSLP_TEST_ENGINE=engine, JSLP_TEST_BACKEND=backend)
    if models:
        env["JSLP_TEST_MODELS"] = models
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "sharded_branch_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("REPORT ")][-1]
    reports = json.loads(line[len("REPORT "):])
    assert len(reports) == nproc
    for rep in reports:
        assert rep["world"] == nproc
        assert not [c["name"] for c in rep["cases"] if not c["ok"]], [c["name"] for c in rep["cases"] if not c["ok"]]
    return reports


@pytest.mark.parametrize("world,port", [(2, 29611), (4, 29621), (8, 29631)])
def test_branch_exchange_over_gloo_with_oracle_engines(oracle_lib, world, port):
    reports = _run("oracle", world, port)
    names = [c["name"] for c in reports[0]["cases"]]
    assert reports[0]["backend"] == "oracle-c"
    assert any(n.startswith("Monster_II batch of 0 node(s) over %d rank(s)" % world) for n in names), names
    assert "Knapsack_1 (branch-record exchange)" in names


@pytest.mark.gpu
def test_branch_exchange_virtual_shards_on_one_gpu(hip_lib):
    reports = _run("hip", 4, 29641)
    assert all(r["backend"] == "hip-gfx950" for r in reports)


@pytest.mark.gpu
def test_branch_exchange_over_rccl_on_one_gpu(hip_lib):
    reports = _run("hip", 1, 29651, backend="nccl")
    assert reports[0]["backend"] == "hip-gfx950"
    # the exchanged payload per node: 32 bytes (the compact form moves 128 + 12 x 112 on Monster_II)
    assert "Monster_II batch of 151 node(s) over 1 rank(s), branch records (32 B per node)" in [c["name"] for c in reports[0]["cases"]]
