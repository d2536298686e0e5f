#!/usr/bin/env python3
"""Branch records (include/jslpx_branch.h) against the compact read-back, on one GPU, on the batch bench.py builds: Monster_II's 151 visited cut
lists x16 = 2416 independent nodes.
  (a) one engine: compact pinned (jslp_engine_relax_batch_watched_pinned) against record pinned (jslpx_engine_relax_batch_branch_pinned);
  (b) the strong-scaling exchange at N = 1 over RCCL: sharding.evaluate_nodes_sharded_watched against evaluate_nodes_sharded_branch;
  (c) Solve(Monster_II, speculate=16) with JSLP_TREE_BRANCH=0 / 1.
Every record is checked against the restatement (engine.branch_record_from_watched) of the compact read-back of the same call before anything
is printed.  Prints ONE JSON line: rates, bytes per node exchanged, per-call microseconds (median of --reps calls after --warmup).
  python tools/branch_record_times.py [--reps 20] [--warmup 10]"""
import argparse
import hashlib
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import golden_util as G  # noqa: E402
from jslpsolver_amd import Solve, _capi  # noqa: E402
from jslpsolver_amd.engine import Tableau, branch_record_from_watched  # noqa: E402


def sources_sha():
    """sha256 (16 hex) over jslpsolver_amd/csrc/* and the two C headers: which sources a line was measured on"""
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "jslpsolver_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(csrc, name), "rb") as fh:
                h.update(name.encode() + b"\0" + fh.read())
    for name in ("jslp_engine.h", "jslpx_branch.h"):
        with open(os.path.join(ROOT, "include", name), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def bits(recs):
    return np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1).view(np.int64)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        per.append(time.perf_counter() - t0)
    return sorted(per)[len(per) // 2], per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    # (torch's device and the one-rank RCCL group first, as tests/sharded_worker.py does: before the engine library has touched the runtime)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    lib = _capi.load_hip()
    g = G.load(os.path.join(G.GOLDEN, "fixtures", "Monster_II.json.gz"))
    tab = g["tableau"]
    calls = g["simplexCalls"]
    m, vibr, vibc = G.dense_tableau(tab)
    t = Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"],
                row_capacity=tab["height"] + max(len(c["cuts"] or []) for c in calls), lib=lib)
    t.applyCuts([], check_cycles=True)
    t.save()
    watched = tab["integerVarIndexes"]
    t.set_watched_variables(watched)
    nodes = [c["cuts"] or [] for c in calls[1:]] * 16
    n = len(nodes)
    pk = t.pack_cut_lists(nodes)
    out = {"tool": "branch_record_times", "sources_sha16": sources_sha(), "nodes": n, "watched": len(watched), "reps": a.reps, "warmup": a.warmup}

    # (a) one engine, pinned read-back of both kinds; the check first
    res_c, rows, vals = t.applyCutsBatchWatched(None, check_cycles=True, packed=pk)
    want = branch_record_from_watched([res_c[i] for i in range(n)], rows[:n], vals[:n], watched, t.precision)
    _r, recs = t.applyCutsBatchBranch(None, check_cycles=True, packed=pk)
    assert np.array_equal(bits(recs), bits(want)), "engine records differ from the restatement"
    med_c, per_c = timed(lambda: t.applyCutsBatchWatched(None, check_cycles=True, packed=pk, copy=False), a.warmup, a.reps)
    med_b, per_b = timed(lambda: t.applyCutsBatchBranch(None, check_cycles=True, packed=pk, copy=False), a.warmup, a.reps)
    out["engine"] = {"compact_pinned": {"rate": n / med_c, "call_us": round(1e6 * med_c, 1), "bytes_per_node": 128 + 12 * len(watched),
                                        "per_call_us": [round(1e6 * x) for x in per_c]},
                     "record_pinned": {"rate": n / med_b, "call_us": round(1e6 * med_b, 1), "bytes_per_node": 128 + 32,
                                       "per_call_us": [round(1e6 * x) for x in per_b]},
                     "record_over_compact": med_c / med_b}

    # (b) the exchange at N = 1 over RCCL (one-rank process group, as bench.py's sharded_batch leg at N = 1)
    from jslpsolver_amd.sharding import (branch_block_bytes, evaluate_nodes_sharded_branch, evaluate_nodes_sharded_watched,
                                         watched_block_bytes)
    grp = dist.group.WORLD
    comp = evaluate_nodes_sharded_watched(t, nodes, True, grp, packed_mine=pk)
    br = evaluate_nodes_sharded_branch(t, nodes, True, grp, packed_mine=pk)
    want = np.concatenate([branch_record_from_watched(comp.result(i), comp.watched_rows(i), comp.watched_values(i), watched, t.precision)
                           for i in range(n)])
    assert np.array_equal(bits(br.records()), bits(want)), "exchanged records differ from the restatement"
    med_w, per_w = timed(lambda: evaluate_nodes_sharded_watched(t, nodes, True, grp, packed_mine=pk, copy=False), a.warmup, a.reps)
    med_r, per_r = timed(lambda: evaluate_nodes_sharded_branch(t, nodes, True, grp, packed_mine=pk, copy=False), a.warmup, a.reps)
    out["sharded_n1_rccl"] = {
        "watched": {"rate": n / med_w, "call_us": round(1e6 * med_w, 1), "exchanged_bytes_per_node": watched_block_bytes(n, len(watched), t.state_record_bytes()) / n,
                    "per_call_us": [round(1e6 * x) for x in per_w]},
        "branch": {"rate": n / med_r, "call_us": round(1e6 * med_r, 1), "exchanged_bytes_per_node": branch_block_bytes(n) / n,
                   "per_call_us": [round(1e6 * x) for x in per_r]},
        "branch_over_compact_engine": (n / med_r) / (n / med_c), "watched_over_compact_engine": (n / med_w) / (n / med_c)}
    dist.destroy_process_group()
    t.close()

    # (c) the speculative tree, compact against branch records
    trees = {}
    for knob in ("0", "1"):
        os.environ["JSLP_TREE_BRANCH"] = knob
        Solve(g["model"], speculate=16)  # warm-up
        per = []
        for _ in range(5):
            t0 = time.perf_counter()
            r = Solve(g["model"], full=True, speculate=16)
            per.append(time.perf_counter() - t0)
        trees[knob] = (sorted(per)[2], r["result"], r["iter"])
    os.environ.pop("JSLP_TREE_BRANCH", None)
    assert trees["0"][1:] == trees["1"][1:], "the tree differs between the read-backs"
    out["tree_speculate16"] = {"compact_ms": round(1e3 * trees["0"][0], 2), "branch_ms": round(1e3 * trees["1"][0], 2), "iterations": trees["1"][2],
                               "result": trees["1"][1]["result"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
