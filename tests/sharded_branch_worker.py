"""Worker for tests/test_sharded_branch.py: launched by torch.distributed.run with WORLD_SIZE ranks.  The branch-record exchange
(sharding.evaluate_nodes_sharded_branch, Solve with JSLP_SHARD_BRANCH=1): on the CPU the oracle's records (restated from its compact read-back)
go over gloo; with JSLP_TEST_ENGINE=hip every rank drives the HIP engine and the records come from the device."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import golden_util as G  # noqa: E402
from jslpsolver_amd import Solve, _capi  # noqa: E402
from jslpsolver_amd.engine import Tableau, branch_record_from_watched  # noqa: E402
from jslpsolver_amd.sharding import evaluate_nodes_sharded_branch, evaluate_nodes_sharded_watched  # noqa: E402


def bits(recs):
    """records as int64 bit patterns (the doubles compared bit for bit)"""
    return np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1).view(np.int64)


def main():
    backend = os.environ.get("JSLP_TEST_BACKEND", "gloo")
    if backend == "nccl":
        import torch
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    dist.init_process_group(backend)
    rank, world = dist.get_rank(), dist.get_world_size()
    if os.environ.get("JSLP_TEST_ENGINE") == "hip":
        lib = _capi.load_hip()
    else:
        lib = _capi.Library(os.path.join(ROOT, "oracle", "libjslp_oracle.so"))
    report = {"rank": rank, "world": world, "backend": lib.backend, "cases": []}
    names = os.environ.get("JSLP_TEST_MODELS", "Monster_II,LargeFarmMIP,Knapsack_1,Sudoku4x4").split(",")
    # 1. whole solves over the branch-record exchange == the reference's result and iteration count
    os.environ["JSLP_SHARD_BRANCH"] = "1"
    for name in names:
        g = G.load(os.path.join(G.GOLDEN, "fixtures", name + ".json.gz"))
        ref = {k: (G.num(v) if not isinstance(v, bool) else v) for k, v in g["result"].items()}
        model = dict(g["model"])
        # (a wall-clock limit -- LargeFarmMIP's options.timeout -- would let ranks that share one GPU stop their replays of the tree at different
        #  iterations and leave the collectives out of step; the reference finished well inside it, so without it the tree is the same)
        model["options"] = {k: v for k, v in (model.get("options") or {}).items() if k != "timeout"}
        out = Solve(model, full=True, lib=lib, speculate=16, group=dist.group.WORLD)
        ok = out["result"] == ref and out["iter"] == g["final"]["branchAndCutIterations"]
        report["cases"].append({"name": name + " (branch-record exchange)", "ok": bool(ok)})
    os.environ.pop("JSLP_SHARD_BRANCH", None)
    # 2. the Monster_II node batch: every node's exchanged record == the restatement of the compact exchange of the same nodes, and the
    #    flags / height of the reference's own relaxation
    g = G.load(os.path.join(G.GOLDEN, "fixtures", "Monster_II.json.gz"))
    tab = g["tableau"]
    m, vibr, vibc = G.dense_tableau(tab)
    calls = g["simplexCalls"]
    t = Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"],
                row_capacity=tab["height"] + max(len(c["cuts"] or []) for c in calls), lib=lib)
    t.applyCuts([], check_cycles=True)
    t.save()
    watched = np.array(tab["integerVarIndexes"], dtype=np.int32)
    t.set_watched_variables(watched)
    nodes = [c["cuts"] or [] for c in calls[1:]]
    for n_take in (len(nodes), 0, 1, max(world - 1, 1), world + 1):  # the whole batch, then ragged / empty ones
        sub = nodes[:n_take]
        br = evaluate_nodes_sharded_branch(t, sub, True, dist.group.WORLD)
        comp = evaluate_nodes_sharded_watched(t, sub, True, dist.group.WORLD)
        ok = len(br) == len(sub) == len(comp) and type(br).__name__ == "ShardedOutcomesBranch"
        if sub:
            want = np.concatenate([branch_record_from_watched(comp.result(i), comp.watched_rows(i), comp.watched_values(i), watched, t.precision)
                                   for i in range(len(sub))])
            got = br.records()
            ok = ok and np.array_equal(bits(got), bits(want))
            for i, call in enumerate(calls[1:1 + n_take]):
                ev = br.node(i)
                ok = ok and bool(ev.res.feasible) == call["feasible"] and ev.res.height == call["height"]
                ok = ok and (not ev.res.optimal or ev.res.evaluation == comp.result(i).evaluation)
        per = max((n_take + world - 1) // world, 1)
        report["cases"].append({"name": "Monster_II batch of %d node(s) over %d rank(s), branch records (%d B per node)"
                                % (n_take, world, br.blocks.shape[1] // per), "ok": bool(ok)})
    t.close()
    gathered = [None] * world
    dist.all_gather_object(gathered, report)
    if rank == 0:
        print("REPORT " + json.dumps(gathered))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
