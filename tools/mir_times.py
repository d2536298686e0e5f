#!/usr/bin/env python3
"""A node's MIR loop in one engine call (include/jslpr_mir.h) against the call-by-call loop, on one GPU.
  (a) per-node wall time on the recorded node lists of Knapsack_1, LargeFarmMIP (first 400 nodes) and Monster_II: the sequential composition
      (applyCuts + mirRound + the host's volume rule, what branch_and_cut.mir_loop does) against ONE applyCutsMIR call per node against
      applyCutsBatchMIR of 16 and of 302 nodes;
  (b) Solve() of the three MIR trees: speculate 1 (round by round), speculate 1 with JSLP_TREE_MIR=1, speculate 8.
Every timed form is first checked against the sequential composition (results, records' round counts, RHS columns).  Medians of --reps
passes after --warmup; the spread (min .. max) is printed next to each median.  Writes a markdown table.
  python tools/mir_times.py profiles/mir_one_launch_times.md [--reps 7] [--warmup 2]"""
import argparse
import copy
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import golden_util as G  # noqa: E402
from jslpsolver_amd import Solve, _capi  # noqa: E402
from jslpsolver_amd.branch_and_cut import mir_loop  # noqa: E402
from jslpsolver_amd.engine import Tableau  # noqa: E402

INPUTS = (("Knapsack_1", None), ("LargeFarmMIP", 400), ("Monster_II", None))
TREES = ("Knapsack_1", "StockCuttingProblem", "LargeFarmMIP")


class _Ints:  # what mir_loop reads of a model
    useMIRCuts = True

    def __init__(self, ints):
        self.integer_index_set = frozenset(ints)


def passes(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        per.append(time.perf_counter() - t0)
    per.sort()
    return per[len(per) // 2], per[0], per[-1]


def cell(stats, n):
    med, lo, hi = stats
    return "%.1f (%.1f .. %.1f)" % (1e6 * med / n, 1e6 * lo / n, 1e6 * hi / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    lib = _capi.load_hip()
    lines = ["# A node's MIR loop: call by call against one call", "",
             "`tools/mir_times.py`, one MI355X, %d passes after %d warm-up passes; every cell is the median wall time PER NODE in microseconds with" % (a.reps, a.warmup),
             "(min .. max) of the passes behind it.  A pass evaluates every node of the list once (the batch forms in chunks of 16 / 302 nodes, the",
             "list repeated to fill the last chunk).  Every form was checked against the call-by-call loop before it was timed.", "",
             "| node list | nodes | MIR rounds per node | call by call | one applyCutsMIR per node | applyCutsBatchMIR x16 | applyCutsBatchMIR x302 |",
             "|---|---|---|---|---|---|---|"]
    for name, limit in INPUTS:
        g = G.load(os.path.join(G.GOLDEN, "fixtures", name + ".json.gz"))
        tab = g["tableau"]
        nodes = [c["cuts"] or [] for c in g["simplexCalls"][1:]][:limit]
        ints = _Ints(tab["integerVarIndexes"])
        m, vibr, vibc = G.dense_tableau(tab)
        t = Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"], row_capacity=tab["height"] + max(len(n) for n in nodes) + 320, lib=lib,
                    integer_variables=tab["integerVarIndexes"])
        t.applyCuts([], check_cycles=True)
        t.save()

        def by_call():
            out = []
            for cuts in nodes:
                _res, rhs, rows = t.applyCuts(cuts, check_cycles=True)
                rhs, rows = mir_loop(t, ints, rhs, rows, True)
                out.append((t.last.as_dict(), rhs.tobytes(), rows.tobytes()))
            return out

        def one_call():
            return [t.applyCutsMIR(cuts) for cuts in nodes]

        def chunks(size):
            idx = list(range(len(nodes)))
            idx += idx[:(-len(idx)) % size]
            return [[nodes[i] for i in idx[k:k + size]] for k in range(0, len(idx), size)], idx

        def batched(size):
            lists, _ = chunks(size)
            return [t.applyCutsBatchMIR(c) for c in lists]

        want = by_call()
        got = one_call()
        for w, (res, _oc, rhs, rows) in zip(want, got):
            d, x = res.as_dict(), dict(w[0])
            d.pop("evaluation"), x.pop("evaluation")
            assert d == x and rhs.tobytes() == w[1] and rows.tobytes() == w[2], "one call differs from the call-by-call loop"
        for size in (16, 302):
            _lists, idx = chunks(size)
            k = 0
            for results, _ocs, rhs, rows in batched(size):
                for j in range(len(results)):
                    h = results[j].height
                    assert rhs[j, :h].tobytes() == want[idx[k]][1] and rows[j, :h].tobytes() == want[idx[k]][2], "a batch differs from the call-by-call loop"
                    k += 1
        rounds = [int(oc["rounds"]) for _r, oc, _x, _w in got]
        s_call, s_one = passes(by_call, a.warmup, a.reps), passes(one_call, a.warmup, a.reps)
        s_16, s_302 = passes(lambda: batched(16), a.warmup, a.reps), passes(lambda: batched(302), a.warmup, a.reps)
        n16, n302 = len(chunks(16)[1]), len(chunks(302)[1])
        lines.append("| %s (%d x %d) | %d | %d .. %d, mean %.2f | %s | %s | %s | %s |" % (
            name, tab["height"], tab["width"], len(nodes), min(rounds), max(rounds), float(np.mean(rounds)), cell(s_call, len(nodes)), cell(s_one, len(nodes)),
            cell(s_16, n16), cell(s_302, n302)))
        t.close()
    lines += ["", "## Solve() of the MIR trees", "",
              "Wall time of `Solve(model with options.useMIRCuts)` in milliseconds, median (min .. max); the recorded iteration count in every column (asserted).", "",
              "| model | iterations | speculate 1 | speculate 1, JSLP_TREE_MIR=1 | speculate 8 |", "|---|---|---|---|---|"]
    import gzip
    import json
    with gzip.open(os.path.join(G.GOLDEN, "mir.json.gz"), "rt") as fh:
        cases = json.load(fh)["cases"]
    for name in TREES:  # the default service's recorded MIR trees (tests/golden/mir.json.gz), options as recorded
        case = next(c for c in cases if os.path.basename(c["file"]) == name + ".json.gz" and c["options"].get("useMIRCuts") and set(c["options"]) <= {"useMIRCuts", "tolerance"})
        model = copy.deepcopy(G.load(os.path.join(G.GOLDEN, case["file"]))["model"])
        model["options"] = case["options"]
        row = []
        for knob, spec in (("0", 1), ("1", 1), ("0", 8)):
            os.environ["JSLP_TREE_MIR"] = knob
            r = Solve(model, full=True, speculate=spec)
            assert r["iter"] == case["iterations"], "the tree differs from the recorded one"
            med, lo, hi = passes(lambda: Solve(model, speculate=spec), 1, max(3, a.reps // 2))
            row.append("%.1f (%.1f .. %.1f)" % (1e3 * med, 1e3 * lo, 1e3 * hi))
        os.environ.pop("JSLP_TREE_MIR", None)
        lines.append("| %s | %d | %s |" % (name, case["iterations"], " | ".join(row)))
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
