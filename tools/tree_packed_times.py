#!/usr/bin/env python3
"""solve_packed on n small MILPs, on this tree and on another checkout of the project (the parent commit), in ONE session.
  python tools/tree_packed_times.py [--parent DIR] [--ns 1,8,64,512,4096] [--reps 3] [--rounds 3] [--soft milps|lps] [--mir] [--enh] [--inc] [--tol] [--parent-twice] [--out profiles/packed_tree_times.md]
Workload: the reference's default-policy fuzz MILPs that need no presolve pre-pass (tests/golden/fuzz_services.jsonl.gz), round robin up
to n models.  On this tree solve_packed walks every tree on the device, one launch for the whole batch (include/jslpt_tree.h); on a tree
without the extension (--parent: a built checkout of the parent commit) the same call walks each tree on the host through Solve.
Each tree runs in a worker process of its own (this file with --worker, importing the package from --root), and the two alternate
round by round, so both see the same machine in the same minutes.  A worker verifies EVERY result of every repetition against the
reference's recorded result (the rule of tests/test_fuzz_services.py::replay) before it reports a time.  Wall time is a host clock
around solve_packed, which ends in its own synchronisation and read-back; one warm-up call per n, then --reps timed calls; the table
reports the best and the median over all rounds.  Nothing is asserted about the ratio: the file records what was measured.
--soft: the workload is the reference's recorded SOFT-constraint runs instead (tests/golden/fuzz_soft.jsonl.gz: no options, no presolve, at
least one optional objective) -- `milps`: those with integer variables under the default service, `lps`: those without.  On a tree with
include/jslps_soft.h they run in the OPT builds of the pack kernels; on one without, solve_packed sends every one of them through Solve.
--mir: every fuzz model gets options.useMIRCuts -- the workload is the reference's recorded runs of the same models with exactly that option
(the same file), so every result is still verified against a record.  On a tree with include/jslpc_tree_mir.h every node's MIR loop runs
in the MIR builds of the tree kernel; on one without, solve_packed sends every one of them through Solve.
--enh: the workload is the reference's recorded runs under the ENHANCED service (the same file: {"nodeSelection": "depth-first"},
{"branching": "strong"}, {"nodeSelection": "best-first", "branching": "most-fractional"}), the three policies interleaved.  On a tree with
include/jslpe_tree_enhanced.h they run in the ENH builds of the tree kernel; on one without, solve_packed sends every one of them through Solve.
--inc: the workload is the reference's recorded runs under the INCREMENTAL service (the same file: {"useIncremental": true}), and the call is
solve_packed(models, incremental=True).  On a tree with include/jslpi_tree_incremental.h they run in the INC builds of the tree kernel, parent
checkpoints on the device; on one whose solve_packed has no such keyword every one of them goes through Solve.  The table then also reports
the share of evaluated nodes that started from a checkpoint (incremental_nodes / iterations over the workload's packs).
--tol: every default-policy fuzz model gets options.tolerance 0.05, and the call is solve_packed(models, tolerance=True).  On a tree with
include/jslpg_tree_tolerance.h the walks end on the reference's toleranceFlag inside the tree kernel; on one whose solve_packed has no such
keyword every one of them goes through Solve.  The reference recorded no run at that tolerance: every result is verified against Solve on the
CPU oracle library of the same checkout (tests/test_tree_tol_cpu.py holds that route to the reference's recorded runs with a tolerance).
--parent-twice: the parent checkout is measured as two entries of the alternation: the ratio of the second to the first is the run-to-run
spread of this tool on one and the same tree."""
import argparse
import gzip
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


ENH_OPTIONS = [{"nodeSelection": "depth-first"}, {"branching": "strong"}, {"branching": "most-fractional", "nodeSelection": "best-first"}]


TOL = 0.05


def cases(root, soft=None, mir=False, enh=False, inc=False, tol=False):
    with gzip.open(os.path.join(root, "tests", "golden", "fuzz_soft.jsonl.gz" if soft else "fuzz_services.jsonl.gz"), "rt") as fh:
        cs = [json.loads(line) for line in fh if line.startswith("{")]
    options = {"useMIRCuts": True} if mir else {"useIncremental": True} if inc else None
    if enh:  # (model after model, each under its three policies)
        cs = sorted((c for c in cs if c["model"].get("options") in ENH_OPTIONS and c["fixed"] == 0 and not c["infeasPre"]),
                    key=lambda c: (c["gen"], c["seed"], ENH_OPTIONS.index(c["model"]["options"])))
        return cs
    cs = [c for c in cs if (c["model"].get("options") or None) == options and c["fixed"] == 0 and not c["infeasPre"]]
    if tol:  # (the same models with the option; what they must give is the worker's to find out)
        cs = [dict(c, model=dict(c["model"], options={"tolerance": TOL})) for c in cs]
    if soft:  # (the selection of tests/soft_pack_util.py::soft_records)
        if root not in sys.path:
            sys.path.insert(0, root)
        from jslpsolver_amd.model import Model
        keep = []
        for c in cs:
            m = Model(c["model"], None)
            _, rows = m.optional_objectives()
            if rows is not None and len(rows) > 0 and (len(m.integerVariables) > 0) == (soft == "milps"):
                keep.append(c)
        cs = keep
    return cs


def worker(a):
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(a.root, "tests"))
    import numpy as np
    import golden_util as G
    from jslpsolver_amd import _capi
    from jslpsolver_amd import solver
    warnings.simplefilter("ignore")
    lib = _capi.Library(os.path.join(a.root, a.lib)) if a.lib else _capi.load_hip()
    cs = cases(a.root, a.soft, a.mir, a.enh, a.inc, a.tol)
    if a.tol:  # the yardstick of this workload: Solve on the CPU oracle, once per model
        oracle = _capi.Library(os.path.join(a.root, "oracle", "libjslp_oracle.so"))
        for c in cs:
            res = solver.Solve(c["model"], lib=oracle)
            c["keys"], c["result"] = list(res.keys()), {k: v for k, v in res.items()}
    # --inc: the keyword, on a tree whose solve_packed has it (the parent's sends these models through Solve whatever it is called with)
    import inspect
    with_keyword = a.inc and "incremental" in inspect.signature(solver.solve_packed).parameters
    solve_packed = (lambda models, lib: solver.solve_packed(models, lib=lib, incremental=True)) if with_keyword else solver.solve_packed
    with_tolerance = a.tol and "tolerance" in inspect.signature(solver.solve_packed).parameters
    if with_tolerance:
        solve_packed = lambda models, lib: solver.solve_packed(models, lib=lib, tolerance=True)  # noqa: E731
    seen = []  # (--inc) every pack the warm-up calls make: (nodes from a checkpoint, nodes) of its incremental LPs
    if with_keyword:
        plain = solver.TableauPack

        class Spy(plain):
            def branch_and_cut(self, check_cycles=True):
                try:
                    return plain.branch_and_cut(self, check_cycles=check_cycles)
                finally:
                    mine = self.is_incremental & (self.status == 0)
                    seen.append((int(self.incremental["incremental_nodes"][mine].sum()), int(self.tree["iterations"][mine].sum())))

    def verify(results, n):
        for k in range(n):
            c, res = cs[k % len(cs)], results[k]
            assert list(res.keys()) == c["keys"], (k, c["gen"], c["seed"])
            for key, v in c["result"].items():
                ref = v if isinstance(v, bool) or a.tol else G.num(v)
                assert res[key] == ref or (isinstance(ref, float) and np.isnan(ref) and np.isnan(res[key])), (k, key)

    for n in [int(x) for x in a.ns.split(",")]:
        models = [cs[k % len(cs)]["model"] for k in range(n)]
        if with_keyword:
            del seen[:]
            solver.TableauPack = Spy
        verify(solve_packed(models, lib=lib), n)  # warm-up: code objects, pooled streams, the allocator
        if with_keyword:
            solver.TableauPack = plain
        for _ in range(a.reps):
            t0 = time.perf_counter()
            results = solve_packed(models, lib=lib)
            dt = time.perf_counter() - t0
            verify(results, n)
            print(json.dumps({"n": n, "wall_ms": 1e3 * dt, "from_checkpoint": sum(x for x, _ in seen), "nodes": sum(y for _, y in seen),
                              "device_tree": with_tolerance and bool(getattr(lib, "has_tree_tol", False)) if a.tol else with_keyword and bool(getattr(lib, "has_tree_inc", False)) if a.inc else bool(getattr(lib, "has_tree_enh" if a.enh else "has_tree_mir" if a.mir else "has_soft" if a.soft else "has_tree", False))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--ns", default="1,8,64,512,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--soft", default=None, choices=["milps", "lps"], help="the recorded soft-constraint runs: those with / without integer variables")
    ap.add_argument("--mir", action="store_true", help="every fuzz model with options.useMIRCuts (the reference's recorded runs with that option)")
    ap.add_argument("--enh", action="store_true", help="the reference's recorded runs under the enhanced service (nodeSelection / branching), three policies")
    ap.add_argument("--inc", action="store_true", help="the reference's recorded runs under the incremental service (useIncremental), solve_packed(..., incremental=True)")
    ap.add_argument("--tol", action="store_true", help="every default-policy fuzz model with options.tolerance 0.05, solve_packed(..., tolerance=True)")
    ap.add_argument("--parent-twice", action="store_true", help="measure the parent checkout as two entries: the tool's spread on one tree")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--lib", default=None, help="engine library, relative to each checkout (default: the HIP product library); "
                    "oracle/libjslp_oracle.so rehearses the tool without a GPU -- its times say nothing")
    a = ap.parse_args()
    if sum(map(bool, (a.mir, a.soft, a.enh, a.inc, a.tol))) > 1:
        ap.error("--mir, --soft, --enh, --inc and --tol are five workloads")
    if a.worker:
        return worker(a)
    trees = [("this commit", HERE)] + ([("parent commit", os.path.abspath(a.parent))] if a.parent else [])
    if a.parent and a.parent_twice:
        trees.append(("parent commit, again", os.path.abspath(a.parent)))
    times = {name: {} for name, _ in trees}
    flags = {}
    shares = {}  # (--inc) n -> (nodes that started from a checkpoint, nodes evaluated) on this tree
    for _ in range(a.rounds):
        for name, root in trees:  # (the two alternate, round by round)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--ns", a.ns, "--reps", str(a.reps)] + (["--lib", a.lib] if a.lib else []) +
                                 (["--soft", a.soft] if a.soft else []) + (["--mir"] if a.mir else []) + (["--enh"] if a.enh else []) + (["--inc"] if a.inc else []) + (["--tol"] if a.tol else []),
                                 check=True, capture_output=True, text=True, timeout=900).stdout
            print("round done: %s" % name, file=sys.stderr, flush=True)
            for line in out.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    times[name].setdefault(r["n"], []).append(r["wall_ms"])
                    flags[name] = r["device_tree"]
                    if r.get("nodes"):
                        shares[r["n"]] = (r["from_checkpoint"], r["nodes"])
    n_models = len(cases(HERE, a.soft, a.mir, a.enh, a.inc, a.tol))
    what = {None: "default-policy fuzz MILPs", "milps": "recorded soft-constraint MILPs", "lps": "recorded soft-constraint LPs"}[a.soft]
    if a.mir:
        what = "fuzz MILPs with `options.useMIRCuts`"
    if a.enh:
        what = "fuzz MILPs under the enhanced service (three policies)"
    if a.inc:
        what = "fuzz MILPs with `options.useIncremental`"
    if a.tol:
        what = "default-policy fuzz MILPs with `options.tolerance` %s" % TOL
    lines = ["# `solve_packed(..., tolerance=True)` on small MILPs with `options.tolerance`: the walk ends on the tolerance inside the tree kernel against one engine per model (MI355X)" if a.tol else
             "# `solve_packed(..., incremental=True)` on small MILPs with `useIncremental`: the incremental service's tree and its checkpoints in the tree kernel against one engine per model (MI355X)" if a.inc else
             "# `solve_packed` on small MILPs with `nodeSelection` / `branching`: the enhanced service's tree in the tree kernel against one engine per model (MI355X)" if a.enh else
             "# `solve_packed` on small MILPs with MIR cuts: every node's MIR loop in the tree kernel against one engine per model (MI355X)" if a.mir else
             "# `solve_packed` on small MILPs: trees walked on the device against trees walked on the host (MI355X)" if not a.soft else
             "# `solve_packed` on the %s: the pack's OPT builds against one engine per model (MI355X)" % what, "",
             "`python tools/tree_packed_times.py --parent <checkout of the parent commit>%s --out %s`: one session, one " % ((" --mir" if a.mir else " --enh" if a.enh else " --inc" if a.inc else " --tol" if a.tol else "") + (" --parent-twice" if a.parent_twice else ""), "profiles/" + os.path.basename(a.out or "packed_tree_times.md")) +
             "device, %d rounds alternating between the two checkouts, each in a process of its own; per round one warm-up call and %d timed "
             "calls per n; wall time of `solve_packed(models)` on n models taken round robin from the %d %s; every result "
             "of every call verified against %s before its time was kept." % (a.rounds, a.reps, n_models, what,
                                                                            "`Solve` on the CPU oracle" if a.tol else "the reference's recorded result"), "",
             "| n | " + " | ".join("%s: best ms | median ms | trees/s (best)" % name for name, _ in trees) + (" | parent / this (best) |" if a.parent else " |") +
             (" parent again / parent (best) |" if a.parent and a.parent_twice else ""),
             "|---|" + "---|---|---|" * len(trees) + ("---|" if a.parent else "") + ("---|" if a.parent and a.parent_twice else "")]
    for n in [int(x) for x in a.ns.split(",")]:
        row, best = ["%d" % n], {}
        for name, _ in trees:
            ts = times[name][n]
            best[name] = min(ts)
            row += ["%.3f" % min(ts), "%.3f" % statistics.median(ts), "%.0f" % (n / (1e-3 * min(ts)))]
        if a.parent:
            row.append("%.2fx" % (best["parent commit"] / best["this commit"]))
            if a.parent_twice:
                row.append("%.2fx" % (best["parent commit, again"] / best["parent commit"]))
        lines.append("| " + " | ".join(row) + " |")
    lines += ["", "- %s: " % ("in the pack" if a.soft else "device-side trees") + ", ".join("%s: %s" % (name, "yes" if flags.get(name) else "no (each tree through `Solve`)") for name, _ in trees) + "."]
    if shares:
        lines.append("- nodes that started from a checkpoint on this commit (`incremental_nodes / iterations`): " +
                     ", ".join("n = %d: %d of %d (%.1f %%)" % (n, x, y, 100.0 * x / y) for n, (x, y) in sorted(shares.items())) + ".")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
