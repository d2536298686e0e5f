#!/usr/bin/env python3
"""Tableaus between 64 KiB and 156 KiB of LDS: the large builds of the pack kernels (include/jslpb_big_lds.h) against what the parent commit
does with the same models, in ONE session.
  python tools/packed_big_times.py --parent DIR [--ns 1,8,64,512,4096] [--reps 3] [--rounds 2] [--workloads lp100,lp138,lp193,sudoku,knapsack]
                                   [--candidates LIB[,LIB...]] [--parent-twice] [--many-max 512] [--out profiles/packed_big_times.md]
LP workloads: n LPs from generators.dense_resource_allocation_tableau at 100 x 100, 138 x 138 and 193 x 65 (four seeds, round robin).  On this
tree they go through ONE TableauPack(big_lds=True); on the parent (--parent: a built checkout of the parent commit) through ONE simplex_many
call over n engines, for n <= --many-max (an engine per LP beyond that is minutes of set-up).  Every LP of every repetition is verified against
a twin engine of the same library that never saw a pack or a batch (result struct, pivot digest, sha256 of the final tableau).
Tree workloads: `sudoku`, the Sudoku4x4 fixture replicated n times through solve_packed(big_lds=True) -- on the parent through solve_packed,
which sends every copy through Solve; `knapsack`, Knapsack_1 replicated n times in a tree pack at row capacity 252 (cut_rows = 200: the large
build) -- on the parent in a tree pack at its default 96 cut rows (the 256-thread build).  Every result is verified against the fixture's
golden (the result object; the knapsack's 79 evaluated nodes, 500 pivots and pivot digest).
Each entry runs in a worker process of its own (this file with --worker) and the entries alternate round by round, so all see the same machine
in the same minutes.  Wall time is a host clock around calls that end in their own synchronisation; one warm-up per n, then --reps timed
calls; the table has the best and the median over all rounds.  --parent-twice measures the parent as two entries: the ratio of the two is the
run-to-run spread of this tool.  --candidates: development libraries of THIS tree built at other thread counts of the large class
(-DJSLP_PACK_BIG_THREADS=256 | 512 | 1024 on every unit), each measured as an entry of its own beside the shipped library; an entry's label is
what its jslpb_pack_big_threads() answers.  Nothing is asserted about a ratio: the file records what was measured."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"lp100": (100, 100), "lp138": (138, 138), "lp193": (193, 65)}
SEEDS = 4
KNAPSACK_BIG_CUT_ROWS = 200  # row capacity 52 + 200 = 252: an image of 111 088 bytes


def worker(a):
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(a.root, "tests"))
    import numpy as np
    import golden_util as G
    from jslpsolver_amd import _capi, generators, solver
    from jslpsolver_amd.engine import Tableau, TableauPack, pivot_digest, simplex_many
    warnings.simplefilter("ignore")
    lib = _capi.Library(os.path.abspath(a.lib)) if a.lib else _capi.load_hip()
    big = bool(getattr(lib, "has_big_lds", False)) and not a.as_parent
    label = "T=%d" % lib.jslpb_pack_big_threads() if big else "parent"
    ns = [int(x) for x in a.ns.split(",")]

    def signature(res, trace, matrix):
        return (tuple(sorted(res.as_dict().items())), pivot_digest(trace), hashlib.sha256(matrix.tobytes()).hexdigest())

    def timed(call, check):
        call()  # warm-up
        check()
        walls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            walls.append(time.perf_counter() - t0)
            check()
        return walls

    for wl in a.workloads.split(","):
        if wl in SHAPES:
            h, w = SHAPES[wl]
            lps = [generators.dense_resource_allocation_tableau(9000 + 17 * k + h, w - 1, h - 1) + ([],) for k in range(SEEDS)]
            expect = []
            for lp in lps:  # the yardstick of every check: a single engine that never saw a batch or a pack
                t = Tableau(*lp, lib=lib)
                expect.append(signature(t.simplex(check_cycles=True), t.pivot_trace(), t.download()[0]))
                t.close()
            for n in ns:
                if big:
                    pack = TableauPack([lps[i % SEEDS] for i in range(n)], lib=lib, trace_cap=2048, max_pivots=100000, big_lds=True)

                    def call():
                        pack.upload()
                        pack.simplex(check_cycles=True)

                    def check():
                        assert pack.is_big.all() and not pack.status.any()
                        for i in range(n):
                            assert tuple(sorted(pack.result(i).as_dict().items())) == expect[i % SEEDS][0], (wl, n, i)
                        for i in range(0, n, max(1, n // 64)):  # (the trace and the final tableau: two read-backs per LP, of a sample)
                            assert signature(pack.result(i), pack.pivot_trace(i), pack.download(i)[0]) == expect[i % SEEDS], (wl, n, i)
                    walls = timed(call, check)
                    dev = pack.device_ms
                    pack.close()
                elif n <= a.many_max:
                    engines = [Tableau(*lps[i % SEEDS], lib=lib) for i in range(n)]
                    out = []

                    def call():
                        for i, t in enumerate(engines):
                            t.upload(*lps[i % SEEDS])
                        del out[:]
                        out.extend(simplex_many(engines, check_cycles=True))

                    def check():
                        for i in range(0, n, max(1, n // 64)):
                            assert signature(out[i], engines[i].pivot_trace(), engines[i].download()[0]) == expect[i % SEEDS], (wl, n, i)
                    walls = timed(call, check)
                    dev = 0.0
                    for t in engines:
                        t.close()
                else:
                    continue
                print(json.dumps(dict(label=label, workload=wl, n=n, walls=walls, device_ms=dev)), flush=True)
        else:
            g = G.load(os.path.join(G.GOLDEN, "fixtures", ("Sudoku4x4" if wl == "sudoku" else "Knapsack_1") + ".json.gz"))
            want = {k: (v if isinstance(v, bool) else G.num(v)) for k, v in g["result"].items()}
            for n in ns:
                models = [g["model"]] * n
                got = []
                if wl == "sudoku":
                    def call():
                        del got[:]
                        got.extend(solver.solve_packed(models, lib=lib, big_lds=True) if big else solver.solve_packed(models, lib=lib))

                    def check():
                        for r in got:
                            assert list(r.keys()) == g["resultKeys"] and r == want, (wl, n)
                    walls = timed(call, check)
                else:
                    sys.path.insert(0, os.path.join(a.root, "tests"))
                    import tree_pack_util as U
                    item = U.Item(g["model"], cut_rows=KNAPSACK_BIG_CUT_ROWS if big else None)
                    kw = dict(big_lds=True) if big else {}
                    pack = TableauPack([item.lp] * n, precision=[item.precision] * n, lib=lib, trace_cap=1024, max_pivots=100000, integers=[item.integers] * n,
                                       cut_rows=[item.cut_rows] * n, heap_cap=256, max_nodes=4096, **kw)

                    def call():
                        pack.upload()
                        pack.branch_and_cut(check_cycles=item.check)

                    def check():
                        assert not pack.status.any() and (pack.is_big.all() if big else True)
                        for i in range(0, n, max(1, n // 64)):
                            U.check_record(pack, i, item, g["nPivots"], g["pivotDigest"], g["final"]["branchAndCutIterations"], g["resultKeys"], g["result"], (wl, n, i))
                    walls = timed(call, check)
                    pack.close()
                print(json.dumps(dict(label=label, workload=wl, n=n, walls=walls, device_ms=0.0)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--ns", default="1,8,64,512,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--workloads", default="lp100,lp138,lp193,sudoku,knapsack")
    ap.add_argument("--candidates", default=None, help="development libraries of this tree at other thread counts of the large class, comma separated")
    ap.add_argument("--parent-twice", action="store_true")
    ap.add_argument("--many-max", type=int, default=512)
    ap.add_argument("--timeout", type=int, default=900, help="seconds one worker may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--as-parent", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    entries = [("this", HERE, None)] + [("cand%d" % k, HERE, p) for k, p in enumerate((a.candidates or "").split(",")) if p]
    if a.parent:
        a.parent = os.path.abspath(a.parent)
        entries += [("parent", a.parent, None)] + ([("parent again", a.parent, None)] if a.parent_twice else [])
    rows = {}  # (workload, n) -> entry name -> [walls]
    labels = {}
    for rnd in range(a.rounds):
        for name, root, lib in entries:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--ns", a.ns, "--reps", str(a.reps), "--workloads", a.workloads,
                   "--many-max", str(a.many_max)] + (["--lib", lib] if lib else []) + (["--as-parent"] if name.startswith("parent") else [])
            out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout, check=True, cwd=root).stdout.decode()
            for line in out.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    labels[name] = r["label"] if not name.startswith("parent") else name
                    rows.setdefault((r["workload"], r["n"]), {}).setdefault(name, []).extend(r["walls"])
            sys.stderr.write("round %d: %s done\n" % (rnd, name))
    names = [n for n, _, _ in entries]
    lines = ["| workload | n | " + " | ".join("%s best ms (median)" % labels.get(n, n) for n in names) + " | parent / this (best) |",
             "|---|---|" + "---|" * (len(names) + 1)]
    for (wl, n), by in rows.items():
        cells = ["%.3f (%.3f)" % (1e3 * min(by[x]), 1e3 * statistics.median(by[x])) if x in by else "-" for x in names]
        ratio = "%.2fx" % (min(by["parent"]) / min(by["this"])) if "parent" in by and "this" in by else "-"
        lines.append("| %s | %d | %s | %s |" % (wl, n, " | ".join(cells), ratio))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n`python tools/packed_big_times.py %s`\n\n%s\n" % (" ".join(x for x in sys.argv[1:]), text))


if __name__ == "__main__":
    main()
