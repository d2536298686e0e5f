#!/usr/bin/env python3
"""n small independent LPs: ONE simplex_many call over n engines (include/jslpm_many.h) against ONE TableauPack (include/jslpp_packed.h).
  python tools/packed_lp_times.py [--reps R] [--ns 1,8,64,256,1024,16384] [--workloads small,farm] [--soft] [--out profiles/packed_lp_times.md]
Workloads: the small reference fixtures without optional objectives, round robin (the workload of tools/many_lp_times.py); copies of the
LargeFarmMIP root (36 x 101: the 256-thread build).  simplex_many is the yardstick: its code is what the parent commit runs, in the same
process; it is run for n <= 1024 (an engine per LP beyond that is minutes of set-up).  At n = 1 a single Tableau.simplex() is timed too.
Every result is checked against the first single-engine result of its fixture (result struct, pivot digest, sha256 of the final tableau)
BEFORE a number is printed.  Wall time is a host clock around calls that end in their own synchronisation (the pack's: launch + the one
read-back + decode); device time comes from HIP events (the engines' around the batch launch, the pack's around its launches on its own
stream).  One warm-up, then the best of R repetitions; the two paths alternate; tableaus are re-uploaded before each repetition (untimed
for simplex_many; timed separately for the pack: `pack wall incl. upload`).
--soft adds the workload `soft`: the fixtures WITH optional objectives (Relaxed, Fertilizer), round robin, in a pack made with
optional_objectives= (include/jslps_soft.h: the OPT build of the pack kernel).  simplex_many takes no such engines, so the yardstick of
that workload is one Tableau.simplex() per LP, one after the other; the check also covers the optional rows after the solve."""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import golden_util as G  # noqa: E402
from jslpsolver_amd import _capi  # noqa: E402
from jslpsolver_amd.engine import Tableau, TableauPack, pivot_digest, simplex_many  # noqa: E402

SMALL = ["Berlin_Air_Lift_Problem", "Chocolate_Problem", "Coffe_Problem", "Computer_Problem", "Wiki_1", "Shift_Work_Problem",
         "Cycling_Fletcher", "Generic_Business_Problem", "Stigler_Diet", "TacoParty", "Chevalier_1", "Wood_Shop_Problem"]
SOFT = ["Relaxed", "Fertilizer"]
MANY_MAX = 1024


def tableau_of(name, soft=False):
    g = G.load(os.path.join(G.GOLDEN, "fixtures", name + ".json.gz"))
    tab = g["tableau"]
    assert bool(tab["optionalObjectives"]) == soft
    m, vibr, vibc = G.dense_tableau(tab)
    oo = np.array([[G.num(v) for v in o["reducedCosts"]] for o in tab["optionalObjectives"]], dtype=np.float64) if soft else None
    return dict(m=m, vibr=vibr, vibc=vibc, unr=tab["unrestricted"], precision=tab["precision"], check=bool(tab["checkForCycles"]), oo=oo)


def signature(res, trace, matrix, optional=None):
    return (tuple(sorted(res.as_dict().items())), pivot_digest(trace), hashlib.sha256(matrix.tobytes()).hexdigest(),
            None if optional is None else hashlib.sha256(optional.tobytes()).hexdigest())


def upload(t, x):
    """the tableau again, and its optional rows as they were given"""
    t.upload(x["m"], x["vibr"], x["vibc"], x["unr"])
    if x["oo"] is not None:
        t.lib.check(t.lib.jslp_engine_set_optional_objectives(t._h, int(x["oo"].shape[0]), _capi.ptr_f64(x["oo"])), "jslp_engine_set_optional_objectives")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ns", default="1,8,64,256,1024,16384")
    ap.add_argument("--workloads", default="small,farm")
    ap.add_argument("--out", default=None)
    ap.add_argument("--soft", action="store_true", help="add the workload of the fixtures with optional objectives")
    a = ap.parse_args()
    lib = _capi.load_hip()
    ns = [int(x) for x in a.ns.split(",")]
    lines = ["| workload | n | simplex_many wall ms | simplex_many device ms | pack simplex wall ms | pack wall ms incl. upload | pack device ms | "
             "simplex_many LPs/s | pack LPs/s | wall ratio |", "|---|---|---|---|---|---|---|---|---|---|"]
    notes = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    print("\n".join(lines), flush=True)
    for wl in a.workloads.split(",") + (["soft"] if a.soft else []):
        soft = wl == "soft"
        names = ["LargeFarmMIP"] if wl == "farm" else SOFT if soft else SMALL
        label = "LargeFarmMIP root 36 x 101" if wl == "farm" else "soft fixtures (yardstick: one `Tableau.simplex()` per LP)" if soft else "small fixtures"
        tabs = {n: tableau_of(n, soft) for n in names}
        expect = {}
        for n in names:  # the yardstick of every check: a single engine that never saw a batch or a pack
            x = tabs[n]
            t = Tableau(x["m"], x["vibr"], x["vibc"], x["unr"], precision=x["precision"], lib=lib, optional_objectives=x["oo"])
            r = t.simplex(check_cycles=x["check"])
            expect[n] = signature(r, t.pivot_trace(), t.download()[0], t.optional_objectives() if soft else None)
            t.close()
        n_eng = min(max(ns), MANY_MAX)
        which_all = [names[i % len(names)] for i in range(max(ns))]
        t0 = time.perf_counter()
        engines = [Tableau(tabs[w]["m"], tabs[w]["vibr"], tabs[w]["vibc"], tabs[w]["unr"], precision=tabs[w]["precision"], lib=lib,
                           optional_objectives=tabs[w]["oo"]) for w in which_all[:n_eng]]
        sys.stderr.write("%s: %d engines created in %.1f s\n" % (wl, n_eng, time.perf_counter() - t0))
        for t in engines:
            t.set_timing(True)
        for n in ns:
            which = which_all[:n]
            checks = [tabs[w]["check"] for w in which]
            t0 = time.perf_counter()
            pack = TableauPack([(tabs[w]["m"], tabs[w]["vibr"], tabs[w]["vibc"], tabs[w]["unr"]) for w in which],
                               precision=[tabs[w]["precision"] for w in which], lib=lib, trace_cap=1024,
                               **({"optional_objectives": [tabs[w]["oo"] for w in which]} if soft else {}))
            create_s = time.perf_counter() - t0
            best = {}
            for rep in range(a.reps + 1):  # (repetition 0 warms up)
                for mode in ("many", "pack", "single"):
                    if mode == "many" and n > MANY_MAX:
                        continue
                    if mode == "single" and n != 1:
                        continue
                    if mode == "pack":
                        u0 = time.perf_counter()
                        pack.upload()
                        w0 = time.perf_counter()
                        pack.simplex(check_cycles=checks)
                        w1 = time.perf_counter()
                        wall, wall_up, dev = w1 - w0, w1 - u0, pack.device_ms
                        # every LP's result struct on every repetition; its trace and final tableau too -- for n > 2048 on the first and the
                        # last repetition (two read-back calls per LP: they would otherwise be most of this tool's run time)
                        full = n <= 2048 or rep in (0, a.reps)
                        for i, w in enumerate(which):
                            assert tuple(sorted(pack.result(i).as_dict().items())) == expect[w][0], (wl, n, i, w)
                            if full:
                                assert signature(pack.result(i), pack.pivot_trace(i), pack.download(i)[0],
                                                 pack.optional_objectives(i) if soft else None) == expect[w], (wl, n, i, w)
                    else:
                        for t, w in zip(engines[:n], which):
                            upload(t, tabs[w])
                        for t in engines[:n]:
                            t.read_rhs()  # (an upload is asynchronous: this waits for it)
                        dev0 = engines[0].get_timing()[2]
                        w0 = time.perf_counter()
                        if mode == "single":
                            res = [engines[0].simplex(check_cycles=checks[0])]
                        elif soft:
                            res = [t.simplex(check_cycles=c) for t, c in zip(engines[:n], checks)]
                        else:
                            res = simplex_many(engines[:n], check_cycles=checks)
                        wall = time.perf_counter() - w0
                        wall_up, dev = wall, engines[0].get_timing()[2] - dev0
                        for t, r, w in zip(engines[:n], res, which):
                            assert signature(r, t.pivot_trace(), t.download()[0], t.optional_objectives() if soft else None) == expect[w], (wl, n, mode, w)
                    if rep and (mode not in best or wall < best[mode][0]):
                        best[mode] = (wall, wall_up, dev)
                    if rep and mode == "pack":
                        best["pack_up"] = min(best.get("pack_up", wall_up), wall_up)
            pw, _, pd = best["pack"]
            pu = best["pack_up"]
            if "many" in best:
                mw, _, md = best["many"]
                emit("| %s | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.0f | %.0f | %.2fx |" % (label, n, 1e3 * mw, md, 1e3 * pw, 1e3 * pu, pd, n / mw, n / pw, mw / pw))
            else:
                emit("| %s | %d | - | - | %.3f | %.3f | %.3f | - | %.0f | - |" % (label, n, 1e3 * pw, 1e3 * pu, pd, n / pw))
            if "single" in best:
                notes.append("- %s, n = 1: a single `Tableau.simplex()` takes %.3f ms wall (%.3f ms device); the pack %.3f ms wall (%.3f ms device)."
                             % (label, 1e3 * best["single"][0], best["single"][2], 1e3 * pw, pd))
            notes.append("- %s, n = %d: `TableauPack(...)` (create + set + first upload) took %.1f ms." % (label, n, 1e3 * create_s))
            pack.close()
        for t in engines:
            t.close()
    print("\n".join(notes), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# `TableauPack` against `simplex_many`: wall and device time (MI355X)\n\n`python tools/packed_lp_times.py --out %s` "
                     "(one session, one device; best of %d after one warm-up; every row verified against single-engine results before it was "
                     "printed).\n\n" % (a.out, a.reps))
            fh.write("\n".join(lines) + "\n\n" + "\n".join(notes) + "\n")


if __name__ == "__main__":
    main()
