#!/usr/bin/env python3
"""n independent LPs: n sequential simplex() calls against ONE simplex_many call (include/jslpm_many.h), n in {1, 8, 64, 256, 1024}.
  python tools/many_lp_times.py [--reps R] [--ns 1,8,64,256,1024] [--workloads monster,small]
Workloads: copies of Monster LP (625 x 553); the small reference fixtures without optional objectives, round robin.  Every result is
checked against the first single-call result of its fixture (result struct, pivot digest, final tableau) before a number is printed.
Wall time is a host clock around calls that end in a synchronisation; device time comes from the engines' HIP events around each
simplex() (sequential: their sum) or around the batch launch (one interval).  Prints a markdown table; best of R repetitions, the
tableaus re-uploaded (untimed) before each."""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as G  # noqa: E402
from jslpsolver_amd import _capi  # noqa: E402
from jslpsolver_amd.engine import Tableau, pivot_digest, simplex_many  # noqa: E402

SMALL = ["Berlin_Air_Lift_Problem", "Chocolate_Problem", "Coffe_Problem", "Computer_Problem", "Wiki_1", "Shift_Work_Problem",
         "Cycling_Fletcher", "Generic_Business_Problem", "Stigler_Diet", "TacoParty", "Chevalier_1", "Wood_Shop_Problem"]


def tableau_of(name):
    g = G.load(os.path.join(G.GOLDEN, "fixtures", name + ".json.gz"))
    tab = g["tableau"]
    assert not tab["optionalObjectives"]
    m, vibr, vibc = G.dense_tableau(tab)
    return dict(m=m, vibr=vibr, vibc=vibc, unr=tab["unrestricted"], precision=tab["precision"], check=bool(tab["checkForCycles"]))


def signature(t, res):
    return (tuple(sorted(res.as_dict().items())), pivot_digest(t.pivot_trace()), hashlib.sha256(t.download()[0].tobytes()).hexdigest())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ns", default="1,8,64,256,1024")
    ap.add_argument("--workloads", default="monster,small")
    a = ap.parse_args()
    lib = _capi.load_hip()
    ns = [int(x) for x in a.ns.split(",")]
    print("| workload | n | sequential wall ms | sequential device ms | batch wall ms | batch device ms | sequential LPs/s | batch LPs/s | speed-up |")
    print("|---|---|---|---|---|---|---|---|---|")
    for wl in a.workloads.split(","):
        names = ["Monster_Problem"] if wl == "monster" else SMALL
        tabs = {n: tableau_of(n) for n in names}
        nmax = max(ns)
        t0 = time.perf_counter()
        engines = [Tableau(tabs[names[i % len(names)]]["m"], tabs[names[i % len(names)]]["vibr"], tabs[names[i % len(names)]]["vibc"],
                           tabs[names[i % len(names)]]["unr"], precision=tabs[names[i % len(names)]]["precision"], lib=lib)
                   for i in range(nmax)]
        sys.stderr.write("%s: %d engines created in %.1f s\n" % (wl, nmax, time.perf_counter() - t0))
        for t in engines:  # total_device_ms is kept only while timing is on (one-workgroup solves take the same launches either way)
            t.set_timing(True)
        which = [names[i % len(names)] for i in range(nmax)]
        checks = [tabs[w]["check"] for w in which]

        def reset(k):
            for t, w in zip(engines[:k], which[:k]):
                x = tabs[w]
                t.upload(x["m"], x["vibr"], x["vibc"], x["unr"])
            for t in engines[:k]:
                t.read_rhs()  # (an upload is asynchronous: this waits for it)

        expect = {}
        reset(len(names))
        for t, w, c in zip(engines, which, checks):
            if w not in expect:
                expect[w] = signature(t, t.simplex(check_cycles=c))
        for n in ns:
            best = {}
            for rep in range(a.reps + 1):  # (repetition 0 warms up)
                for mode in ("seq", "many"):
                    reset(n)
                    dev0 = [t.get_timing()[2] for t in engines[:n]]
                    w0 = time.perf_counter()
                    if mode == "seq":
                        res = [t.simplex(check_cycles=c) for t, c in zip(engines[:n], checks[:n])]
                    else:
                        res = simplex_many(engines[:n], check_cycles=checks[:n])
                    wall = time.perf_counter() - w0
                    dev1 = [t.get_timing()[2] for t in engines[:n]]
                    dev = sum(b - x for b, x in zip(dev1, dev0)) if mode == "seq" else dev1[0] - dev0[0]
                    for t, r, w in zip(engines[:n], res, which[:n]):
                        assert signature(t, r) == expect[w], (wl, n, mode, w)
                        assert t.last_path() == ("workgroup-many" if mode == "many" else "workgroup"), t.last_path()
                    if rep and (mode not in best or wall < best[mode][0]):
                        best[mode] = (wall, dev)
            (sw, sd), (bw, bd) = best["seq"], best["many"]
            print("| %s | %d | %.3f | %.3f | %.3f | %.3f | %.0f | %.0f | %.2fx |" % (
                "Monster LP" if wl == "monster" else "small fixtures", n, 1e3 * sw, sd, 1e3 * bw, bd, n / sw, n / bw, sw / bw), flush=True)
        for t in engines:
            t.close()


if __name__ == "__main__":
    main()
