#!/usr/bin/env python3
"""fp32-vs-fp64 tolerance sweep.  For each model and each tolerance (the reference's `precision`)
the root LP is solved (a) by the fp64 engine created with that tolerance and (b) by the fp32 twin of the same kernels
(jslp_engine_simplex_f32) from the same initial tableau; reported: flags, pivots, objective error against the fp64 run at
the reference's default 1e-8, whether the final basis is the same, device time of the pivot loop.
Then, per model, the fp32 runs once more through the one-launch kernel (k32_simplex_lds, include/jslpf_f32.h): every tolerance alone
and ONE sweep call over all six, one workgroup each -- outcomes (those of the fp32 columns by construction: the tool says so when they
are not) and the device ms next to the select + update pair's, taken in the same process, alternating, REPEATS times each (median,
min .. max).
usage: tools/fp32_sweep.py [out.md] [one_launch_times.md]"""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from jslpsolver_amd import Model, Tableau, _capi, generators  # noqa: E402

TOLERANCES = [1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8]
REPEATS = 3


def fixture_tableau(name):
    with gzip.open(os.path.join(ROOT, "tests", "golden", "fixtures", name + ".json.gz"), "rt") as fh:
        g = json.load(fh)
    m = Model(g["model"])
    matrix, vibr, vibc = m.build_tableau()
    return matrix, vibr, vibc, m.unrestricted


def flags(r):
    return "feasible" if r.feasible and r.optimal else ("infeasible" if not r.feasible else ("unbounded" if not r.bounded else "stopped"))


def _outcome(run):
    r, rhs, rows = run
    return (r.feasible, r.bounded, r.optimal, r.pivots_phase1, r.pivots_phase2, r.obj_cell, rows.tolist(), rhs.tobytes())


def _spread(xs):
    xs = sorted(xs)
    return "%.2f (%.2f .. %.2f)" % (xs[len(xs) // 2], xs[0], xs[-1])


def one_launch_rows(lib, label, matrix, vibr, vibc, unr):
    """the one-launch kernel against jslp_engine_simplex_f32 on one model: a row per tolerance, then the six-tolerance sweep"""
    t = Tableau(matrix, vibr, vibc, unr, precision=1e-8, lib=lib)
    _, auto_path, _ = t.simplex_f32_sweep(TOLERANCES[:1], check_cycles=False, path="auto")
    auto = "one launch" if auto_path == _capi.JSLPF_PATH_ONE_LAUNCH else "select + update"
    try:
        t.simplex_f32_sweep(TOLERANCES, check_cycles=False, path="one_launch")  # warm-up: code object, six arena copies
    except _capi.EngineError as exc:
        t.close()
        return ["| %s | all | n/a | n/a | n/a | n/a | %s | %s |" % (label, auto, str(exc).split(": ", 1)[-1])]
    rows = []
    sum_single, sum_one, pivots_all = [0.0] * REPEATS, [0.0] * REPEATS, 0
    singles = []
    for tol in TOLERANCES:
        ms_old, ms_new, same = [], [], True
        for _ in range(REPEATS):
            r, rhs, rws, ms = t.simplex_f32(tol, check_cycles=False)
            ms_old.append(ms)
            runs, _, ms1 = t.simplex_f32_sweep([tol], check_cycles=False, path="one_launch")
            ms_new.append(ms1)
            same = same and _outcome(runs[0]) == _outcome((r, rhs, rws))
        singles.append((r, rhs, rws))
        pivots = r.pivots_phase1 + max(r.pivots_phase2, 0)
        pivots_all += pivots
        for k in range(REPEATS):
            sum_single[k] += ms_old[k]
            sum_one[k] += ms_new[k]
        rows.append("| %s | %.0e | %s / %d | %s | %s | %.2f | %s | %s |" % (
            label, tol, flags(r), pivots, _spread(ms_old), _spread(ms_new), sorted(ms_old)[REPEATS // 2] / sorted(ms_new)[REPEATS // 2], auto,
            "identical" if same else "DIFFERENT"))
    ms_sweep, same = [], True
    for _ in range(REPEATS):
        runs, _, ms = t.simplex_f32_sweep(TOLERANCES, check_cycles=False, path="one_launch")
        ms_sweep.append(ms)
        same = same and [_outcome(x) for x in runs] == [_outcome(x) for x in singles]
    t.close()
    rows.append("| %s | six in one call | %d pivots in all | %s (sum of six single calls) | %s (ONE sweep call; six one-launch calls: %s) | %.2f | %s | %s |" % (
        label, pivots_all, _spread(sum_single), _spread(ms_sweep), _spread(sum_one), sorted(sum_single)[REPEATS // 2] / sorted(ms_sweep)[REPEATS // 2],
        auto, "identical" if same else "DIFFERENT"))
    return rows


def main(out_path=None, times_path=None):
    lib = _capi.load_hip()
    os.environ.setdefault("JSLP_FORCE_PATH", "sp")  # same launch shape for both widths: select + update per pivot
    cases = [("Vendor Selection root LP (config 5)",) + fixture_tableau("Vendor_Selection"),
             ("Monster LP (config 2)",) + fixture_tableau("Monster_Problem"),
             ("Monster_II root LP (config 4)",) + fixture_tableau("Monster_II")]
    m, vibr, vibc = generators.dense_resource_allocation_tableau(12345, 500, 500)
    cases.append(("dense resource allocation 500x500 (config 3a generator)", m, vibr, vibc, []))
    lines = ["| model | tolerance | fp64: outcome / pivots / objective | fp32: outcome / pivots / objective | fp32 objective rel. error vs fp64@1e-8 | same final basis | device ms fp64 / fp32 (both through k_select + k_update) | fp64 through the engine's DEFAULT path: device ms (path) |",
             "|---|---|---|---|---|---|---|---|"]
    for label, matrix, vibr, vibc, unr in cases:
        ref = Tableau(matrix, vibr, vibc, unr, precision=1e-8, lib=lib)
        r_ref = ref.simplex(check_cycles=False)
        ref.close()
        for tol in TOLERANCES:
            t = Tableau(matrix, vibr, vibc, unr, precision=tol, lib=lib)
            r32, rhs32, rows32, ms32 = t.simplex_f32(tol, check_cycles=False)
            t.set_timing(True)
            r64 = t.simplex(check_cycles=False)
            _, _, ms64 = t.get_timing()
            rhs64, rows64 = t.read_rhs()
            t.close()
            # the same solve the way the engine runs it without knobs (register-resident / one LDS workgroup / fused): what an
            # fp32 variant would have to beat, not the select + update pair
            forced = os.environ.pop("JSLP_FORCE_PATH", None)
            td = Tableau(matrix, vibr, vibc, unr, precision=tol, lib=lib)
            td.set_timing(True)
            td.simplex(check_cycles=False)
            _, _, msd = td.get_timing()
            pathd = td.last_path()
            td.close()
            if forced is not None:
                os.environ["JSLP_FORCE_PATH"] = forced
            err = abs(r32.obj_cell - r_ref.obj_cell) / max(1.0, abs(r_ref.obj_cell))
            lines.append("| %s | %.0e | %s / %d / %.9g | %s / %d / %.9g | %.2e | %s | %.1f / %.1f | %.2f (%s) |" % (
                label, tol, flags(r64), r64.pivots_phase1 + max(r64.pivots_phase2, 0), r64.obj_cell,
                flags(r32), r32.pivots_phase1 + max(r32.pivots_phase2, 0), r32.obj_cell, err,
                "yes" if np.array_equal(rows32, rows64) else "no", ms64, ms32, msd, pathd))
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    lines = ["| model | tolerance | fp32 outcome / pivots | device ms, jslp_engine_simplex_f32 (k_select + k_update per pivot) | device ms, k32_simplex_lds (one launch) | select + update / one launch | AUTO takes | outcomes of the two paths |",
             "|---|---|---|---|---|---|---|---|"]
    for label, matrix, vibr, vibc, unr in cases:
        lines += one_launch_rows(lib, label, matrix, vibr, vibc, unr)
    text = "\n".join(lines) + "\n"
    print(text)
    if times_path:
        with open(times_path, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main(*sys.argv[1:3])
