"""jslpm_simplex_many on the MI355X: many independent LPs in one call, one workgroup per LP (k_simplex_lds_many).

Every LP of a batch is checked twice: against the reference's goldens (flags, evaluation, pivot counts, pivot digest, final tableau), and
against jslp_engine_simplex on a twin engine that never batched (the whole result struct, the final tableau and maps, the pivot trace).
The JSLP_DEBUG_LAUNCH lines say how many batch launches ran and with which build."""
import gzip
import json
import os
import re

import numpy as np
import pytest

import golden_util as G
from jslpsolver_amd import _capi, generators
from jslpsolver_amd.engine import Tableau, pivot_digest, simplex_many
from jslpsolver_amd.solver import _prepare

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"\[jslp\] launch k_simplex_lds_many<(\d+),opt (\d)> n (\d+) lds (\d+)")
SOFT = ("Relaxed", "Fertilizer", "Quadratic_Optimization_1", "Quadratic_Relaxation_1", "Quadratic_Relaxation_2", "Quadratic_Relaxation_3")


def _oo(tab):
    if not tab["optionalObjectives"]:
        return None
    return np.array([[G.num(x) for x in o["reducedCosts"]] + [0.0] * (tab["width"] - len(o["reducedCosts"]))
                     for o in tab["optionalObjectives"]], dtype=np.float64)


def _root_tableau(lib, g):
    """the engine of a golden's first simplex() call (the root relaxation for a MILP)"""
    tab = g["tableau"]
    m, vibr, vibc = G.dense_tableau(tab)
    return Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"], row_capacity=tab["height"], lib=lib,
                   optional_objectives=_oo(tab))


def _fixtures():
    out = {}
    for path in G.fixture_paths():
        g = G.load(path)
        if g["tableau"] is not None and not g["tableau"]["useMIRCuts"]:
            out[G.ident(path)] = g
    return out


def _state(t, res):
    fm, fvibr, fvibc, _, _ = t.download()
    return dict(res=res.as_dict(), evaluation=t.evaluation, trace=t.pivot_trace().tobytes(), matrix=fm.tobytes(),
                vibr=fvibr.tobytes(), vibc=fvibc.tobytes())


def _check_golden(t, res, g):
    """the batched LP against the reference's first simplex() call (and, for an LP, its whole solve)"""
    call = g["simplexCalls"][0]
    assert bool(res.feasible) == call["feasible"] and bool(res.bounded) == call["bounded"]
    assert (res.pivots_phase1, res.pivots_phase2, res.height) == (call["p1"], call["p2"], call["height"])
    ev = G.num(call["evaluation"])
    assert t.evaluation == ev or (np.isnan(ev) and np.isnan(t.evaluation))
    rhs, rows = t.read_rhs()
    assert G.sha_rhs(rhs, rows) == call["rhsSha"]
    trace = t.pivot_trace()
    n_root = call["p1"] + max(call["p2"], 0)
    assert trace.reshape(-1).tolist() == g["pivots"][:2 * n_root]
    if len(g["simplexCalls"]) == 1:  # an LP: the golden's final state is this call's
        assert len(trace) == g["nPivots"] and pivot_digest(trace) == g["pivotDigest"]
        assert G.sha_matrix(t.download()[0]) == g["final"]["matrixSha"]


def _batch_and_twins(lib, makers, check_cycles=True):
    """build each LP twice, solve one copy through simplex_many and the other through simplex(): the states must be identical"""
    batch = [mk() for mk in makers]
    twins = [mk() for mk in makers]
    flags = check_cycles if isinstance(check_cycles, list) else [check_cycles] * len(makers)
    res = simplex_many(batch, check_cycles=flags)
    ref = [t.simplex(check_cycles=c) for t, c in zip(twins, flags)]
    for i, (a, b, ra, rb) in enumerate(zip(batch, twins, res, ref)):
        assert _state(a, ra) == _state(b, rb), "LP %d differs from its twin" % i
    return batch, twins, res


def _close(*lists):
    for ts in lists:
        for t in ts:
            t.close()


def test_fixtures_in_one_launch(hip_lib, monkeypatch, capfd):
    """every small fixture without optional objectives, Monster LP and the Monster_II root: ONE launch, every LP right"""
    fx = _fixtures()
    twins = {n: _root_tableau(hip_lib, g) for n, g in fx.items() if not g["tableau"]["optionalObjectives"]}
    for t in twins.values():
        t.simplex(check_cycles=True)
    names = [n for n, t in twins.items() if t.last_path() == "workgroup"]
    _close(twins.values())
    assert "Monster_Problem" in names and "Monster_II" in names and len(names) >= 30
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    batch, tw, res = _batch_and_twins(hip_lib, [lambda n=n: _root_tableau(hip_lib, fx[n]) for n in names],
                                      [bool(fx[n]["tableau"]["checkForCycles"]) for n in names])
    lines = LAUNCH.findall(capfd.readouterr().err)
    assert len(lines) == 1 and lines[0][1] == "0" and int(lines[0][2]) == len(names), lines
    for n, t, r in zip(names, batch, res):
        assert t.last_path() == "workgroup-many", n
        _check_golden(t, r, fx[n])
    _close(batch, tw)


def _fuzz_soft_lps(lib, limit):
    with gzip.open(os.path.join(G.GOLDEN, "fuzz_soft.jsonl.gz"), "rt") as fh:
        cases = [json.loads(line) for line in fh]
    out = []
    for c in cases:
        m, t, n_int, _ = _prepare(c["model"], None, lib, 0, None)
        if n_int == 0 and t.n_optional > 0:
            out.append((c, m))
        t.close()
        if len(out) == limit:
            break
    return out


def test_mixed_batch_routes_every_lp(hip_lib, monkeypatch, capfd):
    """LPs that do not qualify for the batch are solved after it, through their own path: a dense 2001 x 2001 LP (register-resident),
    engines created with JSLP_NO_WGLDS=1 (generic one-workgroup kernel); the soft-constraint models take the OPT build"""
    fx = _fixtures()
    soft = [n for n in SOFT if n in fx]
    assert len(soft) == len(SOFT)
    dense = generators.dense_resource_allocation_tableau(12345, 2000, 2000)
    fuzz = _fuzz_soft_lps(hip_lib, 6)
    assert fuzz, "no soft-constraint LP among the fuzz goldens"

    def fuzz_tableau(c):
        return _prepare(c["model"], None, hip_lib, 0, None)[1]

    def no_wglds(name):
        monkeypatch.setenv("JSLP_NO_WGLDS", "1")
        try:
            return _root_tableau(hip_lib, fx[name])
        finally:
            monkeypatch.delenv("JSLP_NO_WGLDS")

    makers = ([lambda n=n: _root_tableau(hip_lib, fx[n]) for n in ("Berlin_Air_Lift_Problem", "Monster_Problem")] +
              [lambda: Tableau(*dense, lib=hip_lib)] +
              [lambda n=n: _root_tableau(hip_lib, fx[n]) for n in soft] +
              [lambda c=c: fuzz_tableau(c) for c, _ in fuzz] +
              [lambda n=n: no_wglds(n) for n in ("Chocolate_Problem", "Wiki_1")])
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    flags = [True] * len(makers)
    flags[2] = False  # (the dense golden's setting)
    batch, tw, res = _batch_and_twins(hip_lib, makers, flags)
    err = capfd.readouterr().err
    lines = LAUNCH.findall(err)
    n_soft = len(soft) + len(fuzz)
    n_opt = sum(t.n_optional > 0 for t in batch[3:3 + n_soft])  # (not every soft-constraint fixture keeps an optional objective)
    assert n_opt > len(fuzz)
    assert sorted((o, int(k)) for _, o, k, _ in lines) == [("0", 2 + n_soft - n_opt), ("1", n_opt)], lines
    paths = [t.last_path() for t in batch]
    assert paths[:2] == ["workgroup-many"] * 2
    assert paths[2] == "resident" == tw[2].last_path()
    assert paths[3:3 + n_soft] == ["workgroup-many"] * n_soft
    assert paths[3 + n_soft:] == ["workgroup"] * 2
    _check_golden(batch[0], res[0], fx["Berlin_Air_Lift_Problem"])
    _check_golden(batch[1], res[1], fx["Monster_Problem"])
    g = G.load(os.path.join(G.GOLDEN, "synthetic", "generateResourceAllocation_2000x2000_seed12345.json.gz"))
    assert len(batch[2].pivot_trace()) == g["nPivots"] and pivot_digest(batch[2].pivot_trace()) == g["pivotDigest"]
    assert G.sha_matrix(batch[2].download()[0]) == g["final"]["matrixSha"]
    for k, n in enumerate(soft):
        _check_golden(batch[3 + k], res[3 + k], fx[n])
    for k, (c, _) in enumerate(fuzz):
        t = batch[3 + len(soft) + k]
        assert len(t.pivot_trace()) == c["nPivots"] and pivot_digest(t.pivot_trace()) == c["digest"]
    for k, n in enumerate(("Chocolate_Problem", "Wiki_1")):
        _check_golden(batch[3 + n_soft + k], res[3 + n_soft + k], fx[n])
    _close(batch, tw)


def test_per_lp_cycle_check(hip_lib):
    """the cycle-hit goldens with the check on, side by side in one batch: phase, start and length as the reference reports them"""
    from test_cycle_goldens import _instance, _messages
    paths = sorted(p for p in G.glob.glob(os.path.join(G.GOLDEN, "cycles", "deg_*.json.gz")))
    assert len(paths) >= 5
    inst = [_instance(p) for p in paths]

    def mk(g, m, vibr, vibc):
        return lambda: Tableau(m, vibr, vibc, g["tableau"]["unrestricted"], precision=g["tableau"]["precision"], lib=hip_lib)

    fx = _fixtures()
    makers = [mk(*x) for x in inst] + [lambda: _root_tableau(hip_lib, fx["Berlin_Air_Lift_Problem"])]
    flags = [True] * len(inst) + [False]
    batch, tw, res = _batch_and_twins(hip_lib, makers, flags)
    for (g, _, _, _), t, r in zip(inst, batch, res):
        assert t.last_path() == "workgroup-many"
        assert _messages(r) == g["messages"]
        assert (r.pivots_phase1, r.pivots_phase2) == (g["simplexCalls"][0]["p1"], g["simplexCalls"][0]["p2"])
        assert pivot_digest(t.pivot_trace()) == g["pivotDigest"]
    assert res[-1].cycle_phase == 0
    _check_golden(batch[-1], res[-1], fx["Berlin_Air_Lift_Problem"])
    _close(batch, tw)


def test_per_lp_error_goes_to_its_status(hip_lib):
    """a cycling LP with the check off runs into the iteration cap: its status says so, the call returns it naming the LP, and the
    other LP of the batch is solved and right"""
    from test_cycle_goldens import _instance
    fx = _fixtures()
    g, m, vibr, vibc = _instance(os.path.join(G.GOLDEN, "cycles", "deg_178868.json.gz"))  # (cycles for ever without the check)
    a = _root_tableau(hip_lib, fx["Berlin_Air_Lift_Problem"])
    b = Tableau(m, vibr, vibc, g["tableau"]["unrestricted"], precision=g["tableau"]["precision"], lib=hip_lib)
    out = (_capi.SimplexResult * 2)()
    status = np.full(2, 7, dtype=np.int32)
    handles = (_capi.C.c_void_p * 2)(a._h.value, b._h.value)
    cc = np.array([1, 0], dtype=np.int32)
    assert hip_lib.jslpm_simplex_many(handles, 2, _capi.ptr_i32(cc), out, _capi.ptr_i32(status)) == _capi.JSLP_ERR_CAPACITY
    assert status.tolist() == [_capi.JSLP_OK, _capi.JSLP_ERR_CAPACITY]
    assert b"LP 1" in hip_lib.jslp_last_error() and b"iteration" in hip_lib.jslp_last_error()
    a._absorb(out[0])
    _check_golden(a, out[0], fx["Berlin_Air_Lift_Problem"])
    _close([a, b])


# Residency of k_simplex_lds_many<512, false> (profiles/many_lp_kernel_resources.md): 63 VGPRs / 106 SGPRs -> 7 waves per SIMD; a 512-thread
# workgroup is 2 waves per SIMD -> 3 workgroups per CU (a small LP's LDS, a few KB, does not bind) -> 768 on the 256 CUs.  2048 LPs are
# more than twice what the chip holds at once.
OVERSUBSCRIBED = 2048


def test_oversubscribed_batch(hip_lib, monkeypatch, capfd):
    fx = _fixtures()
    names = ["Berlin_Air_Lift_Problem", "Chocolate_Problem", "Coffe_Problem", "Computer_Problem", "Wiki_1", "Degenerate_Max",
             "Infeasible_1", "Unrestricted", "Cycling_Fletcher", "Shift_Work_Problem"]
    names = [n for n in names if n in fx and not fx[n]["tableau"]["optionalObjectives"]]
    assert len(names) >= 6
    twins = []
    for n in names:
        t = _root_tableau(hip_lib, fx[n])
        r = t.simplex(check_cycles=True)
        twins.append(_state(t, r))
        t.close()
    batch = [_root_tableau(hip_lib, fx[names[i % len(names)]]) for i in range(OVERSUBSCRIBED)]
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    res = simplex_many(batch, check_cycles=True)
    lines = LAUNCH.findall(capfd.readouterr().err)
    assert len(lines) == 1 and lines[0][0] == "512" and int(lines[0][2]) == OVERSUBSCRIBED
    for i, (t, r) in enumerate(zip(batch, res)):
        assert t.last_path() == "workgroup-many"
        assert _state(t, r) == twins[i % len(names)], i
    _close(batch)


def test_engines_stay_usable_after_a_batch(hip_lib):
    """save / restore / relax and a second batch on engines that went through simplex_many: identical to twins that never batched"""
    fx = _fixtures()
    names = ["Integer_Wood_Shop_Problem", "Knapsack_1", "Monster_II"]
    batch = [_root_tableau_with_cuts(hip_lib, fx[n]) for n in names]
    twins = [_root_tableau_with_cuts(hip_lib, fx[n]) for n in names]
    res = simplex_many(batch)
    ref = [t.simplex() for t in twins]
    for a, b, ra, rb in zip(batch, twins, res, ref):
        assert _state(a, ra) == _state(b, rb)
    for n, a, b in zip(names, batch, twins):
        a.save(); b.save()
        cuts = fx[n]["simplexCalls"][1]["cuts"] or []
        ra, rha, rwa = a.applyCuts(cuts)
        rb, rhb, rwb = b.applyCuts(cuts)
        assert ra.as_dict() == rb.as_dict() and rha.tobytes() == rhb.tobytes() and rwa.tobytes() == rwb.tobytes()
        a.restore(); b.restore()
    res = simplex_many(batch)
    ref = [t.simplex() for t in twins]
    for a, b, ra, rb in zip(batch, twins, res, ref):
        assert a.last_path() == "workgroup-many"
        assert _state(a, ra) == _state(b, rb)
    _close(batch, twins)


def _root_tableau_with_cuts(lib, g):
    tab = g["tableau"]
    m, vibr, vibc = G.dense_tableau(tab)
    max_cuts = max([len(c["cuts"] or []) for c in g["simplexCalls"]] + [0])
    return Tableau(m, vibr, vibc, tab["unrestricted"], precision=tab["precision"], row_capacity=tab["height"] + max_cuts, lib=lib)


def test_argument_errors_solve_nothing(hip_lib):
    fx = _fixtures()
    a, b = _root_tableau(hip_lib, fx["Berlin_Air_Lift_Problem"]), _root_tableau(hip_lib, fx["Wiki_1"])
    n = 3
    out = (_capi.SimplexResult * n)()
    status = np.full(n, 7, dtype=np.int32)
    handles = (_capi.C.c_void_p * n)(a._h.value, b._h.value, a._h.value)
    assert hip_lib.jslpm_simplex_many(handles, n, None, out, _capi.ptr_i32(status)) == _capi.JSLP_ERR_ARG
    assert b"twice" in hip_lib.jslp_last_error()
    assert status.tolist() == [7, 7, 7] and len(a.pivot_trace()) == 0 and len(b.pivot_trace()) == 0
    with pytest.raises(_capi.EngineError):
        simplex_many([a, b, a])
    # an engine that was never uploaded
    raw = _capi.C.c_void_p()
    hip_lib.check(hip_lib.jslp_engine_create(_capi.C.byref(raw), 0, 4, 4, 4, 1e-8), "jslp_engine_create")
    handles = (_capi.C.c_void_p * 2)(a._h.value, raw.value)
    assert hip_lib.jslpm_simplex_many(handles, 2, None, out, _capi.ptr_i32(status)) == _capi.JSLP_ERR_STATE
    assert b"engine 1" in hip_lib.jslp_last_error() and b"upload" in hip_lib.jslp_last_error()
    assert status.tolist() == [7, 7, 7] and len(a.pivot_trace()) == 0
    hip_lib.jslp_engine_destroy(raw)
    # afterwards the same engines solve as ever
    twin = _root_tableau(hip_lib, fx["Berlin_Air_Lift_Problem"])
    res = simplex_many([a, b])
    assert _state(a, res[0]) == _state(twin, twin.simplex())
    _close([a, b, twin])


def test_solve_many_on_the_gpu(hip_lib, oracle_lib):
    from jslpsolver_amd import Solve, solve_many
    fx = _fixtures()
    models = [g["model"] for n, g in fx.items() if n not in ("Vendor_Selection", "LargeFarmMIP", "Monster_II", "StockCuttingProblem")]
    got = solve_many(models + models[:3], lib=hip_lib)
    assert [repr(r) for r in got] == [repr(Solve(m, lib=oracle_lib)) for m in models + models[:3]]
