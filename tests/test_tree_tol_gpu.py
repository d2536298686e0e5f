"""jslpg_* on the MI355X: options.tolerance honoured inside k_tree_packed, in every build (include/jslpg_tree_tolerance.h).

The yardsticks are the reference's recorded runs (tests/golden/tolerance.json.gz, the tolerance records of mir.json.gz) and the three Python
host walks on the CPU oracle behind TableauPack's restatement; the pack on the GPU is never compared with itself."""
import copy
import ctypes
import re
import warnings

import numpy as np
import pytest

import soft_pack_util as S
import tree_enh_util as E
import tree_inc_util as I
import tree_mir_util as M
import tree_pack_util as U
import tree_tol_util as T
from jslpsolver_amd import Solve, _capi, solver

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"\[jslp\] launch k_tree_packed<(\d+)(?:,(opt|mir|enh|inc) 1)?(,tol 1)?> n (\d+) lds (\d+)")


def _with(model, **options):
    m = copy.deepcopy(model)
    m["options"] = dict(m.get("options") or {}, **options)
    return m


def test_golden_records_in_one_pack(hip_lib, oracle_lib):
    """the records test_tree_tol_cpu.py replays on the restatement, in ONE pack on the device: states, the tree / MIR / enhanced / incremental
    records, the tolerance record and the pivot trace against the host walks as bytes, then every record's iterations, digest and result"""
    fit = [(c, m, T.lp_of(m)) for c, m in T.golden_records()]
    fit = [(c, m, lp) for c, m, lp in fit if lp is not None and not (c.get("file", "").endswith("LargeFarmMIP.json.gz") and c["options"].get("useMIRCuts"))]
    assert len(fit) == 83
    items, policies = [lp[0] for _, _, lp in fit], [lp[1] for _, _, lp in fit]
    pack, host = T.against_host(hip_lib, oracle_lib, items, policies, [m["options"]["tolerance"] for _, m, _ in fit],
                                [it.model.isMinimization for it in items], heap_cap=8192, trace_cap=max(c["nPivots"] for c, _, _ in fit) + 16)
    assert not pack.status.any() and 1 <= pack.launches <= 8
    for i, (c, _, _) in enumerate(fit):
        T.check_golden(pack, i, items[i], c)
    assert 20 < int(pack.tolerance["stopped"].sum()) < len(fit)
    pack.close()
    host.close()


def test_both_builds_every_service_every_tolerance_both_senses(hip_lib, oracle_lib):
    """Integer_Wood_Shop_Problem (3 x 4, the one-wave build) and Knapsack_1 (52 x 51, 256 threads) under the default service, with one
    constraint made soft (an optional objective: the OPT builds), with MIR cuts, under the nine enhanced pairs and under the incremental
    service, each without a tolerance and at 1e-9, 0.05, 0.5 and 3, as the maximisation it is and as the minimisation of the negated
    objective (the same tableau, the other factor).  Every record starts as 0x5a bytes (tree_tol_util.solve)."""
    items, policies, tolerance, minimize, build = [], [], [], [], []
    for name, threads in (("Integer_Wood_Shop_Problem", 64), ("Knapsack_1", 256)):
        model = U.fixture(name)["model"]
        for sense in (model, T.negated(model)):
            soft = copy.deepcopy(sense)  # one more constraint, soft and wide: an optional objective beside the same hard problem
            soft["constraints"]["soft"] = {"max": 1000, "weight": 1, "priority": 1}
            for v in soft["variables"].values():
                v["soft"] = 1
            lps = [("plain", U.Item(sense), None), ("opt", S.SoftItem(soft), None), ("mir", M.MirItem(_with(sense, useMIRCuts=True)), None)]
            assert lps[1][1].n_optional > 0
            lps += [("enh", U.Item(sense), pair) for pair in E.PAIRS]
            lps.append(("inc", I.Item(sense), I.Inc()))
            assert lps[0][1].lp[0].tobytes() == U.Item(model).lp[0].tobytes()
            for kind, it, policy in lps:
                for tol in T.TOLERANCES:
                    items.append(it)
                    policies.append(policy)
                    tolerance.append(tol)
                    minimize.append(it.model.isMinimization)
                    build.append((kind, threads))
    assert len(items) == 2 * 2 * 13 * 5 and sum(minimize) == len(items) // 2
    pack, host = T.against_host(hip_lib, oracle_lib, items, policies, tolerance, minimize)
    assert pack.launches == 20 and not pack.status.any()  # every build of k_tree_packed and its TOL twin
    rec = pack.tolerance
    for b in sorted(set(build)):
        mine = [j for j in range(len(items)) if build[j] == b and tolerance[j] is not None]
        stopped, ran_on = sum(int(rec[j]["stopped"]) == 1 for j in mine), sum(int(rec[j]["stopped"]) == 0 for j in mine)
        assert stopped >= 1 and ran_on >= 1, (b, stopped, ran_on)
    assert len(set(build)) == 10
    # an LP without tolerance has a record of zeros and is the LP of a pack without the arrays
    none = [j for j in range(len(items)) if tolerance[j] is None]
    assert all(rec[j].tobytes() == bytes(32) for j in none)
    plain = T.solve(hip_lib, [items[j] for j in none], [policies[j] for j in none], None, None, with_arrays=False)
    got = T.states(pack)
    for k, j in enumerate(none):
        assert T.state(plain, k) == got[j], j
        assert pack.optional_objectives(j).tobytes() == plain.optional_objectives(k).tobytes()
    for j in range(len(items)):
        assert pack.optional_objectives(j).tobytes() == host.optional_objectives(j).tobytes(), j
    # a tolerance that never bites (1e-9) leaves the walk of no tolerance and reports why: nothing stopped
    for j in range(len(items)):
        if tolerance[j] == 1e-9 and int(rec[j]["stopped"]) == 0:
            same = dict(got[j - 1], tolerance=got[j]["tolerance"])
            assert same == got[j] and tolerance[j - 1] is None, j
    plain.close()
    pack.close()
    host.close()


def test_the_edges(hip_lib, oracle_lib):
    up = T.EXACT_UP
    lps = [(T.LATE, None, 0.5),                                      # 0: the late node becomes the incumbent
           (T.EXACT, None, 0.25), (T.EXACT, None, up),                  # 1, 2: equality does not stop, the next factor does
           (T.MAXI, ("hybrid", None), 1), (T.MAXI, ("hybrid", None), 3), (T.MAXI, None, 1), (T.MAXI, None, 3), (T.MAXI, None, float("inf")),  # 3 - 7
           (T.LATE_ROOT, None, 0.5), (T.NO_OPTIMUM, None, 0.5),         # 8, 9: bestPossibleEval from the second node, from none
           (T.INTEGRAL_ROOT, None, 0.5),                                # 10
           (T.MAXI, ("hybrid", None), 0.5),                             # 11: the hybrid switch, then the stop
           (T.MAXI, ("depth-first", "most-fractional"), 0.5),           # 12: a depth-first stop
           (T.MAXI, I.Inc(), 0.5), (T.MAXI, I.Inc("depth-first"), 3),   # 13, 14: incremental, checkpoints taken
           (T.negated(T.INTEGRAL_ROOT), None, float("inf")),            # 15: 0 * -Infinity: a NaN threshold
           (T.negated(T.NO_OPTIMUM), None, float("inf"))]               # 16: the same where bestPossibleEval stays 0
    items = [I.Item(m) if isinstance(p, I.Inc) else U.Item(m) for m, p, _ in lps]
    policies, tolerance = [p for _, p, _ in lps], [t for _, _, t in lps]
    minimize = [m["opType"] == "min" for m, _, _ in lps]
    pack, host = T.against_host(hip_lib, oracle_lib, items, policies, tolerance, minimize)
    rec, tree = pack.tolerance, pack.tree
    row = lambda j: (int(tree[j]["iterations"]), float(rec[j]["best_possible"]), float(rec[j]["threshold"]), int(rec[j]["stopped"]), int(rec[j]["left"]))  # noqa: E731
    # 1: a kernel that broke at once would report 8 iterations and 29 (test_tree_tol_cpu.py shows it on the host walk with an immediate break)
    now = T.host_walk(oracle_lib, items[0], None, 0.5, True, _late_stop=False)
    assert (row(0)[0], float(pack.evaluation[0]), row(0)[3:]) == (9, 28.0, (1, 4)) and (now[0], now[2]) == (8, 29.0)
    # 2
    assert row(1) == (5, 100.0, 125.0, 0, 0) and float(pack.evaluation[1]) == 125.0
    assert row(2) == (3, 100.0, 100.0 * float(np.nextafter(1.25, 2)), 1, 2) and row(2)[2] > 125.0 and float(pack.evaluation[2]) == 125.0
    # 3: factors 0 and -2 (and -Infinity): thresholds -0.0, 63 and +Infinity
    assert row(3) == (21, -31.5, 0.0, 1, 4) and np.signbit(rec[3]["threshold"]) and row(4) == (21, -31.5, 63.0, 1, 4)
    assert row(5)[3:] == (0, 0) and row(6) == (5, -31.5, 63.0, 0, 0) and row(7) == (5, -31.5, float("inf"), 0, 0)  # (empty before the flag is looked at)
    # 4
    assert row(8) == (3, -8.0, -4.0, 1, 2) and row(9) == (1, 0.0, 0.0, 0, 0) and not pack.feasible[9]
    # 5: one iteration; bestPossibleEval is the root's evaluation, everything else of the record is zero
    assert row(10) == (1, 50.0, 0.0, 0, 0) and int(tree[10]["is_integral"]) == 1
    # 6: the first incumbent (turn 20) moves the stack into the heap; turn 21 lowers the flag and runs; turn 22 stops
    assert row(11) == (21, -31.5, -15.75, 1, 4) and int(pack.enhanced[11]["moved_to_heap"]) == 5 and int(pack.enhanced[11]["solutions_found"]) == 2
    assert T.host_walk(oracle_lib, items[11], policies[11], 0.5, False, _late_stop=False)[0] == 20
    # 7: the stack is not empty
    assert row(12) == (21, -31.5, -15.75, 1, 4) and int(pack.enhanced[12]["moved_to_heap"]) == 0 and int(pack.enhanced[12]["stack_high_water"]) == 7
    # 8
    for j in (13, 14):
        assert row(j)[3:] == (1, 4) and int(pack.incremental[j]["checkpoints_used"]) == 12 and int(pack.incremental[j]["incremental_nodes"]) == 20
    # a threshold of 0 * -Infinity is reported as the quiet NaN 0x7ff8000000000000 whatever sign the multiplier gave it
    for j in (15, 16):
        assert rec[j]["threshold"].tobytes() == np.float64("nan").tobytes() == bytes.fromhex("000000000000f87f") and row(j)[3:] == (0, 0)
    pack.close()
    host.close()


def test_max_nodes_on_the_turn_that_lowers_the_flag(hip_lib, oracle_lib):
    """9: LATE lowers its flag at the top of turn 9 with 8 nodes evaluated: with max_nodes 8 that turn reports the capacity, not a stop, and
    the LP's entries -- the tolerance record among them -- stay as they were; with 9 the walk ends on the flag"""
    items = [U.Item(T.LATE), U.Item(T.EXACT)]
    for max_nodes, fails in ((8, True), (9, False)):
        out = []
        for lib in (hip_lib, oracle_lib):
            pack = T.make_pack(lib, items, [None, None], [0.5, 0.25], [True, True], max_nodes=max_nodes)
            if lib is hip_lib:
                raw = (ctypes.c_char * 64)()
                assert lib.jslpg_pack_read_tolerance(pack._h, raw) == _capi.JSLP_ERR_STATE  # (before a tree call)
            pack.tolerance[:] = np.frombuffer(b"\x5a" * pack.tolerance.nbytes, dtype=pack.tolerance.dtype)
            try:
                pack.branch_and_cut(check_cycles=[it.check for it in items])
                err = None
            except _capi.EngineError as e:
                err = str(e)
            out.append((pack, err))
        (pack, err), (host, herr) = out
        if fails:
            assert err is not None and "(%d)" % _capi.JSLP_ERR_CAPACITY in err and "LP 0" in err and "max_nodes" in err and "max_nodes" in herr
            assert list(pack.status) == list(host.status) == [_capi.JSLP_ERR_CAPACITY, _capi.JSLP_OK]
            assert pack.tolerance[0].tobytes() == host.tolerance[0].tobytes() == b"\x5a" * 32
        else:
            assert err is None and herr is None and int(pack.tree[0]["iterations"]) == 9 and int(pack.tolerance[0]["stopped"]) == 1
            assert T.state(pack, 0) == T.state(host, 0)
        assert T.state(pack, 1) == T.state(host, 1) and int(pack.tolerance[1]["stopped"]) == 0  # the neighbour is right either way
        pack.close()
        host.close()


def test_one_mixed_pack(hip_lib, oracle_lib, monkeypatch, capfd):
    """LPs with and without a tolerance side by side, one of every kind each: one launch per build -- the LPs without a tolerance in the
    builds, and with the launch lines, of a pack without tolerances, the others in the TOL twins -- and the LPs without one are, byte for
    byte, the LPs of a pack made by jslpi_tree_pack_create"""
    wood, knap = U.fixture("Integer_Wood_Problem")["model"], U.fixture("Knapsack_1")["model"]
    soft = copy.deepcopy(wood)
    name = next(iter(soft["constraints"]))
    soft["constraints"][name] = dict(soft["constraints"][name], weight=1, priority=1)
    kinds = [(lambda: U.Item(wood), None), (lambda: S.SoftItem(soft), None), (lambda: M.MirItem(_with(wood, useMIRCuts=True)), None),
             (lambda: U.Item(knap), ("hybrid", "strong")), (lambda: I.Item(knap), I.Inc()), (lambda: I.Item(T.MAXI), I.Inc("depth-first", "most-fractional", 2))]
    items, policies, tolerance = [], [], []
    for make, policy in kinds:
        for tol in (None, 0.5):
            items.append(make())
            policies.append(policy)
            tolerance.append(tol)
    minimize = [it.model.isMinimization for it in items]
    assert items[2].n_optional > 0
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack, host = T.against_host(hip_lib, oracle_lib, items, policies, tolerance, minimize)
    lines = LAUNCH.findall(capfd.readouterr().err)
    plain = T.solve(hip_lib, items, policies, None, None, with_arrays=False)  # jslpi_tree_pack_create: the pack has incremental LPs
    plain_lines = LAUNCH.findall(capfd.readouterr().err)
    monkeypatch.delenv("JSLP_DEBUG_LAUNCH")
    six = [(64, "inc"), (64, "mir"), (64, "opt"), (64, "plain"), (256, "enh"), (256, "inc")]
    assert pack.launches == 12 and plain.launches == 6
    assert sorted((int(t), kind or "plain", tol, int(n)) for t, kind, tol, n, _ in plain_lines) == [(t, kind, "", 2) for t, kind in six], plain_lines
    # the same six lines for the LPs without a tolerance (one LP each now, the same LDS bytes), and the six TOL twins beside them
    assert sorted((int(t), kind or "plain", tol, int(n)) for t, kind, tol, n, _ in lines) == sorted(
        [(t, kind, "", 1) for t, kind in six] + [(t, kind, ",tol 1", 1) for t, kind in six]), lines
    assert [(t, kind, b) for t, kind, tol, n, b in lines if not tol] == [(t, kind, b) for t, kind, tol, n, b in plain_lines]
    got = T.states(pack)
    for j in range(0, len(items), 2):
        assert T.state(plain, j) == got[j], j
        assert pack.optional_objectives(j).tobytes() == plain.optional_objectives(j).tobytes() == host.optional_objectives(j).tobytes()
        assert pack.optional_objectives(j + 1).tobytes() == host.optional_objectives(j + 1).tobytes()
        assert pack.tolerance[j].tobytes() == bytes(32) and pack.tolerance[j + 1]["best_possible"] != 0
    assert int(pack.tolerance["stopped"].sum()) >= 3
    for p in (pack, host, plain):
        p.close()


def test_solve_packed_with_the_keyword(hip_lib, oracle_lib):
    cases = U._cases("fuzz_services.jsonl.gz")[:60]
    models = [_with(c["model"], tolerance=tol) for c in cases for tol in (0.05, 1)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [repr(Solve(m, lib=oracle_lib)) for m in models]
        assert [repr(r) for r in solver.solve_packed(models, lib=hip_lib, tolerance=True, incremental=True)] == want
        assert [repr(r) for r in solver.solve_packed(models, lib=hip_lib, tolerance=True)] == want
        assert [repr(r) for r in solver.solve_packed(models[:16], lib=hip_lib)] == want[:16]
