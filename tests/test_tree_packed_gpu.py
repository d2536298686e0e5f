"""jslpt_pack_* on the MI355X: small MILPs in a pack, each tree walked by one workgroup inside one launch (k_tree_packed).

The yardsticks are the reference's recorded runs (goldens, fuzz records) and the Python host tree on the CPU oracle
(branch_and_cut.branch_and_cut behind TableauPack's restatement); the pack on the GPU is never compared with itself.  The
JSLP_DEBUG_LAUNCH lines say how many launches ran, with which build and how many LPs each."""
import re

import numpy as np
import pytest

import tree_pack_util as U
from jslpsolver_amd import Solve, _capi
from jslpsolver_amd.engine import Tableau, TableauPack
from test_cycle_goldens import SMALL as CYCLE_GOLDENS, _instance

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"\[jslp\] launch k_tree_packed<(\d+)> n (\d+) lds (\d+)")
LDS_LIMIT = 65536
ROUTING_CELLS = 2048  # PACK_CELLS_WAVE (jslp_hip.hip): at most this many cells AT THE ROW CAPACITY -> the one-wave build


def _launches(capfd):
    return [(int(t), int(n), int(b)) for t, n, b in LAUNCH.findall(capfd.readouterr().err)]


def _against_host(hip_lib, oracle_lib, items, **kw):
    """one pack on the GPU, one call; every LP against the Python host tree on the oracle: result struct, tree counters, evaluation, final
    RHS column and row map, pivot trace -- all as bytes"""
    host = U.solve(oracle_lib, items, **kw)
    pack = U.solve(hip_lib, items, **kw)
    for i, (a, b) in enumerate(zip(U.states(pack), U.states(host))):
        assert a == b, "LP %d differs from the host tree: %s" % (i, [k for k in a if a[k] != b[k]])
    return pack, host


def test_reference_records_in_one_pack(hip_lib, oracle_lib, monkeypatch, capfd):
    cases, n_services = U.fuzz_default_cases()
    assert 80 <= n_services <= 90 and len(cases) - n_services >= 10
    items = [U.Item(c["model"]) for c in cases]
    fx = {n: U.fixture(n) for n in U.TREE_FIXTURES}
    items += [U.Item(fx[n]["model"]) for n in U.TREE_FIXTURES]
    assert all(it.cut_rows >= 1 and len(it.integers) > 0 for it in items)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack, host = _against_host(hip_lib, oracle_lib, items)
    lines = _launches(capfd)
    assert 1 <= len(lines) <= 2 and sum(n for _, n, _ in lines) == len(items) and pack.launches == len(lines), lines
    assert all(b <= LDS_LIMIT for _, _, b in lines)
    for i, c in enumerate(cases):
        U.check_record(pack, i, items[i], c["nPivots"], c["digest"], c["iter"], c["keys"], c["result"], (c["gen"], c["seed"]))
    for k, n in enumerate(U.TREE_FIXTURES):
        g = fx[n]
        U.check_record(pack, len(cases) + k, items[len(cases) + k], g["nPivots"], g["pivotDigest"], g["final"]["branchAndCutIterations"],
                       g["resultKeys"], g["result"], n)
    assert int(pack.tree["iterations"].max()) >= 79  # Knapsack_1's tree
    pack.close()
    host.close()


BERLIN = {"optimize": "capacity", "opType": "max",
          "constraints": {"plane": {"max": 44}, "person": {"max": 512}, "cost": {"max": 300000}},
          "variables": {"brit": {"capacity": 20000, "plane": 1, "person": 8, "cost": 5000},
                        "yank": {"capacity": 30000, "plane": 1, "person": 16, "cost": 9000}},
          "ints": {"brit": 1, "yank": 1}}
INFEASIBLE = {"optimize": "z", "opType": "max", "constraints": {"a": {"max": 4}, "b": {"min": 6}},
              "variables": {"x": {"z": 1, "a": 1, "b": 1}, "y": {"z": 2, "a": 1, "b": 1}}, "ints": {"x": 1, "y": 1}}
UNBOUNDED = {"optimize": "z", "opType": "max", "constraints": {"a": {"min": 1.5}},
             "variables": {"x": {"z": 1, "a": 1}, "y": {"z": 1, "a": 2}}, "ints": {"x": 1, "y": 1}}
# 2 x + 2 y = 3 has no integer point: the root is fractional and every leaf is infeasible
NO_INTEGRAL = {"optimize": "z", "opType": "max", "constraints": {"a": {"equal": 3}, "b": {"max": 10}},
               "variables": {"x": {"z": 1, "a": 2, "b": 1}, "y": {"z": 1, "a": 2, "b": 1}}, "ints": {"x": 1, "y": 1}}


def _node_log(oracle_lib, item, monkeypatch):
    """(optimal, feasible, cycle_phase) of every relaxation of the host tree on the oracle, in order"""
    log = []
    orig = Tableau._absorb
    monkeypatch.setattr(Tableau, "_absorb", lambda self, res: (log.append((res.optimal, res.feasible, res.cycle_phase)), orig(self, res))[1])
    U.solve(oracle_lib, [item]).close()
    monkeypatch.setattr(Tableau, "_absorb", orig)
    return log


def test_tree_edges(hip_lib, oracle_lib, monkeypatch):
    items = [U.Item(BERLIN), U.Item(INFEASIBLE), U.Item(UNBOUNDED), U.Item(NO_INTEGRAL), U.Item(U.fixture("Integer_Wood_Shop_Problem")["model"])]
    # a cycle inside a node: every tests/golden/cycles instance with one variable declared integer cycles AT THE ROOT (node 1) and no later
    # node of any of them does (searched on the CPU over every instance and every column), so the root it is
    g, m, vibr, vibc = _instance(CYCLE_GOLDENS[0])
    cyc = U.RawItem((m, vibr, vibc, g["tableau"]["unrestricted"]), [int(vibc[1])], precision=g["tableau"]["precision"], check=True)
    items.append(cyc)
    pack, host = _against_host(hip_lib, oracle_lib, items)
    t = pack.tree
    # integral at the root: no save, iterations == 1, no cut row
    assert (t[0]["iterations"], t[0]["is_integral"], t[0]["final_height"], t[0]["nodes_pushed"]) == (1, 1, items[0].lp[0].shape[0], 1)
    assert U.result_of(pack, 0, items[0]) == {"feasible": True, "result": 1080000, "bounded": True, "isIntegral": True, "brit": 24, "yank": 20}
    assert t[1]["iterations"] == 1 and not pack.feasible[1] and not t[1]["is_integral"]
    # an unbounded root has the evaluation -Infinity, which prunes nothing: the tree goes on below it and ends on an unbounded node
    assert t[2]["iterations"] > 1 and not pack.bounded[2] and pack.evaluation[2] == -np.inf
    # no integral node: the state is the LAST node's -- an infeasible leaf with cut rows -- and the evaluation the one carried over from
    # the last node that reached an optimum
    log = _node_log(oracle_lib, items[3], monkeypatch)
    assert t[3]["iterations"] == len(log) >= 3 and not t[3]["is_integral"] and log[0][0] and not log[-1][0]
    assert not pack.feasible[3] and t[3]["final_height"] > items[3].lp[0].shape[0] and pack.results[3]["optimal"] == 0
    assert pack.evaluation[3] == host.evaluation[3] != 0.0
    # a node that reaches no optimum between nodes that do
    log = _node_log(oracle_lib, items[4], monkeypatch)
    flags = [o for o, _, _ in log[:-1]]  # (the last entry is the final re-evaluation)
    assert any(not flags[k] and any(flags[:k]) and any(flags[k + 1:]) for k in range(len(flags))), flags
    assert t[4]["iterations"] == len(flags) and t[4]["is_integral"]
    # the cycle: found with the check on, inside node 1; the node is infeasible and the tree ends
    assert pack.results[5]["cycle_phase"] != 0 and pack.results[5]["cycle_length"] > 0 and not pack.feasible[5] and t[5]["iterations"] == 1
    pack.close()
    host.close()


# (height, width, first k structural variables integer, seed): seeds picked on the CPU for trees of 3 .. 200 nodes
DENSE = [(10, 63, 5, 40), (10, 64, 5, 4), (10, 65, 5, 43),         # one wave, a row of 63 / 64 / 65 cells
         (20, 63, 10, 4), (20, 64, 10, 8), (20, 65, 10, 1),          # four waves
         (62, 20, 10, 1), (62, 63, 10, 2),                           # height + cuts crosses 64 during the tree (66 rows), in both builds
         (22, 64, 5, 28), (22, 65, 5, 16), (24, 64, 5, 4)]           # 2048 / 2080 / 2176 cells at the row capacity: both sides of the routing


def test_lane_and_thread_edges(hip_lib, oracle_lib, monkeypatch, capfd):
    items = [U.dense_item(h, w, k, seed) for h, w, k, seed in DENSE]
    # one shape at the LDS limit: the largest cut_rows that fits
    h, w, k, seed = 60, 65, 10, 1
    cut_rows = 2 * k
    while hip_lib.jslpt_lds_bytes(h, w, h + cut_rows + 1) <= LDS_LIMIT:
        cut_rows += 1
    assert hip_lib.jslpt_lds_bytes(h, w, h + cut_rows) <= LDS_LIMIT < hip_lib.jslpt_lds_bytes(h, w, h + cut_rows + 1)
    items.append(U.dense_item(h, w, k, seed, cut_rows=cut_rows))
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack, host = _against_host(hip_lib, oracle_lib, items)
    lines = _launches(capfd)
    n_wave = sum((it.lp[0].shape[0] + it.cut_rows) * it.lp[0].shape[1] <= ROUTING_CELLS for it in items)
    assert sorted((t, n) for t, n, _ in lines) == [(64, n_wave), (256, len(items) - n_wave)] and 0 < n_wave < len(items), lines
    assert max(b for _, _, b in lines) == hip_lib.jslpt_lds_bytes(h, w, h + cut_rows)
    its = host.tree["iterations"]
    assert its.min() >= 3 and its.max() <= 200, its
    crossing = [i for i, (hh, _, _, _) in enumerate(DENSE) if hh == 62]
    assert all(host.tree[i]["final_height"] > 64 for i in crossing)
    pack.close()
    host.close()
    over = U.dense_item(h, w, k, seed, cut_rows=cut_rows + 1)
    with pytest.raises(_capi.EngineError, match=r"\(-6\).*LP 1"):
        U.make_pack(hip_lib, [items[0], over])


def test_oversubscribed_trees(hip_lib, oracle_lib, monkeypatch, capfd):
    names = [n for n in U.TREE_FIXTURES if n != "Knapsack_1"][:8]
    base = [U.Item(U.fixture(n)["model"]) for n in names]
    host = U.solve(oracle_lib, base, trace_cap=128, heap_cap=16)
    want = U.states(host)
    copies = 4096
    items = [base[i % 8] for i in range(copies * 8)]
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack = U.solve(hip_lib, items, trace_cap=128, heap_cap=16)
    lines = _launches(capfd)
    assert len(lines) == 1 and lines[0][:2] == (64, copies * 8), lines
    assert not pack.status.any()
    for j in range(8):  # the result structs and the counters of a fixture's copies, all at once
        assert pack.results[j::8].tobytes() == host.results[j].tobytes() * copies, names[j]
        assert pack.tree[j::8].tobytes() == host.tree[j].tobytes() * copies, names[j]
    for i in range(copies * 8):  # and every copy's RHS column, row map and trace
        assert U.state(pack, i) == want[i % 8], i
    pack.close()
    # isolation: a plain pack and a Solve on the same library are still right
    lps = TableauPack([it.lp for it in base], precision=[it.precision for it in base], lib=hip_lib, trace_cap=128)
    ref = TableauPack([it.lp for it in base], precision=[it.precision for it in base], lib=oracle_lib, trace_cap=128)
    assert lps.simplex().tobytes() == ref.simplex().tobytes()
    assert all(lps.read_rhs(i)[0].tobytes() == ref.read_rhs(i)[0].tobytes() for i in range(8))
    lps.close()
    ref.close()
    g = U.fixture("Knapsack_1")
    assert repr(Solve(g["model"], lib=hip_lib)) == repr(Solve(g["model"], lib=oracle_lib))
    host.close()


def test_per_lp_status(hip_lib, oracle_lib):
    """each capacity of Knapsack_1's tree set exactly to its measure succeeds; set one lower, the LP between two neighbours gets
    JSLP_ERR_CAPACITY naming the LP and the capacity, its out / tree_out sentinels are untouched, and both neighbours are right"""
    knap, wood = U.Item(U.fixture("Knapsack_1")["model"]), U.Item(U.fixture("Integer_Wood_Shop_Problem")["model"])
    host = U.solve(oracle_lib, [wood, knap, wood])
    want = U.states(host)
    m = host.tree[1]
    caps = dict(max_nodes=int(m["iterations"]), heap_cap=int(m["heap_high_water"]), cut_rows=int(m["cuts_high_water"]))
    assert caps["max_nodes"] > 50 and caps["heap_cap"] > 30 and caps["cut_rows"] > 10

    def run(**over):
        c = dict(caps, **over)
        its = [wood, U.RawItem(knap.lp, knap.integers, cut_rows=c["cut_rows"], precision=knap.precision, check=knap.check), wood]
        pack = U.make_pack(hip_lib, its, heap_cap=[256, c["heap_cap"], 256], max_nodes=c["max_nodes"])
        out = np.zeros(3, dtype=_capi.RESULT_DTYPE)
        out["pivots_phase1"] = 777  # sentinels
        tree = np.full(3, 55, dtype=np.int32).repeat(6).view(_capi.TREE_DTYPE)
        status = np.full(3, 7, dtype=np.int32)
        rc = hip_lib.jslpt_pack_branch_and_cut(pack._h, None, out.ctypes.data, tree.ctypes.data, _capi.ptr_i32(status), None)
        return pack, rc, out, tree, status, hip_lib.jslp_last_error().decode()

    pack, rc, out, tree, status, _ = run()
    assert rc == _capi.JSLP_OK and status.tolist() == [0, 0, 0]
    assert out[1].tobytes() == host.results[1].tobytes() and tree[1].tobytes() == host.tree[1].tobytes()
    pack.close()
    for which in ("max_nodes", "heap_cap", "cut_rows"):
        pack, rc, out, tree, status, msg = run(**{which: caps[which] - 1})
        assert rc == _capi.JSLP_ERR_CAPACITY and status.tolist() == [0, _capi.JSLP_ERR_CAPACITY, 0], (which, status)
        assert "LP 1" in msg and which in msg, msg
        assert out[1]["pivots_phase1"] == 777 and out[1]["evaluation"] == 0 and tree[1].tobytes() == np.full(6, 55, dtype=np.int32).tobytes()
        for i in (0, 2):
            assert out[i].tobytes() == host.results[i].tobytes() and tree[i].tobytes() == host.tree[i].tobytes(), (which, i)
            pack.results[i], pack.tree[i] = out[i], tree[i]
            assert U.state(pack, i)["rhs"] == want[i]["rhs"] and U.state(pack, i)["trace"] == want[i]["trace"]
        pack.close()
    host.close()


def test_plain_simplex_and_reuse_of_a_pack_with_cut_rows(hip_lib, oracle_lib):
    """jslpp_pack_simplex on a pack made by jslpt_pack_create is the root relaxation (the layout is the row capacity's, the tableau the LP's);
    after a tree call the arena holds saved roots, so simplex, download and a second tree call ask for an upload, and get on after it"""
    names = ["Integer_Wood_Shop_Problem", "Knapsack_1", "Integer_Sports_Complex_Problem"]
    items = [U.Item(U.fixture(n)["model"]) for n in names]
    pack = U.make_pack(hip_lib, items)
    ref = TableauPack([it.lp for it in items], precision=[it.precision for it in items], lib=oracle_lib, trace_cap=8192)
    assert pack.simplex().tobytes() == ref.simplex().tobytes()
    for i in range(3):
        assert [a.tobytes() for a in pack.read_rhs(i)] == [a.tobytes() for a in ref.read_rhs(i)]
        assert pack.pivot_trace(i).tobytes() == np.ascontiguousarray(ref.pivot_trace(i), dtype=np.int32).tobytes()
        got, want = pack.download(i), ref.download(i)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    ref.close()
    host = U.solve(oracle_lib, items)
    pack.upload()
    pack.branch_and_cut()
    assert U.states(pack) == U.states(host)
    for call in (pack.simplex, pack.branch_and_cut, lambda: pack.download(0)):
        with pytest.raises(_capi.EngineError, match=r"\(-4\).*saved roots"):
            call()
    pack.upload()
    pack.branch_and_cut()
    assert U.states(pack) == U.states(host)
    pack.close()
    host.close()
