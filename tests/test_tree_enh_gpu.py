"""jslpe_* on the MI355X: small MILPs with options.nodeSelection / options.branching in a pack, each tree walked under the ENHANCED service
by one workgroup inside one launch (the ENH builds of k_tree_packed, include/jslpe_tree_enhanced.h).

The yardsticks are the reference's recorded runs (fuzz_services, enhanced.json.gz) and the Python host tree on the CPU oracle
(incremental_branch_and_cut.enhanced_branch_and_cut behind TableauPack's restatement); the pack on the GPU is never compared with itself."""
import re

import numpy as np
import pytest

import tree_enh_util as E
import tree_pack_util as U
from jslpsolver_amd import Solve, _capi
from jslpsolver_amd import incremental_branch_and_cut as ibc
from test_tree_packed_gpu import BERLIN, DENSE, INFEASIBLE, NO_INTEGRAL, UNBOUNDED

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"\[jslp\] launch k_tree_packed<(\d+)(?:,(\w+) 1)?> n (\d+) lds (\d+)")
LDS_LIMIT = 65536
ROUTING_CELLS = 2048  # PACK_CELLS_WAVE (jslp_hip.hip): at most this many cells AT THE ROW CAPACITY -> the one-wave build


def _launches(capfd):
    return [(int(t), kind or "plain", int(n), int(b)) for t, kind, n, b in LAUNCH.findall(capfd.readouterr().err)]


def test_recorded_runs_in_one_pack(hip_lib, oracle_lib, monkeypatch, capfd):
    cases = E.fuzz_enhanced_cases()
    assert len(cases) == 3 * 89
    default, _ = U.fuzz_default_cases()
    items = [U.Item(c["model"]) for c, _ in cases] + [U.Item(c["model"]) for c in default]
    policies = [E.given(c["model"]["options"]) for c, _ in cases] + [None] * len(default)
    assert all(it.cut_rows >= 1 and len(it.integers) > 0 for it in items)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack, host = E.against_host(hip_lib, oracle_lib, items, policies)
    lines = _launches(capfd)
    assert 1 <= len(lines) <= 4 and pack.launches == len(lines) and sum(n for _, _, n, _ in lines) == len(items), lines
    assert sum(n for _, kind, n, _ in lines if kind == "enh") == len(cases) and sum(n for _, kind, n, _ in lines if kind == "plain") == len(default)
    assert all(b <= LDS_LIMIT for _, _, _, b in lines)
    for i, (c, pair) in enumerate(cases):
        assert pack.policy(i) == pair
        U.check_record(pack, i, items[i], c["nPivots"], c["digest"], c["iter"], c["keys"], c["result"], (c["gen"], c["seed"], pair))
    for _, pair in E.FUZZ_POLICIES:
        assert sum(c["iter"] >= 3 for c, p in cases if p == pair) >= 15
    assert not pack.enhanced[len(cases):].tobytes().strip(b"\0")
    # the default LPs: what a pack holding only them leaves
    alone = U.solve(hip_lib, items[len(cases):])
    for k, want in enumerate(U.states(alone)):
        assert U.state(pack, len(cases) + k) == want, k
    for i, c in enumerate(default):
        U.check_record(pack, len(cases) + i, items[len(cases) + i], c["nPivots"], c["digest"], c["iter"], c["keys"], c["result"], (c["gen"], c["seed"]))
    alone.close()
    pack.close()
    host.close()


FIVE = [("hybrid", "pseudocost"), ("best-first", "pseudocost"), ("hybrid", "most-fractional"), ("best-first", "strong"), ("depth-first", "most-fractional")]


def test_fixture_records(hip_lib):
    """tests/golden/enhanced.json.gz: the policies fuzz_services lacks, on the fixtures and the synthetic models that fit"""
    chosen = []
    for c in E.enhanced_fixture_cases():
        it = E.fixture_item(c)
        if it is not None and len(it.integers) > 0 and it.cut_rows >= 1:
            chosen.append((c, it))
    assert len(chosen) >= 150
    items = [it for _, it in chosen]
    pack = E.solve(hip_lib, items, [E.given(c["options"]) for c, _ in chosen], heap_cap=256, trace_cap=max(c["nPivots"] for c, _ in chosen) + 16)
    biggest = {}
    for i, (c, it) in enumerate(chosen):
        U.check_record(pack, i, it, c["nPivots"], c["pivotDigest"], c["iterations"], c["resultKeys"], c["result"], (c["file"], c["options"]))
        biggest[pack.policy(i)] = max(biggest.get(pack.policy(i), 0), c["iterations"])
    for pair in FIVE:
        assert biggest.get(pair, 0) >= 5, (pair, biggest)
    pack.close()


# (height, width, first k structural variables integer, seed, cut rows, policy): seeds picked on the CPU for trees of 3 .. 200 nodes.
# tests/test_tree_packed_gpu.py's DENSE shapes with a seed per policy: rows of 63 / 64 / 65 cells in both builds, height + cuts crossing 64
ENH_DENSE = [(h, w, k, seed, None, pair) for (h, w, k, _), seed, pair in zip(
    DENSE, (40, 36, 107, 4, 8, 7, 4, 9, 53, 64, 4), E.PAIRS + E.PAIRS[:2])]
# 63 / 64 / 65 integer variables in the one-wave build, 255 / 256 / 257 in the 256-thread build: the candidate scan wraps the workgroup
ENH_DENSE += [(6, 70, 63, 4, 20, ("best-first", "strong")), (6, 70, 64, 2, 20, ("depth-first", "pseudocost")), (6, 70, 65, 4, 20, ("hybrid", "most-fractional")),
              (6, 260, 255, 37, 20, ("depth-first", "strong")), (6, 260, 256, 6, 20, ("hybrid", "pseudocost")), (6, 260, 257, 18, 20, ("best-first", "most-fractional"))]
# `strong` with exactly 5 and exactly 6 candidates at some node (the slice of five takes all / leaves one out), in both builds
STRONG_5_6 = [(10, 40, 30, 13, 40, ("hybrid", "strong")), (12, 50, 40, 26, 40, ("depth-first", "strong")), (16, 60, 50, 17, 40, ("depth-first", "strong"))]


def test_all_policy_pairs_at_lane_and_thread_edges(hip_lib, oracle_lib, monkeypatch, capfd):
    table = ENH_DENSE + STRONG_5_6
    assert {pair for *_, pair in table} == set(E.PAIRS) and [d[:3] for d in ENH_DENSE[:len(DENSE)]] == [d[:3] for d in DENSE]
    items = [U.dense_item(h, w, k, seed, cut_rows=cut_rows) for h, w, k, seed, cut_rows, _ in table]
    policies = [pair for *_, pair in table]
    # the candidates of every selectBranchingVariable call of the host walk, per LP (the host's function, watched)
    seen, orig = [], ibc._select_branching_variable

    def watched(model, rhs, rows, precision, branching, pseudo, strong_candidates=5, counters=None):
        n = sum(1 for v in model.integerVariables if rows.get(v["index"], -1) != -1
                and abs(float(rhs[rows.get(v["index"])]) - ibc.js_round(float(rhs[rows.get(v["index"])]))) > precision)
        seen.append((branching, n))
        return orig(model, rhs, rows, precision, branching, pseudo, strong_candidates, counters)

    monkeypatch.setattr(ibc, "_select_branching_variable", watched)
    monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
    capfd.readouterr()
    pack, host = E.against_host(hip_lib, oracle_lib, items, policies, max_nodes=400)
    lines = _launches(capfd)
    n_wave = sum((it.lp[0].shape[0] + it.cut_rows) * it.lp[0].shape[1] <= ROUTING_CELLS for it in items)
    assert sorted((t, kind, n) for t, kind, n, _ in lines) == [(64, "enh", n_wave), (256, "enh", len(items) - n_wave)] and 0 < n_wave < len(items), lines
    for t, _, n, b in lines:
        assert b <= LDS_LIMIT
    its = host.tree["iterations"]
    assert its.min() >= 3 and its.max() <= 200, list(its)
    # height + cuts crosses 64 during the tree, in both builds
    for j, (h, w, *_rest) in enumerate(table):
        if h == 62:
            assert h + int(host.tree["cuts_high_water"][j]) > 64
    counts = {n for rule, n in seen if rule == "strong"}
    assert {5, 6} <= counts, sorted(counts)
    wide = [j for j, d in enumerate(table) if d[1] in (70, 260)]
    assert [len(items[j].integers) for j in wide] == [63, 64, 65, 255, 256, 257]
    e = host.enhanced
    assert (e["moved_to_heap"] > 0).any() and (e["scored_by_pseudocost"] > 0).any()
    assert any(e["pseudo_updates"][j] > 0 for j, p in enumerate(policies) if p[0] == "best-first")
    assert any(e["scored_by_pseudocost"][j] > 0 for j, p in enumerate(policies) if p == ("depth-first", "strong"))  # (no recorded run has this pair)
    pack.close()
    host.close()


# the root's evaluation is exactly 0 (and every node's after it): no node updates a pseudocost, where NO_INTEGRAL -- the same tree with an
# objective -- updates one per child of the root
ZERO_ROOT = {"optimize": "z", "opType": "max", "constraints": {"a": {"equal": 3}, "b": {"max": 10}},
             "variables": {"x": {"z": 0, "a": 2, "b": 1}, "y": {"z": 0, "a": 2, "b": 1}}, "ints": {"x": 1, "y": 1}}


def test_tree_edges_under_each_node_selection(hip_lib, oracle_lib):
    """(no instance with dropped_nodes > 0 exists to be found: a node without a candidate has no integer variable off an integer by more
    than precision, and isIntegral has accepted such a node before selectBranchingVariable is asked -- the counter is compared, at 0)"""
    models = [BERLIN, INFEASIBLE, UNBOUNDED, NO_INTEGRAL, ZERO_ROOT]
    items, policies = [], []
    for pair in E.PAIRS:
        items += [U.Item(m) for m in models]
        policies += [pair] * len(models)
    pack, host = E.against_host(hip_lib, oracle_lib, items, policies, heap_cap=64)
    t, e = pack.tree, pack.enhanced
    for k, pair in enumerate(E.PAIRS):
        b, inf, unb, noint, zero = range(5 * k, 5 * k + 5)
        on_stack = pair[0] != "best-first"
        # integral at the root: no save, iterations == 1, no cut row
        assert (t[b]["iterations"], t[b]["is_integral"], t[b]["final_height"], t[b]["nodes_pushed"]) == (1, 1, items[b].lp[0].shape[0], 1)
        assert (e[b]["solutions_found"], e[b]["stack_high_water"], e[b]["pseudo_updates"]) == (1, int(on_stack), 0)
        assert U.result_of(pack, b, items[b]) == {"feasible": True, "result": 1080000, "bounded": True, "isIntegral": True, "brit": 24, "yank": 20}
        assert t[inf]["iterations"] == 1 and not pack.feasible[inf] and not t[inf]["is_integral"]
        # an unbounded root: evaluation -Infinity, the pseudocost sums go non-finite (|-Infinity - -Infinity| is NaN) and the scores with them
        assert t[unb]["iterations"] >= 3 and not pack.bounded[unb] and pack.evaluation[unb] == -np.inf and e[unb]["pseudo_updates"] >= 2
        assert t[noint]["iterations"] == 9 and not t[noint]["is_integral"] and not pack.feasible[noint] and e[noint]["pseudo_updates"] == 3
        assert t[zero]["iterations"] == 9 and e[zero]["pseudo_updates"] == 0 and pack.evaluation[zero] == 0.0
        assert e[noint]["stack_high_water"] == (3 if on_stack else 0)
    assert not e["dropped_nodes"].any()
    pack.close()
    host.close()


def _with(model, **options):
    import copy
    m = copy.deepcopy(model)
    m["options"] = dict(m.get("options") or {}, **options)
    return m


def test_capacities(hip_lib, oracle_lib):
    knap_json = U.fixture("Knapsack_1")["model"]
    left, right = U.Item(U.fixture("Integer_Wood_Problem")["model"]), U.Item(U.fixture("TacoParty")["model"])
    policies = [None, ("hybrid", "pseudocost"), ("depth-first", None)]
    free = E.solve(oracle_lib, [left, U.Item(knap_json), right], policies, heap_cap=256)
    rec = free.tree[1]
    heap_hw, cuts_hw, nodes = int(rec["heap_high_water"]), int(rec["cuts_high_water"]), int(rec["iterations"])
    assert heap_hw > int(free.enhanced[1]["stack_high_water"]) > 2 and free.enhanced[1]["moved_to_heap"] > 0 and nodes > 20
    free.close()

    def both(heap_cap, cut_rows, max_nodes):
        out = []
        for lib in (hip_lib, oracle_lib):
            items = [left, U.Item(knap_json, cut_rows=cut_rows), right]
            pack = E.make_pack(lib, items, policies, heap_cap=[256, heap_cap, 256], max_nodes=max_nodes)
            pack.results[:] = np.frombuffer(b"\x5a" * pack.results.nbytes, dtype=pack.results.dtype)  # sentinels in out / tree_out
            pack.tree[:] = np.frombuffer(b"\x5a" * pack.tree.nbytes, dtype=pack.tree.dtype)
            try:
                pack.branch_and_cut(check_cycles=[it.check for it in items])
                err = None
            except _capi.EngineError as e:
                err = str(e)
            out.append((pack, err))
        return out

    (pack, err), (host, herr) = both(heap_hw, cuts_hw, nodes)  # exactly the host's measures
    assert err is None and herr is None and E.states(pack) == E.states(host)
    assert (int(pack.tree[1]["heap_high_water"]), int(pack.tree[1]["cuts_high_water"]), int(pack.tree[1]["iterations"])) == (heap_hw, cuts_hw, nodes)
    want = E.states(host)
    pack.close()
    host.close()
    for caps, word in (((heap_hw - 1, cuts_hw, nodes), "heap_cap"), ((heap_hw, cuts_hw - 1, nodes), "cut_rows"), ((heap_hw, cuts_hw, nodes - 1), "max_nodes")):
        (pack, err), (host, herr) = both(*caps)
        assert err is not None and "(%d)" % _capi.JSLP_ERR_CAPACITY in err and "LP 1" in err and word in err, (caps, err)
        assert herr is not None and word in herr
        assert list(pack.status) == [_capi.JSLP_OK, _capi.JSLP_ERR_CAPACITY, _capi.JSLP_OK]
        assert pack.results[1].tobytes() == b"\x5a" * pack.results.itemsize and pack.tree[1].tobytes() == b"\x5a" * pack.tree.itemsize
        got = E.states(pack)
        assert got[0] == want[0] and got[2] == want[2]  # both neighbours are right
        pack.close()
        host.close()


def test_upload_and_second_call(hip_lib, oracle_lib):
    items = [U.Item(U.fixture(n)["model"]) for n in ("Knapsack_1", "Integer_Wood_Shop_Problem", "TacoParty")]
    policies = [("best-first", "strong"), ("hybrid", "strong"), None]  # (both score candidates by pseudocost: 12 and 4 of them)
    host = E.solve(oracle_lib, items, policies)
    pack = E.solve(hip_lib, items, policies)
    first = E.states(pack)
    assert first == E.states(host)
    assert host.enhanced[0]["scored_by_pseudocost"] > 0 and host.enhanced[1]["scored_by_pseudocost"] > 0 and host.enhanced[1]["pseudo_updates"] > 0
    with pytest.raises(_capi.EngineError, match="upload first"):
        pack.branch_and_cut(check_cycles=[it.check for it in items])
    pack.upload()
    pack.branch_and_cut(check_cycles=[it.check for it in items])
    assert E.states(pack) == first  # (a pseudocost table left over from the first call would change `strong`'s choices and the counters)
    pack.close()
    host.close()


def test_oversubscription(hip_lib, oracle_lib):
    names = ["Integer_Berlin_Air_Lift_Problem", "Integer_Chocolate_Problem", "Integer_Clothing_Shop_Problem", "Integer_Clothing_Shop_Problem_II",
             "Integer_Sports_Complex_Problem", "Integer_Wood_Problem", "Integer_Wood_Shop_Problem", "TacoParty"]
    base = [U.Item(U.fixture(n)["model"]) for n in names]
    pair = ("hybrid", "pseudocost")
    host = E.solve(oracle_lib, base, [pair] * len(base), trace_cap=512)
    want = E.states(host)
    copies = 512
    items = [it for it in base for _ in range(copies)]
    pack = E.solve(hip_lib, items, [pair] * len(items), trace_cap=512)
    assert pack.launches <= 2
    for j in range(len(base)):
        for c in range(copies):
            assert E.state(pack, j * copies + c) == want[j], (names[j], c)
    pack.close()
    host.close()
    # afterwards a default-service pack and a Solve on the same library are still right
    later, later_host = U.solve(hip_lib, base), U.solve(oracle_lib, base)
    assert U.states(later) == U.states(later_host)
    later.close()
    later_host.close()
    model = U.fixture("Integer_Wood_Shop_Problem")["model"]
    assert Solve(model, lib=hip_lib) == Solve(model, lib=oracle_lib)
    assert Solve(_with(model, nodeSelection="hybrid"), lib=hip_lib) == Solve(_with(model, nodeSelection="hybrid"), lib=oracle_lib)
