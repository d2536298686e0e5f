"""The pack with trees against the CPU oracle (runs without a GPU): TableauPack's restatement walks branch_and_cut.branch_and_cut on one
oracle engine per LP with the pack's capacities enforced, so the routing of solve_packed, the capacities and their error model are
tested here; the kernel itself is tests/test_tree_packed_gpu.py's."""
import gzip
import json
import os
import warnings

import pytest

import golden_util as G
import tree_pack_util as U
from jslpsolver_amd import Solve, _capi, solver
from jslpsolver_amd.engine import TableauPack

NO_FIT = ["Monster_II", "Sudoku4x4", "Vendor_Selection"]           # integer models whose tableau with cut rows exceeds 64 KiB of LDS
OUT_OF_SCOPE = ["LargeFarmMIP", "StockCuttingProblem"]             # tolerance / timeout: the host's clock decides


@pytest.fixture()
def packs(monkeypatch):
    """every TableauPack solve_packed makes"""
    made = []

    class Spy(TableauPack):
        def __init__(self, *a, **k):
            TableauPack.__init__(self, *a, **k)
            made.append(self)

    monkeypatch.setattr(solver, "TableauPack", Spy)
    return made


def _fixtures():
    return {G.ident(p): G.load(p) for p in G.fixture_paths()}


def test_fixture_routes_and_results(oracle_lib, packs):
    fx = _fixtures()
    assert len(fx) == 47
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = {n: repr(Solve(g["model"], lib=oracle_lib)) for n, g in fx.items()}
        tree_route = []
        for n, g in fx.items():
            del packs[:]
            assert repr(solver.solve_packed([g["model"]], lib=oracle_lib)[0]) == want[n], n
            if any(p.is_tree for p in packs):
                assert len(packs) == 1 and not packs[0].status.any()
                tree_route.append(n)
        assert sorted(tree_route) == sorted(U.TREE_FIXTURES)
        with_ints = sorted(n for n, g in fx.items() if g["tableau"] is not None and g["tableau"]["integerVarIndexes"])
        assert len(with_ints) == 15 and sorted(set(with_ints) - set(tree_route)) == sorted(NO_FIT + OUT_OF_SCOPE)
        # all at once: one pack of plain LPs, one pack of trees, the rest through Solve
        del packs[:]
        names = list(fx)
        got = solver.solve_packed([fx[n]["model"] for n in names], lib=oracle_lib)
        assert [repr(r) for r in got] == [want[n] for n in names]
        assert [p.is_tree for p in packs] == [False, True] and len(packs[1]) == 10
    knap = packs[1].tree[[i for i, n in enumerate(sorted(U.TREE_FIXTURES)) if n == "Knapsack_1"][0]]
    assert int(packs[1].tree["iterations"].max()) == int(knap["iterations"]) == 79


# (seven service policies per seed, one of them the default: a seventh of the first 200 service runs; the soft set has a third with integers,
#  most of them with soft constraints, i.e. optional objectives, which keep a model out of the pack)
@pytest.mark.parametrize("name, at_least", [("fuzz_services.jsonl.gz", 20), ("fuzz_soft.jsonl.gz", 1)])
def test_fuzz_models_through_solve_packed(oracle_lib, packs, name, at_least):
    with gzip.open(os.path.join(G.GOLDEN, name), "rt") as fh:
        models = [json.loads(line)["model"] for line in fh if line.startswith("{")][:200]
    assert len(models) == 200
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = solver.solve_packed(models, lib=oracle_lib)
        for k, m in enumerate(models):
            assert repr(got[k]) == repr(Solve(m, lib=oracle_lib)), k
    trees = [p for p in packs if p.is_tree]
    assert len(trees) == 1 and len(trees[0]) >= at_least and not trees[0].status.any()


def _knapsack_between(oracle_lib, **caps):
    knap, wood = U.Item(U.fixture("Knapsack_1")["model"]), U.Item(U.fixture("Integer_Wood_Shop_Problem")["model"])
    items = [wood, U.RawItem(knap.lp, knap.integers, cut_rows=caps.get("cut_rows", knap.cut_rows), precision=knap.precision, check=knap.check), wood]
    return items, U.make_pack(oracle_lib, items, heap_cap=[256, caps.get("heap_cap", 256), 256], max_nodes=caps.get("max_nodes", 0))


def test_capacities_at_and_below_the_measures(oracle_lib):
    items, pack = _knapsack_between(oracle_lib)
    pack.branch_and_cut()
    want = U.states(pack)
    m = pack.tree[1]  # Knapsack_1's measures, from the instrumented host run
    caps = dict(max_nodes=int(m["iterations"]), heap_cap=int(m["heap_high_water"]), cut_rows=int(m["cuts_high_water"]))
    assert caps == dict(max_nodes=79, heap_cap=62, cut_rows=20) and int(m["nodes_pushed"]) == 131
    pack.close()
    _, exact = _knapsack_between(oracle_lib, **caps)
    exact.branch_and_cut()
    assert U.states(exact) == want
    exact.close()
    for which in caps:
        _, low = _knapsack_between(oracle_lib, **dict(caps, **{which: caps[which] - 1}))
        with pytest.raises(_capi.EngineError, match=r"\(-5\).*LP 1.*%s" % which):
            low.branch_and_cut()
        assert low.status.tolist() == [0, _capi.JSLP_ERR_CAPACITY, 0]
        assert low.results[1].tobytes() == bytes(low.results.dtype.itemsize) and low.tree[1].tobytes() == bytes(24)  # left as they were
        for i in (0, 2):
            assert U.state(low, i) == want[i], (which, i)
        low.close()


def test_solve_packed_falls_back_on_a_capacity(oracle_lib, packs, monkeypatch):
    g = U.fixture("Knapsack_1")
    wood = U.fixture("Integer_Wood_Shop_Problem")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [repr(Solve(x["model"], lib=oracle_lib)) for x in (wood, g, wood)]
        monkeypatch.setattr(solver, "TREE_HEAP_CAP", 61)  # one below Knapsack_1's high-water mark
        got = solver.solve_packed([wood["model"], g["model"], wood["model"]], lib=oracle_lib)
    assert [repr(r) for r in got] == want
    assert len(packs) == 1 and packs[0].status.tolist() == [0, _capi.JSLP_ERR_CAPACITY, 0]


def test_a_pack_without_integers_is_a_plain_simplex(oracle_lib):
    berlin = U.fixture("Berlin_Air_Lift_Problem")
    it = U.Item(berlin["model"])
    assert it.integers == []
    pack = U.solve(oracle_lib, [it])
    plain = TableauPack([it.lp], precision=[it.precision], lib=oracle_lib, trace_cap=64)
    plain.simplex()
    assert pack.results.tobytes() == plain.results.tobytes() and pack.tree[0].tolist() == (0, 0, it.lp[0].shape[0], 0, 0, 0)
    assert pack.read_rhs(0)[0].tobytes() == plain.read_rhs(0)[0].tobytes()
    with pytest.raises(_capi.EngineError, match="without `integers`"):
        plain.branch_and_cut()
    pack.close()
    plain.close()
