"""MIR LPs in a pack with trees against the CPU oracle (runs without a GPU): TableauPack's restatement walks branch_and_cut.branch_and_cut
with its round-by-round MIR loop on one oracle engine per LP, with the pack's capacities enforced and the MIR counters gathered around
mirRound -- held here against the reference's recorded MIR runs; the routing of solve_packed and the error model are tested here too.  The
kernel itself is tests/test_tree_mir_gpu.py's."""
import warnings

import numpy as np
import pytest

import tree_mir_util as M
import tree_pack_util as U
from jslpsolver_amd import Solve, _capi, solver
from jslpsolver_amd.engine import TableauPack
from test_tree_packed_cpu import packs  # noqa: F401  (the fixture: every TableauPack solve_packed makes)


@pytest.fixture(scope="module")
def fuzz_pack(oracle_lib):
    """the fuzz records in one pack on the oracle, solved once"""
    cases = M.fuzz_mir_cases()
    items = [M.MirItem(c["model"]) for c in cases]
    pack = M.solve(oracle_lib, items)
    yield cases, items, pack
    pack.close()


def test_restatement_against_the_fuzz_records(fuzz_pack):
    cases, items, pack = fuzz_pack
    assert len(cases) >= 85
    assert not pack.status.any() and pack.is_mir.all()
    for i, c in enumerate(cases):
        M.check_fuzz_record(pack, i, items[i], c)
    mir, tree = pack.mir, pack.tree
    # what the records exercise: trees of many nodes, rounds without rows, roots that keep MIR rows and branch
    assert int(tree["iterations"].max()) >= 50 and int(mir["rounds"].max()) >= 80
    assert ((mir["root_rows"] > 0) & (tree["iterations"] > 1)).any()
    assert (mir["rounds"] >= tree["iterations"]).all()  # at least one round per node: a round that selects no row still runs its simplex
    assert (mir["simplexes"] >= mir["rounds"] + tree["iterations"]).all() and (mir["rows_added"] <= 10 * mir["rounds"]).all()
    heights = np.array([it.lp[0].shape[0] for it in items])
    assert (tree["final_height"] - heights <= mir["rows_high_water"]).all() and (mir["root_rows"] <= mir["rows_high_water"]).all()
    assert int(mir["rows_high_water"].max()) <= 40 and all(it.row_extra >= 170 for it in items)


def test_restatement_against_the_fixture_records(oracle_lib):
    records = M.fixture_mir_records()
    assert [n for n, _, _ in records] == U.TREE_FIXTURES
    items = [M.MirItem(model) for _, model, _ in records]
    pack = M.solve(oracle_lib, items)
    assert not pack.status.any()
    for i, (name, _, c) in enumerate(records):
        M.check_fixture_record(pack, i, items[i], name, c)
    k = U.TREE_FIXTURES.index("Knapsack_1")
    assert (int(pack.tree[k]["iterations"]), int(pack.mir[k]["rows_added"]), int(pack.tree[k]["final_height"])) == (39, 131, 74)
    # a new upload starts every LP afresh, variable.isInteger included: the same trees again
    first = M.states(pack)
    pack.upload()
    pack.branch_and_cut(check_cycles=[it.check for it in items])
    assert M.states(pack) == first
    pack.close()


def test_solve_packed_routes_mir_models(oracle_lib, packs):  # noqa: F811
    cases = M.fuzz_mir_cases()[:12]
    wood = U.fixture("Integer_Wood_Shop_Problem")["model"]
    berlin = U.fixture("Berlin_Air_Lift_Problem")["model"]
    mir_wood = dict(wood, options={"useMIRCuts": True})
    out_of_scope = [dict(wood, options={"useMIRCuts": True, "tolerance": 0.01}), dict(wood, options={"useMIRCuts": True, "useIncremental": True}),
                    dict(wood, options={"useMIRCuts": True, "nodeSelection": "best-first"})]
    no_fit = dict(U.fixture("Vendor_Selection")["model"], options={"useMIRCuts": True})
    models = [c["model"] for c in cases] + [wood, berlin, mir_wood] + out_of_scope + [no_fit]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [repr(Solve(m, lib=oracle_lib)) for m in models]
        got = solver.solve_packed(models, lib=oracle_lib)
    assert [repr(r) for r in got] == want
    # one pack of plain LPs (Berlin), one pack of trees: the twelve records and mir_wood as MIR LPs, wood as a plain tree LP; the rest: Solve
    assert [(p.is_tree, len(p)) for p in packs] == [(False, 1), (True, 14)]
    assert packs[1].is_mir.tolist() == [True] * 12 + [False, True] and not packs[1].status.any()
    n_int = [len(M.MirItem(c["model"]).integers) for c in cases]
    extra = packs[1].row_extra.tolist()
    assert all(e == 2 * n + 320 or 170 < e < 2 * n + 320 for e, n in zip(extra, n_int)) and sum(e == 2 * n + 320 for e, n in zip(extra, n_int)) >= 8
    assert packs[1].cut_rows.tolist()[:12] == [2 * n for n in n_int] and extra[12] == -1
    assert (packs[1].mir["rounds"][packs[1].is_mir] > 0).all() and packs[1].mir[12].tolist() == (0, 0, 0, 0, 0)


def test_solve_packed_keeps_mir_and_optional_objectives_apart(oracle_lib, packs):  # noqa: F811
    soft = [c["model"] for c in U._cases("fuzz_soft.jsonl.gz")
            if not c["model"].get("options") and c["fixed"] == 0 and not c["infeasPre"] and c["model"].get("ints")][:40]
    mir = [c["model"] for c in M.fuzz_mir_cases()[:3]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [repr(Solve(m, lib=oracle_lib)) for m in soft + mir]
        got = solver.solve_packed(soft + mir, lib=oracle_lib)
    assert [repr(r) for r in got] == want
    trees = [p for p in packs if p.is_tree]
    assert [(p.has_mir, p.has_optional) for p in trees] == [(True, False), (False, True)] and len(trees[0]) == 3


def _knapsack_between(oracle_lib, row_extra, cut_rows):
    records = {n: m for n, m, _ in M.fixture_mir_records()}
    wood = M.MirItem(records["Integer_Wood_Shop_Problem"])
    return [wood, M.MirItem(records["Knapsack_1"], row_extra=row_extra, cut_rows=cut_rows), wood]


def test_row_capacity_at_and_below_the_measure(oracle_lib):
    items = _knapsack_between(oracle_lib, None, None)
    pack = M.solve(oracle_lib, items)
    want = M.states(pack)
    hw, cuts = int(pack.mir[1]["rows_high_water"]), int(pack.tree[1]["cuts_high_water"])
    # Knapsack_1's measures, from the instrumented host run: the tree ends 22 rows above the model's 52, its tallest tableau has 24
    assert (hw, int(pack.tree[1]["final_height"]) - 52) == (24, 22) and 0 < cuts <= hw and int(pack.mir[1]["root_rows"]) > 0
    pack.close()
    exact = M.solve(oracle_lib, _knapsack_between(oracle_lib, hw, cuts))
    assert M.states(exact) == want
    exact.close()
    low = M.make_pack(oracle_lib, _knapsack_between(oracle_lib, hw - 1, cuts))
    with pytest.raises(_capi.EngineError, match=r"\(-5\).*LP 1.*row_extra"):
        low.branch_and_cut()
    assert low.status.tolist() == [0, _capi.JSLP_ERR_CAPACITY, 0]
    assert low.results[1].tobytes() == bytes(low.results.dtype.itemsize) and low.tree[1].tobytes() == bytes(24) and low.mir[1].tobytes() == bytes(20)
    for i in (0, 2):
        assert M.state(low, i) == want[i], i
    low.close()


def test_solve_packed_falls_back_on_the_row_capacity(oracle_lib, packs, monkeypatch):  # noqa: F811
    records = {n: m for n, m, _ in M.fixture_mir_records()}
    models = [records["Integer_Wood_Shop_Problem"], records["Knapsack_1"], records["Integer_Wood_Shop_Problem"]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [repr(Solve(m, lib=oracle_lib)) for m in models]
        monkeypatch.setattr(solver, "tree_mir_rows", lambda h, w, n_int, lib=None: (23, 23))  # one below Knapsack_1's tallest tableau
        got = solver.solve_packed(models, lib=oracle_lib)
    assert [repr(r) for r in got] == want
    assert len(packs) == 1 and packs[0].status.tolist() == [0, _capi.JSLP_ERR_CAPACITY, 0]


def test_create_time_refusals_of_the_restatement(oracle_lib):
    it = M.MirItem(M.fixture_mir_records()[0][1])
    with pytest.raises(_capi.EngineError, match=r"\(%d\).*LP 1.*row_extra" % _capi.JSLP_ERR_ARG):
        M.make_pack(oracle_lib, [it, M.MirItem(M.fixture_mir_records()[0][1], row_extra=1, cut_rows=2)])
    knap = M.MirItem(M.fixture_mir_records()[U.TREE_FIXTURES.index("Knapsack_1")][1])
    assert knap.row_extra == 95
    with pytest.raises(_capi.EngineError, match=r"\(-6\).*LP 1.*64 KiB"):
        M.make_pack(oracle_lib, [it, M.MirItem(M.fixture_mir_records()[U.TREE_FIXTURES.index("Knapsack_1")][1], row_extra=96)])
    with pytest.raises(ValueError, match="optional objectives"):
        TableauPack([it.lp], integers=[it.integers], mir=[True], optional_objectives=[np.zeros((1, it.lp[0].shape[1]))], lib=oracle_lib)
