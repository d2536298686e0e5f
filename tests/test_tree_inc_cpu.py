"""Incremental LPs in the pack with trees against the CPU oracle (runs without a GPU): TableauPack's restatement walks
incremental_branch_and_cut.incremental_branch_and_cut with CountingContainers on one engine per LP, the engine's checkpoints standing in for
the device arena; it is held against the reference's recorded runs; solve_packed(..., incremental=True) routes models with
options.useIncremental into the ONE pack of trees and leaves the rest to Solve; the capacities hold for that LP alone.  The kernel itself
is tests/test_tree_inc_gpu.py's."""
import copy
import warnings

import numpy as np
import pytest

import tree_enh_util as E
import tree_inc_util as I
import tree_pack_util as U
from jslpsolver_amd import Solve, _capi, solver
from jslpsolver_amd.engine import TableauPack
from jslpsolver_amd.incremental_branch_and_cut import CountingContainers, incremental_branch_and_cut


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


def _with(model, **options):
    m = copy.deepcopy(model)
    m["options"] = dict(m.get("options") or {}, **options)
    return m


# ---- the reference's records --------------------------------------------------------------------------------------------------------------
def test_every_recorded_fuzz_run_in_one_pack(oracle_lib):
    """every replayable {"useIncremental": true} run of fuzz_services and fuzz_soft, in one pack with solve_packed's capacities, none of
    which comes near"""
    services, soft = I.fuzz_incremental_cases()
    assert (len(services), len(soft)) == (89, 12)
    cases = services + soft
    items = [I.Item(c["model"]) for c in cases]
    assert all(it.row_extra >= 1 and it.cut_rows == 2 * len(it.integers) for it in items)
    pack = I.solve(oracle_lib, items, [I.Inc()] * len(items), heap_cap=solver.TREE_HEAP_CAP, max_nodes=solver.TREE_MAX_NODES)
    assert pack.is_incremental.all() and pack.is_enhanced.all() and not pack.status.any()
    for i, c in enumerate(cases):
        assert pack.policy(i) == ("hybrid", "pseudocost")
        U.check_record(pack, i, items[i], c["nPivots"], c["digest"], c["iter"], c["keys"], c["result"], (c["gen"], c["seed"]))
    assert int(pack.tree["heap_high_water"].max()) == 42 and int(pack.tree["cuts_high_water"].max()) == 11
    assert int(pack.incremental["rows_high_water"].max()) == 24 and int(pack.incremental["checkpoints_used"].max()) == 27
    assert (pack.incremental["checkpoint_rows_high_water"] <= pack.incremental["rows_high_water"]).all()
    assert sum(c["iter"] >= 3 for c in cases) >= 15 and int(pack.incremental["incremental_nodes"].sum()) > 200
    pack.close()


def test_every_fixture_record_in_scope(oracle_lib):
    """tests/golden/incremental.json.gz under its five policy pairs: the records without tolerance / timeout / presolve fixing whose
    model the host takes and that fit"""
    chosen = I.fixture_cases()
    assert len(chosen) == 115 and {I.inc_of(c["options"]) for c, _ in chosen} == set(I.FIVE)
    items = [it for _, it in chosen]
    pack = I.solve(oracle_lib, items, [I.inc_of(c["options"]) for c, _ in chosen], heap_cap=256, trace_cap=max(c["nPivots"] for c, _ in chosen) + 16)
    for i, (c, it) in enumerate(chosen):
        U.check_record(pack, i, it, c["nPivots"], c["pivotDigest"], c["iterations"], c["resultKeys"], c["result"], (c["file"], c["options"]))
    best_first = np.array([c["options"].get("nodeSelection") == "best-first" for c, _ in chosen])
    assert not pack.incremental["checkpoints_used"][best_first].any() and pack.incremental["checkpoints_used"][~best_first].max() >= 20
    pack.close()


# ---- routing ---------------------------------------------------------------------------------------------------------------------------
def test_incremental_models_join_the_one_pack_of_trees(oracle_lib, packs):
    services, _ = I.fuzz_incremental_cases()
    default, _ = U.fuzz_default_cases()
    enhanced = E.fuzz_enhanced_cases()
    knap = U.fixture("Knapsack_1")["model"]
    wood = U.fixture("Integer_Wood_Problem")["model"]
    soft = _with(wood)
    name = next(iter(soft["constraints"]))
    soft["constraints"][name] = dict(soft["constraints"][name], weight=1, priority=1)
    inside = [c["model"] for c in services[::6]] + [_with(knap, useIncremental=True, nodeSelection=p.node_selection, branching=p.branching)
                                                     for p in I.FIVE]
    others = [c["model"] for c in default[:6]] + [c["model"] for c, _ in enhanced[::40]] + [soft, _with(knap, useMIRCuts=True)]
    outside = [_with(knap, useIncremental=True, useMIRCuts=True), _with(soft, useIncremental=True), _with(knap, useIncremental=True, tolerance=0.01),
               _with(knap, useIncremental=True, branching="pseudo")]
    models = inside + others + outside
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [repr(Solve(m, lib=oracle_lib)) for m in models]
        got = solver.solve_packed(models, lib=oracle_lib, incremental=True)
    assert [repr(r) for r in got] == want
    trees = [p for p in packs if p.is_tree]
    main = max(trees, key=len)  # (the MIR model gets a pack of its own beside the soft one, as before)
    assert len(main) == len(inside) + len(others) - 1 and not main.status.any()
    assert int(main.is_incremental.sum()) == len(inside) and list(main.is_incremental[:len(inside)]) == [True] * len(inside)
    assert int(main.is_enhanced.sum()) == len(inside) + len(enhanced[::40]) and main.has_optional
    assert sum(len(p) for p in trees) == len(inside) + len(others) and sum(int(p.is_incremental.sum()) for p in trees) == len(inside)
    assert (main.max_checkpoints[main.is_incremental] == 50).all() and (main.row_extra[main.is_incremental] >= main.cut_rows[main.is_incremental]).all()
    assert [main.policy(len(inside) - 5 + k) for k in range(5)] == [("hybrid", "pseudocost"), ("depth-first", "pseudocost"), ("best-first", "pseudocost"),
                                                                   ("hybrid", "most-fractional"), ("depth-first", "most-fractional")]
    assert not main.incremental[~main.is_incremental].tobytes().strip(b"\0")
    inc = main.incremental[main.is_incremental]
    assert inc["checkpoints_used"].max() == 50 and inc["incremental_nodes"].sum() > 100
    # a full result keeps its checkpoints / incrementalNodes keys
    lp = solver._PackedLp(main, len(inside) - 4)
    assert (lp.checkpoints_used, lp.incremental_nodes) == (50, 100)
    # without the keyword nothing changes: the incremental models stay with Solve
    del packs[:]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert [repr(r) for r in solver.solve_packed(models, lib=oracle_lib)] == want
    assert not any(p.has_incremental for p in packs) and sum(len(p) for p in packs if p.is_tree) == len(others)


def test_the_arena_budget_splits_consecutive_packs(oracle_lib, packs, monkeypatch):
    knap = _with(U.fixture("Knapsack_1")["model"], useIncremental=True)
    wood = U.fixture("Integer_Wood_Problem")["model"]
    slot = solver.checkpoint_bytes(52, 51, 52 + 96)
    monkeypatch.setattr(solver, "PACK_CHECKPOINT_BYTES", 2 * 50 * slot)  # room for two of them
    models = [knap, wood, knap, knap, wood, knap, knap]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = solver.solve_packed(models, lib=oracle_lib, incremental=True)
        assert [repr(r) for r in got] == [repr(Solve(m, lib=oracle_lib)) for m in models]
    assert [(len(p), int(p.is_incremental.sum())) for p in packs] == [(3, 2), (3, 2), (1, 1)]
    assert solver.PACK_CHECKPOINT_BYTES == 2 * 50 * slot and 4 << 30 == 4 * 1024 ** 3


# ---- TableauPack ---------------------------------------------------------------------------------------------------------------------------
def test_tableau_pack_argument_errors(oracle_lib):
    it = I.Item(U.fixture("Integer_Wood_Problem")["model"])
    kw = dict(lib=oracle_lib, integers=[it.integers] * 2, cut_rows=[it.cut_rows] * 2, precision=it.precision)
    with pytest.raises(ValueError, match="1 incremental flags for 2"):
        TableauPack([it.lp] * 2, incremental=[True], **kw)
    with pytest.raises(ValueError, match="integers"):
        TableauPack([it.lp], lib=oracle_lib, incremental=[True])
    with pytest.raises(ValueError, match="LP 1.*mir"):
        TableauPack([it.lp] * 2, mir=[False, True], incremental=[False, True], **kw)
    oo = np.zeros((1, it.lp[0].shape[1]))
    with pytest.raises(ValueError, match="LP 0.*optional"):
        TableauPack([it.lp] * 2, optional_objectives=[oo, None], incremental=[True, False], **kw)
    with pytest.raises(ValueError, match="LP 1.*max_checkpoints"):
        TableauPack([it.lp] * 2, incremental=[True, True], max_checkpoints=[0, 65], **kw)
    with pytest.raises(_capi.EngineError, match="LP 1.*row_extra"):
        TableauPack([it.lp] * 2, incremental=[False, True], row_extra=[-1, it.cut_rows - 1], **kw)
    with pytest.raises(_capi.EngineError, match="LP 0.*64 KiB"):
        TableauPack([it.lp] * 2, incremental=[True, False], row_extra=[100000, -1], **kw)
    # the defaults: row_extra by incremental_rows, 50 checkpoints, hybrid / pseudocost; `strong` is kept as given and means pseudocost
    pack = TableauPack([it.lp] * 2, incremental=[True, False], branching=["strong", None], **kw)
    assert list(pack.is_incremental) == [True, False] and list(pack.is_enhanced) == [True, False] and pack.has_incremental
    assert list(pack.max_checkpoints) == [50, 0] and list(pack.row_extra) == [it.cut_rows + 256, -1]
    assert list(pack.row_capacity) == [it.lp[0].shape[0] + it.cut_rows + 256, it.lp[0].shape[0] + it.cut_rows]
    assert pack.policy(0) == ("hybrid", "strong") and pack.policy(1) is None and not pack.incremental.tobytes().strip(b"\0")
    pack.close()


def test_default_arguments_of_the_host_function_behave_as_before(oracle_lib):
    """incremental_branch_and_cut without containers and with unbounded CountingContainers walk the same tree"""
    from jslpsolver_amd.solver import _prepare
    model = _with(U.fixture("Knapsack_1")["model"], useIncremental=True)
    out = []
    for boxes in (None, CountingContainers()):
        m, t, _n_int, inc = _prepare(model, None, oracle_lib, 0, None)
        try:
            assert inc
            out.append((incremental_branch_and_cut(t, m, containers=boxes), t.evaluation, t.checkpoints_used, t.incremental_nodes,
                        np.asarray(t.pivot_trace()).tobytes()))
        finally:
            t.close()
    assert out[0] == out[1] and out[0][2:4] == (18, 27)
    assert boxes.rows_high_water - 52 == 20 and boxes.checkpoint_rows_high_water - 52 == 17 and boxes.moved_to_heap > 0


def test_strong_means_pseudocost_and_best_first_takes_no_checkpoint(oracle_lib):
    it = I.Item(U.fixture("Knapsack_1")["model"])
    policies = [I.Inc(s, b) for s in E.NODE_SELECTIONS for b in ("pseudocost", "strong")]
    pack = I.solve(oracle_lib, [it] * len(policies), policies)
    st = I.states(pack)
    for k in range(0, len(policies), 2):
        assert st[k] == st[k + 1], policies[k]
    assert not pack.incremental["checkpoints_used"][:2].any() and not pack.incremental["incremental_nodes"][:2].any()
    assert not pack.enhanced["scored_by_pseudocost"].any()
    # depth-first takes exactly the reference's 50: 189 nodes, 100 of them from a checkpoint; hybrid 18 / 27
    assert [tuple(pack.incremental[k])[:2] + (int(pack.tree[k]["iterations"]),) for k in (2, 4)] == [(50, 100, 189), (18, 27, 88)]
    assert pack.enhanced[4]["moved_to_heap"] > 0
    pack.close()


# ---- the capacities ------------------------------------------------------------------------------------------------------------------------
def test_capacities_are_enforced_for_that_lp_alone(oracle_lib):
    """Integer_Wood_Shop_Problem, depth-first: the smallest tree whose stacked rows exceed its longest cut list"""
    shop_json = U.fixture("Integer_Wood_Shop_Problem")["model"]
    left, right = U.Item(U.fixture("Integer_Wood_Problem")["model"]), I.Item(U.fixture("TacoParty")["model"])
    policies = [("hybrid", None), I.Inc("depth-first"), I.Inc()]
    free = I.solve(oracle_lib, [left, I.Item(shop_json), right], policies)
    want = I.states(free)
    rec, inc = free.tree[1], free.incremental[1]
    heap_hw, cuts_hw, nodes, rows_hw = int(rec["heap_high_water"]), int(rec["cuts_high_water"]), int(rec["iterations"]), int(inc["rows_high_water"])
    assert (rows_hw, cuts_hw, nodes, heap_hw) == (7, 5, 35, 5) and int(inc["checkpoints_used"]) == 17
    free.close()

    def run(heap_cap, cut_rows, max_nodes, row_extra):
        its = [left, I.Item(shop_json, row_extra=row_extra, cut_rows=cut_rows), right]
        pack = I.make_pack(oracle_lib, its, policies, heap_cap=[256, heap_cap, 256], max_nodes=max_nodes)
        try:
            pack.branch_and_cut(check_cycles=[it.check for it in its])
            err = None
        except _capi.EngineError as e:
            err = str(e)
        return pack, err

    pack, err = run(heap_hw, cuts_hw, nodes, rows_hw)  # exactly the host's measures
    assert err is None
    got = I.states(pack)
    for k in ("tree", "enhanced", "incremental", "evaluation", "trace"):
        assert got[1][k] == want[1][k], k
    pack.close()
    for caps, word in (((heap_hw - 1, cuts_hw, nodes, rows_hw), "heap_cap"), ((heap_hw, cuts_hw - 1, nodes, rows_hw), "cut_rows"),
                       ((heap_hw, cuts_hw, nodes - 1, rows_hw), "max_nodes"), ((heap_hw, cuts_hw, nodes, rows_hw - 1), "row_extra")):
        pack, err = run(*caps)
        assert err is not None and "(%d)" % _capi.JSLP_ERR_CAPACITY in err and "LP 1" in err and word in err, (caps, err)
        assert list(pack.status) == [_capi.JSLP_OK, _capi.JSLP_ERR_CAPACITY, _capi.JSLP_OK]
        assert not pack.tree[1].tobytes().strip(b"\0") and not pack.incremental[1].tobytes().strip(b"\0")  # left as they were
        got = I.states(pack)
        assert got[0] == want[0] and got[2] == want[2]
        pack.close()
