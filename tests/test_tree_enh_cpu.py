"""Enhanced LPs in the pack with trees against the CPU oracle (runs without a GPU): include/jslpe_tree_enhanced.h, its ctypes table and
the exports agree; solve_packed routes models with options.nodeSelection / options.branching into the ONE pack of trees and leaves the
rest to Solve; TableauPack's restatement walks incremental_branch_and_cut.enhanced_branch_and_cut with the pack's capacities enforced;
the create and TableauPack refuse bad arguments.  The kernel itself is tests/test_tree_enh_gpu.py's."""
import copy
import ctypes
import os
import warnings

import numpy as np
import pytest

import tree_enh_util as E
import tree_pack_util as U
from jslpsolver_amd import Solve, _capi, solver
from jslpsolver_amd.engine import TableauPack
from jslpsolver_amd.incremental_branch_and_cut import CountingContainers, enhanced_branch_and_cut
from test_many_abi import built, declared_in_header, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jslpe_tree_enhanced.h")
CHAOS = os.path.join(ROOT, "jslpsolver_amd", "csrc", "libjslp_hip_chaos.so")
PREFIX = "jslpe_"


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


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_libraries_agree(oracle_lib):
    declared = declared_in_header(HEADER, PREFIX)
    assert declared == set(_capi.TREE_ENH_SYMBOLS) == {"jslpe_tree_pack_create", "jslpe_tree_pack_create_mixed", "jslpe_pack_read_enhanced"}
    for other in ("jslp_engine.h", "jslpp_packed.h", "jslpt_tree.h", "jslps_soft.h", "jslpc_tree_mir.h", "jslpm_many.h", "jslpx_branch.h", "jslpr_mir.h",
                  "jslpf_f32.h"):
        assert not declared_in_header(os.path.join(ROOT, "include", other), PREFIX)
    assert _capi.ENH_TREE_DTYPE.itemsize == 32
    text = open(HEADER).read()
    order = [text.index("int32_t %s;" % name) for name in _capi.ENH_TREE_DTYPE.names[:6]]  # the struct's members, in the dtype's order
    assert order == sorted(order)
    for name, code in list(_capi.ENH_NODE_SELECTION.items()) + list(_capi.ENH_BRANCHING.items()):
        assert "#define JSLPE_%s %d\n" % (name.upper().replace("-", "_"), code) in text
    assert exported(built(_capi.HIP_LIB_PATH), PREFIX) == declared and exported(built(CHAOS), PREFIX) == declared
    assert _capi.Library(built(_capi.HIP_LIB_PATH)).has_tree_enh
    assert exported(oracle_lib.path, PREFIX) == set() and not oracle_lib.has_tree_enh


def _create(lib, n, heights, widths, cut_rows, heap_cap, node_selection, branching, n_optional=None, row_extra=None, mixed=False):
    h = ctypes.c_void_p()
    arr = lambda a: None if a is None else _capi.ptr_i32(_capi.as_i32(a))  # noqa: E731
    ps = _capi.ptr_f64(_capi.as_f64([1e-8] * max(n, 1)))
    if mixed:
        rc = lib.jslpe_tree_pack_create_mixed(ctypes.byref(h), 0, n, arr(heights), arr(widths), ps, arr(cut_rows), arr(heap_cap), arr(n_optional),
                                              arr(row_extra), arr(node_selection), arr(branching), 0, 0, 0)
    else:
        rc = lib.jslpe_tree_pack_create(ctypes.byref(h), 0, n, arr(heights), arr(widths), ps, arr(cut_rows), arr(heap_cap), arr(node_selection),
                                        arr(branching), 0, 0, 0)
    return rc, h, lib.jslp_last_error()


def test_create_argument_errors_without_a_device():
    """refused before any device call: this host has no GPU, and a call that reached the device would answer JSLP_ERR_DEVICE"""
    lib = _capi.Library(built(_capi.HIP_LIB_PATH))
    assert _create(lib, 1, [3], [3], [2], [4], None, [1])[0] == _capi.JSLP_ERR_ARG
    assert _create(lib, 1, [3], [3], [2], [4], [1], None)[0] == _capi.JSLP_ERR_ARG
    assert _create(lib, 1, [3], [3], None, [4], [1], [1])[0] == _capi.JSLP_ERR_ARG
    for ns, br, word in (([0, 4], [0, 0], b"node_selection"), ([0, -1], [0, 0], b"node_selection"), ([0, 1], [0, 4], b"branching"),
                         ([0, 0], [0, -1], b"branching")):
        rc, h, msg = _create(lib, 2, [3, 3], [3, 3], [2, 2], [4, 4], ns, br)
        assert rc == _capi.JSLP_ERR_ARG and not h.value and b"LP 1" in msg and word in msg, msg
    # the LDS limit is jslpt_pack_create's: Knapsack_1 (52 x 51) holds 96 cut rows, as a default LP and as an enhanced one
    assert lib.jslpt_lds_bytes(52, 51, 52 + 96) <= 65536 < lib.jslpt_lds_bytes(52, 51, 52 + 97)
    for ns in (0, 2):
        rc, h, msg = _create(lib, 2, [3, 52], [3, 51], [4, 97], [8, 8], [0, ns], [0, 0])
        assert rc == _capi.JSLP_ERR_UNSUPPORTED and b"LP 1" in msg and b"64 KiB" in msg
    # an enhanced LP has neither optional objectives nor MIR cuts; a default LP of the same pack may have either
    rc, h, msg = _create(lib, 2, [3, 3], [3, 3], [2, 2], [4, 4], [0, 3], [0, 0], n_optional=[1, 1], mixed=True)
    assert rc == _capi.JSLP_ERR_ARG and b"LP 1" in msg and b"optional" in msg
    rc, h, msg = _create(lib, 2, [3, 3], [3, 3], [2, 2], [4, 4], [0, 0], [0, 2], row_extra=[5, 5], mixed=True)
    assert rc == _capi.JSLP_ERR_ARG and b"LP 1" in msg and b"MIR" in msg
    rc, h, msg = _create(lib, 2, [3, 3], [3, 3], [2, 2], [4, 4], [0, 0], [0, 0], n_optional=[0, 1], row_extra=[-1, 5], mixed=True)
    assert rc == _capi.JSLP_ERR_ARG and b"LP 1" in msg
    assert lib.jslpe_pack_read_enhanced(None, None) == _capi.JSLP_ERR_ARG


def test_tableau_pack_argument_errors(oracle_lib):
    it = U.Item(U.fixture("Integer_Wood_Problem")["model"])
    kw = dict(lib=oracle_lib, integers=[it.integers] * 2, cut_rows=[it.cut_rows] * 2, precision=it.precision)
    with pytest.raises(ValueError, match="node_selection"):
        TableauPack([it.lp] * 2, node_selection=[None, "breadth-first"], **kw)
    with pytest.raises(ValueError, match="branching"):
        TableauPack([it.lp] * 2, branching=["pseudo", None], **kw)
    with pytest.raises(ValueError, match="1 node_selection entries for 2"):
        TableauPack([it.lp] * 2, node_selection=["hybrid"], **kw)
    with pytest.raises(ValueError, match="integers"):
        TableauPack([it.lp], lib=oracle_lib, node_selection=["hybrid"])
    with pytest.raises(ValueError, match="LP 1.*mir"):
        TableauPack([it.lp] * 2, mir=[False, True], branching=[None, "strong"], **kw)
    oo = np.zeros((1, it.lp[0].shape[1]))
    with pytest.raises(ValueError, match="LP 0.*optional"):
        TableauPack([it.lp] * 2, optional_objectives=[oo, None], node_selection=["depth-first", None], **kw)
    with pytest.raises(_capi.EngineError, match="LP 1.*distinct"):
        TableauPack([it.lp] * 2, lib=oracle_lib, integers=[it.integers, it.integers + it.integers[:1]], cut_rows=[it.cut_rows] * 2,
                    branching=[None, "strong"])
    # mixing is fine: a MIR LP and an LP with neither beside an enhanced one; one of the two given fills the other in
    kw.update(integers=[it.integers] * 3, cut_rows=[it.cut_rows] * 3)
    pack = TableauPack([it.lp] * 3, mir=[True, False, False], node_selection=[None, None, "best-first"], branching=[None, "strong", None], **kw)
    assert list(pack.is_enhanced) == [False, True, True] and list(pack.is_mir) == [True, False, False]
    assert [pack.policy(i) for i in range(3)] == [None, ("hybrid", "strong"), ("best-first", "pseudocost")]
    assert not pack.enhanced.tobytes().strip(b"\0")
    pack.close()


# ---- routing ---------------------------------------------------------------------------------------------------------------------------
def test_enhanced_models_join_the_one_pack_of_trees(oracle_lib, packs):
    cases = E.fuzz_enhanced_cases()
    assert len(cases) == 3 * 89
    default, _ = U.fuzz_default_cases()
    models = [c["model"] for c, _ in cases[::7]] + [c["model"] for c in default[:12]]
    knap = U.fixture("Knapsack_1")["model"]
    models += [_with(knap, nodeSelection=s, branching=b) for s, b in E.PAIRS] + [_with(knap, useMIRCuts=True), knap]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [repr(Solve(m, lib=oracle_lib)) for m in models]
        got = solver.solve_packed(models, lib=oracle_lib)
    assert [repr(r) for r in got] == want
    assert [p.is_tree for p in packs] == [True] and len(packs[0]) == len(models) and not packs[0].status.any()
    pack = packs[0]
    n_enh = len(cases[::7]) + 9
    assert int(pack.is_enhanced.sum()) == n_enh and int(pack.is_mir.sum()) == 1
    assert [pack.policy(i) for i in range(len(cases[::7]))] == [pair for _, pair in cases[::7]]
    assert [pack.policy(len(models) - 11 + k) for k in range(9)] == E.PAIRS
    assert not pack.enhanced[~pack.is_enhanced].tobytes().strip(b"\0")
    assert (pack.enhanced["pseudo_updates"][pack.is_enhanced] > 0).sum() >= 9 and pack.enhanced["moved_to_heap"].max() > 0


def test_what_stays_with_solve(oracle_lib, packs):
    knap = U.fixture("Knapsack_1")["model"]
    wood = U.fixture("Integer_Wood_Problem")["model"]
    soft = copy.deepcopy(_with(wood, nodeSelection="hybrid"))
    name = next(iter(soft["constraints"]))
    soft["constraints"][name] = dict(soft["constraints"][name], weight=1, priority=1)
    from jslpsolver_amd.model import Model
    _, rows = Model(soft, None).optional_objectives()
    assert rows is not None and len(rows) > 0  # (the soft constraint makes an optional objective)
    outside = [_with(knap, useMIRCuts=True, nodeSelection="depth-first"), _with(knap, branching="strong", tolerance=0.01),
               _with(knap, useIncremental=True, nodeSelection="hybrid"), soft, _with(wood, nodeSelection="breadth-first")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for m in outside:
            del packs[:]
            assert repr(solver.solve_packed([m], lib=oracle_lib)[0]) == repr(Solve(m, lib=oracle_lib))
            assert not any(p.is_tree and p.has_enhanced for p in packs), m["options"]
            assert not any(p.is_tree for p in packs) or m is soft  # (the soft model may not even reach a pack of trees)
    assert packs == [] or all(not p.has_enhanced for p in packs)


def test_results_equal_solve_on_every_recorded_run(oracle_lib):
    """the restatement against the reference's records: every replayable enhanced run of fuzz_services, in one pack with solve_packed's
    capacities, none of which comes near"""
    cases = E.fuzz_enhanced_cases()
    items = [U.Item(c["model"]) for c, _ in cases]
    pack = E.solve(oracle_lib, items, [E.given(c["model"]["options"]) for c, _ in cases], heap_cap=solver.TREE_HEAP_CAP, max_nodes=solver.TREE_MAX_NODES)
    for i, (c, pair) in enumerate(cases):
        assert pack.policy(i) == pair
        U.check_record(pack, i, items[i], c["nPivots"], c["digest"], c["iter"], c["keys"], c["result"], (c["gen"], c["seed"], pair))
    for pair, peak in ((("depth-first", "pseudocost"), 16), (("hybrid", "strong"), 39), (("best-first", "most-fractional"), 45)):
        mine = np.array([p == pair for _, p in cases])
        assert int(pack.tree["heap_high_water"][mine].max()) == peak
        assert sum(c["iter"] >= 3 for (c, p) in cases if p == pair) >= 15
    assert int(pack.tree["cuts_high_water"].max()) == 12
    assert (pack.enhanced["stack_high_water"][[p[0] == "best-first" for _, p in cases]] == 0).all()
    pack.close()


# ---- the counting containers and the capacities ----------------------------------------------------------------------------------------
def test_default_arguments_of_the_host_function_behave_as_before(oracle_lib):
    """enhanced_branch_and_cut without containers and with unbounded CountingContainers walk the same tree"""
    from jslpsolver_amd.solver import _prepare
    model = _with(U.fixture("Knapsack_1")["model"], nodeSelection="hybrid", branching="strong")
    out = []
    for boxes in (None, CountingContainers()):
        m, t, _n_int, _inc = _prepare(model, None, oracle_lib, 0, None)
        try:
            out.append((enhanced_branch_and_cut(t, m, node_selection="hybrid", branching="strong", containers=boxes), t.evaluation,
                        np.asarray(t.pivot_trace()).tobytes()))
        finally:
            t.close()
    assert out[0] == out[1]
    assert out[0][0][0] > 20 and boxes.pushes % 2 == 1  # (the root and two per branched node)
    assert boxes.high_water >= boxes.stack_high_water > 0 and boxes.moved_to_heap > 0 and boxes.pseudo_updates > 0


def test_capacities_are_enforced_for_that_lp_alone(oracle_lib):
    knap_json = U.fixture("Knapsack_1")["model"]
    knap = U.Item(knap_json)
    left, right = U.Item(U.fixture("Integer_Wood_Problem")["model"]), U.Item(U.fixture("TacoParty")["model"])
    items, policies = [left, knap, right], [None, ("hybrid", "pseudocost"), ("depth-first", None)]
    free = E.solve(oracle_lib, items, policies, heap_cap=256)
    want = E.states(free)
    rec = free.tree[1]
    heap_hw, cuts_hw, nodes = int(rec["heap_high_water"]), int(rec["cuts_high_water"]), int(rec["iterations"])
    assert heap_hw > int(free.enhanced[1]["stack_high_water"]) > 2 and cuts_hw > 3 and nodes > 20 and free.enhanced[1]["moved_to_heap"] > 0
    free.close()

    def run(heap_cap, cut_rows, max_nodes):
        its = [left, U.Item(knap_json, cut_rows=cut_rows), right]
        pack = E.make_pack(oracle_lib, its, policies, heap_cap=[256, heap_cap, 256], max_nodes=max_nodes)
        try:
            pack.branch_and_cut(check_cycles=[it.check for it in its])
            err = None
        except _capi.EngineError as e:
            err = str(e)
        return pack, err

    pack, err = run(heap_hw, cuts_hw, nodes)  # exactly the host's measures
    assert err is None
    got = E.states(pack)
    # (the row capacity differs with cut_rows, so the result struct's and the read-back's sizes may; the tree and its outcome do not)
    for k in ("tree", "enhanced", "evaluation", "trace"):
        assert got[1][k] == want[1][k], k
    pack.close()
    for caps, word in (((heap_hw - 1, cuts_hw, nodes), "heap_cap"), ((heap_hw, cuts_hw - 1, nodes), "cut_rows"), ((heap_hw, cuts_hw, nodes - 1), "max_nodes")):
        pack, err = run(*caps)
        assert err is not None and "(%d)" % _capi.JSLP_ERR_CAPACITY in err and "LP 1" in err and word in err, (caps, err)
        assert list(pack.status) == [_capi.JSLP_OK, _capi.JSLP_ERR_CAPACITY, _capi.JSLP_OK]
        assert not pack.tree[1].tobytes().strip(b"\0") and not pack.enhanced[1].tobytes().strip(b"\0")  # left as they were
        got = E.states(pack)
        assert got[0] == want[0] and got[2] == want[2]
        pack.close()
