"""include/jslpg_tree_tolerance.h without a GPU: the header, its ctypes table and the exports agree and the create refuses bad arguments before any
device call; TableauPack's restatement (the three host walks on the CPU oracle with each LP's tolerance and sense) replays the reference's
recorded runs with options.tolerance; solve_packed routes such models into the pack only with tolerance=True; the edge models of
tests/tree_tol_util.py have the properties the GPU tests rely on."""
import copy
import ctypes
import os
import warnings

import numpy as np
import pytest

import tree_inc_util as I
import tree_pack_util as U
import tree_tol_util as T
from jslpsolver_amd import Solve, _capi, solver
from test_many_abi import built, declared_in_header, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jslpg_tree_tolerance.h")
CHAOS = os.path.join(ROOT, "jslpsolver_amd", "csrc", "libjslp_hip_chaos.so")
PREFIX = "jslpg_"


@pytest.fixture(scope="module")
def lib():
    return _capi.Library(built(_capi.HIP_LIB_PATH))


def test_header_binding_and_libraries_agree(oracle_lib, lib):
    declared = declared_in_header(HEADER, PREFIX)
    assert declared == set(_capi.TREE_TOL_SYMBOLS) == {"jslpg_tree_pack_create", "jslpg_pack_read_tolerance"}
    for other in ("jslp_engine.h", "jslpp_packed.h", "jslpt_tree.h", "jslps_soft.h", "jslpc_tree_mir.h", "jslpe_tree_enhanced.h",
                  "jslpi_tree_incremental.h", "jslpm_many.h", "jslpx_branch.h", "jslpr_mir.h", "jslpf_f32.h"):
        assert not declared_in_header(os.path.join(ROOT, "include", other), PREFIX)
    assert _capi.TOL_TREE_DTYPE.itemsize == 32
    text = open(HEADER).read()
    order = [text.index(" %s;" % name) for name in _capi.TOL_TREE_DTYPE.names[:4]]  # the struct's members, in the dtype's order
    assert order == sorted(order)
    assert [_capi.TOL_TREE_DTYPE[name] for name in _capi.TOL_TREE_DTYPE.names[:4]] == [np.float64, np.float64, np.int32, np.int32]
    assert exported(built(_capi.HIP_LIB_PATH), PREFIX) == declared and exported(built(CHAOS), PREFIX) == declared
    assert lib.has_tree_tol
    assert exported(oracle_lib.path, PREFIX) == set() and not oracle_lib.has_tree_tol


def _create(lib, n, heights, widths, cut_rows, heap_cap, tolerance, minimize, row_extra=None, incremental=None, max_checkpoints=None,
            n_optional=None):
    h = ctypes.c_void_p()
    arr = lambda a: None if a is None else _capi.ptr_i32(_capi.as_i32(a))  # noqa: E731
    zeros = [0] * n
    rc = lib.jslpg_tree_pack_create(ctypes.byref(h), 0, n, arr(heights), arr(widths), _capi.ptr_f64(_capi.as_f64([1e-8] * max(n, 1))), arr(cut_rows),
                                    arr(heap_cap), arr(n_optional), arr(row_extra), arr(zeros), arr(zeros),
                                    arr(zeros if incremental is None else incremental), arr(zeros if max_checkpoints is None else max_checkpoints),
                                    None if tolerance is None else _capi.ptr_f64(_capi.as_f64(tolerance)), arr(minimize), 0, 0, 0)
    return rc, h, lib.jslp_last_error()


def test_create_argument_errors_without_a_device(lib):
    """refused before any device call: this host has no GPU, and a call that reached the device would answer JSLP_ERR_DEVICE"""
    two = dict(n=2, heights=[3, 3], widths=[4, 4], cut_rows=[2, 2], heap_cap=[4, 4])
    for minimize in ([1, 2], [0, -1], [1, 7]):
        rc, h, msg = _create(lib, tolerance=[0.1, 0.1], minimize=minimize, **two)
        assert rc == _capi.JSLP_ERR_ARG and not h.value and b"LP 1" in msg and b"minimize" in msg, msg
    # minimize is checked whatever the tolerances say, also without a tolerance table
    rc, h, msg = _create(lib, tolerance=None, minimize=[2, 1], **two)
    assert rc == _capi.JSLP_ERR_ARG and b"LP 0" in msg and b"minimize" in msg
    # what jslpi_tree_pack_create refuses is refused here, in its words
    rc, h, msg = _create(lib, tolerance=[0.1, 0.1], minimize=[1, 1], incremental=[0, 2], **two)
    assert rc == _capi.JSLP_ERR_ARG and b"LP 1" in msg and b"incremental is 0 or 1" in msg
    rc, h, msg = _create(lib, tolerance=[0.1, 0.1], minimize=[1, 1], incremental=[0, 1], max_checkpoints=[0, 50], row_extra=[-1, 1], **two)
    assert rc == _capi.JSLP_ERR_ARG and b"LP 1" in msg and b"row_extra" in msg
    rc, h, msg = _create(lib, 1, [2 ** 30], [2 ** 30], [0], [8], [0.5], [1])
    assert rc == _capi.JSLP_ERR_UNSUPPORTED and b"LP 0" in msg
    # any tolerance value is an argument the create takes: with nothing else wrong it goes on to the device (none here, or a pack there)
    for tolerance, minimize in (([0.5, float("nan")], [1, 0]), ([-1.0, 0.0], None), ([3.0, float("inf")], [0, 0]), (None, None), (None, [1, 0])):
        rc, h, msg = _create(lib, tolerance=tolerance, minimize=minimize, **two)
        assert rc in (_capi.JSLP_OK, _capi.JSLP_ERR_DEVICE), msg
        if rc == _capi.JSLP_OK:
            lib.jslpp_pack_destroy(h)
    assert lib.jslpg_pack_read_tolerance(None, None) == _capi.JSLP_ERR_ARG


def test_python_refusals(oracle_lib):
    it = U.Item(T.LATE)
    with pytest.raises(ValueError, match="tolerance entries"):
        T.make_pack(oracle_lib, [it], [None], [0.1, 0.2], [True])
    with pytest.raises(ValueError, match="minimize flags"):
        T.make_pack(oracle_lib, [it], [None], [0.1], [True, False])
    with pytest.raises(_capi.EngineError, match=r"LP 0: minimize is 0"):
        from jslpsolver_amd.engine import TableauPack
        TableauPack([it.lp], lib=oracle_lib, integers=[it.integers], tolerance=[0.5], minimize=[2])
    with pytest.raises(ValueError, match="needs `integers`"):
        from jslpsolver_amd.engine import TableauPack
        TableauPack([it.lp], lib=oracle_lib, tolerance=[0.5])


def test_no_tolerance_is_the_pack_without_the_arrays(oracle_lib):
    """None, 0, a negative value and NaN mean none, as `tolerance > 0` decides in the reference"""
    names = ["Integer_Wood_Shop_Problem", "Knapsack_1", "TacoParty"]
    policies = [None, ("hybrid", "strong"), I.Inc("depth-first")]
    items = [I.Item(U.fixture(n)["model"]) if isinstance(p, I.Inc) else U.Item(U.fixture(n)["model"]) for n, p in zip(names, policies)]
    plain = T.solve(oracle_lib, items, policies, None, None, with_arrays=False)
    want = T.states(plain)
    assert not plain.has_tolerance
    for value in (None, 0, 0.0, -0.5, float("nan"), float("-inf")):
        for minimize in (True, False):
            pack = T.solve(oracle_lib, items, policies, [value] * 3, [minimize] * 3)
            assert not pack.has_tolerance and T.states(pack) == want, (value, minimize)
            assert pack.tolerance.tobytes() == bytes(32 * 3)
            pack.close()
    plain.close()


def test_golden_records_on_the_restatement(oracle_lib):
    """every record of tolerance.json.gz and every tolerance record of mir.json.gz that fits a pack: iterations, pivot digest, result,
    bestPossibleEval.  LargeFarmMIP (36 x 101, 100 integer variables) holds 44 cut rows in 64 KiB: its useMIRCuts tree does NOT fit the pack's
    row capacity (the root's MIR rounds alone need more rows) and is left out; so are the records with useMIRCuts under the enhanced or the
    incremental service, which the pack does not have.  Its best-first trees need more heap entries than solve_packed's 128: they run here
    with heap_cap 8192."""
    fit, out = [], []
    for c, model in T.golden_records():
        lp = T.lp_of(model)
        (fit if lp is not None else out).append((c, model, lp))
    assert len(fit) + len(out) == 91 and all(c["options"].get("useMIRCuts") and len(c["options"]) > 2 for c, _, _ in out) and len(out) == 6
    farm_mir = [k for k, (c, _, _) in enumerate(fit) if c.get("file", "").endswith("LargeFarmMIP.json.gz") and c["options"].get("useMIRCuts")]
    assert len(farm_mir) == 2  # (tolerance.json.gz's and mir.json.gz's record of the same run)
    for k in farm_mir:
        c, model, (it, policy) = fit[k]
        with pytest.raises(_capi.EngineError, match="row_extra reached"):
            T.solve(oracle_lib, [it], [policy], [model["options"]["tolerance"]], [it.model.isMinimization])
    fit = [f for k, f in enumerate(fit) if k not in farm_mir]
    items, policies = [lp[0] for _, _, lp in fit], [lp[1] for _, _, lp in fit]
    pack = T.solve(oracle_lib, items, policies, [m["options"]["tolerance"] for _, m, _ in fit], [it.model.isMinimization for it in items],
                   heap_cap=8192, trace_cap=max(c["nPivots"] for c, _, _ in fit) + 16)
    assert not pack.status.any() and pack.has_tolerance and pack.is_tolerance.all()
    for i, (c, _, _) in enumerate(fit):
        T.check_golden(pack, i, items[i], c)
    names = {os.path.basename(c["file"]) for c, _, _ in fit if "file" in c}
    assert names == {"StockCuttingProblem.json.gz", "LargeFarmMIP.json.gz"}
    assert sum(1 for c, _, _ in fit if "file" in c) == 13 + 1 + 12 and sum(1 for c, _, _ in fit if "line" in c) == 57
    # the records show the option at work: trees that stop early, and trees that do not
    stopped = pack.tolerance["stopped"]
    assert 20 < int(stopped.sum()) < len(fit) and (pack.tolerance["left"][stopped == 1] > 0).all() and not pack.tolerance["left"][stopped == 0].any()
    fewer = [c for c, _, _ in fit if "iterationsWithout" in c and c["iterations"] < c["iterationsWithout"]]
    assert len(fewer) >= 8
    pack.close()


def _routed(monkeypatch):
    """the `tolerance=` / `integers=` of every TableauPack solve_packed makes from here on"""
    seen = []
    plain = solver.TableauPack

    class Spy(plain):
        def __init__(self, lps, **kw):
            seen.append((len(lps), kw.get("integers") is not None, kw.get("tolerance"), kw.get("minimize")))
            plain.__init__(self, lps, **kw)

    monkeypatch.setattr(solver, "TableauPack", Spy)
    return seen


def test_routing_with_and_without_the_keyword(oracle_lib, monkeypatch):
    wood = U.fixture("Integer_Wood_Shop_Problem")["model"]

    def with_options(**options):
        m = copy.deepcopy(wood)
        m["options"] = options
        return m

    models = [with_options(tolerance=0.05), with_options(tolerance=0.05, useMIRCuts=True), with_options(tolerance=0.05, nodeSelection="depth-first"),
              with_options(tolerance=0.05, useIncremental=True), with_options(tolerance=0.05, timeout=100000), with_options(),
              T.negated(with_options(tolerance=0.5))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [repr(Solve(m, lib=oracle_lib)) for m in models]
        seen = _routed(monkeypatch)
        assert [repr(r) for r in solver.solve_packed(models, lib=oracle_lib)] == want
        assert seen == [(1, True, None, None)]  # without the keyword only the model without a tolerance is in a pack
        del seen[:]
        assert [repr(r) for r in solver.solve_packed(models, lib=oracle_lib, tolerance=True)] == want
        # useIncremental still needs its own keyword; the timeout model stays out whatever is said
        assert seen == [(5, True, [0.05, 0.05, 0.05, None, 0.5], [False, False, False, False, True])]
        del seen[:]
        assert [repr(r) for r in solver.solve_packed(models, lib=oracle_lib, tolerance=True, incremental=True)] == want
        assert seen == [(6, True, [0.05, 0.05, 0.05, 0.05, None, 0.5], [False, False, False, False, False, True])]
        with pytest.raises(TypeError):
            solver.solve_packed(models, lib=oracle_lib, tolerances=True)


def test_solve_packed_equals_solve_on_fuzz_models_with_a_tolerance(oracle_lib, monkeypatch):
    cases = U._cases("fuzz_services.jsonl.gz")[:200]
    models = []
    for c in cases:
        m = copy.deepcopy(c["model"])
        m["options"] = dict(m.get("options") or {}, tolerance=0.05)
        models.append(m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [repr(Solve(m, lib=oracle_lib)) for m in models]
        seen = _routed(monkeypatch)
        assert [repr(r) for r in solver.solve_packed(models, lib=oracle_lib, tolerance=True, incremental=True)] == want
        in_packs = sum(n for n, trees, tolerance, _ in seen if trees and tolerance is not None)
        assert in_packs >= 150, seen  # (the rest: models without integer variables, and trees beyond the pack's capacities)
        del seen[:]
        assert [repr(r) for r in solver.solve_packed(models, lib=oracle_lib)] == want
        assert all(tolerance is None for _, _, tolerance, _ in seen) and sum(n for n, trees, _, _ in seen if trees) == 0


def test_the_edge_models_have_their_properties(oracle_lib):
    """what tests/test_tree_tol_gpu.py relies on, shown on the host walks"""
    walk = lambda model, policy, tol, **kw: T.host_walk(oracle_lib, I.Item(model) if isinstance(policy, I.Inc) else U.Item(model), policy, tol,  # noqa: E731
                                                        model["opType"] == "min", **kw)
    # 1: the node evaluated after the flag was lowered becomes the incumbent; breaking at once gives one iteration less and another result
    n, rec, evaluation, _ = walk(T.LATE, None, 0.5)
    n_now, rec_now, evaluation_now, _ = walk(T.LATE, None, 0.5, _late_stop=False)
    assert (n, evaluation, rec["stopped"], rec["left"]) == (9, 28.0, 1, 4) and (n_now, evaluation_now, rec_now["left"]) == (8, 29.0, 5)
    # 2: equality does not stop, the next factor above does
    n, rec, evaluation, _ = walk(T.EXACT, None, 0.25)
    assert (n, rec["best_possible"], rec["threshold"], evaluation, rec["stopped"]) == (5, 100.0, 125.0, 125.0, 0)
    assert 1 + T.EXACT_UP == np.nextafter(1.25, 2) and 1 + float(np.nextafter(0.25, 1)) == 1.25
    n, rec, evaluation, _ = walk(T.EXACT, None, T.EXACT_UP)
    assert (n, rec["best_possible"], rec["threshold"], evaluation, rec["stopped"], rec["left"]) == (3, 100.0, 100.0 * float(np.nextafter(1.25, 2)), 125.0, 1, 2)
    assert rec["threshold"] > 125.0
    # 3: a maximisation with tolerance >= 1: the factor is 0 or negative
    for tol, threshold in ((1, -0.0), (3, 63.0)):
        n, rec, _, _ = walk(T.MAXI, ("hybrid", None), tol)
        assert (rec["best_possible"], rec["stopped"], rec["left"]) == (-31.5, 1, 4) and np.float64(rec["threshold"]).tobytes() == np.float64(threshold).tobytes()
        n, rec, _, _ = walk(T.MAXI, None, tol)  # the default service's heap is empty behind the late node: emptiness is tested first
        assert (n, rec["stopped"], rec["left"]) == (5, 0, 0) and walk(T.MAXI, None, tol, _late_stop=False)[0] == 4
    # 4: bestPossibleEval from the second node, or from none
    n, rec, _, optimal = walk(T.LATE_ROOT, None, 0.5)
    assert optimal[:2] == [False, True] and (n, rec["best_possible"], rec["threshold"], rec["stopped"]) == (3, -8.0, -4.0, 1)
    n, rec, _, optimal = walk(T.NO_OPTIMUM, None, 0.5)
    assert optimal == [False] and (n, rec["best_possible"], rec["stopped"]) == (1, 0.0, 0)
    # 5: an integral root
    n, rec, _, _ = walk(T.INTEGRAL_ROOT, None, 0.5)
    assert (n, rec["best_possible"], rec["threshold"], rec["stopped"], rec["left"]) == (1, 50.0, 0.0, 0, 0)
    # 6 - 8: the first incumbent, in turn 20, ends the depth-first phase; turn 21 lowers the flag and still runs; turn 22 stops
    for policy in (("hybrid", None), ("depth-first", "most-fractional"), I.Inc(), I.Inc("depth-first")):
        n, rec, _, _ = walk(T.MAXI, policy, 3)
        assert (n, rec["stopped"], rec["left"]) == (21, 1, 4) and walk(T.MAXI, policy, 3, _late_stop=False)[0] == 20
