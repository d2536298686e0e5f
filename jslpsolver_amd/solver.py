"""`Solve(model)` with the reference's JSON model API and result shape (src/main.ts:94-193), the simplex
hot path running on the MI355X engine.  Model parsing and the branch-and-bound tree stay on the CPU.
"""
import math
import os
import warnings

import numpy as np

from . import _capi
from .branch_and_cut import branch_and_cut, js_round
from .engine import Tableau, TableauPack, checkpoint_bytes, incremental_rows, pack_fits, simplex_many, tree_cut_rows, tree_mir_rows
from .model import Model, js_keys

EPSILON = 2.220446049250313e-16
_presolve_warned = False
# solve_packed: the heap entries and the nodes a tree in the pack may use before it is handed to Solve (include/jslpt_tree.h)
TREE_HEAP_CAP = 128
TREE_MAX_NODES = 1 << 16
# solve_packed(incremental=True): the checkpoints an incremental LP may take (maxCheckpoints of the reference) and the device memory the
# checkpoint arenas of ONE pack may take together -- a memory budget, not a tuned value: the incremental LPs beyond it get a pack of their own
TREE_MAX_CHECKPOINTS = _capi.JSLPI_CHECKPOINTS_DEFAULT
PACK_CHECKPOINT_BYTES = 4 << 30


def _round_value(v, rounding_coeff):
    """Math.round((Number.EPSILON + v) * rc) / rc (solution.ts:55-56)"""
    return js_round((EPSILON + v) * rounding_coeff) / rounding_coeff


def Solve(model, precision=None, full=False, validate=False, lib=None, device=0, row_capacity_extra=None,
          speculate=1, group=None):
    """Drop-in for `solver.Solve(model, precision, full, validate)`.

    speculate > 1: evaluate up to that many branch-and-bound nodes per engine call (speculation with in-order
    commit: identical results, see branch_and_cut); `group`: a torch.distributed process group over which each
    batch is sharded, one GPU per rank (every rank calls Solve with the same model and gets the same result).

    `lib` selects the engine library (default: the HIP product library; tests pass the CPU oracle to exercise
    the host logic without a GPU).  Returns the simplified result dict, or -- with full=True -- a dict that
    also carries the final tableau read-back.

    Differences from the reference host, by design (this Python host exists for pytest and bench.py; the drop-in host
    is the reference's own code under host/gpu-tableau.js): the presolve pre-pass (src/tableau/presolve.ts, on by
    default for models with integer variables) is NOT run -- it can fix variables or declare infeasibility before any
    simplex, so results may differ on models it touches (a UserWarning says so once); `options.keep_solutions` is
    rejected (UnsupportedModel).
    """
    m, t, n_int, incremental = _prepare(model, precision, lib, device, row_capacity_extra)
    try:
        return _solve_on(t, m, n_int, incremental, speculate, group, full)
    finally:
        t.close()  # also on errors (JSLP_ERR_CAPACITY ...): the engine goes back to the library's resource pool


def solve_many(models, precision=None, lib=None, device=0):
    """[Solve(m, precision, lib=lib, device=device) for m in models], in order, with the simplex() of every model without integer
    variables solved in ONE engine call (engine.simplex_many: one workgroup per LP on the GPU).  Models with integer variables go
    through Solve's branch-and-bound as they are.  A model Solve rejects raises the same exception before anything is solved."""
    prepared = []
    try:
        for model in models:
            prepared.append(_prepare(model, precision, lib, device, None))
        lps = [(m, t) for m, t, n_int, _ in prepared if n_int == 0]
        simplex_many([t for _, t in lps], check_cycles=[m.checkForCycles for m, _ in lps])
        return [_solve_on(t, m, n_int, incremental, 1, None, False, simplex_done=n_int == 0)
                for m, t, n_int, incremental in prepared]
    finally:
        for _, t, _, _ in prepared:
            t.close()


class _PackedLp:
    """LP i of a solved TableauPack as _solve_on reads a Tableau: the scalars simplex() folds and the RHS read-back"""

    def __init__(self, pack, i):
        self._pack, self._i = pack, i
        self.evaluation = float(pack.evaluation[i])
        self.feasible = bool(pack.feasible[i])
        self.bounded = bool(pack.bounded[i])
        # (what a full result reports as `checkpoints` / `incrementalNodes`: an incremental LP's, 0 for every other)
        self.checkpoints_used = int(pack.incremental[i]["checkpoints_used"])
        self.incremental_nodes = int(pack.incremental[i]["incremental_nodes"])

    def read_rhs(self):
        return self._pack.read_rhs(self._i)


def _tree_in_scope(m, tolerance=False):
    """whether the default branch-and-cut service alone decides this model's result, with nothing that needs the host or a clock
    (include/jslpt_tree.h).  tolerance=True (all four scope tests): options.tolerance keeps no model out -- the tree kernel honours it
    (include/jslpg_tree_tolerance.h)"""
    return not m.useMIRCuts and _mir_tree_in_scope(m, tolerance)


def _mir_tree_in_scope(m, tolerance=False):
    """_tree_in_scope whatever options.useMIRCuts says: the default service's MIR loop runs in the tree kernel too (include/jslpc_tree_mir.h)"""
    o = m.options
    return not (o.get("useIncremental") is True or o.get("nodeSelection") or o.get("branching") or (m.tolerance and not tolerance) or m.timeout
                or m.keep_solutions)


def _enhanced_tree_in_scope(m, tolerance=False):
    """whether the ENHANCED service alone decides this model's result (main.ts:74-80: options.nodeSelection and/or options.branching, no
    useIncremental), with nothing that needs the host or a clock and without its own MIR loop (include/jslpe_tree_enhanced.h)"""
    o = m.options
    if (o.get("nodeSelection") or "hybrid") not in _capi.ENH_NODE_SELECTION or (o.get("branching") or "pseudocost") not in _capi.ENH_BRANCHING:
        return False  # (a name the service does not know: Solve walks it as the reference does)
    return bool(o.get("nodeSelection") or o.get("branching")) and not (o.get("useIncremental") is True or m.useMIRCuts or (m.tolerance and not tolerance)
                                                                       or m.timeout or m.keep_solutions)


def _incremental_tree_in_scope(m, tolerance=False):
    """whether the INCREMENTAL service alone decides this model's result (main.ts:62-72: options.useIncremental), with nothing that needs
    the host or a clock and without its MIR loop (include/jslpi_tree_incremental.h)"""
    o = m.options
    if (o.get("nodeSelection") or "hybrid") not in _capi.ENH_NODE_SELECTION or (o.get("branching") or "pseudocost") not in _capi.ENH_BRANCHING:
        return False  # (a name the service does not know: Solve walks it as the reference does)
    return o.get("useIncremental") is True and not (m.useMIRCuts or (m.tolerance and not tolerance) or m.timeout or m.keep_solutions)


def solve_packed(models, precision=None, lib=None, device=0, incremental=False, tolerance=False, big_lds=False):
    """[Solve(m, precision, lib=lib, device=device) for m in models], in order, for the workload of many SMALL models.  Every model
    whose tableau -- with its optional objectives, one row per soft constraint priority, when it has any (include/jslps_soft.h) -- fits the
    pack's LDS limit goes through an engine.TableauPack -- one arena, one upload, one launch per kernel build (64 or 256 threads, each with
    or without optional objectives), one read-back, no engine per model:
      * without integer variables (engine.pack_fits): its simplex();
      * with integer variables, under the default branch-and-cut service with no tolerance and no timeout, when the tableau with
        min(2 per integer variable, the most that fit) >= 1 cut rows fits (engine.tree_cut_rows): its whole tree, walked on the device
        (TableauPack.branch_and_cut).  A tree that reaches a capacity of the pack (heap, cut rows, nodes) is solved again through Solve;
      * the same with options.useMIRCuts and no optional objectives (include/jslpc_tree_mir.h), as a MIR LP of that pack, when
        row_extra = min(2 per integer variable + 320, the most rows that fit) >= 1, with cut_rows = min(2 per integer variable, row_extra)
        (engine.tree_mir_rows): every node's MIR loop runs in the kernel as well.  Its further capacities are the row capacity
        height + row_extra, which the root's MIR rows, a node's cuts and the node's MIR rows share, and 64 MIR rounds of one node;
      * with integer variables and options.nodeSelection and/or options.branching -- the enhanced service -- without useIncremental,
        useMIRCuts, tolerance, timeout, keep_solutions and optional objectives (include/jslpe_tree_enhanced.h), as an enhanced LP of
        that same pack, under the cut-row rule of the default service; its depth-first stack and its heap share the heap entries.
      * incremental=True (opt-in): with integer variables and options.useIncremental -- the incremental service -- without useMIRCuts,
        tolerance, timeout, keep_solutions and optional objectives (include/jslpi_tree_incremental.h), as an incremental LP of that same
        pack, when row_extra = min(2 per integer variable + 256, the most rows that fit) >= 1, with cut_rows = min(2 per integer
        variable, row_extra) (engine.incremental_rows) and 50 checkpoints.  Its further capacity is the row capacity height +
        row_extra, which a chain of checkpoints fills one row per level.  The checkpoint arenas of one pack stay within
        PACK_CHECKPOINT_BYTES: the incremental LPs beyond that go into a following pack.  Without the keyword such a model goes through
        Solve.
      * tolerance=True (opt-in): options.tolerance keeps a model out of none of the four tree routes above: its LP carries the tolerance and
        the model's sense into the pack, and its walk ends on the reference's toleranceFlag inside the kernel, one node late as the
        reference's does (include/jslpg_tree_tolerance.h).  options.timeout (a clock) and keep_solutions still keep a model out.  Without
        the keyword a model with a tolerance goes through Solve.
      * big_lds=True (opt-in, include/jslpb_big_lds.h): the packs take tableaus up to JSLPB_LDS_LIMIT, 156 KiB of LDS, instead of 64 KiB.  A
        model that joins a pack under the rules above joins it exactly as without the keyword -- same cut rows, same build.  The keyword only
        ADDS models those rules leave out: a model without integer variables, soft constraints or not, whose tableau fits the larger limit;
        and a default-service tree (no tolerance), soft constraints or not, with min(2 per integer variable, the most cut rows that fit the
        larger limit) >= 1.  They run in the large builds of the pack kernels.  MIR, enhanced and incremental models and models with a
        tolerance keep the 64 KiB rules.  A large tree that reaches a capacity is solved again through Solve like any other.
    Every other model goes through Solve as it is.  A model Solve rejects raises the same exception before anything is solved."""
    lib = lib if lib is not None else _capi.load_hip()
    models = list(models)
    parsed = [_parse(model, precision, 4) for model in models]
    packed = []  # positions of the models that go into the pack of plain LPs
    trees = []   # (position, cut rows, row_extra or -1) of the models whose tree goes into the pack with trees (row_extra >= 0: a MIR LP)
    policies = {}  # position -> (options.nodeSelection or None, options.branching or None) of the enhanced and the incremental LPs among them
    inc = set()    # positions of the incremental LPs among them (their row_extra is their row capacity: no MIR LPs)
    optional = [None] * len(models)  # per model its optional objectives (None: none)
    big = set()    # positions of the models that only the larger limit of big_lds lets in (the large LPs)
    big_limit = _capi.JSLPB_LDS_LIMIT if big_lds else None
    for k, (m, matrix, _, _) in enumerate(parsed):
        _priorities, optional_rows = m.optional_objectives()
        n_opt = 0
        if optional_rows is not None and len(optional_rows) > 0:
            optional[k] = optional_rows
            n_opt = len(optional_rows)
        n_int = len(m.integerVariables)
        if n_int == 0:
            if pack_fits(*matrix.shape, lib=lib, n_optional=n_opt):
                packed.append(k)
            elif big_lds and pack_fits(*matrix.shape, lib=lib, n_optional=n_opt, limit=big_limit):
                packed.append(k)
                big.add(k)
        elif _tree_in_scope(m, tolerance):
            cut_rows = tree_cut_rows(matrix.shape[0], matrix.shape[1], n_int, lib=lib, n_optional=n_opt)
            if cut_rows >= 1:
                trees.append((k, cut_rows, -1))
            elif big_lds and not m.tolerance:  # (an LP with a tolerance keeps the 64 KiB rule)
                cut_rows = tree_cut_rows(matrix.shape[0], matrix.shape[1], n_int, lib=lib, n_optional=n_opt, limit=big_limit)
                if cut_rows >= 1:
                    trees.append((k, cut_rows, -1))
                    big.add(k)
        elif m.useMIRCuts and n_opt == 0 and _mir_tree_in_scope(m, tolerance):
            row_extra, cut_rows = tree_mir_rows(matrix.shape[0], matrix.shape[1], n_int, lib=lib)
            if row_extra >= 1:
                trees.append((k, cut_rows, row_extra))
        elif n_opt == 0 and _enhanced_tree_in_scope(m, tolerance):
            cut_rows = tree_cut_rows(matrix.shape[0], matrix.shape[1], n_int, lib=lib)
            if cut_rows >= 1:
                trees.append((k, cut_rows, -1))
                policies[k] = (m.options.get("nodeSelection") or None, m.options.get("branching") or None)
        elif incremental and n_opt == 0 and _incremental_tree_in_scope(m, tolerance):
            row_extra, cut_rows = incremental_rows(matrix.shape[0], matrix.shape[1], n_int, lib=lib)
            if row_extra >= 1:
                trees.append((k, cut_rows, row_extra))
                inc.add(k)
                policies[k] = (m.options.get("nodeSelection") or None, m.options.get("branching") or None)
    results = [None] * len(models)
    if packed:
        pack = TableauPack([(parsed[k][1], parsed[k][2], parsed[k][3], parsed[k][0].unrestricted) for k in packed],
                           precision=[parsed[k][0].precision for k in packed], lib=lib, device=device,
                           optional_objectives=[optional[k] for k in packed], big_lds=any(k in big for k in packed))
        try:
            pack.simplex(check_cycles=[parsed[k][0].checkForCycles for k in packed])
            for i, k in enumerate(packed):
                results[k] = _solve_on(_PackedLp(pack, i), parsed[k][0], 0, False, 1, None, False, simplex_done=True)
        finally:
            pack.close()
    # (a pack holds MIR LPs or LPs with optional objectives, never both: when both kinds are there, the MIR LPs get a pack of their own)
    mir_trees = [t for t in trees if t[2] >= 0 and t[0] not in inc]
    if mir_trees and any(optional[k] is not None for k, _, _ in trees):
        trees = [t for t in trees if t[2] < 0 or t[0] in inc]
        _solve_tree_pack(mir_trees, parsed, optional, lib, device, results, policies)
    for chunk in _within_checkpoint_budget(trees, inc, parsed, lib):
        _solve_tree_pack(chunk, parsed, optional, lib, device, results, policies, inc, big)
    for k, model in enumerate(models):
        if results[k] is None:
            results[k] = Solve(model, precision, lib=lib, device=device)
    return results


def _within_checkpoint_budget(trees, inc, parsed, lib):
    """`trees` in order, cut into consecutive packs whose checkpoint arenas -- TREE_MAX_CHECKPOINTS slots per incremental LP -- stay within
    PACK_CHECKPOINT_BYTES each (one pack when there is no incremental LP)"""
    chunks, used = [[]], 0
    for entry in trees:
        k, _, row_extra = entry
        need = 0
        if k in inc:
            h, w = parsed[k][1].shape
            slot = lib.jslpi_checkpoint_bytes(h, w, h + row_extra) if getattr(lib, "has_tree_inc", False) else checkpoint_bytes(h, w, h + row_extra)
            need = TREE_MAX_CHECKPOINTS * int(slot)
        if chunks[-1] and used + need > PACK_CHECKPOINT_BYTES:
            chunks.append([])
            used = 0
        chunks[-1].append(entry)
        used += need
    return [c for c in chunks if c]


def _solve_tree_pack(trees, parsed, optional, lib, device, results, policies, inc=frozenset(), big=frozenset()):
    """solve_packed's pack with trees: results[k] for every model of `trees` whose LP reached no capacity (the others stay None: Solve).
    big: the models among them that only the larger limit of big_lds lets in -- with any, the pack is made with big_lds"""
    if trees:
        with_mir = any(e >= 0 and k not in inc for k, _, e in trees)
        with_inc = any(k in inc for k, _, _ in trees)
        with_tol = any(parsed[k][0].tolerance for k, _, _ in trees)  # (solve_packed(tolerance=True) alone lets such a model in)
        pack = TableauPack([(parsed[k][1], parsed[k][2], parsed[k][3], parsed[k][0].unrestricted) for k, _, _ in trees],
                           precision=[parsed[k][0].precision for k, _, _ in trees], lib=lib, device=device,
                           integers=[[v["index"] for v in parsed[k][0].integerVariables] for k, _, _ in trees], cut_rows=[c for _, c, _ in trees],
                           heap_cap=TREE_HEAP_CAP, max_nodes=TREE_MAX_NODES,
                           optional_objectives=None if with_mir else [optional[k] for k, _, _ in trees],
                           mir=[e >= 0 and k not in inc for k, _, e in trees] if with_mir else None,
                           row_extra=[e for _, _, e in trees] if with_mir or with_inc else None,
                           incremental=[k in inc for k, _, _ in trees] if with_inc else None, max_checkpoints=TREE_MAX_CHECKPOINTS,
                           node_selection=[policies.get(k, (None, None))[0] for k, _, _ in trees],
                           branching=[policies.get(k, (None, None))[1] for k, _, _ in trees],
                           tolerance=[parsed[k][0].tolerance or None for k, _, _ in trees] if with_tol else None,
                           minimize=[bool(parsed[k][0].isMinimization) for k, _, _ in trees] if with_tol else None,
                           big_lds=any(k in big for k, _, _ in trees))
        try:
            try:
                pack.branch_and_cut(check_cycles=[parsed[k][0].checkForCycles for k, _, _ in trees])
            except _capi.EngineError:
                if not (pack.status == _capi.JSLP_ERR_CAPACITY).any() or not np.isin(pack.status, (_capi.JSLP_OK, _capi.JSLP_ERR_CAPACITY)).all():
                    raise
            for i, (k, _, _) in enumerate(trees):
                if pack.status[i] == _capi.JSLP_OK:  # (an LP that reached a capacity is left out: Solve)
                    results[k] = _solve_on(_PackedLp(pack, i), parsed[k][0], 0, False, 1, None, False, simplex_done=True,
                                           integral=bool(pack.tree[i]["is_integral"]))
        finally:
            pack.close()


def _parse(model, precision, stacklevel):
    """what Solve checks and builds before any engine exists: the parsed model and its tableau"""
    global _presolve_warned
    if model is None:
        raise ValueError("Solver requires a model to operate on")  # main.ts:110-112
    m = Model(model, precision)
    if m.keep_solutions:
        from .model import UnsupportedModel
        raise UnsupportedModel("options.keep_solutions is not collected by the Python host (use the reference host + binding)")
    if m.usePresolve and len(m.integerVariables) > 0 and not _presolve_warned:
        _presolve_warned = True
        warnings.warn("jslpsolver_amd.Solve does not run the reference's presolve pre-pass (src/tableau/presolve.ts): on models "
                      "where presolve fixes variables or proves infeasibility the result can differ from solver.Solve(); "
                      "pass options.presolve = false to compare like with like, or use the reference host + binding", stacklevel=stacklevel)
    matrix, vibr, vibc = m.build_tableau()
    return m, matrix, vibr, vibc


def _prepare(model, precision, lib, device, row_capacity_extra):
    """Solve's set-up: the parsed model, its engine with the tableau uploaded, the integer count and the service choice"""
    m, matrix, vibr, vibc = _parse(model, precision, 4)
    n_int = len(m.integerVariables)
    # cut rows: at most one "min" and one "max" cut per integer variable (branch-and-cut.ts:166-179)
    extra = 2 * n_int if row_capacity_extra is None else row_capacity_extra
    incremental = n_int > 0 and (m.options.get("useIncremental") is True)
    if incremental and row_capacity_extra is None:
        # the incremental service stacks ONE row per tree level on the parent's tableau and never merges cuts on the
        # same variable (incremental-branch-and-cut.ts:248-253), so its height is bounded by the depth of the tree, not
        # by the number of integer variables; the reference reallocates (cutting-strategies.ts:24-30), device memory
        # is sized once -- a deeper tree fails loudly with JSLP_ERR_CAPACITY (pass row_capacity_extra)
        extra = 2 * n_int + 256
    if n_int > 0 and m.useMIRCuts and row_capacity_extra is None:
        # every MIR round appends up to 10 rows (cutting-strategies.ts:199-212); the default service's loop has no bound
        # but a 10 % volume gain per round (branch-and-cut.ts:38-52): 32 rounds of headroom, loud failure beyond
        extra += 320
    _priorities, optional_rows = m.optional_objectives()
    t = Tableau(matrix, vibr, vibc, m.unrestricted, precision=m.precision, row_capacity=matrix.shape[0] + extra,
                device=device, lib=lib, optional_objectives=optional_rows,
                integer_variables=[v["index"] for v in m.integerVariables] if m.useMIRCuts else None)
    return m, t, n_int, incremental


def _solve_on(t, m, n_int, incremental, speculate, group, full, simplex_done=False, integral=False):
    iterations = 0
    if n_int > 0:  # tableau.ts:250-258
        evaluate = None
        if group is not None:
            from .sharding import make_sharded_evaluator
            evaluate = make_sharded_evaluator(t, m.checkForCycles, group, watched=m.integer_index_array,
                                              branch=os.environ.get("JSLP_SHARD_BRANCH", "0") == "1")
        if incremental:  # selectBranchAndCutService (main.ts:62-72)
            from .incremental_branch_and_cut import incremental_branch_and_cut
            iterations, integral = incremental_branch_and_cut(
                t, m, node_selection=m.options.get("nodeSelection") or "hybrid",
                branching=m.options.get("branching") or "pseudocost")
        elif m.options.get("nodeSelection") or m.options.get("branching"):  # main.ts:74-80
            from .incremental_branch_and_cut import enhanced_branch_and_cut
            iterations, integral = enhanced_branch_and_cut(
                t, m, node_selection=m.options.get("nodeSelection") or "hybrid",
                branching=m.options.get("branching") or "pseudocost")
        else:
            iterations, integral = branch_and_cut(t, m, speculate=speculate, evaluate_batch=evaluate)
    elif not simplex_done:  # (solve_many: the batch has run it)
        t.simplex(check_cycles=m.checkForCycles)
    rhs, rows = t.read_rhs()
    evaluation = t.evaluation if m.isMinimization else -t.evaluation  # tableau.ts:261
    result = {"feasible": t.feasible, "result": evaluation, "bounded": t.bounded}
    if integral:
        result["isIntegral"] = True
    # generateSolutionSet (solution.ts:35-60) + buildSimplifiedResult (main.ts:173-193)
    by_index = {v["index"]: v for v in m.variables}
    rc = js_round(1 / m.precision)
    solution_set = {}
    for r in range(1, len(rows)):
        var = by_index.get(int(rows[r]))
        if var is None:
            continue
        solution_set[var["id"]] = _round_value(float(rhs[r]), rc)
    for vid in js_keys(solution_set):
        if solution_set[vid] != 0:
            result[vid] = solution_set[vid]
    result = {k: result[k] for k in js_keys(result)}  # JS property order: integer-like ids first
    if full:
        fm, fvibr, fvibc, _, _ = t.download()
        result = {"result": result, "solutionSet": solution_set, "matrix": fm, "varIndexByRow": fvibr,
                  "varIndexByCol": fvibc, "iter": iterations, "pivots": t.pivot_trace(), "model": m,
                  "checkpoints": getattr(t, "checkpoints_used", 0), "incrementalNodes": getattr(t, "incremental_nodes", 0)}
    return result
