"""Host-side branch-and-bound tree (CPU), calling the engine for every LP relaxation.

Mirrors the reference's DEFAULT BranchAndCutService (src/tableau/branch-and-cut.ts:54-199) -- best-first
with LIFO ties (src/tableau/min-heap.ts:43-49), most-fractional branching (src/tableau/mip-utils.ts:100-126)
-- because its visiting order decides which incumbent wins.  The three bulk operations of a node
(restore + addCutConstraints + simplex, branch-and-cut.ts:33-37) are ONE engine call (Tableau.applyCuts).
"""
import math
import os
import time

import numpy as np


def js_round(x):
    """Math.round: nearest integer, ties toward +Infinity"""
    if math.isinf(x) or math.isnan(x):
        return x
    f = math.floor(x)
    return f + 1.0 if x - f >= 0.5 else float(f)


class BranchMinHeap:
    """src/tableau/min-heap.ts: key = relaxedEvaluation ascending, ties -> most recently pushed first."""

    def __init__(self):
        self.heap = []
        self.seq = 0

    def __len__(self):
        return len(self.heap)

    @staticmethod
    def _before(a, b):
        if a[0] != b[0]:
            return a[0] < b[0]
        return a[1] > b[1]

    def push(self, relaxed_evaluation, cuts):
        entry = (relaxed_evaluation, self.seq, cuts)
        self.seq += 1
        h = self.heap
        h.append(entry)
        i = len(h) - 1
        while i > 0:
            p = (i - 1) >> 1
            if not self._before(entry, h[p]):
                break
            h[i] = h[p]
            i = p
        h[i] = entry

    def pop(self):
        h = self.heap
        top = h[0]
        last = h.pop()
        n = len(h)
        if n == 0:
            return top
        i = 0
        half = n >> 1
        while i < half:
            c = 2 * i + 1
            if c + 1 < n and self._before(h[c + 1], h[c]):
                c += 1
            if not self._before(h[c], last):
                break
            h[i] = h[c]
            i = c
        h[i] = last
        return top


class TreeCapacity(Exception):
    """a bound of an instrumented tree walk was reached (CountingHeap, branch_and_cut(max_nodes=...)): `which` names it"""

    def __init__(self, which):
        Exception.__init__(self, "branch_and_cut: %s reached" % which)
        self.which = which


class CountingHeap(BranchMinHeap):
    """BranchMinHeap that counts what a device-side tree has to hold (include/jslpt_tree.h): the pushes, the most entries at once and the
    longest cut list pushed -- and enforces the same capacities, in the kernel's order (the cut list first, then the heap)."""

    def __init__(self, heap_cap=None, cut_rows=None):
        BranchMinHeap.__init__(self)
        self.heap_cap, self.cut_rows = heap_cap, cut_rows
        self.pushes = self.high_water = self.cuts_high_water = 0

    def push(self, relaxed_evaluation, cuts):
        if self.cut_rows is not None and len(cuts) > self.cut_rows:
            raise TreeCapacity("cut_rows")
        if self.heap_cap is not None and len(self.heap) >= self.heap_cap:
            raise TreeCapacity("heap_cap")
        BranchMinHeap.push(self, relaxed_evaluation, cuts)
        self.pushes += 1
        self.high_water = max(self.high_water, len(self.heap))
        self.cuts_high_water = max(self.cuts_high_water, len(cuts))


class _RowMap:
    """rowByVarIndex as the host tree reads it: variable index -> row of the final tableau (-1 = not basic)"""
    __slots__ = ("row_of",)

    def __init__(self, vibr):
        v = np.asarray(vibr[1:], dtype=np.int64)
        self.row_of = np.full(int(v.max()) + 2 if v.size else 1, -1, dtype=np.int64)
        self.row_of[v] = np.arange(1, v.size + 1)

    def get(self, index, default=-1):
        if 0 <= index < self.row_of.shape[0]:
            r = int(self.row_of[index])
            return r if r != -1 else default
        return default

    def rows(self, indexes):
        """rows of several variable indexes at once (-1 = not basic)"""
        out = np.full(indexes.shape[0], -1, dtype=np.int64)
        ok = indexes < self.row_of.shape[0]
        out[ok] = self.row_of[indexes[ok]]
        return out


def _rows_by_var(vibr):
    return _RowMap(vibr)


def _js_round_vec(x):
    f = np.floor(x)
    return np.where(x - f >= 0.5, f + 1.0, f)


class _WatchedRows:
    """the compact outcome of a node (jslp_engine_relax_batch_watched*): rowByVarIndex and the RHS cell of the model's integer
    variables, in model.integerVariables order -- everything isIntegral / getMostFractionalVar read (mip-utils.ts:43-61, 100-126)"""
    __slots__ = ("wrows", "wvals")

    def __init__(self, wrows, wvals):
        self.wrows, self.wvals = wrows, wvals


def _integer_values(model, rhs, rows):
    """(variable indexes, values) of the integer variables that are basic, in model.integerVariables order"""
    idx = model.integer_index_array
    if isinstance(rows, _WatchedRows):
        basic = rows.wrows != -1
        return idx[basic], np.asarray(rows.wvals, dtype=np.float64)[basic]
    r = rows.rows(idx)
    basic = r != -1
    return idx[basic], np.asarray(rhs, dtype=np.float64)[r[basic]]


def is_integral(model, rhs, rows, precision):
    """mip-utils.ts:43-61"""
    if isinstance(rows, _NodeEvalBranch):  # decided on the device (include/jslpx_branch.h)
        return rows.integral
    _idx, values = _integer_values(model, rhs, rows)
    return not bool((np.abs(values - _js_round_vec(values)) > precision).any())


def most_fractional_var(model, rhs, rows):
    """mip-utils.ts:100-126: first variable with the strictly biggest |v - round(v)|"""
    if isinstance(rows, _NodeEvalBranch):
        return rows.branch_var, rows.branch_value
    idx, values = _integer_values(model, rhs, rows)
    if values.size == 0:
        return None, 0.0
    fraction = np.abs(values - _js_round_vec(values))
    fraction = np.where(np.isnan(fraction), -1.0, fraction)  # `fraction > biggest` is false for NaN
    k = int(np.argmax(fraction))  # first index of the maximum
    if not fraction[k] > 0.0:
        return None, 0.0
    return int(idx[k]), float(values[k])


def fractional_volume(model, rhs, vibr, precision):
    """computeFractionalVolume(ignoreIntegerValues = true) (mip-utils.ts:67-92): the product, in row order, of |value|
    over the basic integer variables that are not at an integer value"""
    from .engine import fractional_volume_rows
    return fractional_volume_rows(model.integer_index_set, rhs, vibr, precision)


def mir_loop(tableau, model, rhs, vibr, check, max_rounds=None, need_feasible=False):
    """The MIR loop that follows the simplex() of a node: branch-and-cut.ts:38-52 (unbounded, no feasibility test) or
    incremental-branch-and-cut.ts:228-243, 261-276 (at most 3 rounds, feasible tableaus only).  Every round is one
    engine call (applyMIRCuts + simplex + read-back); the stopping rule needs only the RHS column."""
    if not model.useMIRCuts or (need_feasible and not tableau.feasible):
        return rhs, vibr
    rounds = 0
    while max_rounds is None or rounds < max_rounds:
        before = fractional_volume(model, rhs, vibr, tableau.precision)
        _n, _res, rhs, vibr = tableau.mirRound(check_cycles=check)
        after = fractional_volume(model, rhs, vibr, tableau.precision)
        rounds += 1
        if after >= 0.9 * before:
            break
    return rhs, vibr


class _NodeEval:
    """outcome of one LP relaxation as the host tree consumes it"""
    __slots__ = ("res", "rhs", "vibr")

    def __init__(self, res, rhs, vibr):
        self.res, self.rhs, self.vibr = res, rhs, vibr


class _NodeEvalMIR:
    """outcome of a node evaluated WITH its MIR loop (Tableau.applyCutsBatchMIR): the last simplex's result with the folded evaluation,
    the loop's outcome record, and the whole RHS column / row map"""
    __slots__ = ("res", "outcome", "rhs", "vibr")

    def __init__(self, res, outcome, rhs, vibr):
        self.res, self.outcome, self.rhs, self.vibr = res, outcome, rhs, vibr


class _NodeEvalWatched:
    """the same from a COMPACT outcome: the integer variables' rows and values only (the full column of the one leaf the tree commits
    to is re-evaluated at the end, as host/gpu-tableau.js's flush() does)"""
    __slots__ = ("res", "wrows", "wvals")

    def __init__(self, res, wrows, wvals):
        self.res, self.wrows, self.wvals = res, wrows, wvals


class _NodeEvalBranch:
    """the same from a BRANCH RECORD (include/jslpx_branch.h): isIntegral() and getMostFractionalVar() already decided on the device, over
    the integer variables in model.integerVariables order -- 32 bytes per node whatever their number"""
    __slots__ = ("res", "integral", "branch_var", "branch_value")

    def __init__(self, res, record):
        from ._capi import BRANCH_INTEGRAL
        self.res = res
        self.integral = bool(int(record["flags"]) & BRANCH_INTEGRAL)
        k = int(record["branch_var_index"])
        self.branch_var = k if k >= 0 else None
        self.branch_value = float(record["branch_var_value"]) if k >= 0 else 0.0


EVAL_STATS = {"seconds": 0.0, "batches": 0, "nodes": 0}  # speculative batches since the caller last zeroed it (bench.py)
# nodes whose evaluation equalled the incumbent's on a tableau with optional objectives (branch-and-cut.ts:107-127), and how many of them won
# the tie on an objective, since the caller last zeroed it (the tests show with it that their inputs reach that code)
TIE_STATS = {"ties": 0, "won": 0}


def branch_and_cut(tableau, model, speculate=1, evaluate_batch=None, read_back=None, heap=None, max_nodes=None, tolerance_out=None,
                   _late_stop=True):
    """branch-and-cut.ts:54-199.  Leaves `tableau` holding the incumbent; returns the iteration count and
    whether an integral node was accepted (tableau.__isIntegral).

    speculate > 1 turns on SPECULATIVE EVALUATION WITH IN-ORDER COMMIT: whenever the sequential
    loop needs a node that has not been evaluated yet, that node and the next best `speculate - 1` heap entries
    are evaluated as ONE batch of independent relaxations (every node is a pure function of the saved root and
    its cut list); the loop itself still pops, prunes and commits in the reference's order, so the incumbent,
    the iteration count and the result are those of the sequential run.  `evaluate_batch(cut_lists)` may shard
    the batch over several GPUs (jslpsolver_amd.sharding); default: the tableau's own applyCutsBatch.

    read_back ("full" / "compact" / "branch"; None = JSLP_TREE_BRANCH=1 -> "branch", else "compact") picks what a speculative batch reads
    back per node: whole RHS columns + row maps, the integer variables' rows and values, or the 32-byte branch record the engine reduces
    them to (include/jslpx_branch.h).  Opt-in; whichever it is, the tree, its result and its iteration count are the same.

    options.useMIRCuts: a speculative batch evaluates every node WITH its MIR loop (Tableau.applyCutsBatchMIR, include/jslpr_mir.h) and reads
    whole columns back (read_back is ignored); the root, before save(), and the final re-evaluation of the incumbent keep the round-by-round
    loop.  Without speculation JSLP_TREE_MIR=1 makes every node after the root one Tableau.applyCutsMIR call.

    heap: the BranchMinHeap to use (a CountingHeap instruments the walk); max_nodes: raise TreeCapacity before evaluating one node more.

    tolerance_out: a dict that gets what include/jslpg_tree_tolerance.h reports of a model with options.tolerance -- best_possible (the
    tableau's bestPossibleEval), threshold (the last acceptableThreshold computed), stopped (the loop ended on toleranceFlag with entries
    still waiting) and left (how many); default: off.  _late_stop is PRIVATE to the tests: False ends the loop on the very turn that lowers the
    flag, which is NOT the reference's rule (:73-87: that turn still runs), so that a test can show the late node matters; no caller of
    the package passes it.
    """
    branches = heap if heap is not None else BranchMinHeap()
    iterations = 0
    tolerance = model.tolerance or 0
    tolerance_flag = True
    terminal_time = 1e99
    if model.timeout:
        terminal_time = time.time() * 1000.0 + model.timeout
    best_evaluation = math.inf
    best_cuts = None
    found_integral = False
    check = model.checkForCycles
    precision = tableau.precision
    n_opt = getattr(tableau, "n_optional", 0)
    best_optional = [math.inf] * n_opt  # bestOptionalObjectivesEvaluations (:66-69)
    # a MIR node is a pure function of the saved root and its cut list like any other: its batches run each node's MIR loop inside the
    # engine call (Tableau.applyCutsBatchMIR, whole columns read back).  A caller's evaluate_batch knows nothing of the loop
    mir = bool(model.useMIRCuts)
    if n_opt > 0 or (mir and evaluate_batch is not None):
        speculate = 1  # the tie-break below reads the live optional-objective cells / the MIR loop is driven per node
    # JSLP_TREE_MIR=1 (read per call): without speculation, every node after the root is ONE engine call too (Tableau.applyCutsMIR)
    mir_one_call = mir and n_opt == 0 and os.environ.get("JSLP_TREE_MIR", "0") == "1"
    if evaluate_batch is None and tableau.width * tableau.height0 > 1536 * 1024:
        speculate = 1  # one workgroup per node only pays for small tableaus; big ones go node by node through the chip-wide kernels
    cache = {}          # heap sequence number -> _NodeEval
    # (JSLP_TREE_COMPACT=0: whole columns per speculated node, as before round 5)
    # (the engine takes at most row_capacity watched variables -- a model with more integers than rows + cut capacity keeps the
    #  whole-column read-back instead of failing on its first speculative batch)
    if read_back is None:
        read_back = "branch" if os.environ.get("JSLP_TREE_BRANCH", "0") == "1" else "compact"
    if read_back not in ("full", "compact", "branch"):
        raise ValueError("branch_and_cut: read_back must be 'full', 'compact' or 'branch'")
    compact_ok = (evaluate_batch is None and read_back != "full" and os.environ.get("JSLP_TREE_COMPACT", "1") != "0"
                  and not mir and hasattr(tableau, "applyCutsBatchWatched") and 0 < len(model.integer_index_array) <= getattr(tableau, "row_capacity", 0))
    branch_ok = compact_ok and read_back == "branch"
    watched_set = []
    watched_before = list(getattr(tableau, "watched", []) or [])  # the caller's own registration, put back when the tree is done
    saved = False
    last_cuts = None    # cuts of the node the sequential run evaluated last
    speculated = 0

    def run_batch(cut_lists):
        # (wall time of the evaluation share of the tree -- the engine calls, and for a sharded tree the exchange step --, so that
        #  a strong-scaling run can be read: bench.py's `tree.eval_ms` / `tree.host_ms`)
        t0 = time.perf_counter()
        try:
            if evaluate_batch is not None:
                return evaluate_batch(cut_lists)
            if mir:
                results, outcomes, rhs, vibr = tableau.applyCutsBatchMIR(cut_lists, check_cycles=check)
                return [_NodeEvalMIR(results[i], outcomes[i].copy(), rhs[i, :results[i].height].copy(), vibr[i, :results[i].height].copy())
                        for i in range(len(cut_lists))]
            if compact_ok:
                # the compact read-back (jslp_engine_relax_batch_watched): per node the integer variables' rows and values -- what the loop
                # below reads (mip-utils.ts:43-61, 100-126) -- instead of whole RHS columns + row maps; the leaf the tree commits to is
                # evaluated once more with the full read-back at the end (tableau.applyCuts(best_cuts))
                if not watched_set:
                    tableau.set_watched_variables(model.integer_index_array)
                    watched_set.append(True)
                if branch_ok:  # the branching decision itself, made on the device (include/jslpx_branch.h)
                    results, recs = tableau.applyCutsBatchBranch(cut_lists, check_cycles=check)
                    return [_NodeEvalBranch(results[i], recs[i]) for i in range(len(cut_lists))]
                results, wrows, wvals = tableau.applyCutsBatchWatched(cut_lists, check_cycles=check)
                return [_NodeEvalWatched(results[i], wrows[i].copy(), wvals[i].copy()) for i in range(len(cut_lists))]
            results, rhs, vibr = tableau.applyCutsBatch(cut_lists, check_cycles=check)
            return [_NodeEval(results[i], rhs[i, :results[i].height].copy(), vibr[i, :results[i].height].copy())
                    for i in range(len(cut_lists))]
        finally:
            EVAL_STATS["seconds"] += time.perf_counter() - t0
            EVAL_STATS["batches"] += 1
            EVAL_STATS["nodes"] += len(cut_lists)

    def report(threshold):
        if tolerance_out is not None and tolerance > 0:
            stopped = not tolerance_flag and len(branches) > 0
            tolerance_out.update(best_possible=float(tableau.bestPossibleEval), threshold=float(threshold), stopped=int(stopped),
                                 left=len(branches) if stopped else 0)

    acceptable = 0.0
    branches.push(-math.inf, [])
    while len(branches) > 0 and tolerance_flag and time.time() * 1000.0 < terminal_time:
        if model.isMinimization:
            acceptable = tableau.bestPossibleEval * (1 + tolerance)
        else:
            acceptable = tableau.bestPossibleEval * (1 - tolerance)
        if tolerance > 0 and best_evaluation < acceptable:
            tolerance_flag = False
            if not _late_stop:
                break
        relaxed, seq, cuts = branches.pop()
        if relaxed > best_evaluation:
            continue
        if max_nodes is not None and iterations >= max_nodes:
            raise TreeCapacity("max_nodes")
        if speculate > 1 and saved:
            if seq not in cache:
                # this node + the entries the heap would hand out next (best first, LIFO ties); nodes already
                # prunable by the current incumbent are not worth speculating on
                ahead = sorted(branches.heap, key=lambda e: (e[0], -e[1]))
                batch = [(seq, cuts)] + [(e[1], e[2]) for e in ahead if e[1] not in cache and e[0] <= best_evaluation][:speculate - 1]
                for (sq, _), ev in zip(batch, run_batch([c for _, c in batch])):
                    cache[sq] = ev
                speculated += len(batch)
            ev = cache.pop(seq)
            if isinstance(ev, _NodeEvalMIR):
                tableau._absorb_mir(ev.res, ev.outcome)
            else:
                tableau._absorb(ev.res)
            if isinstance(ev, _NodeEvalBranch):
                rhs, vibr = None, ev
            elif isinstance(ev, _NodeEvalWatched):
                rhs, vibr = None, _WatchedRows(ev.wrows, ev.wvals)
            else:
                rhs, vibr = ev.rhs, ev.vibr
        elif mir_one_call and saved:
            _res, _outcome, rhs, vibr = tableau.applyCutsMIR(cuts, check_cycles=check)  # :33-52 in one engine call
        else:
            _res, rhs, vibr = tableau.applyCuts(cuts, check_cycles=check)
            rhs, vibr = mir_loop(tableau, model, rhs, vibr, check)  # :38-52
        last_cuts = cuts
        iterations += 1
        if not tableau.feasible:
            continue
        evaluation = tableau.evaluation
        if evaluation > best_evaluation:
            continue
        optional_cells = None
        if evaluation == best_evaluation:  # :107-127: ties are broken on the optional objectives, in priority order
            worse = True
            if n_opt > 0:
                optional_cells = tableau.optional_objectives()[:, 0]
                for o in range(n_opt):
                    if optional_cells[o] > best_optional[o]:
                        break
                    if optional_cells[o] < best_optional[o]:
                        worse = False
                        break
            if n_opt > 0:
                TIE_STATS["ties"] += 1
                TIE_STATS["won"] += 0 if worse else 1
            if worse:
                continue
        rows = vibr if isinstance(vibr, (_WatchedRows, _NodeEvalBranch)) else _rows_by_var(vibr)
        if is_integral(model, rhs, rows, precision):
            found_integral = True
            if iterations == 1:
                report(acceptable)
                return iterations, True
            best_cuts = cuts
            best_evaluation = evaluation
            if n_opt > 0:
                if optional_cells is None:
                    optional_cells = tableau.optional_objectives()[:, 0]
                best_optional = [float(x) for x in optional_cells]
        else:
            if iterations == 1:
                tableau.save()
                saved = True
            var_index, var_value = most_fractional_var(model, rhs, rows)
            cuts_high, cuts_low = [], []
            for cut in cuts:
                if cut["varIndex"] == var_index:
                    if cut["type"] == "min":
                        cuts_low.append(cut)
                    else:
                        cuts_high.append(cut)
                else:
                    cuts_high.append(cut)
                    cuts_low.append(cut)
            cuts_high.append({"type": "min", "varIndex": var_index, "value": float(math.ceil(var_value))})
            cuts_low.append({"type": "max", "varIndex": var_index, "value": float(math.floor(var_value))})
            branches.push(evaluation, cuts_high)
            branches.push(evaluation, cuts_low)
    report(acceptable)
    if best_cuts is not None:
        _res, rhs, vibr = tableau.applyCuts(best_cuts, check_cycles=check)
        mir_loop(tableau, model, rhs, vibr, check)
    elif speculate > 1 and saved and last_cuts is not None:
        # no incumbent: the reference's tableau is left on the node it evaluated last, MIR rows included; put ours there too
        _res, rhs, vibr = tableau.applyCuts(last_cuts, check_cycles=check)
        mir_loop(tableau, model, rhs, vibr, check)
    if watched_set and watched_before != list(model.integer_index_array):
        tableau.set_watched_variables(watched_before)  # (the caller's registration was borrowed for the compact read-back)
    tableau.speculated_nodes = speculated
    if tolerance_out:  # (the final re-evaluation is a simplex like any other: tableau.ts:420-430)
        tolerance_out["best_possible"] = float(tableau.bestPossibleEval)
    return iterations, found_integral
