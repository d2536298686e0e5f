"""Incremental branch-and-bound: children start from their PARENT's solved tableau instead of the root.

Mirrors the reference's `createIncrementalBranchAndCutService` (src/tableau/incremental-branch-and-cut.ts:130-499),
the service `Solve` picks for `options.useIncremental === true` (src/main.ts:62-72).  What it changes against the
default service is where a node starts: while the tree is walked depth-first every branched node leaves a
checkpoint (:440-445) and its two children are evaluated as restoreCheckpoint + ONE new cut + simplex (:248-253)
instead of restore(root) + the whole cut list (:254-258).  The reference keeps each checkpoint as a host copy of the
matrix (:55-70); here it is a device buffer (jslp_engine_checkpoint_*): a child costs one HBM-to-HBM copy, one
cut row and a handful of repair pivots, all in one engine call, and nothing crosses PCIe but the RHS column.

Host-side policy restated here because it decides which incumbent wins: depth-first stack / best-first heap and
the hybrid switch after the first incumbent (:295-299, 418-428), pseudocost branching with its order-dependent
update from `tableau.evaluation` (:339, 354-365, 172-221), the checkpoint budget (:132, 442).
"""
import math
import os
import time

from .branch_and_cut import BranchMinHeap, TreeCapacity, _rows_by_var, is_integral, js_round, mir_loop


class _Branch:
    """IncrementalBranch (:49-53)"""
    __slots__ = ("relaxed", "cuts", "depth", "checkpoint", "new_cut")

    def __init__(self, relaxed, cuts, depth, checkpoint=None, new_cut=None):
        self.relaxed, self.cuts, self.depth, self.checkpoint, self.new_cut = relaxed, cuts, depth, checkpoint, new_cut


class _PseudoCosts:
    """:138-174"""

    def __init__(self):
        self.data = {}

    def _get(self, var_index):
        d = self.data.get(var_index)
        if d is None:
            d = self.data[var_index] = [0.0, 0, 0.0, 0]  # upSum, upCount, downSum, downCount
        return d

    def update(self, var_index, up, improvement, fraction):
        d = self._get(var_index)
        normalized = improvement / ((1 - fraction) if up else fraction)
        if up:
            d[0] += normalized
            d[1] += 1
        else:
            d[2] += normalized
            d[3] += 1

    def score(self, var_index, fraction):
        d = self._get(var_index)
        up = d[0] / d[1] if d[1] > 0 else 1
        down = d[2] / d[3] if d[3] > 0 else 1
        return max(up * (1 - fraction), 1e-6) * max(down * fraction, 1e-6)


class CountingContainers:
    """The depth-first stack and the min-heap of the enhanced service, counting what a device-side tree has to hold
    (include/jslpe_tree_enhanced.h) and enforcing the same capacities in the kernel's order: per child the cut list first, then the
    entries stack and heap hold TOGETHER (heap_cap); max_nodes before a node more is evaluated.  What branch_and_cut.CountingHeap is
    for the default service.  Under the incremental service it also keeps the tallest tableau a node had and the tallest one a checkpoint
    holds (include/jslpi_tree_incremental.h), as heights."""

    def __init__(self, heap_cap=None, cut_rows=None, max_nodes=None):
        self.heap = BranchMinHeap()
        self.stack = []
        self.heap_cap, self.cut_rows, self.max_nodes = heap_cap, cut_rows, max_nodes
        self.pushes = self.high_water = self.cuts_high_water = 0
        self.solutions_found = self.stack_high_water = self.moved_to_heap = 0
        self.pseudo_updates = self.scored_by_pseudocost = self.dropped_nodes = 0
        self.rows_high_water = self.checkpoint_rows_high_water = 0

    def _admit(self, branch):
        if self.cut_rows is not None and len(branch.cuts) > self.cut_rows:
            raise TreeCapacity("cut_rows")
        if self.heap_cap is not None and len(self.stack) + len(self.heap) >= self.heap_cap:
            raise TreeCapacity("heap_cap")

    def _count(self, branch):
        self.pushes += 1
        self.high_water = max(self.high_water, len(self.stack) + len(self.heap))
        self.stack_high_water = max(self.stack_high_water, len(self.stack))
        self.cuts_high_water = max(self.cuts_high_water, len(branch.cuts))

    def push_stack(self, branch):
        self._admit(branch)
        self.stack.append(branch)
        self._count(branch)

    def push_heap(self, branch):
        self._admit(branch)
        self.heap.push(branch.relaxed, branch)
        self._count(branch)

    def move_to_heap(self):
        """the hybrid switch: the stack's entries, from the top, into the heap (not counted as pushes)"""
        while self.stack:
            b = self.stack.pop()
            self.heap.push(b.relaxed, b)
            self.moved_to_heap += 1

    def record(self):
        """jslpe_tree_result, field for field"""
        return (self.solutions_found, self.stack_high_water, self.moved_to_heap, self.pseudo_updates, self.scored_by_pseudocost,
                self.dropped_nodes)


def _select_branching_variable(model, rhs, rows, precision, branching, pseudo, strong_candidates=5, counters=None):
    """selectBranchingVariable (incremental-branch-and-cut.ts:176-221; enhanced-branch-and-cut.ts:112-196, which adds the
    "strong" rule): (varIndex, value) or None"""
    candidates = []
    for var in model.integerVariables:
        r = rows.get(var["index"], -1)
        if r != -1:
            value = float(rhs[r])
            fraction = abs(value - js_round(value))
            if fraction > precision:
                candidates.append((var["index"], value, fraction))
    if not candidates:
        return None
    if branching == "most-fractional":  # stable sort by descending fraction, first element (:203-206)
        best = candidates[0]
        for c in candidates[1:]:
            if c[2] > best[2]:
                best = c
        return best[0], best[1]
    if branching == "strong":  # enhanced-branch-and-cut.ts:161-193: the 5 most fractional, scored by pseudocosts once both
        # directions of a variable have been seen twice, by fraction * (1 - fraction) until then
        ranked = sorted(candidates, key=lambda c: -c[2])[:strong_candidates]  # stable, like Array.prototype.sort
        best_score, best = -math.inf, ranked[0]
        for c in ranked:
            d = pseudo._get(c[0])
            if counters is not None and d[1] >= 2 and d[3] >= 2:
                counters.scored_by_pseudocost += 1
            score = pseudo.score(c[0], c[2]) if d[1] >= 2 and d[3] >= 2 else c[2] * (1 - c[2])
            if score > best_score:
                best_score, best = score, c
        return best[0], best[1]
    best_score, best = -math.inf, candidates[0]
    for c in candidates:
        score = pseudo.score(c[0], c[2])
        if score > best_score:
            best_score, best = score, c
    return best[0], best[1]


def enhanced_branch_and_cut(tableau, model, node_selection="hybrid", branching="pseudocost", containers=None, tolerance_out=None,
                            _late_stop=True):
    """createEnhancedBranchAndCutService (src/tableau/enhanced-branch-and-cut.ts:58-437), the service `Solve` picks for
    `options.nodeSelection` / `options.branching` (src/main.ts:74-80): the same tree walk as the incremental service
    with every node evaluated from the saved root (no checkpoints) and the "strong" branching rule.
    containers: a CountingContainers to walk the tree with (it instruments the walk and enforces a device-side tree's capacities).
    tolerance_out, _late_stop: as branch_and_cut.branch_and_cut's."""
    return incremental_branch_and_cut(tableau, model, node_selection=node_selection, branching=branching, max_checkpoints=0,
                                      incremental_rules=False, containers=containers, tolerance_out=tolerance_out, _late_stop=_late_stop)


def incremental_branch_and_cut(tableau, model, node_selection="hybrid", branching="pseudocost", max_checkpoints=50,
                               incremental_rules=True, containers=None, tolerance_out=None, _late_stop=True):
    """branchAndCut (:283-495).  Leaves `tableau` holding the incumbent; returns (iterations, found_integral).
    `tableau.checkpoints_used` / `tableau.incremental_nodes` report how many checkpoints were taken and how many
    nodes started from one.  incremental_rules=False: the enhanced service's variant of the two places where the
    services differ (which branching rules exist; both update pseudocosts from the node's last cut).
    containers: a CountingContainers whose stack and heap the walk uses (None: plain ones, nothing counted, no capacity).
    The checkpoints go back to the engine when the walk ends, also when a capacity (TreeCapacity, the engine's row capacity) ends it.
    tolerance_out, _late_stop: as branch_and_cut.branch_and_cut's (left counts stack and heap together)."""
    checkpoints = []
    try:
        return _walk(tableau, model, node_selection, branching, max_checkpoints, incremental_rules, containers, checkpoints, tolerance_out,
                     _late_stop)
    finally:
        for c in checkpoints:
            tableau.releaseCheckpoint(c)


def _walk(tableau, model, node_selection, branching, max_checkpoints, incremental_rules, containers, checkpoints, tolerance_out=None,
          _late_stop=True):
    cc = containers
    heap = cc.heap if cc is not None else BranchMinHeap()     # entries carry the _Branch in the `cuts` position
    stack = cc.stack if cc is not None else []
    iterations = 0
    checkpoint_count = 0
    incremental_nodes = 0
    tolerance = model.tolerance or 0
    tolerance_flag = True
    terminal_time = 1e99
    if model.timeout:
        terminal_time = time.time() * 1000.0 + model.timeout
    best_evaluation = math.inf
    best_branch = None
    found_integral = False
    check = model.checkForCycles
    precision = tableau.precision
    n_opt = getattr(tableau, "n_optional", 0)
    best_optional = [math.inf] * n_opt
    # JSLP_TREE_MIR=1 (read per call): every node after the root is evaluated WITH its MIR loop by one engine call
    mir_one_call = bool(model.useMIRCuts) and n_opt == 0 and os.environ.get("JSLP_TREE_MIR", "0") == "1"
    pseudo = _PseudoCosts()
    solutions_found = 0
    use_depth_first = node_selection in ("depth-first", "hybrid")

    root = _Branch(-math.inf, [], 0)
    if cc is not None:
        (cc.push_stack if use_depth_first else cc.push_heap)(root)
    elif use_depth_first:
        stack.append(root)
    else:
        heap.push(root.relaxed, root)

    def report(threshold):
        if tolerance_out is not None and tolerance > 0:
            stopped = not tolerance_flag and (len(stack) > 0 if use_depth_first else len(heap) > 0)
            tolerance_out.update(best_possible=float(tableau.bestPossibleEval), threshold=float(threshold), stopped=int(stopped),
                                 left=len(stack) + len(heap) if stopped else 0)

    acceptable = 0.0
    while (len(stack) > 0 if use_depth_first else len(heap) > 0) and tolerance_flag and time.time() * 1000.0 < terminal_time:
        if model.isMinimization:
            acceptable = tableau.bestPossibleEval * (1 + tolerance)
        else:
            acceptable = tableau.bestPossibleEval * (1 - tolerance)
        if tolerance > 0 and best_evaluation < acceptable:
            tolerance_flag = False
            if not _late_stop:
                break
        if use_depth_first and stack:
            branch = stack.pop()
        elif len(heap) > 0:
            branch = heap.pop()[2]
        else:
            break
        if branch.relaxed > best_evaluation:
            continue
        if cc is not None and cc.max_nodes is not None and iterations >= cc.max_nodes:
            raise TreeCapacity("max_nodes")
        parent_eval = tableau.evaluation
        # applyIncrementalCuts (:246-259) and the MIR loop (:261-276)
        from_checkpoint = branch.checkpoint is not None and branch.new_cut is not None
        if mir_one_call and iterations > 0:  # both in ONE engine call (Tableau.applyCutsMIR); the root keeps the round-by-round path
            _res, _outcome, rhs, vibr = tableau.applyCutsMIR([branch.new_cut] if from_checkpoint else branch.cuts, max_rounds=3, need_feasible=True,
                                                             checkpoint=branch.checkpoint if from_checkpoint else None, check_cycles=check)
        else:
            if from_checkpoint:
                (res, rhs, vibr), = tableau.applyCutsFrom(branch.checkpoint, [[branch.new_cut]], check_cycles=check)
                tableau.absorb_from(branch.checkpoint, res)
            else:
                _res, rhs, vibr = tableau.applyCuts(branch.cuts, check_cycles=check)
            rhs, vibr = mir_loop(tableau, model, rhs, vibr, check, max_rounds=3, need_feasible=True)
        incremental_nodes += 1 if from_checkpoint else 0
        iterations += 1
        if cc is not None:
            cc.rows_high_water = max(cc.rows_high_water, tableau.last.height)
        if not tableau.feasible:
            continue
        evaluation = tableau.evaluation
        if evaluation > best_evaluation:
            continue
        # :354-365; the enhanced service takes the node's LAST cut instead (enhanced-branch-and-cut.ts:299-311), which also
        # exists for nodes that came through the best-first heap
        observed = branch.new_cut if incremental_rules else (branch.cuts[-1] if branch.cuts else None)
        if observed is not None and parent_eval != 0:
            pseudo.update(observed["varIndex"], observed["type"] == "min", abs(evaluation - parent_eval), 0.5)
            if cc is not None:
                cc.pseudo_updates += 1
        optional_cells = None
        if evaluation == best_evaluation:  # :367-388
            worse = True
            if n_opt > 0:
                optional_cells = tableau.optional_objectives()[:, 0]
                for o in range(n_opt):
                    if optional_cells[o] > best_optional[o]:
                        break
                    if optional_cells[o] < best_optional[o]:
                        worse = False
                        break
            if worse:
                continue
        rows = _rows_by_var(vibr)
        if is_integral(model, rhs, rows, precision):
            found_integral = True
            solutions_found += 1
            if cc is not None:
                cc.solutions_found += 1
            if iterations == 1:
                tableau.checkpoints_used, tableau.incremental_nodes = 0, 0
                report(acceptable)
                return iterations, True
            best_branch = branch
            best_evaluation = evaluation
            if n_opt > 0:
                if optional_cells is None:
                    optional_cells = tableau.optional_objectives()[:, 0]
                best_optional = [float(x) for x in optional_cells]
            if node_selection == "hybrid" and solutions_found >= 1:  # :418-428
                use_depth_first = False
                if cc is not None:
                    cc.move_to_heap()
                while stack:
                    b = stack.pop()
                    heap.push(b.relaxed, b)
        else:
            if iterations == 1:
                tableau.save()
            rule = branching if (not incremental_rules or branching == "most-fractional") else "pseudocost"  # (:203-221)
            sel = _select_branching_variable(model, rhs, rows, precision, rule, pseudo, counters=cc)
            if sel is None:
                if cc is not None:
                    cc.dropped_nodes += 1
                continue
            var_index, var_value = sel
            checkpoint = None
            if use_depth_first and checkpoint_count < max_checkpoints:  # :440-445
                checkpoint = tableau.createCheckpoint()
                checkpoints.append(checkpoint)
                checkpoint_count += 1
                if cc is not None:
                    cc.checkpoint_rows_high_water = max(cc.checkpoint_rows_high_water, tableau.last.height)
            cuts_high, cuts_low = [], []
            for cut in branch.cuts:
                if cut["varIndex"] == var_index:
                    if cut["type"] == "min":
                        cuts_low.append(cut)
                    else:
                        cuts_high.append(cut)
                else:
                    cuts_high.append(cut)
                    cuts_low.append(cut)
            cut_high = {"type": "min", "varIndex": var_index, "value": float(math.ceil(var_value))}
            cut_low = {"type": "max", "varIndex": var_index, "value": float(math.floor(var_value))}
            cuts_high.append(cut_high)
            cuts_low.append(cut_low)
            depth = branch.depth + 1
            if use_depth_first:
                b_low, b_high = _Branch(evaluation, cuts_low, depth, checkpoint, cut_low), _Branch(evaluation, cuts_high, depth, checkpoint, cut_high)
                if cc is not None:
                    cc.push_stack(b_low)
                    cc.push_stack(b_high)
                else:
                    stack.append(b_low)
                    stack.append(b_high)
            else:  # best-first nodes start from the root (:485-488)
                b_high, b_low = _Branch(evaluation, cuts_high, depth), _Branch(evaluation, cuts_low, depth)
                if cc is not None:
                    cc.push_heap(b_high)
                    cc.push_heap(b_low)
                else:
                    heap.push(b_high.relaxed, b_high)
                    heap.push(b_low.relaxed, b_low)
    report(acceptable)
    if best_branch is not None:
        _res, rhs, vibr = tableau.applyCuts(best_branch.cuts, check_cycles=check)  # :491-493, always from the root
        mir_loop(tableau, model, rhs, vibr, check, max_rounds=3, need_feasible=True)  # :228-243
        if cc is not None:
            cc.rows_high_water = max(cc.rows_high_water, tableau.last.height)
    tableau.checkpoints_used, tableau.incremental_nodes = checkpoint_count, incremental_nodes
    if tolerance_out:  # (the final re-evaluation is a simplex like any other: tableau.ts:420-430)
        tolerance_out["best_possible"] = float(tableau.bestPossibleEval)
    return iterations, found_integral
