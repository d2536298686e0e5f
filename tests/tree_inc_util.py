"""Shared by tests/test_tree_inc_cpu.py and tests/test_tree_inc_gpu.py: packs with INCREMENTAL LPs (include/jslpi_tree_incremental.h) built
from the items of tests/tree_pack_util.py, the reference's recorded runs under the incremental service, and the state such a pack leaves,
as bytes."""
import collections
import gzip
import json
import os

import golden_util as G
import tree_enh_util as E
import tree_pack_util as U
from jslpsolver_amd.engine import TableauPack, incremental_rows
from jslpsolver_amd.model import Model, UnsupportedModel

# an incremental LP's policy: (node selection or None, branching or None, max_checkpoints).  Beside it a pack takes None (the default
# service) and tree_enh_util's (node selection, branching) pairs (the enhanced service).
Inc = collections.namedtuple("Inc", "node_selection branching max_checkpoints", defaults=(None, None, 50))
FIVE = [Inc(), Inc("depth-first"), Inc("best-first"), Inc(None, "most-fractional"), Inc("depth-first", "most-fractional")]  # incremental.json.gz's pairs


def inc_of(options, max_checkpoints=50):
    return Inc(options.get("nodeSelection"), options.get("branching"), max_checkpoints)


class Item(U.Item):
    """a model as solve_packed(..., incremental=True) gives it to the pack: row_extra = min(2 per integer variable + 256, what fits) and
    cut_rows = min(2 per integer variable, row_extra), or the caller's"""

    def __init__(self, model_json, row_extra=None, cut_rows=None):
        U.Item.__init__(self, model_json, cut_rows=cut_rows)
        h, w = self.lp[0].shape
        extra, cuts = incremental_rows(h, w, len(self.integers))
        self.row_extra = extra if row_extra is None else row_extra
        self.cut_rows = min(cuts, self.row_extra) if cut_rows is None else cut_rows


def make_pack(lib, items, policies, trace_cap=8192, heap_cap=256, max_nodes=0, max_pivots=0):
    """policies: per item None, an enhanced (node_selection, branching) pair, or an Inc.  An item of tree_mir_util (`mir`) is a MIR LP, one of
    soft_pack_util (`optional`) brings its optional objectives."""
    is_inc = [isinstance(p, Inc) for p in policies]
    mir = [bool(getattr(it, "mir", False)) for it in items]
    optional = [getattr(it, "optional", None) for it in items]
    pairs = [(p[0], p[1]) if p is not None else (None, None) for p in policies]
    return TableauPack([it.lp for it in items], precision=[it.precision for it in items], lib=lib, trace_cap=trace_cap, max_pivots=max_pivots,
                       integers=[it.integers for it in items], cut_rows=[it.cut_rows for it in items], heap_cap=heap_cap, max_nodes=max_nodes,
                       node_selection=[p[0] for p in pairs], branching=[p[1] for p in pairs], incremental=is_inc,
                       max_checkpoints=[p.max_checkpoints if f else 0 for p, f in zip(policies, is_inc)],
                       row_extra=[it.row_extra if f or m else -1 for it, f, m in zip(items, is_inc, mir)],
                       optional_objectives=optional if any(o is not None for o in optional) else None, mir=mir if any(mir) else None)


def solve(lib, items, policies, **kw):
    pack = make_pack(lib, items, policies, **kw)
    pack.branch_and_cut(check_cycles=[it.check for it in items])
    return pack


def state(pack, i):
    """tree_enh_util.state with the LP's incremental record"""
    s = E.state(pack, i)
    s["incremental"] = pack.incremental[i].tobytes()
    s["mir"] = pack.mir[i].tobytes()
    return s


def states(pack):
    return [state(pack, i) for i in range(len(pack))]


def against_host(hip_lib, oracle_lib, items, policies, **kw):
    """one pack on the GPU, one call; every LP against the Python host tree on the oracle, everything as bytes"""
    host = solve(oracle_lib, items, policies, **kw)
    pack = solve(hip_lib, items, policies, **kw)
    for i, (a, b) in enumerate(zip(states(pack), states(host))):
        assert a == b, "LP %d (%s) differs from the host tree: %s" % (i, policies[i], [k for k in a if a[k] != b[k]])
    return pack, host


def fuzz_incremental_cases():
    """the reference's recorded runs under the INCREMENTAL service that need no presolve pre-pass: (the plain {"useIncremental": true} runs
    of fuzz_services, the ones of fuzz_soft with integer variables and no soft constraint)"""
    def runs(name):
        with gzip.open(os.path.join(G.GOLDEN, name), "rt") as fh:
            cases = [json.loads(line) for line in fh if line.startswith("{")]
        return [c for c in cases if c["model"].get("options") == {"useIncremental": True} and c["fixed"] == 0 and not c["infeasPre"]]
    soft = []
    for c in runs("fuzz_soft.jsonl.gz"):
        m = Model(c["model"], None)
        _, oo = m.optional_objectives()
        if len(m.integerVariables) > 0 and (oo is None or len(oo) == 0):
            soft.append(c)
    return runs("fuzz_services.jsonl.gz"), soft


def fixture_cases():
    """the records of tests/golden/incremental.json.gz a pack can replay -- no tolerance, no timeout, no variable fixed by the presolve
    pre-pass, a model the Python host takes, integer variables, at least one row of row_extra: [(record, Item)]"""
    with gzip.open(os.path.join(G.GOLDEN, "incremental.json.gz"), "rt") as fh:
        cases = json.load(fh)
    out = []
    for c in cases:
        if "tolerance" in c["options"] or "timeout" in c["options"] or c["presolveFixed"] != 0:
            continue
        model = dict(G.load(os.path.join(G.GOLDEN, c["file"]))["model"])
        model["options"] = dict(c["options"])
        try:
            it = Item(model)
        except UnsupportedModel:
            continue
        _, oo = it.model.optional_objectives()
        if len(it.integers) > 0 and it.row_extra >= 1 and (oo is None or len(oo) == 0):
            out.append((c, it))
    return out
