"""Shared by tests/test_tree_enh_cpu.py and tests/test_tree_enh_gpu.py: packs with ENHANCED LPs (include/jslpe_tree_enhanced.h) built from
the items of tests/tree_pack_util.py, the reference's recorded runs under the enhanced service, and the state such a pack leaves, as bytes."""
import gzip
import json
import os

import golden_util as G
import tree_pack_util as U
from jslpsolver_amd.engine import TableauPack
from jslpsolver_amd.model import Model

NODE_SELECTIONS = ("best-first", "depth-first", "hybrid")
BRANCHINGS = ("most-fractional", "pseudocost", "strong")
PAIRS = [(s, b) for s in NODE_SELECTIONS for b in BRANCHINGS]
# the three enhanced policies tests/golden/fuzz_services.jsonl.gz records, as options and as the (node selection, branching) they mean
FUZZ_POLICIES = [({"nodeSelection": "depth-first"}, ("depth-first", "pseudocost")),
                 ({"branching": "strong"}, ("hybrid", "strong")),
                 ({"branching": "most-fractional", "nodeSelection": "best-first"}, ("best-first", "most-fractional"))]


def given(options):
    """(node_selection, branching) as TableauPack takes them: the model's options, None where it has none"""
    return options.get("nodeSelection"), options.get("branching")


def make_pack(lib, items, policies, trace_cap=8192, heap_cap=256, max_nodes=0, max_pivots=0):
    """policies: per item None (the default service) or (node_selection or None, branching or None)"""
    policies = [p if p is not None else (None, None) for p in policies]
    return TableauPack([it.lp for it in items], precision=[it.precision for it in items], lib=lib, trace_cap=trace_cap, max_pivots=max_pivots,
                       integers=[it.integers for it in items], cut_rows=[it.cut_rows for it in items], heap_cap=heap_cap, max_nodes=max_nodes,
                       node_selection=[p[0] for p in policies], branching=[p[1] for p in policies])


def solve(lib, items, policies, **kw):
    pack = make_pack(lib, items, policies, **kw)
    pack.branch_and_cut(check_cycles=[it.check for it in items])
    return pack


def state(pack, i):
    """tree_pack_util.state with the LP's enhanced record"""
    s = U.state(pack, i)
    s["enhanced"] = pack.enhanced[i].tobytes()
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


def fuzz_enhanced_cases():
    """the reference's recorded runs under the ENHANCED service that need no presolve pre-pass: [(case, (node selection, branching))], the
    cases of one policy after those of the one before"""
    with gzip.open(os.path.join(G.GOLDEN, "fuzz_services.jsonl.gz"), "rt") as fh:
        cases = [json.loads(line) for line in fh if line.startswith("{")]
    out = []
    for options, pair in FUZZ_POLICIES:
        out += [(c, pair) for c in cases if c["model"].get("options") == options and c["fixed"] == 0 and not c["infeasPre"]]
    return out


def enhanced_fixture_cases():
    """the records of tests/golden/enhanced.json.gz a pack can replay: no tolerance, no timeout, no variable fixed by the presolve pre-pass"""
    with gzip.open(os.path.join(G.GOLDEN, "enhanced.json.gz"), "rt") as fh:
        cases = json.load(fh)
    return [c for c in cases if "tolerance" not in c["options"] and "timeout" not in c["options"] and c["presolveFixed"] == 0]


def fixture_item(case):
    """the item of an enhanced.json.gz record, as tests/test_incremental_bnb.py::run_case builds its model; None when Model refuses it"""
    from jslpsolver_amd.model import UnsupportedModel
    model = dict(G.load(os.path.join(G.GOLDEN, case["file"]))["model"])
    model["options"] = dict(case["options"])
    try:
        Model(model)
    except UnsupportedModel:
        return None
    return U.Item(model)
