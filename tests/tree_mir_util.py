"""Shared by tests/test_tree_mir_cpu.py and tests/test_tree_mir_gpu.py: the LPs of a pack whose trees run their MIR-cut loop in the kernel
(include/jslpc_tree_mir.h), the reference's recorded MIR runs they are held against, and the state a solved pack leaves, as bytes."""
import copy
import gzip
import json
import os

import golden_util as G
import tree_pack_util as U
from jslpsolver_amd.engine import TableauPack, tree_mir_rows

MIR_OPTIONS = {"useMIRCuts": True}


class MirItem(U.Item):
    """a model as a MIR LP of a pack: solve_packed's row_extra and cut_rows unless given"""

    def __init__(self, model_json, row_extra=None, cut_rows=None):
        U.Item.__init__(self, model_json, cut_rows=0)
        h, w = self.lp[0].shape
        extra, cuts = tree_mir_rows(h, w, len(self.integers))
        self.cut_rows = cuts if cut_rows is None else cut_rows
        self.row_extra = extra if row_extra is None else row_extra
        self.mir = True


class RawMirItem(U.RawItem):
    """a tableau with some variables declared integer, as a MIR LP"""

    def __init__(self, lp, integers, row_extra=None, cut_rows=None, precision=1e-8, check=True):
        U.RawItem.__init__(self, lp, integers, cut_rows=cut_rows, precision=precision, check=check)
        h, w = lp[0].shape
        extra, cuts = tree_mir_rows(h, w, len(self.integers), cut_rows=self.cut_rows)
        self.row_extra = extra if row_extra is None else row_extra
        self.cut_rows = min(cuts, self.row_extra)
        self.mir = True


def dense_mir_item(h, w, k, seed, row_extra=None):
    """tree_pack_util.dense_item as a MIR LP"""
    it = U.dense_item(h, w, k, seed)
    return RawMirItem(it.lp, it.integers, row_extra=row_extra)


def is_mir(item):
    return bool(getattr(item, "mir", False))


def make_pack(lib, items, trace_cap=8192, heap_cap=256, max_nodes=0, max_pivots=0):
    """MIR LPs and plain tree LPs in one pack"""
    return TableauPack([it.lp for it in items], precision=[it.precision for it in items], lib=lib, trace_cap=trace_cap, max_pivots=max_pivots,
                       integers=[it.integers for it in items], cut_rows=[it.cut_rows for it in items], heap_cap=heap_cap, max_nodes=max_nodes,
                       mir=[is_mir(it) for it in items], row_extra=[it.row_extra if is_mir(it) else -1 for it in items])


def solve(lib, items, **kw):
    pack = make_pack(lib, items, **kw)
    pack.branch_and_cut(check_cycles=[it.check for it in items])
    return pack


def state(pack, i):
    """tree_pack_util.state with the MIR counters"""
    return dict(U.state(pack, i), mir=pack.mir[i].tobytes())


def states(pack):
    return [state(pack, i) for i in range(len(pack))]


def fuzz_mir_cases():
    """the reference's recorded runs with options exactly {"useMIRCuts": true} under the default service that need no presolve pre-pass"""
    return [c for c in U._cases("fuzz_services.jsonl.gz") if c["model"].get("options") == MIR_OPTIONS and c["fixed"] == 0 and not c["infeasPre"]]


def fixture_mir_records():
    """(name, model with the option set, the reference's record) of the ten TREE_FIXTURES in tests/golden/mir.json.gz"""
    with gzip.open(os.path.join(G.GOLDEN, "mir.json.gz"), "rt") as fh:
        doc = json.load(fh)
    by_name = {os.path.basename(c["file"])[:-len(".json.gz")]: c for c in doc["cases"] if c["options"] == MIR_OPTIONS}
    out = []
    for name in U.TREE_FIXTURES:
        model = copy.deepcopy(U.fixture(name)["model"])
        model["options"] = dict(MIR_OPTIONS)
        out.append((name, model, by_name[name]))
    return out


def check_fuzz_record(pack, i, item, c):
    U.check_record(pack, i, item, c["nPivots"], c["digest"], c["iter"], c["keys"], c["result"], (c["gen"], c["seed"]))


def check_fixture_record(pack, i, item, name, c):
    assert c["presolveFixed"] == 0, name
    U.check_record(pack, i, item, c["nPivots"], c["pivotDigest"], c["iterations"], c["resultKeys"], c["result"], name)
    assert int(pack.mir[i]["rows_added"]) == c["mirCuts"], name
    assert int(pack.tree[i]["final_height"]) == c["height"], name


def round_log(lib, item):
    """what every MIR round of the item's host tree on `lib` (the oracle) saw before it appended its rows: (height, rows eligible for a
    cut in row order, rows contributing to the fractional volume) -- the conditions of applyMIRCuts (cutting-strategies.ts:82-90) and of
    computeFractionalVolume(true) (mip-utils.ts:67-92) restated on the RHS column and the row map"""
    import numpy as np

    from jslpsolver_amd.engine import Tableau
    log = []
    ints = frozenset(int(v) for v in item.integers)
    orig = Tableau.mirRound

    def spy(self, check_cycles=True):
        rhs, vibr = self.read_rhs()
        p = self.precision
        rows = [r for r in range(1, len(rhs)) if int(vibr[r]) in ints]
        f = {r: rhs[r] - np.floor(rhs[r]) for r in rows}
        eligible = [r for r in rows if not (f[r] < p or f[r] > 1 - p)]
        d = {r: abs(rhs[r]) for r in rows}
        volume = [r for r in rows if not (min(d[r] - np.floor(d[r]), np.floor(d[r] + 1)) < p)]
        log.append((len(rhs), eligible, volume))
        return orig(self, check_cycles=check_cycles)

    Tableau.mirRound = spy
    try:
        solve(lib, [item]).close()
    finally:
        Tableau.mirRound = orig
    return log
