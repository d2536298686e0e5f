"""Every create entry point of the pack (jslpp_ / jslps_ / jslpt_ / jslps_tree_ / jslpc_tree_ / jslpe_tree_ (two) / jslpi_tree_pack_create) refuses
bad arguments before any device call, so this runs without a GPU.  One table of bad inputs is driven through every entry point that can reach
the rule an input breaks; the code and the FULL text of jslp_last_error are compared with tests/golden/pack_create_refusals.json, which was
recorded from the library as it stood before the pack's host path was gathered into one creation request (`python
tests/test_pack_create_refusals.py --record` writes the file from whatever library is built: re-record only to ADD cases, and diff the result).
Inputs that break two rules at once fix the precedence: null arrays against a per-LP rule, incremental against MIR against optional
objectives, the two 64 KiB refusals, an early LP's late rule against a late LP's early rule."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from jslpsolver_amd import _capi  # noqa: E402
from test_many_abi import built  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pack_create_refusals.json")
NAN = float("nan")

# the arguments of every entry point between (out, device, n) and (trace_cap, max_pivots[, max_nodes]), in its own order
SHAPE = ("heights", "widths", "precision")
TREE = SHAPE + ("cut_rows", "heap_cap")
ENTRIES = {
    "jslpp_pack_create": SHAPE,
    "jslps_pack_create": SHAPE + ("n_optional",),
    "jslpt_pack_create": TREE,
    "jslps_tree_pack_create": TREE + ("n_optional",),
    "jslpc_tree_pack_create": TREE + ("row_extra",),
    "jslpe_tree_pack_create": TREE + ("node_selection", "branching"),
    "jslpe_tree_pack_create_mixed": TREE + ("n_optional", "row_extra", "node_selection", "branching"),
    "jslpi_tree_pack_create": TREE + ("n_optional", "row_extra", "node_selection", "branching", "incremental", "max_checkpoints"),
}
ALL = tuple(ENTRIES)
WITH_TREES = tuple(e for e in ALL if "cut_rows" in ENTRIES[e])
WITH_OPTIONAL = tuple(e for e in ALL if "n_optional" in ENTRIES[e])
WITH_ROW_EXTRA = tuple(e for e in ALL if "row_extra" in ENTRIES[e])
WITH_POLICY = tuple(e for e in ALL if "branching" in ENTRIES[e])
MIXED = ("jslpe_tree_pack_create_mixed", "jslpi_tree_pack_create")
INC = ("jslpi_tree_pack_create",)
# two LPs, both fine: 3 x 4, two cut rows, a heap of four; what an entry point does not take it does not see
FINE = dict(out=True, n=2, heights=[3, 3], widths=[4, 4], precision=[1e-8, 1e-8], cut_rows=[2, 2], heap_cap=[4, 4], n_optional=None, row_extra=None,
            node_selection=[0, 0], branching=[0, 0], incremental=[0, 0], max_checkpoints=[0, 0], trace_cap=0, max_pivots=0, max_nodes=0)
KNAP = dict(heights=[3, 52], widths=[4, 51])  # Knapsack_1's 52 x 51 holds 96 rows beyond its own as a tree LP, 95 as a MIR LP (test_the_limits_the_table_leans_on)
INC1 = dict(incremental=[0, 1], max_checkpoints=[0, 50], row_extra=[-1, 5])  # LP 1 a well-formed incremental LP

# (name, the entry points that can reach the rule, what differs from FINE)
CASES = [
    # ---- one fault: null tables and scalars
    ("null out", ALL, dict(out=False)),
    ("negative n", ALL, dict(n=-1)),
    ("null heights", ALL, dict(heights=None)),
    ("null widths", ALL, dict(widths=None)),
    ("null precision", ALL, dict(precision=None)),
    ("null cut_rows", WITH_TREES, dict(cut_rows=None)),
    ("null heap_cap", WITH_TREES, dict(heap_cap=None)),
    ("null row_extra", ("jslpc_tree_pack_create",), dict(row_extra=None)),
    ("null node_selection", WITH_POLICY, dict(node_selection=None)),
    ("null branching", WITH_POLICY, dict(branching=None)),
    ("null incremental", INC, dict(incremental=None)),
    ("null max_checkpoints", INC, dict(max_checkpoints=None)),
    ("negative trace_cap", ALL, dict(trace_cap=-1)),
    ("negative max_pivots", ALL, dict(max_pivots=-1)),
    ("negative max_nodes", WITH_TREES, dict(max_nodes=-1)),
    # ---- one fault: the per-LP rules, in LP 1
    ("one row", ALL, dict(heights=[3, 1])),
    ("one column", ALL, dict(widths=[4, 1])),
    ("precision nan", ALL, dict(precision=[1e-8, NAN])),
    ("negative cut_rows", WITH_TREES, dict(cut_rows=[2, -1])),
    ("heap_cap 0", WITH_TREES, dict(heap_cap=[4, 0])),
    ("heap_cap above 2^24", WITH_TREES, dict(heap_cap=[4, (1 << 24) + 1])),
    ("negative n_optional", WITH_OPTIONAL, dict(n_optional=[0, -1])),
    ("mir row_extra below cut_rows", WITH_ROW_EXTRA, dict(row_extra=[-1, 1])),
    ("node_selection 4", WITH_POLICY, dict(node_selection=[0, 4])),
    ("node_selection -1", WITH_POLICY, dict(node_selection=[0, -1])),
    ("branching 4", WITH_POLICY, dict(branching=[0, 4])),
    ("branching -1", WITH_POLICY, dict(branching=[0, -1])),
    ("enhanced with mir", MIXED, dict(node_selection=[0, 2], row_extra=[-1, 5])),
    ("enhanced by branching with optional", MIXED, dict(branching=[0, 1], n_optional=[0, 1])),
    ("mir with optional", MIXED, dict(row_extra=[-1, 5], n_optional=[0, 1])),
    ("incremental 2", INC, dict(INC1, incremental=[0, 2])),
    ("incremental -1", INC, dict(INC1, incremental=[0, -1])),
    ("max_checkpoints 65", INC, dict(INC1, max_checkpoints=[0, 65])),
    ("max_checkpoints -1", INC, dict(INC1, max_checkpoints=[0, -1])),
    ("incremental without row_extra", INC, dict(INC1, row_extra=None)),
    ("incremental row_extra below cut_rows", INC, dict(INC1, row_extra=[-1, 1])),
    ("incremental row_extra negative", INC, dict(INC1, row_extra=[-1, -1])),
    ("incremental with optional", INC, dict(INC1, n_optional=[0, 1])),
    # ---- one fault: the 64 KiB refusals
    ("lds plain", ("jslpp_pack_create", "jslps_pack_create"), dict(heights=[3, 200], widths=[4, 200])),
    ("lds with optional rows", ("jslps_pack_create",), dict(heights=[3, 86], widths=[4, 86], n_optional=[0, 3])),
    ("lds tree", WITH_TREES, dict(KNAP, cut_rows=[2, 97])),
    ("lds tree with optional rows", ("jslps_tree_pack_create",) + MIXED, dict(KNAP, cut_rows=[2, 96], n_optional=[0, 1])),
    ("lds mir", WITH_ROW_EXTRA, dict(KNAP, row_extra=[-1, 96])),
    ("lds incremental", INC, dict(KNAP, **dict(INC1, row_extra=[-1, 97]))),
    ("absurd shape", ALL, dict(heights=[3, 2 ** 30], widths=[4, 2 ** 30])),
    ("absurd mir", WITH_ROW_EXTRA, dict(row_extra=[-1, 2 ** 30], widths=[4, 2 ** 30])),
    # ---- two faults: a null table against a per-LP rule, a scalar against a per-LP rule
    ("null heights, one column", ALL, dict(heights=None, widths=[4, 1])),
    ("null heap_cap, one row", WITH_TREES, dict(heap_cap=None, heights=[1, 3])),
    ("null out, negative trace_cap", ALL, dict(out=False, trace_cap=-1)),
    ("negative trace_cap, one row", ALL, dict(trace_cap=-1, heights=[1, 3])),
    ("null branching, node_selection 4", WITH_POLICY, dict(branching=None, node_selection=[0, 4])),
    ("null max_checkpoints, incremental 2", INC, dict(INC1, max_checkpoints=None, incremental=[0, 2])),
    ("null out, mir with optional", MIXED, dict(out=False, row_extra=[-1, 5], n_optional=[0, 1])),
    ("null heights, mir with optional", MIXED, dict(heights=None, row_extra=[-1, 5], n_optional=[0, 1])),
    ("negative trace_cap, mir with optional", MIXED, dict(trace_cap=-1, row_extra=[-1, 5], n_optional=[0, 1])),
    ("null node_selection, mir with optional", MIXED, dict(node_selection=None, row_extra=[-1, 5], n_optional=[0, 1])),
    # ---- two faults in one LP: the order of the rules
    ("one row, precision nan", ALL, dict(heights=[3, 1], precision=[1e-8, NAN])),
    ("precision nan, negative cut_rows", WITH_TREES, dict(precision=[1e-8, NAN], cut_rows=[2, -1])),
    ("heap_cap 0, negative n_optional", ("jslps_tree_pack_create",) + MIXED, dict(heap_cap=[4, 0], n_optional=[0, -1])),
    ("negative n_optional, incremental 2", INC, dict(INC1, n_optional=[0, -1], incremental=[0, 2])),
    ("negative n_optional, node_selection 4", MIXED, dict(n_optional=[0, -1], node_selection=[0, 4])),
    ("max_checkpoints 65, incremental row_extra below cut_rows", INC, dict(INC1, max_checkpoints=[0, 65], row_extra=[-1, 1])),
    ("incremental row_extra below cut_rows, with optional", INC, dict(INC1, row_extra=[-1, 1], n_optional=[0, 1])),
    ("incremental with optional, branching 4", INC, dict(INC1, n_optional=[0, 1], branching=[0, 4])),
    ("incremental with optional and node_selection", INC, dict(INC1, n_optional=[0, 1], node_selection=[0, 2])),
    ("node_selection 4, branching 4", WITH_POLICY, dict(node_selection=[0, 4], branching=[0, 4])),
    ("enhanced with mir whose row_extra is below cut_rows", MIXED, dict(branching=[0, 3], row_extra=[-1, 1])),
    ("enhanced with mir and optional", MIXED, dict(node_selection=[0, 1], row_extra=[-1, 5], n_optional=[0, 1])),
    ("mir row_extra below cut_rows, too tall", WITH_ROW_EXTRA, dict(KNAP, cut_rows=[2, 200], row_extra=[-1, 199])),
    ("negative cut_rows, too tall", WITH_TREES, dict(heights=[3, 200], widths=[4, 200], cut_rows=[2, -1])),
    # ---- two faults in two LPs: the first LP's wins whatever its rule, except that `a MIR LP has no optional objectives` is looked for first
    ("LP 0 too tall, LP 1 one row", ALL, dict(heights=[200, 1], widths=[200, 4])),
    ("LP 0 incremental with optional, LP 1 mir with optional", INC, dict(incremental=[1, 0], max_checkpoints=[50, 0], row_extra=[5, 5], n_optional=[1, 1])),
    ("LP 0 enhanced with optional, LP 1 mir with optional", MIXED, dict(node_selection=[1, 0], row_extra=[-1, 5], n_optional=[1, 1])),
    ("LP 0 one row, LP 1 mir with optional", MIXED, dict(heights=[1, 3], row_extra=[-1, 5], n_optional=[0, 1])),
    # ---- the two 64 KiB refusals side by side
    ("mir fits as a tree LP only", WITH_ROW_EXTRA, dict(KNAP, cut_rows=[2, 96], row_extra=[-1, 96])),
    ("LP 0 mir too tall, LP 1 incremental too tall", INC, dict(heights=[52, 52], widths=[51, 51], incremental=[0, 1], max_checkpoints=[0, 50], row_extra=[97, 97])),
    ("LP 0 incremental too tall, LP 1 mir too tall", INC, dict(heights=[52, 52], widths=[51, 51], incremental=[1, 0], max_checkpoints=[50, 0], row_extra=[97, 97])),
    ("LP 0 tree too tall, LP 1 mir too tall", ("jslpe_tree_pack_create_mixed", "jslpi_tree_pack_create", "jslpc_tree_pack_create"),
     dict(heights=[52, 52], widths=[51, 51], cut_rows=[97, 2], row_extra=[-1, 97])),
]


@pytest.fixture(scope="module")
def lib():
    return _capi.Library(built(_capi.HIP_LIB_PATH))


def create(lib, entry, **changes):
    """(code, whether a handle came back, jslp_last_error) of one create call"""
    kw = dict(FINE, **changes)
    if entry == "jslpc_tree_pack_create" and "row_extra" not in changes:
        kw["row_extra"] = [-1, -1]  # (its row_extra is no optional table: two plain tree LPs)
    h = ctypes.c_void_p()
    keep = []  # (the arrays outlive the call)

    def table(name):
        v = kw[name]
        if v is None:
            return None
        keep.append(_capi.as_f64(v) if name == "precision" else _capi.as_i32(v))
        return _capi.ptr_f64(keep[-1]) if name == "precision" else _capi.ptr_i32(keep[-1])

    args = [ctypes.byref(h) if kw["out"] else None, 0, kw["n"]] + [table(name) for name in ENTRIES[entry]] + [kw["trace_cap"], kw["max_pivots"]]
    if entry in WITH_TREES:
        args.append(kw["max_nodes"])
    rc = getattr(lib, entry)(*args)
    return rc, bool(h.value), lib.jslp_last_error().decode()


def runs():
    return [(name, entry, changes) for name, entries, changes in CASES for entry in entries]


def test_the_table_is_well_formed():
    names = [name for name, _, _ in CASES]
    assert len(set(names)) == len(names)
    for name, entries, changes in CASES:
        assert entries and set(entries) <= set(ALL) and set(changes) <= set(FINE), name
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert sorted(golden) == sorted("%s: %s" % (entry, name) for name, entry, _ in runs())
    # every rule's text is pinned through every entry point that can reach it
    for word, entries in (("bad arguments", ALL), ("negative trace_cap", ALL), ("at least 2 rows", ALL), ("not a number", ALL), ("jslpp_lds_bytes", ALL[:2]),
                          ("jslpt_lds_bytes", WITH_TREES), ("heap_cap between", WITH_TREES), ("n_optional is at least 0", WITH_OPTIONAL),
                          ("row_extra of a MIR LP", WITH_ROW_EXTRA), ("jslpc_tree_lds_bytes", WITH_ROW_EXTRA), ("node_selection is 0", WITH_POLICY),
                          ("branching is 0", WITH_POLICY), ("an enhanced LP", MIXED), ("a MIR LP has no optional objectives", MIXED),
                          ("incremental is 0 or 1", INC), ("max_checkpoints of an incremental LP", INC), ("row_extra of an incremental LP", INC),
                          ("an incremental LP has no optional objectives", INC), ("jslpi_tree_lds_bytes", INC)):
        for entry in entries:
            assert any(key.startswith(entry + ":") and word in text for key, (_, text) in golden.items()), (word, entry)


def test_the_limits_the_table_leans_on(lib):
    assert lib.jslpt_lds_bytes(52, 51, 52 + 96) <= 65536 < lib.jslpt_lds_bytes(52, 51, 52 + 97)
    assert lib.jslpc_tree_lds_bytes(52, 51, 52 + 95) <= 65536 < lib.jslpc_tree_lds_bytes(52, 51, 52 + 96)
    assert lib.jslps_tree_lds_bytes(52, 51, 52 + 95, 1) <= 65536 < lib.jslps_tree_lds_bytes(52, 51, 52 + 96, 1)
    assert lib.jslps_lds_bytes(86, 86, 2) <= 65536 < lib.jslps_lds_bytes(86, 86, 3)
    for entry in ALL:  # what every case starts from is no refusal: it reaches the device (none here, or a pack there)
        rc, made, text = create(lib, entry)
        assert rc in (_capi.JSLP_OK, _capi.JSLP_ERR_DEVICE), (entry, text)


@pytest.mark.parametrize("entry", ALL)
def test_refusals_without_a_device(lib, entry):
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    mine = [(name, changes) for name, e, changes in runs() if e == entry]
    assert len(mine) >= 15
    for name, changes in mine:
        code, text = golden["%s: %s" % (entry, name)]
        assert code in (_capi.JSLP_ERR_ARG, _capi.JSLP_ERR_UNSUPPORTED) and text.startswith("pack_create: ")
        assert create(lib, entry, **changes) == (code, False, text), (entry, name)


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    hip = _capi.Library(os.environ.get("JSLP_HIP_LIBRARY") or built(_capi.HIP_LIB_PATH))
    record = {}
    for name, entry, changes in runs():
        rc, made, text = create(hip, entry, **changes)
        assert not made, (entry, name)
        record["%s: %s" % (entry, name)] = [rc, text]
    with open(GOLDEN, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(len(record), "refusals recorded from", hip.path)
