"""Subprocess body of test_selection_through_the_node_queue (JSLP_GROUP_MAX is read once per process): every planted case of
test_selection_edges saved UNSOLVED and solved as the nodes of applyCutsBatch calls larger than the slots they get (k_node_queue),
against the oracle engine evaluating the same cut lists one at a time: zero-cut nodes, and for the phase-1 leaving-row cases a unit
row cut on a non-basic variable whose RHS ties the planted rows (the appended row is the last one: the first planted row still wins)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jslpsolver_amd import _capi  # noqa: E402
from jslpsolver_amd.engine import Tableau  # noqa: E402
import test_selection_edges as S  # noqa: E402

assert os.environ.get("JSLP_GROUP_MAX") == "4"
TIE_CUT = {"p1_leave_tie": 3.0, "p1_leave_negative_infinity": float("inf")}  # -x_499 <= -value: the RHS of the planted tie
hip = _capi.load_hip()
oracle = _capi.Library(os.path.join(S.ROOT, "oracle", "libjslp_oracle.so"))
for name in S.CASES:
    A, vibr, vibc, unr, _ = S._case(name)
    nodes = [[] for _ in range(6)]
    if name in TIE_CUT:
        cut = {"type": "min", "varIndex": 499, "value": TIE_CUT[name]}
        assert 499 not in vibr.tolist()  # (non-basic: the cut row is the unit row itself)
        nodes += [[cut] for _ in range(3)]
    ts = [Tableau(A, vibr, vibc, unr, precision=S.PREC, lib=lib, row_capacity=S.H + 1) for lib in (oracle, hip)]
    for t in ts:
        t.save()
    ref = []
    for cuts in nodes:
        ts[0].restore()
        r, rhs, rows = ts[0].applyCuts(cuts, check_cycles=True)
        ref.append(S._node_answer(r, rhs[:r.height], rows[:r.height]))
    for call in range(3):  # (the first batch brings the slots in sync through the per-group launches; the queue takes the next ones)
        results, rhs, rows = ts[1].applyCutsBatch(nodes, check_cycles=True)
        for j, r in enumerate(results):
            got = S._node_answer(r, rhs[j, :r.height], rows[j, :r.height])
            assert got == ref[j], (name, call, j, got[:6], ref[j][:6])
    assert ts[1].get_counters()["node_queue_launches"] > 0, name  # (a fresh engine per case: its own count)
    assert ts[1].last_path() == "workgroup", name
    for t in ts:
        t.close()
print("ok")
