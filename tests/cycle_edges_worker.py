"""Subprocess body of tests/test_cycle_edges.py::test_node_and_batch_kernels_across_the_128_boundary (JSLP_WG_BATCH_THREADS and
JSLP_GROUP_MAX are read once per process): the 128-boundary instances as NODES of their own unsolved root -- save() right after the
upload, then batches of EMPTY cut lists, so that every node is restore + simplex of the root and the node kernels run the history of the
plain solve -- and side by side through simplex_many.  Every node and every LP against the reference's golden of the instance; the
kernels that ran are read from the JSLP_DEBUG_LAUNCH lines (stderr goes to the file argv[2]) and compared with what the mode (argv[1]) must reach:
  nodes        default knobs: 1, 8 and 300 nodes, each call twice -- the first goes through the eager sequence (k_simplex_lds<1024> / <512>:
               the slots are not in sync with the snapshot yet), the second through k_node_lds<1024> (one node, small batch) / <512>
  queue        JSLP_GROUP_MAX=100: 300 nodes on 100 slots, the second call through k_node_queue<512>
  threads1024  JSLP_WG_BATCH_THREADS=1024: batches through the eager sequence with k_simplex_lds<1024>, k_simplex_lds_many<1024>
  threads256   JSLP_WG_BATCH_THREADS=256: there is no LDS build for 256 threads -- the generic k_simplex_wg<256,1024> (one global
               history, jslp_core.inc.h); k_simplex_lds_many stays at 512
A batch larger than a group reports a hit without its [start, length] (the slots' histories are reused): the pivot counts pin the stop."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cycle_edges as E  # noqa: E402
import golden_util as G  # noqa: E402
from jslpsolver_amd import _capi  # noqa: E402
from jslpsolver_amd.engine import Tableau, pivot_digest, simplex_many  # noqa: E402

MODE = sys.argv[1]
NAMES = ("deg_35358_k84", "deg_35358_k85", "deg_35358_k86", "deg_35358_k87", "unr_3_k123", "unr_3_k124")
SIZES = {"nodes": (1, 8, 300), "queue": (300,), "threads1024": (1, 8, 40), "threads256": (1, 8, 40)}[MODE]
MUST = {"nodes": {"k_simplex_lds<1024", "k_simplex_lds<512", "k_node_lds<1024", "k_node_lds<512"},
        "queue": {"k_simplex_lds<512", "k_node_queue<512"},
        "threads1024": {"k_simplex_lds<1024", "k_simplex_lds_many<1024"},
        "threads256": {"k_simplex_lds<1024", "k_simplex_wg<256", "k_simplex_lds_many<512"}}[MODE]
MUST_NOT = {"nodes": {"k_node_queue<512"}, "queue": set(),
            "threads1024": {"k_simplex_lds<512", "k_node_lds<512", "k_node_queue<512", "k_simplex_wg<256"},
            "threads256": {"k_simplex_lds<512", "k_node_lds<512", "k_node_queue<512"}}[MODE]
KERNEL = re.compile(r"^\[jslp\] launch (?:restore\+add_cuts\+simplex\+gather )?(k_\w+<\d+)", re.M)

lib = _capi.load_hip()
seen = set()


# this process's stderr (the engine's fprintf included) goes to a file, as in node_edges_worker.py
_err_out = open(sys.argv[2], "wb")
os.dup2(_err_out.fileno(), 2)
_err_in = open(sys.argv[2], "rb")


def launched():
    """the kernels named on stderr since the last look"""
    sys.stderr.flush()
    return set(KERNEL.findall(_err_in.read().decode(errors="replace")))


for name in NAMES:
    inst = E.BY_NAME[name]
    g = G.load(os.path.join(E.EDGES, "%s.json.gz" % name))
    call = g["simplexCalls"][0]
    start, length = int(g["messages"][1].split(":")[1]), int(g["messages"][2].split(":")[1])
    t = Tableau(*E.build(inst), lib=lib)
    t.save()
    for n in SIZES:
        for rep in range(2):
            launched()
            res, rhs, rows = t.applyCutsBatch([[] for _ in range(n)], check_cycles=True)
            kernels = launched()
            seen |= kernels
            assert kernels, (name, n, rep)
            for i, r in enumerate(res):
                assert (bool(r.feasible), bool(r.bounded), bool(r.optimal), r.height, r.cycle_phase) == (False, True, False, g["tableau"]["height"], 2), (name, n, rep, i)
                assert (r.pivots_phase1, r.pivots_phase2) == (call["p1"], call["p2"]), (name, n, rep, i, r.pivots_phase2)
                assert (r.cycle_start, r.cycle_length) in ((start, length), (0, 0)), (name, n, rep, i, r.cycle_start, r.cycle_length)
                if n <= 8:
                    assert (r.cycle_start, r.cycle_length) == (start, length), (name, n, rep, i)
                assert G.sha_rhs(rhs[i, :r.height], rows[i, :r.height]) == call["rhsSha"], (name, n, rep, i)
    t.close()

# the same instances side by side in one simplex_many launch
ts = [Tableau(*E.build(E.BY_NAME[n]), lib=lib) for n in NAMES]
launched()
out = simplex_many(ts, check_cycles=True)
seen |= launched()
for name, t, r in zip(NAMES, ts, out):
    g = G.load(os.path.join(E.EDGES, "%s.json.gz" % name))
    call = g["simplexCalls"][0]
    assert ["Cycle in phase %d" % r.cycle_phase, "Start :%d" % r.cycle_start, "Length :%d" % r.cycle_length] == g["messages"], name
    assert (r.pivots_phase1, r.pivots_phase2) == (call["p1"], call["p2"]), name
    trace = t.pivot_trace()
    assert len(trace) == g["nPivots"] and pivot_digest(trace) == g["pivotDigest"], name
    assert G.sha_matrix(t.download()[0]) == g["final"]["matrixSha"], name
    t.close()

print("kernels", sorted(seen))
assert MUST <= seen and not (MUST_NOT & seen), (sorted(MUST - seen), sorted(MUST_NOT & seen))
print("ok")
