"""Subprocess body of tests/test_mir_one_call_gpu.py::test_one_launch (the node-path knobs are latched per process): Monster_II's recorded
nodes through jslpr_engine_relax_mir as 1, 16 and 302 nodes, each call behind a marker line on stderr so that the parent can count the
JSLP_DEBUG_LAUNCH lines of that call alone; every outcome is checked against the oracle library here as well (with JSLP_GROUP_MAX the
302 nodes take the queue kernel, which no other test reaches)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jslpsolver_amd import _capi  # noqa: E402
import test_mir_one_call as T  # noqa: E402


def mark(text):
    os.write(2, ("### %s\n" % text).encode())


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    oracle = _capi.Library(os.path.join(root, "oracle", "libjslp_oracle.so"))
    hip = _capi.load_hip()
    tab, nodes = T.load_nodes("Monster_II")
    _root_eval, ex = T.expectations(oracle, tab, nodes, -1, False)
    t = T.root_tableau(hip, tab, nodes)
    t.applyCutsBatch(nodes * 2)  # every slot a later call uses is in sync with the saved root from here on
    prev = t.applyCutsBatch([nodes[0]])[0][0].evaluation  # (the engine's evaluation: the last node's)
    mark("mir call 1")
    got = t.applyCutsMIR(nodes[5])
    mark("end")
    T.same_node(got, ex[5], prev)
    prev = got[0].evaluation
    for idx in (list(range(16)), list(range(len(nodes))) * 2):
        mark("mir call %d" % len(idx))
        results, ocs, rhs, vibr = t.applyCutsBatchMIR([nodes[i] for i in idx])
        mark("end")
        for k, i in enumerate(idx):
            T.same_node((results[k], ocs[k], rhs[k], vibr[k]), ex[i], prev)
        prev = results[-1].evaluation
    t.close()


if __name__ == "__main__":
    main()
