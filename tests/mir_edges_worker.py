"""Subprocess body of tests/test_mir_edges_gpu.py::test_one_call_paths (the node-path knobs are latched per process): every instance of
tests/mir_edges.py sent through the one-call form of a node's MIR loop in the launch shape this process's environment selects --

    lds1024  (no knob)                   one node (k_node_lds<1024> MIR build, g 1) and a batch of 3 differing nodes (the same build, g 3)
    lds512   (JSLP_SMALL_BATCH_1024=0)   the same batch of 3 through the 512-thread build
    queue    (JSLP_GROUP_MAX=2)          a batch of 5 through k_node_queue<512>'s MIR build: two slots, five nodes, slots reused

-- each call behind a marker line on stderr, so that the parent can tell from the JSLP_DEBUG_LAUNCH lines of that call alone which kernel
ran.  Every outcome is checked here against the oracle library's sequence (tests/test_mir_edges.expectation): result, outcome record with
the volumes as bit patterns, RHS column and row map; for the single node also the live tableau and the pivot trace."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jslpsolver_amd import _capi  # noqa: E402
import mir_edges as E  # noqa: E402
import test_mir_edges as C  # noqa: E402


def mark(text):
    os.write(2, ("### %s\n" % text).encode())


def single_node(hip, oracle, inst, cuts, e):
    """[] or one branching cut through applyCutsMIR; the live tableau and the trace against the same calls on the oracle library"""
    rounds = E.rounds_of(inst)
    outs = []
    for lib in (oracle, hip):
        t, _ = E.root_tableau(lib, inst, E.ONE_CALL_EXTRA_ROWS)
        t.applyCuts([])  # (slot 0 in sync with the saved root: the next node is the one-launch shape)
        prev = t.evaluation
        if lib is hip:
            mark("call single %s %d" % (inst["name"], len(cuts)))
        got = t.applyCutsMIR(cuts, max_rounds=rounds)
        if lib is hip:
            mark("end")
        C.same_node(got, e, prev)
        outs.append((C.final_state(t), t.pivot_trace().tobytes(), t.height, t.feasible, t.simplexIters))
        t.close()
    assert outs[0] == outs[1], inst["name"]


def batch(hip, inst, idx, ex, root_eval):
    rounds = E.rounds_of(inst)
    nodes = E.nodes_of(inst)
    t, _ = E.root_tableau(hip, inst, E.ONE_CALL_EXTRA_ROWS)
    t.applyCutsBatch([nodes[i] for i in idx])  # every slot the call uses is in sync with the saved root from here on
    prev = t.applyCutsBatch([nodes[0]])[0][0].evaluation  # (the engine's evaluation: the last node's)
    for turn in range(2):  # twice: the second call starts from the slots the first one's MIR rows left dirty
        mark("call batch %s %d" % (inst["name"], len(idx)))
        results, ocs, rhs, vibr = t.applyCutsBatchMIR([nodes[i] for i in idx], max_rounds=rounds)
        mark("end")
        for k, i in enumerate(idx):
            C.same_node((results[k], ocs[k], rhs[k], vibr[k]), ex[i], prev)
        prev = results[-1].evaluation
    t.close()


def main(mode):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    oracle = _capi.Library(os.path.join(root, "oracle", "libjslp_oracle.so"))
    hip = _capi.load_hip()
    for name in C.ONE_CALL:
        inst = E.BY_NAME[name]
        _, root_eval, ex = C.expectation(oracle, name)
        if mode == "lds1024":
            nodes = E.nodes_of(inst)
            single_node(hip, oracle, inst, nodes[0], ex[0])
            single_node(hip, oracle, inst, nodes[4], ex[4])
            batch(hip, inst, [0, 2, 4], ex, root_eval)
        elif mode == "lds512":
            batch(hip, inst, [0, 2, 4], ex, root_eval)
        else:
            batch(hip, inst, [0, 1, 2, 3, 4], ex, root_eval)
    mark("done")


if __name__ == "__main__":
    main(sys.argv[1])
