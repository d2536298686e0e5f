"""The MIR row builders and the volume rule at their edges, on the GPU: every instance of tests/mir_edges.py through
every path that builds rows or volumes --

    applyMIRCuts() alone          k_mir_cuts; the rows against the restatement cell by cell, no simplex in between (all non-finite instances)
    mirRound()                    k_mir_cuts + simplex; against the simplex of the restatement's grown tableau on the oracle library
    applyCutsMIR, one node        k_node_lds_mir<1024>, behind [] and behind one branching cut      }
    applyCutsBatchMIR, 3 nodes    k_node_lds_mir<1024>, one group                                   }  tests/mir_edges_worker.py, one process
    the same, 512-thread build    k_node_lds_mir<512>   (JSLP_SMALL_BATCH_1024=0)                   }  per setting, the kernel asserted from
    5 nodes on 2 slots            k_node_queue_mir<512> (JSLP_GROUP_MAX=2)                          }  the JSLP_DEBUG_LAUNCH lines
    one node from a checkpoint    the host-sequenced form: k_mir_cuts + k_fractional_volume + relax_mir_sequence's rule

-- against the oracle library's sequence (tests/test_mir_one_call.by_hand), bit for bit as test_mir_one_call.same_node compares: the
result, the outcome record with the volumes as bit patterns, the RHS column and the row map; for the single-node calls also download() and
pivot_trace().  A NaN equals a NaN (the sign of a NaN the arithmetic made is the hardware's); no tolerance anywhere.  No test reads the reference: the restatement is pinned to it on the CPU (tests/test_mir_edges.py).
"""
import os
import subprocess
import sys

import pytest

import golden_util as G
import mir_edges as E
import test_mir_edges as C

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", C.NAMES)
def test_apply_mir_cuts_alone(hip_lib, name):
    C.check_apply_mir_cuts_direct(hip_lib, name)


@pytest.mark.parametrize("name", C.NAMES)
def test_mir_round(hip_lib, oracle_lib, name):
    C.check_mir_round(hip_lib, oracle_lib, name)


MODES = {"lds1024": ({}, "k_node_lds<1024,opt 0,cow 0,mir 1> g %d lds", None),
         "lds512": ({"JSLP_SMALL_BATCH_1024": "0"}, "k_node_lds<512,opt 0,cow 0,mir 1> g %d lds", None),
         "queue": ({"JSLP_GROUP_MAX": "2"}, None, "k_node_queue<512,cow 0,opt 0,mir 1> g 2 n %d lds")}


@pytest.mark.parametrize("mode", list(MODES))
def test_one_call_paths(tmp_path, mode):
    """one worker process per setting, under JSLP_DEBUG_LAUNCH=1: every marked call printed exactly one node-kernel line, the intended build's"""
    knobs, group_line, queue_line = MODES[mode]
    env = dict(os.environ, JSLP_DEBUG_LAUNCH="1", **knobs)
    for k in ("JSLP_SMALL_BATCH_1024", "JSLP_GROUP_MAX"):
        if k not in knobs:
            env.pop(k, None)
    log = tmp_path / "stderr.txt"
    with open(log, "w") as fh:
        p = subprocess.run([sys.executable, os.path.join(HERE, "mir_edges_worker.py"), mode], env=env, stderr=fh, stdout=subprocess.PIPE, text=True, timeout=240)
    text = open(log).read()
    assert p.returncode == 0, text[-3000:]
    assert text.rstrip().endswith("### done")
    calls = [c.split("### end")[0] for c in text.split("### call ")[1:]]
    seen = {}
    for c in calls:
        kind, name, n = c.split("\n")[0].split()
        lines = [l for l in c.split("\n")[1:] if l.startswith("[jslp] launch")]
        want = (queue_line or group_line) % int(n) if kind == "batch" else "k_node_lds<1024,opt 0,cow 0,mir 1> g 1 lds"
        assert len(lines) == 1 and want in lines[0], (kind, name, lines)
        seen.setdefault(name, []).append(kind)
    per_instance = ["single", "single", "batch", "batch"] if mode == "lds1024" else ["batch", "batch"]
    assert seen == {name: per_instance for name in C.ONE_CALL}
    assert {E.BY_NAME[n]["family"] for n in seen} == {"scan", "value", "width", "volume", "loop"}


@pytest.mark.parametrize("name", C.ONE_CALL)
def test_one_node_from_a_checkpoint(hip_lib, oracle_lib, name, monkeypatch, capfd):
    """the host-sequenced form: a node of a checkpoint (a bound that holds, so the checkpointed state is the planted one) with one more cut"""
    inst = E.BY_NAME[name]
    nodes = E.nodes_of(inst)
    rounds = E.rounds_of(inst)
    outs = []
    for lib in (oracle_lib, hip_lib):
        t, _ = E.root_tableau(lib, inst, E.ONE_CALL_EXTRA_ROWS)
        t.applyCuts(nodes[1])
        ck = t.createCheckpoint()
        trace0 = len(t.pivot_trace())
        if lib is hip_lib:
            capfd.readouterr()
            monkeypatch.setenv("JSLP_DEBUG_LAUNCH", "1")
        res, oc, x, w = t.applyCutsMIR(nodes[4], max_rounds=rounds, checkpoint=ck)
        if lib is hip_lib:
            monkeypatch.delenv("JSLP_DEBUG_LAUNCH")
            err = capfd.readouterr().err
            assert "[jslp] launch" in err and "mir 1" not in err  # no MIR build of a node kernel: the loop was sequenced by the host
        trace = t.pivot_trace()
        assert len(trace) - trace0 == int(oc["pivots"])
        d = res.as_dict()
        d["obj_cell"], d["evaluation"] = C.nan_bits(d["obj_cell"]), C.nan_bits(d["evaluation"])
        outs.append((d, tuple(int(oc[k]) for k in ("rounds", "rows_added", "optimal_count", "pivots")),
                     C.nan_bits(oc["volume_before"]), C.nan_bits(oc["volume_after"]), E.hex_doubles(G.canon_nan(x)), w.tobytes(), C.final_state(t),
                     trace.tobytes(), C.nan_bits(t.evaluation), t.feasible, t.simplexIters))
        t.releaseCheckpoint(ck)
        t.close()
    assert outs[0][1][0] >= 1  # the loop ran
    for a, b in zip(outs[0], outs[1]):
        assert a == b


def test_capacity(hip_lib, oracle_lib):
    C.check_capacity(hip_lib, oracle_lib, batch=True)


def test_round_limit(hip_lib, oracle_lib):
    C.check_round_limit(hip_lib, oracle_lib, batch=True)
