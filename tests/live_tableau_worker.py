"""Subprocess body of tests/test_live_tableau.py (the JSLP_* knobs are read once per process): `walks` replays the recorded walks of the
named roots on the product library, one engine per root, and compares the observation of every step with the oracle's from the plan
file; `mir` runs the crafted uploads through applyMIRCuts().  Every relax call's JSLP_DEBUG_LAUNCH lines are compared with LiveDispatch:
node_edges_worker.Dispatch plus the calls a walk makes between the nodes (checkpoints, simplex(), pivot(), JSLP_FORCE_PATH=sp)."""
import os
import pickle
import sys
import traceback

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jslpsolver_amd import _capi  # noqa: E402
import node_edges_worker as W  # noqa: E402
import test_live_tableau as L  # noqa: E402


class LiveDispatch(W.Dispatch):
    """relax_batch_impl's choice for the calls of a walk.  A call from a checkpoint never takes a one-launch kernel: every group is
    k_restore (from the checkpoint) + k_add_cuts + k_simplex_* + k_gather, the slots are in sync with nothing afterwards, and with several
    nodes on the workgroup path the LAST node is a group of its own, in slot 0 (the live tableau it must leave)."""

    def __init__(self, root, env):
        super().__init__(root, env)
        self.sp = env.get("JSLP_FORCE_PATH", "") == "sp"  # force_path 2: no workgroup kernel, no one-launch node

    def call(self, n, branch=False, first_g=None):
        if self.sp:
            self.synced0, self.synced_n = False, max(self.synced_n, 1)
            return [(W.MULTI + "chip-wide", 1, None, 0)] * n
        return super().call(n, branch=branch, first_g=first_g)

    def from_checkpoint(self, n):
        wg = not self.sp and (self.cells <= (W.WG_CELLS_BATCH if n > 1 else W.WG_CELLS_CHILD) or self.cells <= W.WG_CELLS_SINGLE)
        sizes = [1] * n
        if wg:
            group = min(n, self.group_max or 1024)
            if group > self.n_slots:
                self.n_slots = group
            rest = n - 1 if n > 1 else n  # the last of several nodes alone, in slot 0
            sizes = [min(group, rest - a) for a in range(0, rest, group)] + ([1] if n > 1 else [])
        self.synced0, self.synced_n = False, 0
        out = []
        for g in sizes:
            if not wg:
                out.append((W.MULTI + "chip-wide", g, None, 0))
                continue
            opt = bool(self.lds) and self.opt
            shape = 1024 if g == 1 or opt else self.threads
            if opt or (self.lds and shape != 256):
                out.append((W.MULTI + "k_simplex_lds<%d,opt %d>" % (shape, opt), g, None, self.lds))
            else:
                out.append((W.MULTI + "k_simplex_wg<%d,%d>" % (shape, 4 * shape), g, None, 0))
        return out

    def step(self, step, got, lines):
        """-> the lines the step must have printed; the bookkeeping moves as the engine's does"""
        op, refused = step[0], "error" in got
        if op == "cuts":
            want = self.call(1)
            if refused:
                self.refused(want[0][0], 1)
            return want
        if op == "batch":
            return self.call(len(step[1]), first_g=lines[0][1] if lines else None)
        if op == "from":
            return self.from_checkpoint(len(step[2]))
        if op == "save":
            self.save()
        elif op == "restore":
            self.restore()
        elif op == "rck":
            self.synced0, self.synced_n = False, 0
        elif op in ("simplex", "pivot") or (op == "mir" and not refused):
            self.synced0 = False  # k_begin / k_prepare zero the slot's generation
        return []


def describe(step):
    return " ".join(str(x) if not isinstance(x, list) else "[%d]" % len(x) for x in step)[:120]


def compare(name, i, step, want, got):
    where = (name, "step %d" % i, describe(step))
    assert ("error" in want) == ("error" in got) and want.get("error") == got.get("error"), where + ("error code", want.get("error"), got.get("error"))
    assert sorted(want) == sorted(got), where + (sorted(want), sorted(got))
    for key, w in want.items():
        g = got[key]
        if key == "live":
            for k in L.LIVE:
                if k in w and w[k] != g[k]:
                    what = L.first_difference(w[k], g[k]) if isinstance(w[k], tuple) else "expected %r, found %r" % (w[k], g[k])
                    raise AssertionError(where + ("live tableau", k, what))
        elif key == "nodes":
            bad = [j for j, (a, b) in enumerate(zip(w, g)) if a != b]
            assert not bad and len(w) == len(g), where + ("outcomes of nodes", bad[:8], "of", len(w))
        elif key == "out":
            for label, a, b in zip(("RHS column", "row map"), w, g):
                assert a == b, where + ("returned", label, L.first_difference(a, b))
        else:
            assert w == g, where + (key, w, g)


def run_walk(hip, walk, env, err):
    root, name = walk["root"], walk["root"]["name"]
    run = L.Runner(hip, root)
    d = LiveDispatch(root, env)
    kernels = set()
    err.lines()
    try:
        for i, (step, want) in enumerate(zip(walk["steps"], walk["obs"])):
            got = run.do(step)
            lines = err.lines()
            compare(name, i, step, want, got)
            expected = d.step(step, got, lines)
            assert lines == expected, (name, "step %d" % i, describe(step), "launched", lines[:4], "expected", expected[:4])
            kernels |= {ln[0] for ln in lines}
    finally:
        run.close()
    return kernels


def main():
    mode, plan_file, names = sys.argv[1], sys.argv[2], [n for n in sys.argv[3].split("\n") if n]
    err = W.Stderr(plan_file + ".stderr.%d" % os.getpid())
    try:
        with open(plan_file, "rb") as fh:
            plan = pickle.load(fh)
        hip = _capi.load_hip()
        env = dict(os.environ)
        if mode == "walks":  # (the first failure of any kind ends the process: nothing more is started on a GPU that may have faulted)
            for name in names:
                walk = plan["walks"][name]
                kernels = run_walk(hip, walk, env, err)
                print("walk ok | %s | %d steps | %s" % (name, len(walk["steps"]), " ; ".join(sorted(kernels))), flush=True)
        else:
            for case in plan["mir"]:
                got = L.run_mir_case(hip, case)
                want = case["want"]
                assert sorted(want) == sorted(got), (case["name"], want.get("error"), got.get("error"))
                if "error" in want:
                    assert want["error"] == got["error"], (case["name"], want["error"], got["error"])
                    want, got = want["again"], got["again"]
                assert want["added"] == got["added"], (case["name"], "rows appended", want["added"], got["added"])
                for label, a, b in zip(("matrix", "vibr", "vibc", "rbv", "cbv", "read_rhs", "read_rhs rows"), want["arrays"] + want.get("rhs", []), got["arrays"] + got.get("rhs", [])):
                    assert a == b, (case["name"], label, L.first_difference(a, b))
                print("mir ok | %s" % case["name"], flush=True)
        print("ok", flush=True)
    except BaseException:
        print(traceback.format_exc(), flush=True)
        err.out.flush()
        with open(err.path, "rb") as fh:
            print("---- stderr ----\n" + fh.read().decode(errors="replace")[-3000:], flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
