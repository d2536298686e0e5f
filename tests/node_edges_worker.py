"""Subprocess body of tests/test_node_edges.py (the JSLP_* knobs are read once per process): `families` runs every node family of the
named roots through every launch shape of the node on one engine per root, `errors` plants refused cut lists in batches and checks the
calls that follow them.  The oracle's answers come from the plan file the parent wrote.  Every call's JSLP_DEBUG_LAUNCH lines are read
back (stderr of this process goes to a file) and compared with Dispatch, the host bookkeeping of relax_batch_impl restated."""
import os
import pickle
import re
import struct
import sys
import traceback
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jslpsolver_amd import _capi  # noqa: E402
from jslpsolver_amd.engine import branch_record_from_watched  # noqa: E402
import test_node_edges as N  # noqa: E402

LINE = re.compile(r"^\[jslp\] launch (.+?) g (\d+)(?: n (\d+))?(?: lds (\d+))?$", re.M)
WG_CELLS_CHILD, WG_CELLS_BATCH, WG_CELLS_SINGLE = 1536 * 1024, 4 * 1024 * 1024, 64 * 1024
MULTI = "restore+add_cuts+simplex+gather "


class Dispatch:
    """which node kernel relax_batch_impl launches for a call, from the engine's host bookkeeping (slot0_synced, slots_synced, n_slots).
    A restatement of the dispatcher inside the test: the price of asserting the kernel of EVERY call, not of a few.  A change to the
    dispatcher needs its twin here, made from the dispatcher's code and not from the lines it prints; test_node_edges._meant says in
    plain words, independently of this class, which kernels each root is there for.  The one thing read off the engine's output is the
    number of resident workgroups of the queue kernel (first_g), which the occupancy query decides."""

    def __init__(self, root, env):
        self.ld = (root["cols"] + 15) // 16 * 16
        self.cells = root["cap"] * self.ld
        b = N.wglds_bytes(self.ld, root["cap"])
        self.lds = b if b <= N.WGLDS_MAX_BYTES and env.get("JSLP_NO_WGLDS", "")[:1] != "1" else 0
        self.opt = root["oo"] is not None
        self.cow = int(env.get("JSLP_NODE_COW", "1")) != 0
        self.cow_small = int(env.get("JSLP_NODE_COW_SMALL", "1")) != 0
        self.cow_single = int(env.get("JSLP_NODE_COW_SINGLE", "1")) != 0
        self.queue = int(env.get("JSLP_NODE_QUEUE", "2")) != 0
        self.node_kernel = env.get("JSLP_NO_NODE_KERNEL", "")[:1] != "1"
        self.threads = int(env.get("JSLP_WG_BATCH_THREADS", "512"))
        if self.threads not in (256, 1024):
            self.threads = 512
        self.small = int(env.get("JSLP_SMALL_BATCH_1024", "256"))
        self.group_max = int(env["JSLP_GROUP_MAX"]) if "JSLP_GROUP_MAX" in env else None
        self.queue_wgs = None  # resident workgroups of the queue kernel: read off the first launch that is cut by it
        self.synced0, self.synced_n, self.n_slots = False, 0, 1

    def save(self):
        self.synced0, self.synced_n = False, 0

    def restore(self):
        self.synced0, self.synced_n = True, max(self.synced_n, 1)

    def uses_queue(self):
        return bool(self.lds) and self.queue and self.threads == 512 and self.node_kernel and self.cells <= WG_CELLS_BATCH

    def call(self, n, branch=False, first_g=None):
        """-> [(kernel, grid, nodes of a queue launch or None, dynamic LDS bytes)] of a call of n nodes; first_g: the grid of the call's first line"""
        lds = self.lds
        if n == 1 and self.synced0 and self.node_kernel and self.cells <= WG_CELLS_CHILD and not branch:
            if lds and self.opt:
                return [("k_node_lds<1024,opt 1,cow 0>", 1, None, lds)]
            if lds:
                return [("k_node_lds<1024,opt 0,cow %d>" % self.cow_single, 1, None, lds)]
            return [("k_node_wg<1024,4096>", 1, None, 0)]
        wg = self.cells <= (WG_CELLS_BATCH if n > 1 else WG_CELLS_CHILD) or self.cells <= WG_CELLS_SINGLE
        group = 1
        if wg:
            group = min(n, self.group_max or 1024)
            if lds and self.queue and self.threads == 512 and n > 1:
                if self.group_max:
                    group = min(n, self.group_max)
                elif n <= 256:
                    group = n  # (at least one resident workgroup on each of the 256 CUs)
                else:
                    if self.queue_wgs is None:
                        assert first_g is not None and first_g >= 256, first_g
                        self.queue_wgs = first_g if first_g < n else 1 << 30
                    group = min(n, self.queue_wgs)
            if group > self.n_slots:
                self.n_slots, self.synced_n = group, min(self.synced_n, 1)
        if wg and lds and self.queue and n > group and self.synced0 and group <= self.synced_n and self.node_kernel and self.threads == 512:
            name = "k_node_queue<512,cow 0,opt 1>" if self.opt else "k_node_queue<512,cow %d,opt 0>" % self.cow
            return [(name, group, n, lds)]
        out, first = [], 0
        while first < n:
            g = min(group, n - first)
            first += g
            if wg and g > 1 and self.synced0 and g <= self.synced_n and self.node_kernel and self.threads == 512:
                if lds and self.opt:
                    out.append(("k_node_lds<1024,opt 1,cow 0>", g, None, lds))
                elif lds and g <= self.small:
                    out.append(("k_node_lds<1024,opt 0,cow %d>" % (self.cow_small and self.cow), g, None, lds))
                elif lds:
                    out.append(("k_node_lds<512,opt 0,cow 0>", g, None, lds))
                else:
                    out.append(("k_node_wg<512,2048>", g, None, 0))
                continue
            self.synced0, self.synced_n = True, max(self.synced_n, g)
            if not wg:
                out.append((MULTI + "chip-wide", g, None, 0))
                self.synced0 = False  # (run_simplex: the chip-wide kernels do not keep the dirty-row flags)
                continue
            opt = bool(lds) and self.opt
            shape = 1024 if g == 1 or opt else self.threads
            if opt or (lds and shape != 256):
                out.append((MULTI + "k_simplex_lds<%d,opt %d>" % (shape, opt), g, None, lds))
            else:
                out.append((MULTI + "k_simplex_wg<%d,%d>" % (shape, 4 * shape), g, None, 0))
        return out

    def refused(self, first_kernel, n):
        """the bookkeeping after a call of n nodes that ended in a refused cut list; first_kernel: the name on the call's first launch line"""
        if first_kernel.startswith("k_node_") and n == 1:
            self.synced0 = False  # the one-launch single node: slot 0 alone
        elif not first_kernel.endswith("chip-wide"):  # (the chip-wide sequence stops at the refused cuts, behind its restore)
            self.synced0, self.synced_n = False, 0


class Stderr:
    """this process's stderr (the engine's fprintf included) in a file; lines() returns what arrived since the last look"""

    def __init__(self, path):
        self.path = path
        self.out = open(path, "wb")
        os.dup2(self.out.fileno(), 2)
        self.inp = open(path, "rb")

    def lines(self):
        sys.stderr.flush()
        text = self.inp.read().decode(errors="replace")
        return [(m.group(1), int(m.group(2)), int(m.group(3)) if m.group(3) else None, int(m.group(4)) if m.group(4) else 0)
                for m in LINE.finditer(text) if m.group(1).startswith(("k_node_", "restore+"))]


def bits(x):
    return struct.pack("<d", x)


class Root:
    def __init__(self, hip, root, env, err):
        self.root, self.err, self.name = root, err, root["name"]
        self.fam, self.want = root["family"], root["want"]
        self.t = N.tableau(hip, root)
        res = self.t.simplex(check_cycles=root["check"])
        assert res.feasible and res.bounded and res.optimal, self.name
        rhs, rows = self.t.read_rhs()
        assert rhs.tobytes() == root["root_rhs"] and rows.tobytes() == root["root_rows"], (self.name, "the root itself differs")
        assert bits(self.t.evaluation) == bits(root["root_eval"]), self.name
        self.t.save()
        self.watched = list(root["watched"])
        self.watched_dup = self.watched + [self.watched[len(self.watched) // 2], self.watched[0]]
        self.t.set_watched_variables(self.watched)
        self.eval = root["root_eval"]  # what a node without an optimum reports: the evaluation its call started from
        self.d = Dispatch(root, env)
        self.d.save()
        self.err.lines()
        self.kernels = set()
        self._compact = {}
        self.calls = 0

    def close(self):
        self.t.close()

    # ---- expectations --------------------------------------------------------------------------------------------------------------
    def compact_of(self, k, dup):
        key = (k, dup)
        if key not in self._compact:
            w = self.want[k]
            rows = np.frombuffer(w["rows"], dtype=np.int32)
            rhs = np.frombuffer(w["rhs"], dtype=np.float64)
            row_of = {int(v): r for r, v in enumerate(rows) if r > 0}
            watched = self.watched_dup if dup else self.watched
            r = np.array([row_of.get(v, -1) for v in watched], dtype=np.int32)
            v = np.where(r > 0, rhs[np.maximum(r, 0)], 0.0)
            self._compact[key] = (r, v)
        return self._compact[key]

    def expected_eval(self, k, prev):
        w = self.want[k]
        return w["evaluation"] if w["optimal"] else (float("-inf") if not w["bounded"] else prev)

    def check_lines(self, n, what, branch=False):
        got = self.err.lines()
        want = self.d.call(n, branch=branch, first_g=got[0][1] if got else None)
        assert got == want, (self.name, what, "launched", got[:4], "expected", want[:4])
        self.kernels |= {g[0] for g in got}
        return got

    def check_state(self, k, res, prev, what, pivots=True):
        w = self.want[k]
        got = (bool(res.feasible), bool(res.bounded), bool(res.optimal), res.height)
        assert got == (w["feasible"], w["bounded"], w["optimal"], w["height"]), (self.name, what, k, self.root["what"][k], got)
        if pivots:
            assert (res.pivots_phase1, res.pivots_phase2, res.cycle_phase) == (w["p1"], w["p2"], w["cycle"]), (self.name, what, k, "pivots")
        assert bits(res.obj_cell) == bits(w["obj_cell"]), (self.name, what, k, "objective cell")
        assert bits(res.evaluation) == bits(self.expected_eval(k, prev)), (self.name, what, k, "evaluation", res.evaluation, self.expected_eval(k, prev))

    def check_full(self, k, res, rhs, rows, prev, what):
        self.check_state(k, res, prev, what)
        w, h = self.want[k], res.height
        assert np.ascontiguousarray(rhs[:h]).tobytes() == w["rhs"], (self.name, what, k, self.root["what"][k], "RHS column")
        assert np.ascontiguousarray(rows[:h]).tobytes() == w["rows"], (self.name, what, k, self.root["what"][k], "row map")

    # ---- calls ---------------------------------------------------------------------------------------------------------------------
    def single(self, k, restore, compact=False):
        what = "single%s%s" % (" after restore()" if restore else "", " compact" if compact else "")
        if restore:
            self.t.restore()
            self.d.restore()
        prev = self.eval
        self.calls += 1
        if compact:
            res, wrows, wvals = self.t.applyCutsWatched(self.fam[k], check_cycles=True)
            self.check_lines(1, what)
            self.check_state(k, res, prev, what)
            r, v = self.compact_of(k, False)
            assert wrows.tobytes() == r.tobytes() and wvals.tobytes() == v.tobytes(), (self.name, what, k, "watched rows / values")
        else:
            res, rhs, rows = self.t.applyCuts(self.fam[k], check_cycles=True)
            self.check_lines(1, what)
            self.check_full(k, res, rhs, rows, prev, what)
        self.eval = self.expected_eval(k, prev)

    def repeats(self, ks):
        """a batch that is the whole family over and over: the first repetition is checked node by node, the others against it, array-wise"""
        nf = len(self.fam)
        return len(ks) // nf if len(ks) > nf and len(ks) % nf == 0 and list(ks[:nf]) == list(range(nf)) and list(ks) == list(ks[:nf]) * (len(ks) // nf) else 0

    def same_as_first(self, a, mult, what, label, heights=None):
        """a: [mult * nf, ...] bytes-comparable array of one call; every repetition equals the first (up to each node's height)"""
        nf = len(self.fam)
        a = np.ascontiguousarray(a[:mult * nf])
        a = a.view(np.uint8).reshape(mult, nf, -1)
        if heights is None:
            assert (a[1:] == a[0]).all(), (self.name, what, label, "a repetition differs from the first")
            return
        item = a.shape[2] // heights[1]
        for k in range(nf):
            h = heights[0][k] * item
            assert (a[1:, k, :h] == a[0, k, :h]).all(), (self.name, what, k, label, "a repetition differs from the first")

    @staticmethod
    def raw_results(res, n):
        arr = res if isinstance(res, _capi.C.Array) else res[0]._b_base_
        return np.frombuffer(arr, dtype=np.uint8).reshape(-1, _capi.C.sizeof(_capi.SimplexResult))[:n]

    def batch(self, ks, kind):
        """kind: full | pinned | compact | compact-dup | branch"""
        nodes = [self.fam[k] for k in ks]
        n, prev, what = len(ks), self.eval, "%s batch of %d" % (kind, len(ks))
        self.calls += 1
        mult = self.repeats(ks)
        all_ks = ks
        if mult:
            ks = ks[:len(self.fam)]
        if kind in ("full", "pinned"):
            res, rhs, rows = self.t.applyCutsBatch(nodes, check_cycles=True, copy=kind == "full")
            self.check_lines(n, what)
            for j, k in enumerate(ks):
                self.check_full(k, res[j], rhs[j], rows[j], prev, what)
            if mult:
                heights = ([self.want[k]["height"] for k in ks], rhs.shape[1])
                self.same_as_first(self.raw_results(res, n), mult, what, "result")
                self.same_as_first(rhs, mult, what, "RHS column", heights)
                self.same_as_first(rows, mult, what, "row map", heights)
        elif kind in ("compact", "compact-dup"):
            dup = kind == "compact-dup"
            if dup:
                self.t.set_watched_variables(self.watched_dup)
            try:
                res, wrows, wvals = self.t.applyCutsBatchWatched(nodes, check_cycles=True, copy=not dup)
                self.check_lines(n, what)
                for j, k in enumerate(ks):
                    self.check_state(k, res[j], prev, what)
                    r, v = self.compact_of(k, dup)
                    assert np.asarray(wrows[j]).tobytes() == r.tobytes(), (self.name, what, k, "watched rows")
                    assert np.asarray(wvals[j]).tobytes() == v.tobytes(), (self.name, what, k, "watched values")
                if mult:
                    self.same_as_first(self.raw_results(res, n), mult, what, "result")
                    self.same_as_first(np.asarray(wrows), mult, what, "watched rows")
                    self.same_as_first(np.asarray(wvals), mult, what, "watched values")
            finally:
                if dup:
                    self.t.set_watched_variables(self.watched)
        else:
            res, recs = self.t.applyCutsBatchBranch(nodes, check_cycles=True)
            self.check_lines(n, what, branch=True)
            for j, k in enumerate(ks):
                w = self.want[k]
                self.check_state(k, res[j], prev, what, pivots=False)
                fake = types.SimpleNamespace(feasible=w["feasible"], bounded=w["bounded"], optimal=w["optimal"], height=w["height"],
                                             unbounded_var_index=w["unbounded_var"], obj_cell=w["obj_cell"])
                r, v = self.compact_of(k, False)
                exp = branch_record_from_watched([fake], r[None, :], v[None, :], self.watched, self.t.precision)
                assert recs[j:j + 1].tobytes() == exp.tobytes(), (self.name, what, k, self.root["what"][k], recs[j], exp[0])
            if mult:
                self.same_as_first(self.raw_results(res, n), mult, what, "result")
                self.same_as_first(np.asarray(recs), mult, what, "branch records")
        self.eval = self.expected_eval(all_ks[-1], prev)

    def refused(self, nodes, code, what):
        self.calls += 1
        try:
            if len(nodes) == 1:
                self.t.applyCuts(nodes[0], check_cycles=True)
            else:
                self.t.applyCutsBatch(nodes, check_cycles=True)
        except _capi.EngineError as e:
            assert N.error_code(e) == code, (self.name, what, str(e), code)
        else:
            raise AssertionError((self.name, what, "no error"))
        got = self.check_lines(len(nodes), what)
        self.d.refused(got[0][0], len(nodes))

    def big(self):
        """the family many times over: more nodes than the queue kernel has resident workgroups"""
        n = len(self.fam)
        mult = 30 if self.d.group_max else max(30, -(-1100 // n))
        return [k for _ in range(mult) for k in range(n)]


def window(n, start, size):
    return [(start + i) % n for i in range(size)]


def run_families(r):
    n = len(r.fam)
    for rep in range(2):
        for k in range(n):
            r.single(k, restore=True)
    for rep in range(2):
        for k in range(n):
            r.single(k, restore=False)
    for k in range(n):
        r.single(k, restore=False, compact=True)
    for size in (2, 8, 16, 17, n):  # the whole family cut into batches of that size (the last one filled up from the front), each batch twice
        for kind in ("full", "pinned", "compact", "branch") + (("compact-dup",) if size in (8, n) else ()):
            for a in range(0, n, size):
                r.batch(window(n, a, size), kind)
                r.batch(window(n, a, size), kind)
    q0 = r.t.get_counters()["node_queue_launches"]
    ks = r.big()
    # (JSLP_GROUP_MAX=4: four workgroups walk the whole batch, and every batch above already went through the queue -- fewer repeats)
    kinds = ("full", "full", "compact", "branch") if r.d.group_max else ("full", "full", "full", "compact", "pinned", "branch", "compact-dup")
    for kind in kinds:
        r.batch(ks, kind)
    if r.d.uses_queue():
        assert r.t.get_counters()["node_queue_launches"] >= q0 + len(kinds) - 2, (r.name, "the queue kernel did not run")
        assert any(k.startswith("k_node_queue") for k in r.kernels), r.name
    # and small calls again, on the slots the queue left behind
    r.batch(window(n, 3, 8), "full")
    r.single(0, restore=False)
    r.single(n - 1, restore=False)


def run_large(r):
    n = len(r.fam)
    for k in range(n):
        r.single(k, restore=True)
    for k in range(n):
        r.single(k, restore=False)
    for size in (2, 8, 17, n):
        for kind in ("full", "compact", "branch"):
            for a in range(0, n, size):
                r.batch(window(n, a, size), kind)
                r.batch(window(n, a, size), kind)
    if not r.name.startswith("dirty"):
        return None
    # more dirty rows than the list of k_node_wg holds: the call that restores them (its list-free loop) must still be right
    k, cap = N.dirty_node(r.root), N.wg_list_cap(r.name)
    r.t.set_counting(True)
    if cap == 4096:  # the single node
        calls = [lambda: r.single(k, restore=False)] * 3
        want = "k_node_wg<1024,4096>"
    else:  # a batch: slot 0 idles on the node without cuts, slot 1 repeats the node that pivots
        calls = [lambda: r.batch([0, k], "full")] * 3
        want = "k_node_wg<512,2048>"
    calls[0]()
    calls[1]()
    before = r.t.get_counters()["restored_rows"]
    calls[2]()  # restores what the second call dirtied
    restored = r.t.get_counters()["restored_rows"] - before
    r.t.set_counting(False)
    assert want in r.kernels, (r.name, sorted(r.kernels))
    assert restored > cap, (r.name, "restored_rows", restored, "the list holds", cap)
    print("%s: restored_rows +%d in one %s node (list capacity %d)" % (r.name, restored, want, cap), flush=True)
    for kk in range(n):  # and every node once more on the slot that loop restored
        r.single(kk, restore=False)
    return None


def run_errors(r):
    n = len(r.fam)
    big = r.big()
    follow = (("single", lambda: [r.single(k, restore=False) for k in range(n)]),
              ("small batch", lambda: r.batch(list(range(n)), "full")),
              ("queue", lambda: r.batch(big, "compact")))
    # first bring every shape's slots in sync, so that the refused calls meet the one-launch kernels (the predicted error codes)
    for _, f in follow:
        f()
        f()
    count = 0
    for label, cuts, code in r.root["bad"]:
        for size in (1, 8, 17, len(big)):
            for pos in ("first", "middle", "last") if size > 1 else ("only",):
                at = {"only": 0, "first": 0, "middle": size // 2, "last": size - 1}[pos]
                nodes = [r.fam[k] for k in (big[:size] if size > 17 else window(n, count, size))]
                nodes[at] = cuts
                for shape, f in follow:
                    what = "%s, %s of %d, then %s" % (label, pos, size, shape)
                    r.refused(nodes, code, what)
                    f()  # the very next call, without a restore()
                    f()  # and the one after it
                    count += 1
    return count


def main():
    mode, plan_file, names = sys.argv[1], sys.argv[2], sys.argv[3].split("\n")
    err = Stderr(plan_file + ".stderr.%d" % os.getpid())
    try:
        with open(plan_file, "rb") as fh:
            plan = pickle.load(fh)
        hip = _capi.load_hip()
        env = dict(os.environ)
        for name in names:
            r = Root(hip, plan[name], env, err)
            try:
                extra = {"families": run_families, "large": run_large, "errors": run_errors}[mode](r)
            finally:
                r.close()
            print("root ok | %s | %d calls%s | %s" % (name, r.calls, "" if extra is None else ", %d refused" % extra, " ; ".join(sorted(r.kernels))), flush=True)
        print("ok", flush=True)
    except BaseException:
        print(traceback.format_exc(), flush=True)
        err.out.flush()
        with open(err.path, "rb") as fh:
            print("---- stderr ----\n" + fh.read().decode(errors="replace")[-3000:], flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
