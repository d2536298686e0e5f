#!/usr/bin/env python3
"""bench.py -- headline measurement (BASELINE.json): simplex pivots/sec on the synthetic dense LP
generateResourceAllocation({seed:12345, numVariables:2000, numConstraints:2000, density:1.0}) (config 3a:
2001 x 2001 fp64 tableau, 9726 pivots, cycle check off -- the FASTER reference setting), 1 GPU; with --gpus N every
rank solves its own replica (a single LP does not shard: SURVEY.md 8e "replicas only").  With --full, riding along in
the same JSON line: the same LP with the reference's DEFAULT cycle check on, the all-phase-1 instance 3b, the streaming
instance beyond the register file, the drop-in through the reference host, and config 4's LP relaxations/sec
(Monster_II): an independent node batch sharded over the ranks (weak scaling) and ONE real branch-and-bound tree
sharded over the ranks with RCCL as the exchange step (strong scaling).

A "step" = one complete simplex() of the workload with the tableau already resident in HBM (restored from the
device-side snapshot; the 32 MB host upload happens once, outside the timed region).

  python bench.py [--gpus N] [--steps K] [--warmup W]          (N > 1: spawns N ranks itself, one per GPU, RCCL)
  python bench.py ... --dump-outputs DIR   (also writes the last timed step's result and tableau as DIR/<name>.npy, float64, <= 64 MB)
  python bench.py ... --full               (every other leg, check and baseline below; the --no-* options trim it)
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...   (the driver's form)

Prints ONE JSON line on rank 0.  A plain run does only what the headline needs: set-up, warm-up, the timed steps, the
dump if asked for, and the line (headline figure + the roofline of the timed steps' own event-timed kernel).  With
--full every result that has a reference answer is CHECKED (pivot digests of SURVEY.md Appendix C, the reference's
per-node outcomes and final result of Monster_II): a wrong answer exits non-zero instead of printing a number.  GPU
legs run back to back first; the CPU baselines (the reference itself under node) last.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X spec (MI355X_MICROARCH.md)
# pivot digests of the reference itself (options.exitOnCycles = false and the default give the same
# pivots on these instances: no cycle is ever detected)
DIGEST_3A = {100: "b5dedd09", 200: "27aaaa0b", 500: "1cda2607", 1000: "77bfa35c", 2000: "e8cab46c"}
DIGEST_3B = {100: "7f16dba0", 200: "d9715450", 500: "1ff155dd", 1000: "854e8f4", 2000: "5dd32458"}
PIVOTS_3A = {100: 20, 200: 242, 500: 657, 1000: 2833, 2000: 9726}


class WrongAnswer(SystemExit):
    def __init__(self, what):
        super().__init__("bench.py: WRONG ANSWER -- %s" % what)


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` outside a torchrun world: launch N ranks (one per GPU, RCCL) and relay rank 0's line"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    return subprocess.call(cmd, env=env)


def cpu_baseline(n, sample_pivots):
    """The reference itself (oracle/_ref, type-erased TypeScript under node, 1 thread) on the SAME instance,
    stopped after `sample_pivots` pivots of its simplex(); time = simplex entry -> last sampled pivot."""
    script = os.path.join(ROOT, "oracle", "ref_pivot_rate.js")
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "src", "solver.js")):
        return None
    try:
        out = subprocess.run(["node", "--max-old-space-size=8192", script, str(n), str(sample_pivots)],
                             capture_output=True, text=True, timeout=900)
        line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
        r = json.loads(line)
        base = {"value": r["pivots_per_sec"], "unit": "pivots/s", "cores": 1, "kind": "reference",
                "sample": "first %d of the %d pivots of the same %dx%d instance, reference TS (type-erased) under node %s, "
                          "options.exitOnCycles=false, simplex() time only; host has %d cores"
                          % (r["pivots"], PIVOTS_3A.get(n, -1), n + 1, n + 1, r["node"], os.cpu_count())}
        try:  # the reference's FULL run of the same instance on a box of this class, measured once per round (tools/gpu_round.sh cpufull)
            with open(os.path.join(ROOT, "profiles", "r05_cpu_full_run.json")) as fh:
                full = json.load(fh)
            if full.get("n") == n:
                base["full_run_committed"] = {"value": full["pivots_per_sec"], "pivots": full["pivots"], "seconds": full["seconds"],
                                              "source": "profiles/r05_cpu_full_run.json (all %d pivots, not timed in this run)" % full["pivots"]}
        except Exception:
            pass
        return base
    except Exception as e:  # the baseline is reported, never required
        return {"value": None, "unit": "pivots/s", "cores": 1, "kind": "reference", "sample": "failed: %r" % (e,)}


DROPIN_NODE = r"""
const fs=require('fs'),path=require('path'),zlib=require('zlib');
const root=process.argv[1], mode=process.argv[2];
const solver=require(path.join(root,'oracle/_ref/src/solver.js')).default;
let addon=null,gpu=null;
if(mode!=='cpu'){const T=require(path.join(root,'oracle/_ref/src/tableau/tableau.js')).default;
 const {SlackVariable}=require(path.join(root,'oracle/_ref/src/expressions.js'));
 gpu=require(path.join(root,'host/gpu-tableau.js'));gpu.loadEngine({});gpu.install(T,{SlackVariable,solver});
 addon=require(path.join(root,'addon/jslp_napi.node'));}
// time inside Model.solve (tableau build, simplex / branch-and-cut, read-out) apart from the reference's own JSON parsing and result
// assembly around it, whose garbage (a scavenge of 1-1.5 ms in most solves) makes the totals of the small configurations noisy
const M=require(path.join(root,'oracle/_ref/src/model.js')).default;let tSolve=0;const origSolve=M.prototype.solve;
M.prototype.solve=function(){const t0=process.hrtime.bigint();try{return origSolve.apply(this,arguments);}finally{tSolve+=Number(process.hrtime.bigint()-t0)/1e6;}};
const out={};const q=(a,f)=>{const b=a.slice().sort((x,y)=>x-y);return b[Math.min(b.length-1,Math.floor(f*b.length))];};
// the binding's calls, grouped into the phases of a Solve() (addon.timings(): wall clock inside each N-API function)
const PH={create_pin:['create','hostMatrix'],upload:['upload','setOptionalObjectives','setIntegerVariables','setWatchedVariables','save'],
 simplex:['simplex','relax','relaxWatched','relaxBatch','relaxBatchWatched','relaxFrom','addCuts','applyMirCuts','checkpointCreate','checkpointRestore','checkpointRelease'],
 read_back:['readRhs','getOptionalObjectives','download','dims','pivotTrace'],release:['detach','destroy','poolDestroy']};
for(const spec of process.argv.slice(3)){
 const [name,warm,runs]=spec.split(':');
 let g;
 if(name[0]==='@'){const gen=require(path.join(root,'oracle/_ref/src/test-utils/problem-generator.js'));const [n,m,d]=name.slice(1).split('x').map(Number);
  g={model:gen.generateResourceAllocation({seed:7,numVariables:n,numConstraints:m,density:d}),result:{result:null}};}
 else g=JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(root,'tests/golden/fixtures',name+'.json.gz'))).toString());
 const run=()=>{const m=JSON.parse(JSON.stringify(g.model));tSolve=0;if(addon)addon.timings(true);const t0=process.hrtime.bigint();const r=solver.Solve(m);
  const ms=Number(process.hrtime.bigint()-t0)/1e6;const ph={};let calls=0;
  if(addon){const t=addon.timings(true);for(const k of Object.keys(PH)){ph[k]=0;for(const f of PH[k])if(t[f]){ph[k]+=t[f][0];calls+=t[f][1];delete t[f];}}
   ph.other_calls=0;for(const f of Object.keys(t)){ph.other_calls+=t[f][0];calls+=t[f][1];}}
  return {ms,res:r.result,solve:tSolve,ph,calls};};
 for(let i=0;i<Number(warm||12);i++)run();const a=[],b=[],phs=[];let calls=0;
 for(let i=0;i<Number(runs||31);i++){const r=run();a.push(r.ms);b.push(r.solve);phs.push(r.ph);calls=r.calls;}
 const e={ms:q(a,0.5),min_ms:Math.min(...a),p90_ms:q(a,0.9),model_solve_ms:q(b,0.5),model_solve_min_ms:Math.min(...b),model_solve_p90_ms:q(b,0.9),runs:a.length,result:run().res,want:g.result.result};
 if(addon){e.on_engine=calls>0;e.binding_calls=calls;e.phases_ms={};for(const k of Object.keys(phs[0]))e.phases_ms[k]=q(phs.map((p)=>p[k]),0.5);
  // what is left of Model.solve once the binding's calls are taken out: the reference's own host code (tableau build in the pinned buffer, B&B tree, read-out)
  const inSolve=['create_pin','upload','simplex','read_back','other_calls'].reduce((s,k)=>s+e.phases_ms[k],0);e.phases_ms.host_in_model_solve=Math.max(0,e.model_solve_ms-inSolve);
  e.phases_ms.json_and_result=Math.max(0,e.ms-e.model_solve_ms-e.phases_ms.release);}
 out[name]=e;}
console.log(JSON.stringify(out));
"""


def dropin_leg(with_cpu):
    """THE drop-in, end to end: solver.Solve(model) through the reference's own host (oracle/_ref: JSON parsing, presolve, the
    branch-and-bound tree) + host/gpu-tableau.js + the N-API addon + the HIP engine, default install() options, JIT-warm min / median /
    p90 of 31 (totals, and the time inside Model.solve apart), with the binding's own per-phase wall times (addon.timings()) -- next to
    the unpatched reference on this box's CPU.  Runs in a child process BEFORE this process touches the GPU."""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "src", "solver.js")) or not os.path.exists(os.path.join(ROOT, "addon", "jslp_napi.node")):
        return None
    # name[:warm-up solves:timed solves]; "@n x m x density" = the reference's generateResourceAllocation(seed 7) -- a dense mid-size LP the
    # default policy DOES send to the engine (Monster LP, 1 % dense, it does not: host/gpu-tableau.js `structuralNnz`)
    specs = ["Monster_Problem", "Monster_II", "Vendor_Selection:4:7", "@300x225x0.8:4:9"]
    names = [s.split(":")[0] for s in specs]
    res = {}
    for mode in (("gpu", "cpu") if with_cpu else ("gpu",)):
        try:
            out = subprocess.run(["node", "-e", DROPIN_NODE, ROOT, mode] + specs, capture_output=True, text=True, timeout=900)
            res[mode] = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        except Exception as e:
            res[mode] = {"error": repr(e)}
    leg = {"what": "solver.Solve(model) through the reference host (type-erased TS under node) + host/gpu-tableau.js + N-API addon + HIP engine, "
                   "default install(Tableau, {solver}) options (work-aware size policy: LPs by structural non-zeros, MILPs by cells; 16-node speculative "
                   "batches); JIT-warm min / median / p90, ms; phases_ms = median wall time inside the binding's calls of one Solve (addon.timings())",
           "configs": {}}
    for n in names:
        g, c = res.get("gpu", {}).get(n), res.get("cpu", {}).get(n)
        want = (g or {}).get("want")
        if want is None and c:
            want = c.get("result")  # generated models: the unpatched reference's own answer of this run
        if g and want is not None and g.get("result") != want:
            raise WrongAnswer("drop-in Solve(%s): %r, the reference: %r" % (n, g.get("result"), want))
        leg["configs"][n] = {"dropin_ms": g and g["ms"], "dropin_min_ms": g and g["min_ms"], "dropin_p90_ms": g and g.get("p90_ms"),
                             "reference_cpu_ms": c and c["ms"], "reference_cpu_min_ms": c and c.get("min_ms"), "reference_cpu_p90_ms": c and c.get("p90_ms"),
                             "speedup": (c["ms"] / g["ms"]) if (g and c and g.get("ms") and c.get("ms")) else None,
                             # inside Model.solve only (tableau build + simplex / branch-and-cut + read-out: what the binding replaces),
                             # without the reference's JSON handling around it
                             "model_solve_ms": g and g.get("model_solve_ms"), "reference_cpu_model_solve_ms": c and c.get("model_solve_ms"),
                             "model_solve_speedup": (c["model_solve_ms"] / g["model_solve_ms"]) if (g and c and g.get("model_solve_ms") and c.get("model_solve_ms")) else None,
                             "on_engine": g and g.get("on_engine"), "binding_calls": g and g.get("binding_calls"), "phases_ms": g and g.get("phases_ms"),
                             "runs": g and g.get("runs"), "result": g and g["result"]}
    return leg


# MI355X constants of the latency floor below (MI355X_MICROARCH.md: chip table, "Persistent kernels: price list")
SHADER_CLOCK_HZ = 2.4e9
FP64_FLOP_PER_CLK_PER_CU = 128.0   # 78.6 TFLOP/s fp64 vector / 256 CUs / 2.4 GHz
HANDOFF_US = 0.8                   # row handoff-1to1, idle, 8-byte granule: one producer -> one consumer through the fabric
ROW_FETCH_US = 1.0                 # row handoff-payload: a freshly published 16 KB tile is read at 12-20 GB/s (latency-bound)


def resident_latency_floor(H, W, n_cus=256):
    """What bounds a register-resident pivot.  No tableau byte has to cross HBM (the tableau lives in the chip's registers), so
    the HBM roofline does not apply; per pivot there remains a dependency chain no scheduling can shorten:
      ratio test = a min over ALL rows, which live in 256 CUs    -> one fabric hand-off of the summaries (>= handoff-1to1)
      the winner's row must reach every CU                        -> a 16 KB read of freshly published data (handoff-payload)
      every CU eliminates its rows                                 -> (cells per CU) x (mul + add) fp64 on its four SIMDs
    Pricing and the per-workgroup reductions are priced at zero (they are what the kernel can still shave)."""
    rows_per_wg = -(-H // n_cus)
    ld = -(-W // 16) * 16
    valu_us = rows_per_wg * ld * 2.0 / FP64_FLOP_PER_CLK_PER_CU / SHADER_CLOCK_HZ * 1e6
    return {"summary_handoff_us": HANDOFF_US, "row_fetch_us": ROW_FETCH_US, "valu_us": valu_us, "floor_us": HANDOFF_US + ROW_FETCH_US + valu_us,
            "source": "MI355X_MICROARCH.md price list: handoff-1to1 (idle, 8 B) 0.8 us; handoff-payload 16 KB at 12-20 GB/s ~ 1.0 us; "
                      "fp64 vector 78.6 TFLOP/s = 128 flop/clk/CU at 2.4 GHz"}


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(out_dir, t, res):
    """--dump-outputs: what the caller of the timed path receives from its last step -- the simplex result and the tableau state
    (jslp_engine_download) -- as out_dir/<name>.npy, float64, so that two builds can be compared output for output.  A tableau too
    large for the 64 MB budget is cut to a fixed, seeded sample of its rows (tableau_rows.npy holds their indices)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    m, vibr, vibc, rbv, cbv = t.download()
    out = {"simplex_result": np.array([float(getattr(res, name)) for name, _ in res._fields_], dtype=np.float64),
           "var_index_by_row": vibr.astype(np.float64), "var_index_by_col": vibc.astype(np.float64),
           "rows_by_var": rbv.astype(np.float64), "cols_by_var": cbv.astype(np.float64)}
    room = DUMP_CAP_BYTES - sum(a.nbytes for a in out.values())
    if m.nbytes > room:
        keep = max(1, (room - 8 * m.shape[0]) // (8 * m.shape[1]))
        rows = np.sort(np.random.default_rng(12345).choice(m.shape[0], size=min(keep, m.shape[0]), replace=False))
        out["tableau_rows"] = rows.astype(np.float64)
        m = m[rows]
    out["tableau"] = np.ascontiguousarray(m, dtype=np.float64)
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(out)


def kernel_sources_sha():
    """identity of the tree a measurement belongs to, as far as the kernels go: sha256 over jslpsolver_amd/csrc/* and the C ABI header
    (the GPU boxes have no .git; tools/pmc_latest.py stamps the PMC summary with the same hash)"""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "jslpsolver_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(csrc, name), "rb") as fh:
                h.update(name.encode() + b"\0" + fh.read())
    with open(os.path.join(ROOT, "include", "jslp_engine.h"), "rb") as fh:
        h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_traffic(key, kernel, alg_bytes):
    """HBM bytes per unit of the dominant kernel from the PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate
    runs, gfx950 FETCH_SIZE x2 correction): counters cannot be read from inside this process, so the committed summary of
    the latest pass on this workload is reported with its provenance (tools/gpu_round.sh pmc regenerates it)."""
    path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    try:
        with open(path) as fh:
            d = json.load(fh)[key]
        if d["kernel"] != kernel or abs(d["algorithmic_bytes_per_unit"] - alg_bytes) > 1e-2 * alg_bytes:  # (which node a slot evaluated before decides what it restores: ~0.3 % run to run)
            return None, "profiles/pmc_latest.json[%s] is for another workload / kernel (%s)" % (key, d["kernel"])
        if d.get("kernel_sources_sha") != kernel_sources_sha():  # a summary taken on other kernel sources is not this build's traffic
            return None, ("profiles/pmc_latest.json[%s] was taken on other kernel sources (%s, this tree: %s): re-run tools/gpu_round.sh pmc"
                          % (key, d.get("kernel_sources_sha"), kernel_sources_sha()))
        return d["traffic_bytes_per_unit"], "profiles/pmc_latest.json[%s] (%s; %s)" % (key, d["kernel"], d["source"])
    except Exception:
        return None, "no PMC summary committed for %s" % key


def pmc_sq(key, kernel):
    """what the waves of the dominant kernel did per unit of work (tools/pmc_sq.py: rocprofv3 --pmc SQ_* passes over the same workload,
    folded into profiles/pmc_latest.json[<key>_sq]); reported only when it was taken on this tree's kernel sources"""
    path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    try:
        with open(path) as fh:
            d = json.load(fh)[key + "_sq"]
        if d["kernel"] != kernel:
            return {"note": "profiles/pmc_latest.json[%s_sq] is for another kernel (%s)" % (key, d["kernel"])}
        if d.get("kernel_sources_sha") != kernel_sources_sha():
            return {"note": "profiles/pmc_latest.json[%s_sq] was taken on other kernel sources (%s, this tree: %s): re-run tools/gpu_round.sh sq sqp"
                            % (key, d.get("kernel_sources_sha"), kernel_sources_sha())}
        keep = ("valu_per_wave_per_pivot", "salu_per_wave_per_pivot", "useful_valu_per_wave_per_pivot", "useful_valu_frac", "waves_per_dispatch",
                "wait_any_share_of_wave_cycles", "issuing_share_of_wave_cycles", "note")
        out = {k: d[k] for k in keep if k in d}
        out["source"] = "profiles/pmc_latest.json[%s_sq] (%s; %s)" % (key, d["kernel"], d["source"])
        return out
    except Exception:
        return {"note": "no SQ-counter summary committed for %s" % key}


def pool_devices_leg(device, ndev, reps):
    """child process of the relaxation legs (N = 1, several devices visible): the fixed 151 x reps Monster_II batch through ONE engine on `device` (compact
    read-back: the comparison base) and through jslp_pool_relax_batch_watched_pinned over devices [device, others...]; every node of the pool's last call is
    compared with the single engine's outcome; prints one JSON object."""
    import gzip
    import numpy as np
    from jslpsolver_amd import Model, _capi
    from jslpsolver_amd.engine import DevicePool, Tableau
    lib = _capi.load_hip()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "fixtures", "Monster_II.json.gz"), "rt") as fh:
        g = json.load(fh)
    model = Model(g["model"])
    m, vibr, vibc = model.build_tableau()
    nodes = [c["cuts"] or [] for c in g["simplexCalls"][1:]] * reps
    t = Tableau(m, vibr, vibc, model.unrestricted, precision=model.precision, row_capacity=m.shape[0] + 2 * len(model.integerVariables), device=device, lib=lib)
    t.applyCuts([], check_cycles=True)
    t.save()
    ints = [int(v) for v in model.integer_index_array]
    t.set_watched_variables(ints)
    packed = t.pack_cut_lists(nodes)
    r1, rows1, vals1 = t.applyCutsBatchWatched(None, check_cycles=True, packed=packed, copy=True)
    devs = [device] + [d for d in range(ndev) if d != device]
    pool = DevicePool(t, devs)
    pool.set_watched_variables(ints)
    fn = lambda: pool.applyCutsBatchWatched(None, check_cycles=True, packed=packed, copy=False)
    for _ in range(8):
        fn()
    per = []
    for _ in range(10):
        t0 = time.perf_counter(); rN, rowsN, valsN = fn(); per.append(time.perf_counter() - t0)
    for i in range(len(nodes)):
        if (rN[i].height != r1[i].height or rN[i].feasible != r1[i].feasible or not np.array_equal(rowsN[i], rows1[i])
                or not np.array_equal(np.asarray(valsN[i]).view(np.int64), np.asarray(vals1[i]).view(np.int64))):
            raise WrongAnswer("device pool over %d devices: node %d differs from the single engine's" % (ndev, i))
    el = sum(per) / len(per)
    print(json.dumps({"value": len(nodes) / el, "unit": "LP relaxations/s", "members": pool.size, "devices": devs, "scaling": "strong",
                      "per_call_us": [round(1e6 * x) for x in per], "outcomes_checked": "every node of the last call == the single engine's compact outcome",
                      "note": "jslp_pool_relax_batch_watched_pinned over the visible devices (one engine + host thread + stream each, root fan-out by peer copy); "
                              "run in a child process under a time limit"}))
    pool.close()
    t.close()


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--pool-devices-leg":  # (the relaxation legs' child process: see pool_devices_leg)
        return pool_devices_leg(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lp-size", dest="n", type=int, default=2000, help="variables = constraints of the dense LP (2000 = config 3)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-pivots", type=int, default=3000)
    ap.add_argument("--no-relaxations", action="store_true")
    ap.add_argument("--only-relaxations", action="store_true", help="with --full, profiling runs: skip the dense-LP legs")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the other dense-LP legs (sustained, cycle check on, 3b, streaming instance)")
    ap.add_argument("--sustain-s", type=float, default=6.0, help="seconds of back-to-back headline solves after the timed steps (0 = off)")
    ap.add_argument("--no-dropin", action="store_true", help="skip the end-to-end Solve() leg through the reference host (node)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one computed (result + tableau) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the answer checks, the other legs and configurations, and the CPU baselines (the --no-* / --only-* options trim it)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.only_relaxations and not args.full:
        ap.error("--only-relaxations selects legs of the full run: add --full")
    if args.dump_outputs and args.only_relaxations:
        ap.error("--dump-outputs writes the dense-LP headline's outputs: it cannot be combined with --only-relaxations")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))

    import numpy as np
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d rank(s)" % (args.gpus, world))
    # one rank per GPU over RCCL.  JSLP_BENCH_BACKEND=gloo (tests only) lets several ranks share the one GPU of the
    # test box so that the N > 1 code path of this file can be exercised there.
    backend = os.environ.get("JSLP_BENCH_BACKEND", "nccl")
    device_index = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(device_index)
    red_device = "cuda" if backend == "nccl" else "cpu"
    if world > 1:
        if backend == "nccl":
            if torch.cuda.device_count() < world:
                raise SystemExit("bench.py: --gpus %d over RCCL needs %d visible GPUs, found %d" % (world, world, torch.cuda.device_count()))
            dist.init_process_group("nccl", device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group(backend)
        if dist.get_world_size() != args.gpus or dist.get_backend() != backend:
            raise SystemExit("bench.py: process group is %s x %d, wanted %s x %d" % (dist.get_backend(), dist.get_world_size(), backend, args.gpus))

    dropin = None
    if args.full and rank == 0 and world == 1 and not args.no_dropin and not args.only_relaxations:
        dropin = dropin_leg(with_cpu=not args.no_cpu_baseline)  # (a child process, before this one creates its HIP context)

    from jslpsolver_amd import _capi, generators
    from jslpsolver_amd.engine import Tableau, pivot_digest

    lib = _capi.load_hip()

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def reduce_ranks(x, op):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=red_device)
        dist.all_reduce(t, op=op)
        return float(t.item())

    def gather_ranks(x):
        """every rank's value, in rank order (a one-hot all-reduce: works on both backends)"""
        if world == 1:
            return [float(x)]
        t = torch.zeros(world, dtype=torch.float64, device=red_device)
        t[rank] = float(x)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return [float(v) for v in t.tolist()]

    max_over_ranks = lambda x: reduce_ranks(x, dist.ReduceOp.MAX)
    sum_over_ranks = lambda x: reduce_ranks(x, dist.ReduceOp.SUM)
    ctx = {"lib": lib, "device": device_index, "rank": rank, "world": world, "barrier": barrier, "max": max_over_ranks,
           "sum": sum_over_ranks, "gather": gather_ranks, "group": dist.group.WORLD if world > 1 else None}

    line = None
    n = args.n
    extra_legs = args.full and not args.no_extras  # (a plain run: the timed headline steps only)
    if not args.only_relaxations:
        # ---- workload: config 3a ------------------------------------------------------------------------
        m, vibr, vibc = generators.dense_resource_allocation_tableau(12345, n, n)
        H, W = m.shape
        t = Tableau(m, vibr, vibc, device=device_index, lib=lib)
        t.save()  # device-resident copy of the initial tableau: every step restarts from it without touching PCIe

        def timed_steps(check_cycles, warmup, steps):
            """W untimed + K timed steps bracketed by barrier + synchronize, max over ranks; the dominant kernel is
            event-timed inside the SAME steps (HIP events on the engine's stream)"""
            import gc
            res = None
            for _ in range(warmup):
                t.restore()
                res = t.simplex(check_cycles=check_cycles)
            gc.collect()
            gc.disable()  # keep CPython's cyclic collector out of the timed region (re-enabled right after it)
            t.set_timing(True)
            barrier()
            t0 = time.perf_counter()
            pivots = 0
            for _ in range(steps):
                t.restore()
                res = t.simplex(check_cycles=check_cycles)
                pivots += res.pivots_phase1 + max(res.pivots_phase2, 0)
            barrier()
            elapsed = max_over_ranks(time.perf_counter() - t0)
            kern_ms, launches, _total_ms = t.get_timing()
            t.set_timing(False)
            gc.enable()
            return res, pivots, elapsed, kern_ms, launches

        res, pivots, elapsed, kern_ms, launches = timed_steps(False, args.warmup, args.steps)
        dumped = None
        if args.dump_outputs and rank == 0:
            dumped = dump_outputs(args.dump_outputs, t, res)  # (before verify() below hands the tableau over again)
        total_pivots = sum_over_ranks(float(pivots))
        value = total_pivots / elapsed
        pivots_per_solve = res.pivots_phase1 + max(res.pivots_phase2, 0)
        path_used = t.last_path()
        evaluation = t.evaluation

        def verify(check_cycles, want_digest, what):
            """the answer of the path that was just timed: a fresh hand-over (new pivot trace), one solve, the digest"""
            t.upload(m, vibr, vibc)
            t.save()
            r = t.simplex(check_cycles=check_cycles)
            got = pivot_digest(t.pivot_trace())
            if want_digest is not None and got != want_digest:
                raise WrongAnswer("%s: pivot digest %s, the reference's is %s" % (what, got, want_digest))
            if not (r.feasible and r.optimal):
                raise WrongAnswer("%s: not solved to optimality" % what)
            return got

        digest = verify(False, DIGEST_3A.get(n), "config 3a (%d x %d), cycle check off" % (H, W)) if args.full else None

        # ---- roofline of the dominant kernel, from the timed steps themselves ---------------------------------------
        # unit of work = one pivot = 16*H*W algorithmic bytes; the register-resident kernel runs all pivots of
        # a solve in ONE launch, so its per-unit time is (event-timed launch duration) / pivots
        bytes_per_unit = 16.0 * H * W
        kernel_name = {"resident": "k_simplex_resident", "fused": "k_pivot_fused", "select+update": "k_update",
                       "workgroup": "k_simplex_wg"}.get(path_used, path_used)
        roofline = None
        if rank == 0:
            avg_s = (kern_ms / 1e3) / max(launches, 1)
            achieved = bytes_per_unit / avg_s if launches else 0.0
            traffic, traffic_note = pmc_traffic("pivots", kernel_name, bytes_per_unit)
            rate = 1.0 / avg_s if launches else 0.0
            if path_used == "resident":
                # register-resident: the HBM roofline is not the bound (see resident_latency_floor); the fraction on algorithmic
                # bytes stays as a figure of merit against a streaming implementation, the real HBM use comes from the PMC passes
                # round 6 (VERDICT r05, (d) caveat): the TOP-LEVEL figures are SURVEY.md 8(d)'s -- algorithmic bytes per pivot / measured kernel time
                # per pivot against the HBM peak -- as the contract of this line says; the fraction exceeds 1 because this kernel does the work without
                # streaming the tableau (its real HBM use is `traffic`, from the PMC passes).  The on-chip latency floor it is priced against -- what
                # actually bounds it -- is the `latency_floor` sub-object (round 5's top level).
                fl = resident_latency_floor(H, W)
                roofline = {"bound": "hbm", "kernel": kernel_name, "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                            "frac": achieved / HBM_PEAK, "avg_unit_us": avg_s * 1e6,
                            "frac_note": "> 1: the register-resident kernel keeps the tableau in the chip's vector registers for the whole solve -- the 16*H*W algorithmic "
                                         "bytes of a pivot never cross HBM (traffic = what does); see latency_floor for what bounds it",
                            "latency_floor": {"bound": "on-chip sync latency", "achieved": rate, "peak": 1e6 / fl["floor_us"], "unit": "pivots/s (one kernel, one tableau)",
                                              "frac": fl["floor_us"] / (avg_s * 1e6) if launches else None, "floor_model": fl}}
            else:
                roofline = {"bound": "hbm", "kernel": kernel_name, "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                            "frac": achieved / HBM_PEAK, "avg_unit_us": avg_s * 1e6}
            roofline.update({
                "traffic": traffic, "traffic_source": traffic_note, "units": launches,
                "unit_of_work": "one pivot", "timed_in": "the %d timed steps (HIP events on the engine's stream)" % args.steps,
                "algorithmic": {"bytes_per_unit": bytes_per_unit, "gb_s": achieved / 1e9, "frac_of_hbm_peak": achieved / HBM_PEAK,
                                "whole_step_frac": (bytes_per_unit * value / max(world, 1)) / HBM_PEAK,
                                "note": "16*H*W bytes per pivot (SURVEY.md 8d) / measured kernel time per pivot: what a streaming implementation would "
                                        "have to sustain to match; may exceed 1.0 for the register-resident kernel, which does not stream"},
                "hbm": {"bytes_per_unit": traffic, "gb_s": (traffic / avg_s / 1e9) if traffic else None,
                        "frac_of_hbm_peak": (traffic / avg_s / HBM_PEAK) if traffic else None,
                        "note": "PMC FETCH_SIZE + WRITE_SIZE of the same kernel on the same workload (separate rocprofv3 passes, committed summary)"},
                # the issue budget: vector instructions one wave issues per pivot against the 32 that are the update itself
                "issue": pmc_sq("pivots", kernel_name)})

        extras = {}
        if extra_legs and rank == 0 and args.sustain_s > 0:
            # the timed region above is ~1 s: a few more seconds of the same solves back to back (also what a 5 s sampler of GPU
            # activity gets to see); same answer checked by the digest above
            t.restore(); t.simplex(check_cycles=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter(); n_s = 0; piv_s = 0
            while time.perf_counter() - t0 < args.sustain_s:
                t.restore()
                r_s = t.simplex(check_cycles=False)
                piv_s += r_s.pivots_phase1 + max(r_s.pivots_phase2, 0)
                n_s += 1
            el_s = time.perf_counter() - t0
            extras["sustained"] = {"solves": n_s, "seconds": el_s, "value": piv_s / el_s, "unit": "pivots/s",
                                   "note": "the headline workload repeated for ~%.0f s on rank 0, restore + simplex per solve, wall clock" % args.sustain_s}
        if extra_legs:
            # ---- the reference's DEFAULT: checkForCycles on (model.ts:73; simplex.ts:415-440 after every selection) ----------
            # (every rank runs it: the timed region is bracketed by the same barriers; rank 0 reports its own replica)
            k2 = max(1, min(args.steps, 3))
            r2, piv2, el2, km2, ln2 = timed_steps(True, 1, k2)
            d2 = verify(True, DIGEST_3A.get(n), "config 3a, cycle check on (the reference's default)")
            extras["cycle_check_on"] = {"workload": "config 3a with options.exitOnCycles = true (the reference's default, src/model.ts:73)",
                                        "value": sum_over_ranks(float(piv2)) / el2, "unit": "pivots/s", "steps": k2, "ms_per_step": 1e3 * el2 / k2,
                                        "pivot_digest": d2, "kernel": t.last_path(),
                                        # (same two figures as the headline's `roofline` object, for this leg's own event-timed pivots)
                                        "latency_floor_frac": (resident_latency_floor(H, W)["floor_us"] / ((km2 * 1e3) / max(ln2, 1))) if (ln2 and t.last_path() == "resident") else None,
                                        "algorithmic_frac_of_hbm_peak": (bytes_per_unit / ((km2 / 1e3) / max(ln2, 1))) / HBM_PEAK if ln2 else None}
            # the register-resident kernels must not have been rolled back / handed on behind the numbers above
            hc = t.get_counters()
            if hc["resident_aborts"] or hc["resident_handovers"]:
                raise WrongAnswer("resident kernel health: %s (a rolled-back launch times the streaming fallback)" % {k: hc[k] for k in ("resident_aborts", "resident_handovers", "resident_launches")})
            extras["resident_health"] = {k: hc[k] for k in ("resident_launches", "resident_aborts", "resident_handovers", "resident_fetch_retries")}
        t.close()

        # ---- the other config-3 instance (3b: generateRandomLP, every pivot is a phase-1 pivot; ends infeasible) -------------
        if rank == 0 and extra_legs:
            m1, vibr1, vibc1, _op = generators.dense_random_lp_tableau(12345, n, n)
            t1 = Tableau(m1, vibr1, vibc1, device=device_index, lib=lib)
            t1.save()
            t1.simplex(check_cycles=False)
            reps1 = max(1, min(args.steps, 3))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps1):
                t1.restore()
                r1 = t1.simplex(check_cycles=False)
            dt = (time.perf_counter() - t0) / reps1
            d1 = pivot_digest(t1.pivot_trace()[-r1.pivots_phase1:])
            if DIGEST_3B.get(n) is not None and (d1 != DIGEST_3B[n] or r1.feasible):
                raise WrongAnswer("config 3b: digest %s feasible %s, the reference: %s infeasible" % (d1, bool(r1.feasible), DIGEST_3B[n]))
            extras["phase1_instance"] = {"workload": "config 3b: generateRandomLP(seed 12345, %d x %d, density 1.0), phase 1 only" % (n, n),
                                         "pivots": r1.pivots_phase1, "feasible": bool(r1.feasible), "pivots_per_s": r1.pivots_phase1 / dt,
                                         "pivot_digest": d1, "kernel": t1.last_path()}
            t1.close()

        # ---- the STREAMING path at a size that takes it by default (round 5): 5001 x 3001 does not fit the chip's vector registers, so the
        #      default policy runs one k_pivot_fused<2> launch per pivot -- 16 x H x W algorithmic bytes each: the kernel north_star's
        #      ">= 40 % of the HBM roofline" literally describes.  One solve (30 844 pivots), checked against the instance's known answer
        #      (tests/golden/stress_expect.json: data, written by tests/golden/gen_stress_expect.py), kernel time from HIP events per launch.
        if rank == 0 and extra_legs and n >= 2000:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import known_answers as KA
            # round 6: the instance is the reference's OWN golden at this shape (generateResourceAllocation(12345, 3000 vars, 5000 constraints),
            # tests/golden/wide/tall_RA_3000x5000: 32 645 pivots recorded from oracle/_ref), and the solve runs TWICE from the saved tableau: once
            # with a HIP event pair around every launch (the kernel's own rate), once without (the whole-solve rate: round 5 took both from one
            # event-timed solve and charged the events' serialisation to the launch loop -- VERDICT r05 weak #4 read that as a 12 % launch tax)
            ns_, ms_ = 3000, 5000
            want_s = KA.expected_dense("ra", ns_, ms_)
            As, vr_s, vc_s = generators.dense_resource_allocation_tableau(12345, ns_, ms_)
            ts_ = Tableau(As, vr_s, vc_s, device=device_index, lib=lib)
            ts_.save()
            ts_.set_timing(True)
            torch.cuda.synchronize()
            rs_ = ts_.simplex(check_cycles=False)
            k_ms, k_launches, _tot = ts_.get_timing()
            ts_.set_timing(False)
            sig = KA.solve_signature(ts_, rs_, pivot_digest)
            cs_ = ts_.get_counters()
            path_s = ts_.last_path()
            if want_s is None or (sig["pivots"], sig["digest"], sig["final_sha"]) != (want_s["pivots"], want_s["digest"], want_s["final_sha"]):
                raise WrongAnswer("streaming instance 5001x3001: %s, the reference's golden %s" % ({k: sig[k] for k in ("pivots", "digest")}, want_s and {k: want_s[k] for k in ("pivots", "digest")}))
            ts_.restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rs2_ = ts_.simplex(check_cycles=False)
            wall_s = time.perf_counter() - t0
            sig2 = KA.solve_signature(ts_, rs2_, pivot_digest)
            ts_.close()
            if (sig2["pivots"], sig2["digest"], sig2["final_sha"]) != (want_s["pivots"], want_s["digest"], want_s["final_sha"]):
                raise WrongAnswer("streaming instance 5001x3001, second solve: %s" % {k: sig2[k] for k in ("pivots", "digest")})
            bytes_unit = 16.0 * As.shape[0] * As.shape[1]
            extras["streaming_instance"] = {
                "workload": "generateResourceAllocation(seed 12345, 3000 vars x 5000 constraints): 5001x3001 fp64 tableau, beyond the register file, DEFAULT policy, cycle check off; "
                            "two solves from the saved tableau -- one with an event pair per launch (roofline), one without (whole_solve)",
                "kernel": "k_pivot_fused<2>" if path_s == "fused" else path_s, "path": path_s, "pivots": sig["pivots"], "pivot_digest": sig["digest"],
                "checked_against": "tests/golden/wide/tall_RA_3000x5000.json.gz: the reference's own run (pivot count, digest, sha256 of the final tableau), both solves",
                "resident_launches": cs_["resident_launches"],
                "roofline": {"bound": "hbm", "achieved": bytes_unit * k_launches / (k_ms * 1e-3) / 1e9 if k_ms > 0 else None, "peak": (HBM_PEAK / 1e9), "unit": "GB/s",
                             "frac": (bytes_unit * k_launches / (k_ms * 1e-3) / 1e9 / (HBM_PEAK / 1e9)) if k_ms > 0 else None,
                             "bytes_per_unit": bytes_unit, "unit_of_work": "one pivot = one launch", "launches_timed": int(k_launches),
                             "avg_launch_us": (1e3 * k_ms / k_launches) if k_launches else None,
                             "traffic": "profiles/r05_streaming_workload_rows.md: PMC FETCH_SIZE x2 + WRITE_SIZE = 1.008 x algorithmic on this kernel at this shape"},
                "whole_solve": {"pivots_per_s": sig["pivots"] / wall_s, "seconds": wall_s,
                                "frac_of_hbm_roofline": bytes_unit * sig["pivots"] / wall_s / 1e9 / (HBM_PEAK / 1e9),
                                "note": "host clock around the second simplex() (no timing events): launch gaps and the chunked launch loop's state polls included"}}

        if rank == 0:
            line = {
                "metric": "simplex pivots/sec", "value": value, "unit": "pivots/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / max(args.steps, 1), "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
                "config": {"workload": "config 3a: generateResourceAllocation(seed 12345, %d vars x %d constraints, density 1.0), "
                                       "%dx%d fp64 tableau, %d pivots per solve, cycle check off; one replica per GPU"
                                       % (n, n, H, W, pivots_per_solve),
                           "result_evaluation": evaluation, "parallelism": "replicas%d" % world,
                           "rccl_ranks": world if (world > 1 and backend == "nccl") else 0},
                "roofline": roofline,
            }
            if args.full:
                line["config"].update({"pivot_digest": digest,
                                       "pivot_digest_checked_against": DIGEST_3A.get(n) and "SURVEY.md Appendix C (the reference's own trace)"})
            line.update(extras)
            if dumped is not None:
                line["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped, "of": "the last timed step"}
            if dropin is not None:
                line["dropin_js"] = dropin

    # ---- LP relaxations/sec: Monster_II (config 4) ----------------------------------------------------------------------
    relax = None
    if args.full and not args.no_relaxations:
        relax = relaxation_legs(ctx, args)
        if line is not None and relax is not None:
            line["relaxations"] = relax
        elif rank == 0 and relax is not None:
            line = {"metric": "LP relaxations/sec", "value": relax["value"], "unit": relax["unit"], "n_gpus": world, "relaxations": relax}

    # ---- CPU baselines last: the GPU legs above ran back to back -----------------------------------------------------
    if rank == 0 and line is not None:
        if args.full and not args.no_cpu_baseline and world == 1:
            if relax is not None:
                relax["cpu_baseline"] = cpu_relaxation_baseline()
                if relax["cpu_baseline"] and relax["cpu_baseline"].get("value"):
                    relax["speedup_vs_cpu_1_thread"] = relax["value"] / relax["cpu_baseline"]["value"]
                    if relax["cpu_baseline"].get("aggregate_value"):
                        relax["speedup_vs_cpu_all_cores"] = relax["value"] / relax["cpu_baseline"]["aggregate_value"]
            if not args.only_relaxations:
                line["cpu_baseline"] = cpu_baseline(n, args.cpu_sample_pivots)
                if line["cpu_baseline"] and line["cpu_baseline"].get("value"):
                    line["speedup_vs_cpu_baseline"] = line["value"] / line["cpu_baseline"]["value"]
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


def gated_bytes(c, W, n_idx, H_root, readback_per_node=None):
    """Algorithmic bytes of the counted relaxations: what restore + addCutConstraints + simplex + read-back have
    to move given what the reference's loops touch -- rows restored / appended (read + write a row), per pivot the
    selection reads (cost row, pivot column, RHS column), the pivot row (read + write) and the gated cells
    (simplex.ts:370-387: read + write), the index maps restored per relaxation, the read-back."""
    row = 16.0 * W
    return (row * (c["restored_rows"] + c["cut_rows"]) + c["pivots"] * (row + 8.0 * W) + 16.0 * c["height_sum"] * c["pivots"] / max(c["simplex_calls"], 1)
            + 16.0 * c["gated_cells"] + c["relaxations"] * 8.0 * (H_root + W + 2 * n_idx)
            + (12.0 * c["height_sum"] if readback_per_node is None else readback_per_node * c["relaxations"]))


def relaxation_legs(ctx, args, reps=16):
    """Config 4.
    (i)  throughput variant: the 151 cut lists the reference visits on Monster_II x reps, evaluated as independent nodes;
         rank r takes nodes r, r+world, ... (weak scaling: reps x 151 per rank, no collective in the data path);
    (ii) the same batch once more with the kernels' work counters on -> gated algorithmic bytes -> roofline fraction;
    (iii) ONE real tree: Solve(Monster_II) with speculative batches of 8 x world nodes sharded over the ranks, outcomes
         all-gathered (RCCL) -- strong scaling of the tree itself (~3.5x at 4, ~5.3x at 8 GPUs);
    (iv) N = 1 only: the batch of (i) through the engine's own device pool with 4 virtual devices on the one GPU."""
    import gzip
    import gc
    import numpy as np
    from jslpsolver_amd import Model, Solve
    from jslpsolver_amd.engine import DevicePool, Tableau
    lib, device, rank, world = ctx["lib"], ctx["device"], ctx["rank"], ctx["world"]
    barrier, max_over_ranks, sum_over_ranks = ctx["barrier"], ctx["max"], ctx["sum"]
    path = os.path.join(ROOT, "tests", "golden", "fixtures", "Monster_II.json.gz")
    if not os.path.exists(path):
        return None
    with gzip.open(path, "rt") as fh:
        g = json.load(fh)
    model = Model(g["model"])
    m, vibr, vibc = model.build_tableau()
    H, W = m.shape
    calls = g["simplexCalls"][1:]
    nodes = [c["cuts"] or [] for c in calls] * (reps * world)
    mine = nodes[rank::world]
    cap = H + 2 * len(model.integerVariables)
    t = Tableau(m, vibr, vibc, model.unrestricted, precision=model.precision, row_capacity=cap, device=device, lib=lib)
    t.applyCuts([], check_cycles=True)  # root relaxation
    t.save()
    packed = t.pack_cut_lists(mine)

    def check_outcomes(results, rhs, rows, which, what):
        """every node's outcome against the reference's own (sha256 of RHS column + row map per relaxation)"""
        for i, k in enumerate(which):
            call = calls[k % len(calls)]
            h = results[i].height
            sha = hashlib.sha256(np.ascontiguousarray(rhs[i, :h]).tobytes() + np.ascontiguousarray(rows[i, :h]).tobytes()).hexdigest()
            if h != call["height"] or bool(results[i].feasible) != call["feasible"] or sha != call["rhsSha"]:
                raise WrongAnswer("%s: node %d differs from the reference's relaxation outcome" % (what, k))

    def timed_calls(fn, warm, calls_n):
        per_call = []
        for _ in range(warm):
            fn()
        gc.collect()
        gc.disable()  # a generation-2 pass of CPython's collector (~6 ms over the model's dicts) otherwise lands in a random call
        barrier()
        t0 = time.perf_counter()
        out = None
        for _ in range(calls_n):
            t1 = time.perf_counter()
            out = fn()
            per_call.append(time.perf_counter() - t1)
        barrier()
        el = max_over_ranks(time.perf_counter() - t0) / calls_n
        gc.enable()
        return out, el, per_call

    # (i) the first call allocates the slots and restores them in full; ~10-15 ms into a new burst of work one call stalls
    # for ~6 ms (clock ramp): warm up past that
    fn = lambda: t.applyCutsBatch(None, check_cycles=True, packed=packed, copy=False)
    (results, rhs, rows), el, per_call = timed_calls(fn, 25, 10)
    if rank == 0:
        check_outcomes(results, rhs, rows, list(range(rank, len(nodes), world)), "relaxation batch")
    total = sum_over_ranks(float(len(mine)))
    per_rank_rate = ctx["gather"](len(mine) / (sum(per_call) / len(per_call)))  # every rank's own clock, before the max over ranks
    piv = sum_over_ranks(float(sum(results[i].pivots_phase1 + max(results[i].pivots_phase2, 0) for i in range(len(mine)))))
    # the same batch with the compact read-back (jslp_engine_relax_batch_watched_pinned): per node only rowByVarIndex / the RHS
    # cell of the integer variables, which is what a host walking the tree reads between relaxations (mip-utils.ts:43-61, 100-126)
    rhs, rows = np.array(rhs), np.array(rows)  # (views of the pinned buffer the next calls overwrite)
    ints = [int(v) for v in model.integer_index_array]
    t.set_watched_variables(ints)
    fnw = lambda: t.applyCutsBatchWatched(None, check_cycles=True, packed=packed, copy=False)
    (res_w, rows_w, vals_w), el_w, per_call_w = timed_calls(fnw, 5, 10)
    rows_w_keep, vals_w_keep = np.array(rows_w), np.array(vals_w)  # (the pool leg below compares with them)
    res_w = [res_w[i] for i in range(len(mine))]
    if rank == 0:  # against the full read-back checked above, node by node
        ints_a = np.asarray(ints)
        for i in range(len(mine)):
            h = results[i].height
            row_of = np.full(int(max(rows[i, :h].max(), ints_a.max())) + 1, -1, dtype=np.int64)
            row_of[rows[i, 1:h]] = np.arange(1, h)
            r = row_of[ints_a]
            want_v = np.where(r > 0, rhs[i, np.maximum(r, 0)], 0.0)
            if (res_w[i].height != h or res_w[i].feasible != results[i].feasible or not np.array_equal(rows_w[i], r.astype(np.int32))
                    or not np.array_equal(vals_w[i].view(np.int64), want_v.view(np.int64))):
                raise WrongAnswer("compact read-back: node %d differs from the full read-back" % i)
    full_bytes = 12.0 * H  # per node, before the cut rows (RHS column 8 B + row map 4 B per row)
    out = {"value": total / el, "unit": "LP relaxations/s", "nodes": int(total), "pivots": int(piv), "seconds": el,
           "read_back": "full: every node's RHS column + row map land in pinned host memory (%.1f KB per node, written by the kernel itself); "
                        "this leg is bound by the PCIe link, not by the GPU: %.1f GB/s of outcomes" % (full_bytes / 1e3, sum(results[i].height for i in range(len(mine))) * 12.0 / el / 1e9),
           "compact_read_back": {"value": total / el_w, "unit": "LP relaxations/s", "seconds": el_w, "bytes_per_node": 12 * len(ints),
                                 "per_call_us": [round(1e6 * x) for x in per_call_w],
                                 "note": "jslp_engine_relax_batch_watched_pinned: rowByVarIndex + RHS cell of the %d integer variables per node; "
                                         "checked node by node against the full read-back" % len(ints)},
           "calls_averaged": 10, "per_call_us": [round(1e6 * x) for x in per_call], "scaling": "weak",
           "per_rank_relaxations_per_s": per_rank_rate,
           "outcomes_checked": "sha256(RHS column + row map) of every node of the last call == the reference's (rank 0's share)",
           "workload": "config 4: Monster_II (935x925 root, 112 ints), the reference's 151 visited cut lists x%d as one batch of "
                       "independent nodes per rank, sharded round-robin over %d rank(s)" % (reps, world)}
    # (i-b) round 5: the LATENCY of a small batch -- what every dependent batch of a real tree waits for (a speculative batch is <= 16
    #       nodes: one 1024-thread workgroup per node, each on its own CU): wall time of one call with the compact read-back for the first
    #       1 / 8 / 16 visited nodes of the reference's tree, median of 30 calls
    if rank == 0:
        lat = {}
        for n_small in (1, 8, 16):
            sub = mine[3:3 + n_small]  # (this rank's share -- what res_w / rows_w_keep hold; at N = 1 a dive of the reference's tree: nodes 3.. carry 2-5 cuts each)
            packed_s = t.pack_cut_lists(sub)
            fns = lambda: t.applyCutsBatchWatched(None, check_cycles=True, packed=packed_s, copy=False)
            for _ in range(5):
                fns()
            ts = []
            for _ in range(30):
                t1 = time.perf_counter()
                r_s, rows_s, vals_s = fns()
                ts.append(time.perf_counter() - t1)
            for i in range(n_small):  # against the big batch's (already verified) compact outcome of the same node
                if r_s[i].height != res_w[3 + i].height or not np.array_equal(np.array(rows_s[i]), rows_w_keep[3 + i]) or not np.array_equal(np.array(vals_s[i]).view(np.int64), vals_w_keep[3 + i].view(np.int64)):
                    raise WrongAnswer("small batch of %d: node %d differs from the verified outcome" % (n_small, i))
            ts.sort()
            piv_s = sum(r_s[i].pivots_phase1 + max(r_s[i].pivots_phase2, 0) for i in range(n_small))
            lat[str(n_small)] = {"us_per_call_median": 1e6 * ts[len(ts) // 2], "us_per_call_min": 1e6 * ts[0], "us_per_node": 1e6 * ts[len(ts) // 2] / n_small, "pivots": int(piv_s)}
        out["small_batch_latency"] = dict(lat, note="one jslp_engine_relax_batch_watched_pinned call (upload of the cut lists, one launch of k_node_lds<1024>, "
                                                    "compact read-back, one synchronisation), host clock; what one dependent batch of a speculative tree costs")
    # (ii) gated algorithmic bytes from the kernels' own counters (a separate, untimed pass over the same batch)
    if rank == 0:
        t.set_counting(True)
        fn()
        c = t.get_counters()
        t.set_counting(False)
        n_idx = W + 2 * cap + 2
        alg = gated_bytes(c, W, n_idx, H)
        per_node = alg / max(c["relaxations"], 1)
        node_kernel = "k_node_queue"
        traffic, note = pmc_traffic("relaxations", node_kernel, per_node)
        dense = 16.0 * H * W * (c["relaxations"] + c["pivots"])  # SURVEY.md 8d's dense figure, for reference only
        # the kernel's own rate: the compact leg (the full one waits for the PCIe link), with that leg's read-back bytes
        per_node_kernel = gated_bytes(c, W, n_idx, H, readback_per_node=12.0 * len(ints)) / max(c["relaxations"], 1)
        out["roofline_kernel_bound_leg"] = {"leg": "compact_read_back", "achieved": per_node_kernel * len(mine) / el_w / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                                            "frac": per_node_kernel * len(mine) / el_w / HBM_PEAK, "bytes_per_unit": per_node_kernel}
        rate_rank0 = len(mine) / el
        out["roofline"] = {"bound": "hbm", "kernel": node_kernel, "achieved": per_node * rate_rank0 / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                           "frac": per_node * rate_rank0 / HBM_PEAK, "bytes_per_unit": per_node, "unit_of_work": "one LP relaxation",
                           "traffic": traffic, "traffic_source": note,
                           "traffic_over_algorithmic": (traffic / per_node) if traffic else None,
                           "issue": pmc_sq("relaxations", node_kernel),
                           "counters": c, "dense_bytes_per_unit_survey_8d": dense / max(c["relaxations"], 1),
                           "note": "algorithmic bytes = what restore + addCutConstraints + simplex + read-back must move for the cells the "
                                   "reference's own loops touch (gated rows x live pivot-row columns, counted by the kernels: "
                                   "jslp_work_counters); SURVEY.md 8d's dense 16*H*W per restore and per pivot would be %.1fx that"
                                   % (dense / max(alg, 1.0))}
    # (v) round 6 STRONG scaling of the batch: the SAME fixed batch (151 x reps nodes, whatever N) split round-robin over
    #     the ranks by sharding.evaluate_nodes_sharded_watched -- one engine call per rank on its share, then the all-gather of the COMPACT
    #     outcomes (RCCL; at N = 1 a one-rank group, so that the N = 1 figure walks the same code) and the ONE device-to-host copy of the
    #     gathered block, all INSIDE the timed region; every rank checks every node's outcome (its own engine's verified compact outcomes
    #     of the same cut lists: rank 0's were checked against the reference above, so a disagreement between GPUs cannot pass)
    try:
        import torch.distributed as dist
        from jslpsolver_amd.sharding import EXCHANGE_STATS as XS, evaluate_nodes_sharded_watched
        own_group = False
        sgroup = ctx["group"]
        if world == 1 and not dist.is_initialized():
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            dist.init_process_group(os.environ.get("JSLP_BENCH_BACKEND", "nccl"), init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
            own_group = True
            sgroup = dist.group.WORLD
        fixed = [c["cuts"] or [] for c in calls] * reps
        packed_fixed = t.pack_cut_lists(fixed[rank::world])
        # this rank's table of verified compact outcomes by cut list (mine[i] is cut list (rank + i * world) % len(calls): every residue occurs)
        by_call = {}
        for i in range(len(mine)):
            by_call.setdefault((rank + i * world) % len(calls), i)
        fns_ = lambda: evaluate_nodes_sharded_watched(t, fixed, True, sgroup, packed_mine=packed_fixed, copy=False)  # (views of the pinned landing buffer: checked below, before any further exchange)
        for _ in range(25):  # (the first call creates the communicator: seconds; and, as for the legs above, the few-ms stall ~3-15 ms into a new burst of work)
            fns_()
        for k in XS:
            XS[k] = 0 * XS[k]
        outs, el_s, per_s = timed_calls(fns_, 0, 20)
        xs = dict(XS)
        # (the rate is taken over the MEDIAN call: one call in a few hundred stalls for milliseconds inside the runtime -- 10.4 ms among ten 545 us calls in one of the
        #  round's runs, profiles/r06_tree_latency.md -- and a mean over ten or twenty calls then reports the stall, not the path; mean, max and a health note beside it)
        srt_s = sorted(per_s)
        med_s = max_over_ranks(srt_s[len(srt_s) // 2])
        for k in range(len(fixed)):
            i = by_call[k % len(calls)]
            r_k = outs.result(k)
            if (r_k.height != res_w[i].height or bool(r_k.feasible) != bool(res_w[i].feasible) or not np.array_equal(outs.watched_rows(k), rows_w_keep[i])
                    or not np.array_equal(outs.watched_values(k).view(np.int64), vals_w_keep[i].view(np.int64))):
                raise WrongAnswer("sharded batch: node %d differs from this rank's verified outcome of the same cut list (rank %d)" % (k, rank))
        calls_x = max(xs["calls"], 1)
        out["sharded_batch"] = {"value": len(fixed) / med_s, "unit": "LP relaxations/s", "scaling": "strong", "nodes": len(fixed), "seconds": med_s,
                                "value_over_mean_call": len(fixed) / el_s, "mean_call_seconds": el_s, "max_call_us": round(1e6 * srt_s[-1]),
                                "health": "ok" if srt_s[-1] < 10 * med_s else "OUTLIER: the slowest of %d calls took %.2f ms against a median of %.3f ms (rank 0)" % (len(per_s), 1e3 * srt_s[-1], 1e3 * med_s),
                                "exchange_ms": 1e3 * xs["seconds"] / calls_x, "bytes_per_rank": xs["bytes"] / calls_x,
                                "per_call_us": [round(1e6 * x) for x in per_s], "ranks": world,
                                "workload": "config 4: ONE fixed batch of %d Monster_II nodes (151 cut lists x%d) split round-robin over %d rank(s): "
                                            "per rank one jslp_engine_relax_batch_watched_device call on its share, then all_gather_into_tensor of the "
                                            "compact outcomes (%s) + one D2H of the gathered block, inside the timed region; every rank verified every node"
                                            % (len(fixed), reps, world, dist.get_backend(sgroup))}
        if own_group:
            dist.destroy_process_group()
        if world > 1:
            #  at N > 1 the leg that PAYS for its communication is the relaxation figure: the weak-scaling leg (independent batches per rank, no
            # exchange in the timed region) moves into `weak_scaling`
            out["weak_scaling"] = {k: out[k] for k in ("value", "unit", "nodes", "pivots", "seconds", "scaling", "per_rank_relaxations_per_s") if k in out}
            out["value"], out["nodes"], out["seconds"], out["scaling"] = out["sharded_batch"]["value"], out["sharded_batch"]["nodes"], out["sharded_batch"]["seconds"], "strong"
            out["value_leg"] = "sharded_batch: ONE fixed batch split over the ranks, all-gather of the compact outcomes + D2H inside the timed region (the per-rank independent batches: weak_scaling)"
    except WrongAnswer:
        raise
    except Exception as e:  # (never lose the whole line to this leg)
        out["sharded_batch"] = {"value": None, "error": repr(e)[:300]}
    # (iv) the engine's own device pool (single process): 4 virtual devices on this GPU
    if world == 1:
        pool = DevicePool(t, [device] * 4)
        fnp = lambda: pool.applyCutsBatch(None, check_cycles=True, packed=packed, copy=False)
        (r4, rhs4, rows4), el4, per4 = timed_calls(fnp, 10, 10)
        check_outcomes(r4, rhs4, rows4, list(range(len(nodes))), "device pool batch")
        out["pool_virtual4"] = {"value": len(mine) / el4, "unit": "LP relaxations/s", "members": pool.size,
                                "note": "jslp_pool_relax_batch_pinned: the same batch split over 4 engines (own stream + host thread each) on "
                                        "the one visible GPU; on a multi-GPU node the members sit on different devices and the root is "
                                        "fanned out with hipMemcpyPeerAsync", "per_call_us": [round(1e6 * x) for x in per4]}
        # the same over the pool's compact read-back (round 4: jslp_pool_relax_batch_watched_pinned), checked node by node against the
        # single engine's compact outcomes above
        pool.set_watched_variables(ints)
        fnpw = lambda: pool.applyCutsBatchWatched(None, check_cycles=True, packed=packed, copy=False)
        (r4w, rows4w, vals4w), el4w, per4w = timed_calls(fnpw, 5, 10)
        for i in range(len(mine)):
            if (r4w[i].height != res_w[i].height or r4w[i].feasible != res_w[i].feasible or not np.array_equal(rows4w[i], rows_w_keep[i])
                    or not np.array_equal(vals4w[i].view(np.int64), vals_w_keep[i].view(np.int64))):
                raise WrongAnswer("device pool, compact read-back: node %d differs from the single engine's" % i)
        out["pool_virtual4"]["compact"] = {"value": len(mine) / el4w, "unit": "LP relaxations/s", "per_call_us": [round(1e6 * x) for x in per4w],
                                           "vs_single_engine_compact": (len(mine) / el4w) / (len(mine) / el_w)}
        pool.close()
        #  ... and the same in-process pool over the REAL devices when this process sees more than one (the driver's 8-GPU node; the
        # gpurun box has one): the primary's saved root fanned out with hipMemcpyPeerAsync, the fixed batch split over the members -- strong scaling
        # inside one process, no collective.  Never run on hardware by the builder: it runs in a child process under a time limit (`--pool-devices-leg`),
        # so that a fault or a hang in it costs this leg, not the line.
        try:
            import subprocess
            import torch
            ndev = min(torch.cuda.device_count(), 8)
            if ndev >= 2:
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--pool-devices-leg", str(device), str(ndev), str(reps)],
                                       capture_output=True, text=True, timeout=240)
                lines = [ln for ln in child.stdout.splitlines() if ln.startswith("{")]
                if child.returncode == 0 and lines:
                    out["pool_devices"] = json.loads(lines[-1])
                    out["pool_devices"]["vs_single_engine_compact"] = out["pool_devices"]["value"] / (len(mine) / el_w)
                else:
                    out["pool_devices"] = {"value": None, "error": ("rc %d: " % child.returncode) + (child.stderr or child.stdout)[-300:]}
        except Exception as e:
            out["pool_devices"] = {"value": None, "error": repr(e)[:300]}
    t.close()
    # (iii) strong scaling: one real branch-and-bound tree, speculative batches of 8 x world nodes sharded over the ranks
    group = ctx["group"]
    spec = 8 * world
    want = {k: (float(v) if isinstance(v, (int, float)) and not isinstance(v, bool) else v) for k, v in g["result"].items()}

    def solve_tree():
        return Solve(g["model"], full=True, lib=lib, device=device, speculate=spec, group=group)

    from jslpsolver_amd.branch_and_cut import EVAL_STATS
    from jslpsolver_amd.sharding import EXCHANGE_STATS
    for _ in range(3):
        solve_tree()
    for st in (EVAL_STATS, EXCHANGE_STATS):
        for k in st:
            st[k] = 0 * st[k]
    N_TREE = 15
    sol, el_tree, per_tree = timed_calls(solve_tree, 0, N_TREE)
    eval_ms = 1e3 * EVAL_STATS["seconds"] / N_TREE
    exch_ms = 1e3 * EXCHANGE_STATS["seconds"] / N_TREE
    srt = sorted(per_tree)
    med_tree, max_tree = srt[len(srt) // 2], srt[-1]
    if sol["iter"] != g["final"]["branchAndCutIterations"] or sol["result"].get("result") != want.get("result"):
        raise WrongAnswer("Monster_II tree: result %r after %d relaxations, the reference: %r after %d"
                          % (sol["result"].get("result"), sol["iter"], want.get("result"), g["final"]["branchAndCutIterations"]))
    out["tree"] = {"workload": "one solver.Solve(Monster_II): %d committed relaxations, speculative batches of %d nodes sharded over %d rank(s), "
                               "outcomes all-gathered (%s)" % (sol["iter"], spec, world, "RCCL" if (world > 1 and os.environ.get("JSLP_BENCH_BACKEND", "nccl") == "nccl") else ("gloo" if world > 1 else "no exchange at N = 1")),
                   "scaling": "strong", "ms_per_solve": 1e3 * el_tree, "solves_per_s": 1.0 / el_tree, "committed_relaxations_per_s": sol["iter"] / el_tree,
                   "result": sol["result"].get("result"), "result_checked": "result and relaxation count == the reference's (%s, %d)" % (want.get("result"), g["final"]["branchAndCutIterations"]),
                   "per_solve_ms": [round(1e3 * x, 2) for x in per_tree],
                   # round 6 (one solve of a committed round-5 line took 592 ms): median and max beside the mean, and a
                   # `health` note when a solve is an outlier -- profiles/r06_tree_latency.md: 2500 consecutive solves, max / median <= 1.61
                   "median_ms": 1e3 * med_tree, "max_ms": 1e3 * max_tree, "solves": N_TREE,
                   "health": ("OUTLIER: the slowest of %d solves took %.1f ms, %.1fx the median %.2f ms (rank 0's clock)" % (N_TREE, 1e3 * max_tree, max_tree / med_tree, 1e3 * med_tree))
                             if max_tree > 10 * med_tree else "ok (max / median = %.2f)" % (max_tree / med_tree),
                   # what shards and what does not (rank 0's clock): the evaluation share = the speculative batches (engine calls +
                   # exchange step); the rest = model parsing, upload, root LP, tree bookkeeping on one host thread
                   "eval_ms": eval_ms, "exchange_ms": exch_ms, "host_ms": 1e3 * el_tree - eval_ms,
                   # round 5: the exchange payload is COMPACT -- per node the 128-byte state record + row / RHS cell of the 112 integer
                   # variables (jslp_engine_relax_batch_watched_device) instead of the whole RHS column + row map (11.4 KB per node)
                   "exchange_bytes_per_batch_per_rank": (EXCHANGE_STATS["bytes"] / EXCHANGE_STATS["calls"]) if EXCHANGE_STATS["calls"] else 0,
                   "exchange_bytes_per_node": (128 + 12 * len(g["tableau"]["integerVarIndexes"])) if world > 1 else 0,
                   "node_outcome": "compact (integer variables' rows + values; the committed leaf re-evaluated with the full read-back)",
                   "eval_batches_per_solve": EVAL_STATS["batches"] / N_TREE, "eval_nodes_per_solve": EVAL_STATS["nodes"] / N_TREE, "includes": "model parsing, upload, root LP, the whole tree and the read-back (host logic in Python)",
                   "host": "python mirror of the reference host, no presolve (the drop-in is `dropin_js`: the reference's own host under node)"}
    return out if rank == 0 else None


def cpu_relaxation_baseline(seconds=4.0):
    """The reference itself on config 4 on this box's host cores: LP relaxations/s of solver.Solve(Monster_II) with one
    thread, and the aggregate of one such process per core (the generous CPU figure of SURVEY.md 8d)."""
    script = os.path.join(ROOT, "oracle", "ref_relax_rate.js")
    fixture = os.path.join(ROOT, "tests", "golden", "fixtures", "Monster_II.json.gz")
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "src", "solver.js")):
        return None

    def run(n_proc):
        procs = [subprocess.Popen(["node", script, fixture, str(seconds)], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                  stdin=subprocess.DEVNULL, text=True) for _ in range(n_proc)]
        rates = []
        for pr in procs:
            try:
                out, _ = pr.communicate(timeout=120)
                rates.append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["relaxations_per_sec"])
            except Exception:
                pr.kill()
        return rates

    try:
        one = run(1)
        cores = os.cpu_count() or 1
        many = run(cores)
        return {"value": one[0] if one else None, "unit": "LP relaxations/s", "cores": 1, "kind": "reference",
                "aggregate_value": sum(many) if many else None, "aggregate_processes": len(many),
                "sample": "solver.Solve(Monster_II) repeated for ~%.0f s per process after one warm-up (151 B&B relaxations + root + "
                          "final per solve), clock = Tableau.solve() only; aggregate = one independent node process per host core "
                          "(%d), all running concurrently" % (seconds, cores)}
    except Exception as e:
        return {"value": None, "unit": "LP relaxations/s", "cores": 1, "kind": "reference", "sample": "failed: %r" % (e,)}


if __name__ == "__main__":
    main()
