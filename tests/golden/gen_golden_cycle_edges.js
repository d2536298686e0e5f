// Golden vectors for cycles DETECTED AT THE HISTORY LENGTHS WHERE THE KERNELS' CHECK CHANGES CODE PATHS (TEST INFRASTRUCTURE; build
// container only):
//   python oracle/build_ref.py && node --max-old-space-size=8000 tests/golden/gen_golden_cycle_edges.js [instance name ...]
// (no name: every instance, one after the other; the large ones take minutes each under node -- run a few names per process, side by side).
// The instances are those of tests/cycle_edges.py (same names, same construction, key for key):
//   * `<small>_k<k>`: k FILLERS in front of a small cycling LP of gen_golden_cycles.js.  A filler is a constraint fc_i: {max: 1 + i % 3}
//     and a variable f_i: {fc_i: 1, obj: -+1e6}: the most attractive column once, one pivot, never again, its row zero in every other
//     column -- the small LP's own run follows k rows, k columns and k pivots later, and its hit lands at a history of k + start + 2 length
//     pairs: 127, 128, 129, 130 and beyond (the one-workgroup kernels' LDS history holds 128 pairs).
//   * `late_<small>_k<k>`: the dense block of gen_golden_late_cycle.js (generateResourceAllocation, seed 3, 1000 x 1000, as a minimisation),
//     k fillers in front, the small LP behind: hits at 4064 .. 4164 pairs (the lean register-resident kernel keeps 4096 pairs in LDS).
//   * `..._tall` / `..._wide`: the same with gen_golden_cycles.js `embed`'s zero-cost variables and constraints appended last, for the
//     <512,4,16> and <512,6,12> geometries.
// Recorded "lite" (tests/golden/cycle_edges/*.json.gz): the model is rebuilt at test time from the small golden + `meta`; matrixSha pins it.
"use strict";
const path = require("path");
const zlib = require("zlib"), fs = require("fs");
const { run, write, gen } = require("./gen_golden.js");
const solver = require(path.join(__dirname, "..", "..", "oracle", "_ref", "src", "solver.js")).default;

function rng(seed) { let s = seed >>> 0; return () => { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; return s / 4294967296; }; }
function smallModel(name) {
    return JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(__dirname, "cycles", name + ".json.gz"))).toString()).model;
}
function withFillers(model, k) {
    const cost = model.opType !== "max" ? -1e6 : 1e6;
    const big = { optimize: model.optimize, opType: model.opType, constraints: {}, variables: {} };
    for (let i = 0; i < k; i++) {
        big.constraints["fc_" + i] = { max: 1 + (i % 3) };
        const v = {};
        v["fc_" + i] = 1;
        v[model.optimize] = cost;
        big.variables["f_" + i] = v;
    }
    for (const c of Object.keys(model.constraints)) big.constraints[c] = model.constraints[c];
    for (const v of Object.keys(model.variables)) big.variables[v] = Object.assign({}, model.variables[v]);
    if (model.unrestricted) big.unrestricted = Object.assign({}, model.unrestricted);
    big.options = { presolve: false };
    return big;
}
function lateCycle(small, n, seed) {  // gen_golden_late_cycle.js
    const ra = gen.generateResourceAllocation({ seed, numVariables: n, numConstraints: n, density: 1.0 });
    const big = { optimize: "obj", opType: "min", constraints: {}, variables: {} };
    for (const k of Object.keys(ra.constraints)) big.constraints[k] = ra.constraints[k];
    for (const k of Object.keys(ra.variables)) {
        const v = Object.assign({}, ra.variables[k]);
        v.obj = -v[ra.optimize];
        delete v[ra.optimize];
        big.variables[k] = v;
    }
    for (const k of Object.keys(small.constraints)) big.constraints["z_" + k] = small.constraints[k];
    for (const k of Object.keys(small.variables)) {
        const v = {};
        for (const a of Object.keys(small.variables[k])) v[a === small.optimize ? "obj" : "z_" + a] = small.variables[k][a];
        big.variables["z_" + k] = v;
    }
    return big;
}
function embed(model, extraVars, extraCons, seed) {  // gen_golden_cycles.js
    const r = rng(seed);
    const big = JSON.parse(JSON.stringify(model));
    for (let i = 0; i < extraCons; i++) big.constraints["fc" + i] = { max: 100 + Math.floor(r() * 900) };
    for (let j = 0; j < extraVars; j++) {
        const v = {};
        for (let i = 0; i < extraCons; i++) v["fc" + i] = 1 + Math.floor(r() * 20);
        big.variables["f" + j] = v;
    }
    big.options = { presolve: false };
    return big;
}

const N = 1000, SEED = 3, TALL = [40, 500], WIDE = [500, 8];
const table = [];
const fill = (small, ks) => ks.forEach((k) => table.push({ name: small + "_k" + k, kind: "fill", small, k, n: 0, seed: 0, extra: null }));
const late = (small, k, extra, tag) => table.push({ name: "late_" + small + "_k" + k + (tag || ""), kind: "late", small, k, n: N, seed: SEED, extra: extra || null });
fill("deg_35358", [84, 85, 86, 87, 100, 110]);
fill("unr_3", [122, 123, 124, 125]);
fill("deg_233528", [103, 104]);
fill("deg_178868", [102, 103]);
for (const s of ["deg_292715", "deg_347708", "deg_233528", "deg_178868", "deg_398167", "deg_137788", "deg_35358"]) late(s, 650);
late("deg_35358", 600);
late("deg_35358", 700);
for (const s of ["deg_233528", "deg_178868", "deg_35358"]) late(s, 650, TALL, "_tall");
for (const s of ["deg_233528", "deg_178868", "deg_35358"]) late(s, 650, WIDE, "_wide");

const only = process.argv.slice(2);
for (const t of table) {
    if (only.length && !only.includes(t.name)) continue;
    const small = smallModel(t.small);
    let model = t.kind === "fill" ? withFillers(small, t.k) : withFillers(lateCycle(small, t.n, t.seed), t.k);
    if (t.extra) model = embed(model, t.extra[0], t.extra[1], 777);
    const out = run(model, true, true);
    out.model = null;
    out.messages = solver.lastSolvedModel.messages.slice();
    out.tableau.rows = out.tableau.cols = out.tableau.vals = null; out.tableau.variableIds = null; out.final.rhs = null;
    out.meta = { kind: "cycle_edge_" + t.kind, small: t.small, k: t.k, n: t.n, seed: t.seed, extra: t.extra };
    write(path.join(__dirname, "cycle_edges"), t.name, out);
    console.log(t.name, out.tableau.height + "x" + out.tableau.width, out.nPivots, out.pivotDigest, out.final.feasible, JSON.stringify(out.messages), out.refWallMs);
}
