// Golden vectors for the MIR row builders and the volume rule at their edges (TEST INFRASTRUCTURE; build container only):
//   python oracle/build_ref.py && node tests/golden/gen_golden_mir_edges.js
// The instances are tests/mir_edges.py's (`python tests/mir_edges.py --dump`: pre-solved tableaus built from seeds, doubles as hex).  Each
// is planted into a reference Tableau -- the tableau of a tiny model, so that the object is the reference's own: the matrix cells, the
// four maps, isInteger on the listed indexes (the reference's IntegerVariable / Variable objects), height, width, precision, the element
// counter -- and the reference's own computeFractionalVolume(true) and applyMIRCuts() run on it.  Recorded per instance:
//   * sha:     sha256 of the input (matrix bytes, the two maps, the integer indexes, the precision), as tests/mir_edges.sha_input computes it
//   * volume:  computeFractionalVolume(true) of the planted tableau, the hex of the double
//   * n, rows: the appended rows, the hex of their doubles with every NaN written as the one NaN JavaScript stores for the NaN literal
//              (the bytes of a NaN depend on the hardware that made it; gen_golden_nonfinite.js does the same)
//   * vibr:    the new entries of varIndexByRow; rbv / cbv: rowByVarIndex / colByVarIndex at those indexes; last: lastElementIndex after
// Output: tests/golden/mir_edges.json.gz
"use strict";
const path = require("path");
const fs = require("fs");
const zlib = require("zlib");
const crypto = require("crypto");
const { execFileSync } = require("child_process");

const refRoot = path.join(__dirname, "..", "..", "oracle", "_ref", "src");
const Model = require(path.join(refRoot, "model.js")).default;
const { Variable, IntegerVariable } = require(path.join(refRoot, "expressions.js"));

const TINY = { optimize: "obj", opType: "max", constraints: { c: { max: 4 } }, variables: { x: { obj: 1, c: 1 } } };

function doubles(hex) {
    const b = Buffer.from(hex, "hex");
    return new Float64Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength));
}
function hexOf(values) {
    const a = Float64Array.from(values, (x) => (Number.isNaN(x) ? NaN : x));
    return Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString("hex");
}
function shaInput(inst, matrix, precision) {
    const vibr = Int32Array.from(inst.vibr), vibc = Int32Array.from(inst.vibc), ints = Int32Array.from(inst.ints);
    const h = crypto.createHash("sha256");
    h.update(Buffer.from(matrix.buffer, matrix.byteOffset, matrix.byteLength));
    for (const a of [vibr, vibc, ints]) h.update(Buffer.from(a.buffer, a.byteOffset, a.byteLength));
    h.update(Buffer.from(Float64Array.of(precision).buffer));
    return h.digest("hex");
}

function plant(inst) {
    const precision = doubles(inst.precision)[0];
    const matrix = doubles(inst.matrix);
    const H = inst.H, W = inst.W;
    if (matrix.length !== H * W) throw new Error(inst.name + ": matrix size");
    const model = new Model(precision).loadJson(TINY);
    const t = model.tableau.setModel(model);
    t.precision = precision;
    t.width = W;
    t.height = H;
    t.matrix = Float64Array.from(matrix);
    t.varIndexByRow = Array.from(inst.vibr);
    t.varIndexByCol = Array.from(inst.vibc);
    t.nVars = W + H - 2;
    t.lastElementIndex = t.nVars;  // tableau.ts:312-316
    t.availableIndexes = [];
    t.rowByVarIndex = new Array(t.nVars).fill(-1);
    t.colByVarIndex = new Array(t.nVars).fill(-1);
    for (let r = 1; r < H; r++) t.rowByVarIndex[inst.vibr[r]] = r;
    for (let c = 1; c < W; c++) t.colByVarIndex[inst.vibc[c]] = c;
    const ints = new Set(inst.ints);
    t.variablesPerIndex = [];
    for (let v = 0; v < t.nVars; v++) t.variablesPerIndex[v] = ints.has(v) ? new IntegerVariable("v" + v, 0, v, 0) : new Variable("v" + v, 0, v, 0);
    return { t, sha: shaInput(inst, matrix, precision) };
}

const dump = execFileSync("python3", [path.join(__dirname, "..", "mir_edges.py"), "--dump"], { maxBuffer: 1 << 28 });
const out = {};
for (const inst of JSON.parse(dump.toString())) {
    const { t, sha } = plant(inst);
    if (sha !== inst.sha) throw new Error(inst.name + ": the input's sha256 differs between the two sides");
    const H = inst.H, W = inst.W;
    const volume = t.computeFractionalVolume(true);
    t.applyMIRCuts();
    const n = t.height - H;
    const planted = doubles(inst.matrix);
    for (let i = 0; i < H * W; i++) {  // applyMIRCuts only appends
        if (!Object.is(t.matrix[i], planted[i])) throw new Error(inst.name + ": cell " + i + " of the planted rows changed");
    }
    const vibr = t.varIndexByRow.slice(H, H + n);
    out[inst.name] = {
        sha, n, volume: hexOf([volume]), rows: hexOf(t.matrix.slice(H * W, (H + n) * W)), vibr,
        rbv: vibr.map((v) => t.rowByVarIndex[v]), cbv: vibr.map((v) => t.colByVarIndex[v]), last: t.lastElementIndex,
    };
    console.log(inst.name, "H", H, "W", W, "cuts", n, "volume", volume);
}
fs.writeFileSync(path.join(__dirname, "mir_edges.json.gz"), zlib.gzipSync(Buffer.from(JSON.stringify(out)), { level: 9 }));
