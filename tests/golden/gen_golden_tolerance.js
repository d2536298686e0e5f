// Golden vectors for options.tolerance under the three branch-and-cut services (TEST INFRASTRUCTURE; build container only):
//   python oracle/build_ref.py && node tests/golden/gen_golden_tolerance.js
//
// Runs oracle/_ref (the type-erased reference itself) on
//   - the two fixtures under tests/golden/fixtures that show the option, StockCuttingProblem (tolerance 3) and LargeFarmMIP (tolerance
//     0.005), with their options.timeout REMOVED (a clock cannot be pinned) and their tolerance kept, under the default service, with
//     useMIRCuts, under the enhanced service (three node selections x most-fractional / pseudocost) and under the incremental service
//     (the five pairs tests/golden/incremental.json.gz records);
//   - the default-policy models of tests/golden/fuzz_services.jsonl.gz whose recorded run took at least 3 iterations and which the presolve
//     pre-pass leaves alone, each with options.tolerance 0.01, 0.2 and 1
// and records what a re-implementation must reproduce: every pivot (FNV-1a digest), the number of relaxations, bestPossibleEval, the final
// height and the Solve() result.  Output: tests/golden/tolerance.json.gz (the models themselves are in the fixture files and in
// fuzz_services.jsonl.gz: a fuzz record names its model by `line`, the 0-based index among that file's JSON lines).
"use strict";
const fs = require("fs");
const path = require("path");
const zlib = require("zlib");

const refRoot = path.join(__dirname, "..", "..", "oracle", "_ref", "src");
const solver = require(path.join(refRoot, "solver.js")).default;
const Tableau = require(path.join(refRoot, "tableau", "tableau.js")).default;

function num(x) {
    if (Number.isFinite(x)) return Object.is(x, -0) ? "-0" : x;
    return String(x);
}

let rec = null;
const P = Tableau.prototype;
const origPivot = P.pivot;
P.pivot = function (r, c) {
    if (rec) {
        rec.n += 1;
        rec.h = Math.imul(rec.h ^ r, 16777619);
        rec.h = Math.imul(rec.h ^ c, 16777619);
    }
    return origPivot.call(this, r, c);
};

function run(model) {
    rec = { n: 0, h: 2166136261 | 0 };
    const solution = solver.Solve(JSON.parse(JSON.stringify(model)), undefined, true);
    const r = rec;
    rec = null;
    const t = solution._tableau;
    const result = solver.buildSimplifiedResult(solution);
    return {
        nPivots: r.n,
        pivotDigest: (r.h >>> 0).toString(16),
        iterations: t.branchAndCutIterations,
        isIntegral: !!t.__isIntegral,
        feasible: solution.feasible,
        bounded: solution.bounded,
        evaluation: num(solution.evaluation),
        bestPossibleEval: num(t.bestPossibleEval),
        height: t.height,
        result: JSON.parse(JSON.stringify(result, (k, v) => (typeof v === "number" ? num(v) : v))),
        resultKeys: Object.keys(result),
    };
}

const services = [{}, { useMIRCuts: true }];
for (const nodeSelection of ["best-first", "depth-first", "hybrid"])
    for (const branching of ["most-fractional", "pseudocost"]) services.push({ nodeSelection, branching });
for (const pair of [{}, { nodeSelection: "depth-first" }, { nodeSelection: "best-first" }, { branching: "most-fractional" },
                    { nodeSelection: "depth-first", branching: "most-fractional" }])
    services.push(Object.assign({ useIncremental: true }, pair));

const cases = [];
for (const name of ["StockCuttingProblem", "LargeFarmMIP"]) {
    const file = "fixtures/" + name + ".json.gz";
    const g = JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(__dirname, file))).toString());
    for (const service of services) {
        const model = JSON.parse(JSON.stringify(g.model));
        const options = Object.assign({}, model.options || {}, service);
        delete options.timeout;
        model.options = options;
        const out = run(model);
        out.file = file;
        out.options = options;
        out.presolveFixed = g.presolve ? g.presolve.nFixed : 0;
        cases.push(out);
        console.log(name, JSON.stringify(options), out.iterations, out.nPivots, out.pivotDigest, out.result.result);
    }
}
const lines = zlib.gunzipSync(fs.readFileSync(path.join(__dirname, "fuzz_services.jsonl.gz"))).toString().split("\n").filter((l) => l.startsWith("{"));
lines.forEach((text, line) => {
    const c = JSON.parse(text);
    if ((c.model.options && Object.keys(c.model.options).length) || c.fixed !== 0 || c.infeasPre || !(c.iter >= 3)) return;
    for (const tolerance of [0.01, 0.2, 1]) {
        const model = JSON.parse(JSON.stringify(c.model));
        model.options = { tolerance };
        const out = run(model);
        out.line = line;
        out.gen = c.gen;
        out.seed = c.seed;
        out.options = model.options;
        out.iterationsWithout = c.iter;
        cases.push(out);
    }
});
fs.writeFileSync(path.join(__dirname, "tolerance.json.gz"), zlib.gzipSync(Buffer.from(JSON.stringify(cases)), { level: 9 }));
console.log(cases.length, "cases");
