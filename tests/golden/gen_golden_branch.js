// Branch-decision golden generator (TEST INFRASTRUCTURE).  Runs in the build container only, where the reference exists:
//   python oracle/build_ref.py && node tests/golden/gen_golden_branch.js
//
// Drives oracle/_ref (the type-erased reference itself) through gen_golden.js's recorder and wraps Tableau.isIntegral: every
// time the default branch-and-cut service asks it (branch-and-cut.ts:129), the answer is recorded next to the simplex() call it
// followed, together with what getMostFractionalVar() (mip-utils.ts:100-126, a pure read of the same tableau) answers at that
// moment -- the reference's own isIntegral / {index, value} of that relaxation, bit for bit (JSON round-trips shortest-repr doubles).
// The relaxations themselves (cut lists, heights, flags, evaluations) are those of tests/golden/fixtures/<name>.json.gz; `rhsShas`
// ties this file to them.
// Output: tests/golden/branch/<name>.json.gz
"use strict";
const fs = require("fs");
const path = require("path");

const G = require("./gen_golden.js");  // (installs the recorder on Tableau.prototype)
const REF = process.env.JSLP_REFERENCE || "/root/reference";
const refRoot = path.join(__dirname, "..", "..", "oracle", "_ref", "src");
const Tableau = require(path.join(refRoot, "tableau", "tableau.js")).default;

function num(x) {
    if (Number.isFinite(x)) return Object.is(x, -0) ? "-0" : x;
    return String(x);
}

const P = Tableau.prototype;
const orig = { simplex: P.simplex, isIntegral: P.isIntegral, getMostFractionalVar: P.getMostFractionalVar };
let calls = -1;      // simplex() calls of the current solve (the index of the last one)
let decisions = null;

P.simplex = function () {
    const r = orig.simplex.call(this);
    calls += 1;
    return r;
};
P.isIntegral = function () {
    const answer = orig.isIntegral.call(this);
    if (decisions) {
        const v = orig.getMostFractionalVar.call(this);
        decisions.push({ call: calls, isIntegral: answer, index: v.index === null ? -1 : v.index, value: num(v.value) });
    }
    return answer;
};

// output name -> reference fixture (the names of tests/golden/fixtures)
const FIXTURES = { Monster_II: "Monster_II", LargeFarmMIP: "LargeFarmMIP", Knapsack_1: "Knapsack 1",
    Integer_Wood_Shop_Problem: "Integer Wood Shop Problem", Sudoku4x4: "Sudoku4x4" };
const fixDir = path.join(REF, "test", "test-sanity");
for (const name of Object.keys(FIXTURES)) {
    if (process.argv[2] && process.argv[2] !== name) continue;
    const model = JSON.parse(fs.readFileSync(path.join(fixDir, FIXTURES[name] + ".json"), "utf8"));
    calls = -1;
    decisions = [];
    const out = G.run(model, false);
    const mine = decisions;
    decisions = null;
    const rec = {
        name,
        source: "test/test-sanity/" + FIXTURES[name] + ".json",
        integerVarIndexes: out.tableau.integerVarIndexes,
        precision: out.tableau.precision,
        nCalls: out.simplexCalls.length,
        rhsShas: out.simplexCalls.map((c) => c.rhsSha),
        branchAndCutIterations: out.final.branchAndCutIterations,
        decisions: mine,
    };
    G.write(path.join(__dirname, "branch"), name, rec);
    console.log("branch", name, rec.nCalls, "calls", mine.length, "decisions");
}
