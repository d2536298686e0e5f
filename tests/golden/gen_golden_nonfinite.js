// Golden vectors for NON-FINITE values that the reference makes out of finite models (TEST INFRASTRUCTURE; build container only):
//   python oracle/build_ref.py && node tests/golden/gen_golden_nonfinite.js
// Small models recorded through gen_golden.js's `run`, on which the reference's own arithmetic leaves the finite range:
//   * overflow_ratio: a bound of 1e301 on a row with coefficient 2e-8 -- the ratio 1e301 / 2e-8 overflows to +Infinity, which the
//     ratio test's strict `minQuotient > quotient` from +Infinity never takes: unbounded;
//   * unrestricted_zero / unrestricted_zero_neg: an unrestricted variable absent from a violated ">=" row -- phase 1's quotient
//     -cost / 0 is -Infinity (never taken) or +Infinity (min: it enters, the pivot divides by zero and the tableau fills with NaN);
//   * overflow_pivot: coefficients of 1e200 in the pivot row and the pivot column: their product overflows in the update;
//   * unrestricted_zero_mip (unrestricted_zero_neg) / overflow_pivot_mip: the same with integer variables; the reference ends both
//     at the root;
//   * branch_overflow_mip / branch_nonfinite_mip: MILPs that branch -- a finite root, then children (cut rows, restores) in whose
//     pivots the values overflow; found by searching small random MILPs with coefficients of 1e150 .. 1e200 and 1e-8 in the
//     reference, kept verbatim.
// Besides everything gen_golden.js records, the final matrix and every call's RHS column are hashed with NaN canonicalised (one NaN:
// what JavaScript stores for the NaN literal) -- the raw bytes of a NaN depend on the hardware that made it.
// Output: tests/golden/nonfinite.json.gz
"use strict";
const path = require("path");
const fs = require("fs");
const zlib = require("zlib");
const crypto = require("crypto");
const { run } = require("./gen_golden.js");
const Tableau = require(path.join(__dirname, "..", "..", "oracle", "_ref", "src", "tableau", "tableau.js")).default;

function canonSha(values, ints) {
    const a = Float64Array.from(values, (x) => (Number.isNaN(x) ? NaN : x));
    const parts = [Buffer.from(a.buffer, a.byteOffset, a.byteLength)];
    if (ints) { const b = Int32Array.from(ints); parts.push(Buffer.from(b.buffer, b.byteOffset, b.byteLength)); }
    return crypto.createHash("sha256").update(Buffer.concat(parts)).digest("hex");
}
let calls = null;
let callNonFinite = null;
let last = null;
const P = Tableau.prototype;
const inner = P.simplex;  // (gen_golden.js's recording hook)
P.simplex = function () {
    const r = inner.call(this);
    if (calls) {
        let nonFinite = 0;
        for (let i = 0; i < this.width * this.height; i++) if (!Number.isFinite(this.matrix[i])) nonFinite++;
        callNonFinite.push(nonFinite);
        const rhs = [];
        for (let i = 0; i < this.height; i++) rhs.push(this.matrix[i * this.width]);
        calls.push(canonSha(rhs, this.varIndexByRow.slice(0, this.height)));
    }
    last = this;
    return r;
};

const MODELS = {
    overflow_ratio: { optimize: "obj", opType: "max", constraints: { big: { max: 1e301 }, cap: { max: 10 } },
        variables: { x: { obj: 1, big: 2e-8 }, y: { obj: 1, cap: 1 } } },
    unrestricted_zero: { optimize: "obj", opType: "max", constraints: { need: { min: 5 }, cap: { max: 20 } },
        variables: { y: { obj: 1, need: 1, cap: 1 }, u: { obj: 3, cap: 1 } }, unrestricted: { u: 1 } },
    unrestricted_zero_neg: { optimize: "obj", opType: "min", constraints: { need: { min: 5 }, cap: { max: 20 } },
        variables: { y: { obj: 1, need: 1, cap: 1 }, u: { obj: 3, cap: 1 } }, unrestricted: { u: 1 } },
    overflow_pivot: { optimize: "obj", opType: "max", constraints: { a: { max: 1 }, c: { max: 3 } },
        variables: { x: { obj: 2, a: 1, c: 1e200 }, y: { obj: 1, a: 1e200, c: 1 } } },
};
MODELS.unrestricted_zero_mip = Object.assign(JSON.parse(JSON.stringify(MODELS.unrestricted_zero_neg)), { ints: { y: 1 } });
MODELS.overflow_pivot_mip = Object.assign(JSON.parse(JSON.stringify(MODELS.overflow_pivot)), { ints: { x: 1 } });
MODELS.branch_overflow_mip = { optimize: "obj", opType: "max", constraints: { c0: { max: 7 }, c1: { max: 1e200 }, c2: { max: 10 }, c3: { max: 5e300 } },
    variables: { x0: { obj: 2, c0: 1e200, c1: 5, c2: 1e150 }, x1: { obj: 3, c0: 2, c2: 1, c3: 1 }, x2: { obj: 2, c0: 5, c1: 1e200 } }, ints: { x1: 1 } };
MODELS.branch_nonfinite_mip = { optimize: "obj", opType: "min", constraints: { c0: { min: 2 }, c1: { max: 1e200 }, c2: { max: 5e300 }, c3: { min: 2 } },
    variables: { x0: { obj: -1, c1: -5, c2: 2e-8 }, x1: { obj: -1, c0: -2, c3: 5 }, x2: { obj: -1, c0: 1e200, c3: 3 } },
    ints: { x0: 1, x1: 1, x2: 1 }, unrestricted: { x0: 1 } };

const out = {};
for (const [name, model] of Object.entries(MODELS)) {
    calls = [];
    callNonFinite = [];
    const g = run(model, true);
    const t = last;
    g.model = model;
    g.canonical = {
        callRhsSha: calls,
        callNonFinite,
        finalMatrixSha: canonSha(t.matrix.slice(0, t.width * t.height)),
        nonFinite: Array.from(t.matrix.slice(0, t.width * t.height)).filter((x) => !Number.isFinite(x)).length,
    };
    calls = null;
    out[name] = g;
    console.log(name, "pivots", g.nPivots, "calls", g.simplexCalls.length, "feasible", g.final.feasible, "bounded", g.final.bounded,
        "non-finite cells", g.canonical.nonFinite, "result", JSON.stringify(g.result));
}
fs.writeFileSync(path.join(__dirname, "nonfinite.json.gz"), zlib.gzipSync(Buffer.from(JSON.stringify(out)), { level: 9 }));
