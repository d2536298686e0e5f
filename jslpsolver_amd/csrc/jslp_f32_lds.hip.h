// jslp_f32_lds.hip.h -- the fp32 twin in ONE launch: k32_simplex_lds, one workgroup = one whole fp32 simplex() of the live tableau at
// one tolerance, `n` tolerances = `n` workgroups of the same launch (include/jslpf_f32.h, jslpf_simplex_f32_sweep).
// Included by jslp_hip.hip behind every other kernel (needs f32::Slots / f32::nonzero16 / f32::eliminate, DevState, begin_simplex).
//
// The rules are those of select_step / prepare_pivot / update_rows_wg (jslp_core.inc.h) read in IEEE binary32, exactly as
// tests/fp32_reference.py states them: `precision` narrowed once, the 1e-16 zero test made in double, 1.0 / quot a double division
// narrowed afterwards, `eliminate` rounded twice, IEEE divisions, subnormals kept.  The launch shape is that of jslp_wglds.hip.h: the cost
// row, the RHS column, the pivot column, the normalised pivot row, both variable maps and the gated-row list live in dynamic LDS (floats
// / int32: half of what the fp64 kernel needs), the loop-carried scalars in registers.  A pivot touches global memory for the strided
// pivot-column gather, the pivot row, and the rows the reference's gate lets through (simplex.ts:370-375) -- all of it on the
// workgroup's OWN fp32 copy, which the prologue narrows from the live fp64 slot 0 and which stays in L2.
// Workgroups share nothing: no cross-workgroup communication, no cooperative launch, no spin; every loop ends on iters_cap.
// Not handled here (the host refuses): optional objectives, tableaus whose LDS state exceeds the dynamic LDS budget.
#pragma once

#define F32L_HIST 128  // first pairs of the cycle-check history kept in LDS (the suffix test runs on them: wave 0 alone)
#define F32L_SEL 256   // threads that take part in a selection: four waves, one per SIMD (see WGL_SEL)
#define F32L_UN 4      // 16-byte loads a lane has in flight in one row-update work item: 64 lanes x 4 floats x 4 = 1024 columns
#define F32L_TURN 256  // columns one wave covers with one 16-byte load per lane
#define F32L_KP 2      // pivot-row values a thread keeps in registers across the cycle check (ld <= F32L_KP * threads)

// every byte of LDS the kernel uses is dynamic (a static in front of the dynamic region could push it off its 16-byte alignment)
struct F32Smem {
    unsigned long long red[2][F32L_SEL / 64];  // cross-wave stage of the selections, double-buffered by call parity
    int2 hist[F32L_HIST];
    int32_t n_list;   // length of the gated-row list
    int32_t cyc_hit;  // verdict of the cycle check while the history fits `hist`
    int32_t or_flag;  // block-wide OR of the long-history suffix test
    int32_t pad;
};
struct F32Lds {
    F32Smem* sm;
    float* r0;      // [ld]  cost row (row 0), kept in step with the copy by the row update
    float* prow;    // [ld]  normalised pivot row of the current pivot
    int32_t* vibc;  // [ld]  varIndexByCol
    float* pcol;    // [Hc]  pivot column of the current pivot
    float* rhs;     // [Hc]  column 0
    int32_t* list;  // [Hc]  rows passing the gate
    int32_t* vibr;  // [Hc]  varIndexByRow
};
__host__ __device__ __forceinline__ size_t f32lds_bytes(int ld, int cap_rows) {
    const size_t hc = ((size_t)cap_rows + 3) & ~(size_t)3;  // (every piece starts 16-byte aligned: ld is a multiple of 16)
    return sizeof(F32Smem) + 4 * (3 * (size_t)ld + 4 * hc);
}
__device__ __forceinline__ F32Lds f32lds_carve(char* base, int ld, int cap_rows) {
    const int hc = (cap_rows + 3) & ~3;
    F32Lds L;
    L.sm = reinterpret_cast<F32Smem*>(base);
    L.r0 = reinterpret_cast<float*>(base + sizeof(F32Smem));
    L.prow = L.r0 + ld;
    L.vibc = reinterpret_cast<int32_t*>(L.prow + ld);
    L.pcol = reinterpret_cast<float*>(L.vibc + ld);
    L.rhs = L.pcol + hc;
    L.list = reinterpret_cast<int32_t*>(L.rhs + hc);
    L.vibr = L.list + hc;
    return L;
}

// ---- one 64-bit key per candidate: (order-preserving image of the float) << 32 | index; the minimum IS the selection ---------------
// -0 is folded into +0 (the reference compares them equal and lets the first index win); NaN never becomes a candidate (every
// candidate passed a strict comparison); no candidate's key is all ones
#define F32L_NONE (~0ull)
__device__ __forceinline__ unsigned f32l_asc(float v) {
    const unsigned b = __float_as_uint(v + 0.0f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long f32l_key(unsigned image, int index) { return ((unsigned long long)image << 32) | (unsigned)index; }
__device__ __forceinline__ unsigned long long f32l_min(unsigned long long a, unsigned long long b) { return b < a ? b : a; }
template <int CTRL>
__device__ __forceinline__ unsigned long long f32l_dpp(unsigned long long x) {
    const int lo = (int)(unsigned)x, hi = (int)(unsigned)(x >> 32);
    return ((unsigned long long)(unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false) << 32) |
           (unsigned long long)(unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ unsigned long long f32l_readlane(unsigned long long x, int lane) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), lane) << 32) |
           (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, lane);
}
__device__ __forceinline__ unsigned long long f32l_wave_min(unsigned long long x) {  // a whole wave; the result in every lane
    x = f32l_min(x, f32l_dpp<0xB1>(x));   // quad_perm [1,0,3,2]: lane ^ 1
    x = f32l_min(x, f32l_dpp<0x4E>(x));   // quad_perm [2,3,0,1]: lane ^ 2
    x = f32l_min(x, f32l_dpp<0x141>(x));  // row_half_mirror: the other quad of the 8-lane half
    x = f32l_min(x, f32l_dpp<0x140>(x));  // row_mirror: the other half of the 16-lane row
    unsigned long long r = f32l_readlane(x, 0);
    r = f32l_min(r, f32l_readlane(x, 16));
    r = f32l_min(r, f32l_readlane(x, 32));
    return f32l_min(r, f32l_readlane(x, 48));
}
// the workgroup's minimum in ONE barrier: the first F32L_SEL threads hold candidates, every thread gets the result
__device__ __forceinline__ unsigned long long f32l_block_min(unsigned long long x, F32Smem* sm, int& par) {
    const int w = threadIdx.x >> 6;
    if (w < F32L_SEL / 64) {
        x = f32l_wave_min(x);
        int l0 = threadIdx.x & 63;
        asm volatile("" : "+v"(l0));  // (the lane test stays a compare at its use: see block_min_ki)
        if (l0 == 0) sm->red[par][w] = x;
    }
    __syncthreads();
    unsigned long long r = sm->red[par][0];
#pragma unroll
    for (int i = 1; i < F32L_SEL / 64; i++) r = f32l_min(r, sm->red[par][i]);
    par ^= 1;  // the next call writes the other buffer
    return r;
}

// suffix_is_square (jslp_core.inc.h; checkForCycles, simplex.ts:415-440) on the run's global history, beyond the LDS prefix
__device__ __forceinline__ bool f32l_suffix_is_square(const int2* h, int n, F32Smem* sm) {
    int found = 0;
    const int2 last = h[n - 1];
    for (int L = 1 + threadIdx.x; 2 * L <= n; L += blockDim.x) {
        const int2 a = h[n - 1 - L];
        if (a.x != last.x || a.y != last.y) continue;
        bool eq = true;
        for (int i = 0; i < L - 1; i++) {
            const int2 x = h[n - 2 * L + i], y = h[n - L + i];
            if (x.x != y.x || x.y != y.y) { eq = false; break; }
        }
        if (eq) found = 1;
    }
    __syncthreads();  // every thread is past its read of the previous verdict
    if (threadIdx.x == 0) sm->or_flag = 0;
    __syncthreads();
    if (found) sm->or_flag = 1;
    __syncthreads();
    return sm->or_flag != 0;
}

// one work item of the row update: row r, columns [col_begin, col_begin + 1024) -- one wave, 16 bytes per lane, the loads of the
// item in flight together; only the quads the reference's column gate lets through are read and written (simplex.ts:376-387)
__device__ __forceinline__ void f32l_update_row(float* A, const F32Lds& L, int ld, int r, float k, int pc, float quot, int lane, int col_begin) {
    float* row = A + (long long)r * ld;
    const int base = col_begin + lane * 4;
    float4 a[F32L_UN];
    unsigned live = 0;
#pragma unroll
    for (int j = 0; j < F32L_UN; j++) {
        const int c0 = base + F32L_TURN * j;
        a[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (c0 < ld) {
            const float4 p = *reinterpret_cast<const float4*>(L.prow + c0);
            if (f32::nonzero16(p.x) || f32::nonzero16(p.y) || f32::nonzero16(p.z) || f32::nonzero16(p.w) || (pc & ~3) == c0) {
                live |= 1u << j;
                a[j] = *reinterpret_cast<const float4*>(row + c0);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < F32L_UN; j++) {
        if (!(live & (1u << j))) continue;
        const int c0 = base + F32L_TURN * j;
        const float4 p = *reinterpret_cast<const float4*>(L.prow + c0);
        float4 x = a[j];
        if (f32::nonzero16(p.x)) x.x = f32::eliminate(x.x, k, p.x);
        if (f32::nonzero16(p.y)) x.y = f32::eliminate(x.y, k, p.y);
        if (f32::nonzero16(p.z)) x.z = f32::eliminate(x.z, k, p.z);
        if (f32::nonzero16(p.w)) x.w = f32::eliminate(x.w, k, p.w);
        if ((pc & ~3) == c0) {  // :387 overwrites whatever the loop did to column pc
            const float nv = -k / quot;
            const int q = pc & 3;
            if (q == 0) x.x = nv; else if (q == 1) x.y = nv; else if (q == 2) x.z = nv; else x.w = nv;
        }
        *reinterpret_cast<float4*>(row + c0) = x;
        if (c0 == 0) L.rhs[r] = x.x;
        if (r == 0) *reinterpret_cast<float4*>(L.r0 + c0) = x;
    }
}

struct F32Precisions { float v[64]; };  // run r's tolerance, narrowed once by the host: (float)precisions[r]

// Grid = runs, THREADS threads.  s: the engine's fp64 slots (slot 0 = the live tableau, read only); d: the fp32 arena, run r = its
// copy r; run r's outcome goes to states_out[r], rhs_out / rows_out [r * out_stride ...] (the engine's read-back buffer).
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k32_simplex_lds(Slots s, f32::Slots d, F32Precisions precs, int check_cycles, int iters_cap, int cap_rows,
                                                          double* rhs_out, int32_t* rows_out, DevState* states_out, int out_stride) {
    extern __shared__ __attribute__((aligned(16))) char f32l_dyn[];
    const int run = blockIdx.x;
    const int tid = threadIdx.x, nt = THREADS, lane = tid & 63, w = tid >> 6, nw = THREADS / 64;
    const int ld = d.ld, W = d.W;
    const F32Lds L = f32lds_carve(f32l_dyn, ld, cap_rows);
    F32Smem* sm = L.sm;
    const int H = s.st->H;  // fixed during a simplex() call
    const float precision = precs.v[run];
    float* A = d.A + (long long)run * d.A_stride;
    int32_t* g_vibr = d.vibr + (long long)run * d.vibr_stride;
    int32_t* g_vibc = d.vibc + (long long)run * d.vibc_stride;
    int32_t* g_rbv = d.rbv + (long long)run * d.idx_stride;
    int32_t* g_cbv = d.cbv + (long long)run * d.idx_stride;
    int2* g_hist = d.hist + (long long)run * d.hist_cap;

    // ---- prologue: narrow the live fp64 tableau into my copy (k32_convert), the four maps, column 0 / row 0 / the maps into LDS ----
    {
        const long long n4 = (long long)H * ld / 4;
        const double2* src = reinterpret_cast<const double2*>(s.A);
        float4* dst = reinterpret_cast<float4*>(A);
        for (long long i = tid; i < n4; i += nt) {
            const double2 lo = src[2 * i], hi = src[2 * i + 1];
            dst[i] = make_float4((float)lo.x, (float)lo.y, (float)hi.x, (float)hi.y);
        }
        for (int r = tid; r < H; r += nt) {
            const int v = s.vibr[r];
            g_vibr[r] = v;
            L.vibr[r] = v;
            L.rhs[r] = (float)s.A[(long long)r * s.ld];
        }
        for (int col = tid; col < ld; col += nt) {
            L.r0[col] = (float)s.A[col];
            if (col < W) {
                const int v = s.vibc[col];
                g_vibc[col] = v;
                L.vibc[col] = v;
            }
        }
        for (int i = tid; i < s.idx_stride; i += nt) { g_rbv[i] = s.rbv[i]; g_cbv[i] = s.cbv[i]; }
        if (tid == 0) sm->n_list = 0;
    }
    const int live_err = s.st->err;
    const int err0 = (live_err == ERR_CUT_ARG || live_err == ERR_CAPACITY) ? live_err : (int)ERR_NONE;  // (what begin_simplex keeps)
    __syncthreads();  // my copy and the LDS state are complete (a workgroup's global writes are visible to itself after a barrier)

    int phase = 1, it1 = 0, it2 = 0, hist_n = 0, iters_left = iters_cap, entered2 = 0, par = 0;
    // outcome: 0 running, 1 optimal, 2 unbounded, 3 cycle, 4 infeasible, 5 iteration cap, 6 history full, 7 refused (a cut error in the live state)
    int outcome = err0 != ERR_NONE ? 7 : 0, unbounded_col = 0;
    const bool row_in_regs = ld <= F32L_KP * nt;
    while (outcome == 0) {
        if (iters_left <= 0) { outcome = 5; break; }
        int pr = 0, pc = 0, neg_flag = 0;
        float pv0 = 0.0f, pv1 = 0.0f;  // my two columns of the pivot row (raw), loaded as early as the row is known
        bool have_pv = false;
        auto gather_column = [&](int col) {  // the pivot column into LDS: two rows per thread and turn, both loads before either store
            for (int r0 = tid; r0 < H; r0 += 2 * nt) {
                const int r1 = r0 + nt, r1c = r1 < H ? r1 : H - 1;
                const float v0 = A[(long long)r0 * ld + col], v1 = A[(long long)r1c * ld + col];
                L.pcol[r0] = v0;
                L.pcol[r1c] = v1;  // (the clamped row's value is that row's own)
            }
        };
        if (phase == 1) {
            // leaving row: most negative RHS below -precision, first index on ties (simplex.ts:39-49)
            float bv = -precision;
            int bi = 0;
            if (tid < F32L_SEL)
                for (int r = 1 + tid; r < H; r += F32L_SEL) {
                    const float v = L.rhs[r];
                    if (v < bv) { bv = v; bi = r; }
                }
            unsigned long long x = bi != 0 ? f32l_key(f32l_asc(bv), bi) : F32L_NONE;
            x = f32l_block_min(x, sm, par);
            if (x == F32L_NONE) {  // :51-54 feasible: phase 2 starts in this same iteration with a fresh history (:102)
                phase = 2; entered2 = 1; hist_n = 0;
            } else {
                pr = (int)(unsigned)x;
                // entering column: max -cost / coef over unrestricted or coef < -precision, strict from -Infinity (simplex.ts:56-71)
                const float* row = A + (long long)pr * ld;
                if (row_in_regs) {
                    pv0 = tid < ld ? row[tid] : 0.0f;
                    pv1 = tid + nt < ld ? row[tid + nt] : 0.0f;
                    have_pv = true;
                    if (tid < ld) L.prow[tid] = pv0;  // (raw: the normalisation below overwrites it)
                    if (tid + nt < ld) L.prow[tid + nt] = pv1;
                } else {
                    for (int col = tid; col < ld; col += nt) L.prow[col] = row[col];
                }
                __syncthreads();
                float qv = -INFINITY;
                int qi = 0;
                if (tid < F32L_SEL)
                    for (int col = 1 + tid; col < W; col += F32L_SEL) {
                        const float coef = L.prow[col];
                        const bool un = d.has_unr && d.unr[L.vibc[col]] != 0;
                        if (un || coef < -precision) {
                            const float quo = -L.r0[col] / coef;
                            if (qv < quo) { qv = quo; qi = col; }
                        }
                    }
                unsigned long long q = qi != 0 ? f32l_key(~f32l_asc(qv), qi) : F32L_NONE;
                q = f32l_block_min(q, sm, par);
                if (q == F32L_NONE) { outcome = 4; break; }  // :73-76 infeasible
                pc = (int)(unsigned)q;
                gather_column(pc);
                __syncthreads();
            }
        }
        if (phase == 2) {
            // Dantzig pricing with the reference's batch rule (simplex.ts:118-219) on the LDS cost row: the first batch holding a
            // candidate wins, inside it the largest value, first index on ties
            float ev = precision;
            int ei = 0, eb = 0;
            if (tid < F32L_SEL)
                for (int col = 1 + tid; col < W; col += F32L_SEL) {
                    const float rc = L.r0[col];
                    const bool un = d.has_unr && d.unr[L.vibc[col]] != 0;
                    const int b = d.use_partial ? (col - 1) / d.batch : 0;
                    const float val = (un && rc < 0) ? -rc : rc;
                    if (val > precision) {
                        const bool take = ei == 0 || b < eb || (b == eb && val > ev);  // my columns ascend: ties keep the earlier one
                        ev = take ? val : ev;
                        ei = take ? col : ei;
                        eb = take ? b : eb;
                    }
                }
            if (d.use_partial) {  // which batch?
                unsigned long long b = ei != 0 ? f32l_key((unsigned)eb, 0) : F32L_NONE;
                b = f32l_block_min(b, sm, par);
                if (b == F32L_NONE || (unsigned)(b >> 32) != (unsigned)eb) ei = 0;  // nothing prices in / my best sits in a later batch
            }
            unsigned long long e = ei != 0 ? f32l_key(~f32l_asc(ev), ei) : F32L_NONE;
            e = f32l_block_min(e, sm, par);
            if (e == F32L_NONE) { outcome = 1; break; }  // optimal (simplex.ts:265-269)
            pc = (int)(unsigned)e;
            {
                const float rc = L.r0[pc];
                const bool un = d.has_unr && d.unr[L.vibc[pc]] != 0;
                neg_flag = (un && rc < 0) ? 1 : 0;
            }
            // ratio test (simplex.ts:271-296) in its order-free form: the first degenerate row wins outright (image 0), else the
            // first-index minimum of the accepted quotients, strict from +Infinity
            gather_column(pc);
            __syncthreads();
            float mv = INFINITY;
            int mi = 0, rdeg = 0x7fffffff;
            if (tid < F32L_SEL)
                for (int r = 1 + tid; r < H; r += F32L_SEL) {
                    const float colv = L.pcol[r];
                    const float rhs = L.rhs[r];
                    if (-precision < colv && colv < precision) continue;
                    if (colv > 0 && precision > rhs && rhs > -precision) {
                        if (r < rdeg) rdeg = r;
                        continue;
                    }
                    const float quo = neg_flag ? -rhs / colv : rhs / colv;
                    if (quo > precision && mv > quo) { mv = quo; mi = r; }
                }
            unsigned long long m = F32L_NONE;
            if (rdeg != 0x7fffffff) m = f32l_key(0u, rdeg);
            else if (mi != 0) m = f32l_key(f32l_asc(mv), mi);  // (a quotient above `precision` is positive: its image is above 0)
            m = f32l_block_min(m, sm, par);
            if (m == F32L_NONE) { outcome = 2; unbounded_col = pc; break; }  // unbounded (simplex.ts:298-303)
            pr = (int)(unsigned)m;
        }
        // ---- the pivot (pr, pc) is chosen: my columns of the pivot row leave now; the gate and the cycle check run under them ----
        float* prow_A = A + (long long)pr * ld;
        if (row_in_regs && !have_pv) {
            pv0 = tid < ld ? prow_A[tid] : 0.0f;
            pv1 = tid + nt < ld ? prow_A[tid + nt] : 0.0f;
            have_pv = true;
        }
        int leaving = 0, entering = 0;
        if (tid == 0) { leaving = L.vibr[pr]; entering = L.vibc[pc]; }
        // the rows that pass the reference's gate (simplex.ts:370-375), compacted (the list holds every row: it cannot overflow)
        for (int r = tid; r < H; r += nt)
            if (r != pr && f32::nonzero16(L.pcol[r])) L.list[atomicAdd(&sm->n_list, 1)] = r;
        // cycle check (simplex.ts:78-93 / 305-320): append first, test, stop WITHOUT pivoting on a hit
        if (check_cycles) {
            if (hist_n >= d.hist_cap) { outcome = 6; break; }
            const bool short_hist = hist_n < F32L_HIST;
            if (w == 0) {
                if (tid == 0) {
                    const int2 pair = make_int2(leaving, entering);
                    g_hist[hist_n] = pair;
                    if (short_hist) sm->hist[hist_n] = pair;
                }
                if (short_hist) {  // wave 0 alone, on the LDS prefix: lane l tests block length l + 1 (and + 64)
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): thread 0's LDS store is this wave's own
                    const int n1 = hist_n + 1;
                    const int2 last = sm->hist[n1 - 1];
                    int found = 0;
                    for (int len = 1 + lane; 2 * len <= n1; len += 64) {
                        const int2 a = sm->hist[n1 - 1 - len];
                        if (a.x != last.x || a.y != last.y) continue;
                        bool eq = true;
                        for (int i = 0; i < len - 1; i++) {
                            const int2 x = sm->hist[n1 - 2 * len + i], y = sm->hist[n1 - len + i];
                            if (x.x != y.x || x.y != y.y) { eq = false; break; }
                        }
                        if (eq) found = 1;
                    }
                    const unsigned long long hit = __ballot(found != 0);
                    if (lane == 0) sm->cyc_hit = hit != 0ull ? 1 : 0;
                }
            }
            __syncthreads();  // the list, the appended pair and the verdict are complete
            hist_n += 1;
            const bool cycle = short_hist ? sm->cyc_hit != 0 : f32l_suffix_is_square(g_hist, hist_n, sm);
            if (cycle) { outcome = 3; break; }
        } else {
            __syncthreads();  // the list is complete
        }
        const int n = sm->n_list;
        const bool anyrow = n > 0;  // any row that executes the inner loop lazily zeroes the tiny pivot-row entries (:381-383)
        // ---- pivot row (simplex.ts:352-364) ----
        const float quot = L.pcol[pr];  // = A[pr, pc] (:335)
        auto normalise = [&](int col, float val) {
            float v = 0.0f;
            if (col < W) {
                const bool innz = f32::nonzero16(val);                         // :356
                v = innz ? val / quot : 0.0f;                                  // :357 / :361 (IEEE division)
                if (col == pc) v = (float)(1.0 / (double)quot);               // :364: a double division, narrowed
                if (innz && anyrow && !f32::nonzero16(v) && v != 0.0f) v = 0.0f;  // :381-383
                prow_A[col] = v;
                if (col == 0) L.rhs[pr] = v;
            }
            L.prow[col] = v;
        };
        if (have_pv) {
            if (tid < ld) normalise(tid, pv0);
            if (tid + nt < ld) normalise(tid + nt, pv1);
        } else {
            for (int col = tid; col < ld; col += nt) normalise(col, prow_A[col]);
        }
        if (tid == 0) {  // :339-349
            g_vibr[pr] = entering;
            g_vibc[pc] = leaving;
            L.vibr[pr] = entering;
            L.vibc[pc] = leaving;
            g_rbv[entering] = pr;
            g_rbv[leaving] = -1;
            g_cbv[entering] = -1;
            g_cbv[leaving] = pc;
        }
        if (phase == 1) it1 += 1; else it2 += 1;
        iters_left -= 1;
        __syncthreads();  // L.prow complete
        {   // work items = (gated row, pass of 1024 columns), one wave each
            const int passes = (ld + F32L_TURN * F32L_UN - 1) / (F32L_TURN * F32L_UN);
            for (int it = w; it < n * passes; it += nw) {
                const int i = it / passes, ps = it - i * passes;
                const int r = L.list[i];
                f32l_update_row(A, L, ld, r, L.pcol[r], pc, quot, lane, ps * F32L_TURN * F32L_UN);
            }
        }
        if (tid == 0) sm->n_list = 0;  // for the next pivot (several barriers away from its first use)
        __syncthreads();
    }
    // ---- epilogue (k32_gather): the state, the RHS column widened to double and the row map into run `run`'s slice ----
    __syncthreads();
    for (int r = tid; r < H; r += nt) {
        if (rhs_out) rhs_out[(long long)run * out_stride + r] = (double)L.rhs[r];
        if (rows_out) rows_out[(long long)run * out_stride + r] = L.vibr[r];
    }
    if (tid == 0) {
        // the live state as k32_convert copies it (nobody writes it during this launch), then begin_simplex and what the loop
        // carried in registers -- built in place: a DevState of the thread's own is parked in scratch
        DevState* o = states_out + run;
        *o = *s.st;
        o->gen = 0;
        o->trace_n = 0;
        o->rhs_valid = 0;
        f32::begin_simplex(o, iters_cap);
        o->phase = phase;
        o->it1 = it1;
        o->it2 = it2;
        o->hist_n = hist_n;
        o->iters_left = iters_left;
        o->entered_phase2 = entered2;
        if (entered2) o->feasible = 1;
        if (outcome == 1) o->optimal = 1;
        if (outcome == 2) { o->bounded = 0; o->unbounded_var = L.vibc[unbounded_col]; }
        if (outcome == 3) { o->cycle_phase = phase; o->feasible = 0; }
        if (outcome == 4) o->feasible = 0;
        if (outcome == 5) o->err = ERR_ITER_LIMIT;
        if (outcome == 6) o->err = ERR_HIST_FULL;
        o->status = ST_DONE;
        o->do_pivot = 0;
        o->obj_cell = (double)L.r0[0];
    }
}
