// jslp_tree_mir.hip.h -- the MIR-cut loop of a node INSIDE the packed tree kernel (include/jslpc_tree_mir.h): the device functions of the
// MIR builds of k_tree_packed (jslp_tree.hip.h includes this file in front of the kernel).  What jslp_mir.hip.h does for the node kernels
// of an engine, restated over the tableau that LDS holds: between two pk_simplex runs the LP's workgroup computes
// computeFractionalVolume(true) (mip-utils.ts:67-92) and appends applyMIRCuts' rows (cutting-strategies.ts:74-212) at the end of the
// tableau, maps included.  Nothing here touches global memory, and every value a caller branches on is the same in every thread.
// Needs js_max0 / js_min0 (jslp_kernels.hip.h).  (TMIR_MAX_ROUNDS, the bound of the loop built on these, is the layout's: jslp_tree.hip.h.)
#ifndef JSLP_TREE_MIR_DEVICE
#define JSLP_TREE_MIR_DEVICE

#define TMIR_MAX_CUTS 10    // applyMIRCuts' default maxCuts (cutting-strategies.ts:199)

struct TreeMirSm {
    unsigned long long masks[4];  // one ballot per wave of an ordered compaction (at most 256 threads)
    int32_t sel[TMIR_MAX_CUTS];   // source rows of this round's cuts
    double volume;
};

// one step of an ordered compaction over the workgroup: how many threads before mine hold `ok`, and how many in all (uniform).
// One wave needs its ballot alone.
template <int THREADS>
__device__ __forceinline__ int tmir_rank(bool ok, TreeMirSm& ms, int* total) {
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(ok);
    int before = __popcll(m & ((1ull << lane) - 1));
    if constexpr (THREADS == 64) {
        *total = __popcll(m);
    } else {
        const int wave = threadIdx.x >> 6;
        if (lane == 0) ms.masks[wave] = m;
        __syncthreads();
        int all = 0;
        for (int k = 0; k < THREADS / 64; k++) {
            const int n = __popcll(ms.masks[k]);
            if (k < wave) before += n;
            all += n;
        }
        __syncthreads();  // (the masks are free for the next step)
        *total = all;
    }
    return before;
}

// computeFractionalVolume(ignoreIntegerValues = true) of rows [1, H) of the tableau at A (row stride S): the ORDERED product of |value|
// over the basic integer variables that are not at an integer value, with mir_volume_wg's NaN rules (Math.min(NaN, x) is NaN and
// NaN < precision is false, so a NaN or infinite row multiplies in).  The contributing rows are compacted in row order into `scratch`
// (>= H doubles of LDS: the pivot column) and ONE lane multiplies them in that order: a tree reduction would round differently.
template <int THREADS>
__device__ __forceinline__ double tmir_volume(const double* A, int S, const int32_t* vibr, int H, const uint8_t* is_int, double precision, double* scratch,
                                              TreeMirSm& ms) {
    int base = 0;
    for (int r0 = 1; r0 < H; r0 += THREADS) {
        const int r = r0 + (int)threadIdx.x;
        bool ok = false;
        double distance = 0.0;
        if (r < H) {
            const int v = vibr[r];
            if (v >= 0 && is_int[v]) {
                distance = fabs(A[r * S]);
                const double a = distance - floor(distance), b = floor(distance + 1);
                const bool nan = a != a || b != b;
                ok = nan || !((a < b ? a : b) < precision);
            }
        }
        int total;
        const int before = tmir_rank<THREADS>(ok, ms, &total);
        if (ok) scratch[base + before] = distance;
        base += total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double volume = -1.0;
        for (int i = 0; i < base; i++) volume = volume == -1.0 ? scratch[i] : volume * scratch[i];
        ms.volume = volume == -1.0 ? 0.0 : volume;
    }
    __syncthreads();
    const double volume = ms.volume;
    __syncthreads();  // (ms.volume may be written again)
    return volume;
}

// applyMIRCuts (cutting-strategies.ts:199-212) on the H x W tableau at A: the first TMIR_MAX_CUTS rows, in row order, whose basic variable
// is integer and whose RHS fraction lies inside [precision, 1 - precision] each get a lower-bound MIR row, rows H .. H+n-1, with
// mir_append_wg's arithmetic; the maps follow as for a branch cut.  Every cut row reads rows below H and the column map only, so the rows
// are built side by side, one (cut, column) cell per thread and step.  Returns n (uniform; 0: no row qualified), or -1 with nothing
// written when H + n rows exceed the row capacity RC.  A barrier in front (the tableau is complete) is the caller's; one behind is here.
template <int THREADS>
__device__ __forceinline__ int tmir_append(double* A, int S, int W, int H, int RC, int32_t* vibr, const int32_t* vibc, int32_t* rbv, int32_t* cbv,
                                           const uint8_t* is_int, double precision, TreeMirSm& ms) {
    int base = 0;
    for (int r0 = 1; r0 < H && base < TMIR_MAX_CUTS; r0 += THREADS) {
        const int r = r0 + (int)threadIdx.x;
        bool ok = false;
        if (r < H) {
            const int v = vibr[r];
            if (v >= 0 && is_int[v]) {  // :82-85
                const double rhs = A[r * S];
                const double f = rhs - floor(rhs);
                ok = !(f < precision || f > 1 - precision);  // :88-90
            }
        }
        int total;
        const int before = tmir_rank<THREADS>(ok, ms, &total);
        if (ok && base + before < TMIR_MAX_CUTS) ms.sel[base + before] = r;
        base += total;
    }
    __syncthreads();
    const int n = base < TMIR_MAX_CUTS ? base : TMIR_MAX_CUTS;
    if (H + n > RC) return -1;
    for (int q = threadIdx.x; q < n * W; q += THREADS) {
        const int k = q / W, col = q - k * W;
        const double* src = A + ms.sel[k] * S;
        const double rhs = src[0];
        double out;
        if (col == 0) {
            out = floor(rhs) - rhs;  // :112 then :128-130
        } else {
            const double f = rhs - floor(rhs);
            const double a = src[col];
            const int v = vibc[col];
            double cut;
            if (v >= 0 && is_int[v]) {  // :117-123
                const double fl = floor(a);
                cut = fl + js_max0(a - fl - f) / (1 - f);
            } else {
                cut = js_min0(a / (1 - f));  // :124-125
            }
            out = cut - a;  // :128-130
        }
        A[(H + k) * S + col] = out;
    }
    for (int k = threadIdx.x; k < n; k += THREADS) {  // :104-109
        const int slack = W + H - 2 + k;
        vibr[H + k] = slack;
        rbv[slack] = H + k;
        cbv[slack] = -1;
    }
    __syncthreads();
    return n;
}
#endif  // JSLP_TREE_MIR_DEVICE
