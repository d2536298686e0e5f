// jslp_resident_table.hip.h -- the register-resident kernel's geometries and its INSTANCES: the one table every build flavour launches from.
// Included once per unit, behind jslp_kernels.hip.h: by jslp_hip.hip (the host code) and by each part of jslp_tu_resident.hip (inside the part's own
// namespace).  A unit instantiates the rows res_row_built() lets through and answers "not mine" (-1) for every other key:
//   * product build: jslp_hip.hip with -DJSLP_SPLIT_TU holds no row; its resident_dispatch() asks part 1, then part 2 of jslp_tu_resident.hip;
//   * single-unit build (`hipcc jslp_hip.hip`: tools/kernel_resources.py, isa_mix.py, build_dbg.sh, resident_phase_timing.py): every row, in this unit;
//   * development builds (single-unit, never shipped): -DJSLP_DEV_HEADLINE_ONLY, -DJSLP_DEV_TALL_ONLY[=2], -DJSLP_DEV_XL_ONLY keep one geometry's lean rows
//     (40 s instead of 2.5 min); a solve that needs another row is refused with RES_DEV_REFUSAL.
#pragma once

// Geometry of the register-resident kernel for a tableau: lanes x columns per lane must cover a row (ld), rows per
// workgroup x 256 workgroups the height, and rows x columns per lane must fit the lane's registers.  0 = does not fit.
//   1: <1024, 2, 8>   ld <= 2048, H <= 2048 (the headline shape)      2: <512, 4, 8>  (JSLP_RES_CPT=4, measured slower)
//   3: <512, 4, 16>   ld <= 2048, H <= 4096                            4: <512, 6, 12> ld <= 3072, H <= 3072 (3001 x 3001: 72 MB)
//   5: <512, 8, 8>    ld <= 4096, H <= 2048
//   6: <512, 2, 32> XL ld <= 1024, H <= 1024, on the <= 32 workgroups of ONE XCD (round 4): the hand-offs of a pivot go through
//      that XCD's L2 instead of memory.  Mid-size tableaus: Monster LP 625 x 553, Monster_II's root 945 x 925, 501 x 501 ...
// (256-lane geometries -- ONE wave per SIMD, 512 registers per lane: <256, 8, 8> compiles without a spill -- were measured and
//  dropped: 72.5 k against 105.7 k pivots/s on a 2001 x 2001 LP, 17.4 k on 4001 x 2001, r02_z: a lone wave per SIMD does not hide
//  its own instruction latency)
// Round 5: the XCD-local instances are compiled into the TEST library only (-DJSLP_CHAOS_BUILD implies -DJSLP_WITH_XL; a hipcc run with
// -DJSLP_WITH_XL builds a product-like library with them): the default policy never picked the geometry (parity with the chip-wide kernel on
// an eighth of the chip, profiles/r04_xl_times.md), and its two instances cost the shipped library 40 s of compile time and 320 spilled
// SGPRs of dead weight.  The shipped library ignores JSLP_XL and refuses JSLP_FORCE_PATH=xl loudly (jslp_engine_create).
struct ResGeom { int threads, cols, rows, max_ld; };  // lanes per workgroup, columns per lane, rows per workgroup, widest padded row
static constexpr ResGeom RES_GEOM[7] = {{0, 0, 0, 0}, {1024, 2, 8, 2048}, {512, 4, 8, 2048}, {512, 4, 16, 2048}, {512, 6, 12, 3072}, {512, 8, 8, 4096}, {512, 2, 32, 1024}};
static constexpr int RES_GEOM_XL = 6;

// ---- which rows of the table this unit builds ---------------------------------------------------------------------------------------
#ifndef JSLP_TU_PART
#define JSLP_TU_PART 0  // not a part of jslp_tu_resident.hip: every row (part 1: the 1024-lane geometry and <512, 4, 8>; part 2: the rest)
#endif
#ifdef JSLP_WITH_XL
static constexpr bool RES_WITH_XL = true;
#else
static constexpr bool RES_WITH_XL = false;
#endif
#ifdef JSLP_DEV_HEADLINE_ONLY
static constexpr bool RES_DEV_HEADLINE = true;
#else
static constexpr bool RES_DEV_HEADLINE = false;
#endif
#ifdef JSLP_DEV_TALL_ONLY
static constexpr int RES_DEV_TALL = JSLP_DEV_TALL_ONLY;  // (register budget work; 2: the OPT rows)
#else
static constexpr int RES_DEV_TALL = 0;
#endif
#ifdef JSLP_DEV_XL_ONLY
static constexpr bool RES_DEV_XL = true;  // (implies -DJSLP_WITH_XL: jslp_hip.hip)
#else
static constexpr bool RES_DEV_XL = false;
#endif
static constexpr const char* RES_DEV_REFUSAL = RES_DEV_HEADLINE ? "development build: headline lean geometry only"
                                               : RES_DEV_TALL   ? "development build: tall lean geometry only"
                                               : RES_DEV_XL     ? "development build: XCD-local geometry only"
                                                                : nullptr;
constexpr bool res_row_built(int T, int C, int R, bool unr, bool lean, bool opt, bool xl) {
    if (xl && !RES_WITH_XL) return false;
    if (JSLP_TU_PART != 0 && (JSLP_TU_PART == 1) != (!xl && R == 8 && C <= 4)) return false;
    if (RES_DEV_HEADLINE) return T == 1024 && lean && !unr && !opt;
    if (RES_DEV_TALL) return R == 16 && lean && !unr && opt == (RES_DEV_TALL == 2);
    if (RES_DEV_XL) return xl;
    return true;
}

// key: {threads, columns per lane, rows per workgroup, unr, lean, opt, chk, xl}, flags 0 / 1; chk of the general build (lean 0) is 1: it is compiled
// with CHK = true and reads check_cycles at run time.  resident_dispatch() returns the hipError_t of the launch, or -1: no such instance in this unit.
#if !defined(JSLP_SPLIT_TU)
// one row: launches when the key is its own.  A row this unit does not build instantiates nothing
template <int T, int C, int R, bool UNR, bool LEAN, bool OPT, bool CHK, bool XL>
static bool launch(const int* key, unsigned grid, const void* rc_bytes, hipStream_t s, int* le) {
    if constexpr (!res_row_built(T, C, R, UNR, LEAN, OPT, XL)) {
        return false;
    } else {
        const int mine[8] = {T, C, R, UNR, LEAN, OPT, CHK, XL};
        if (memcmp(mine, key, sizeof mine) != 0) return false;
        ResCtx rc = *static_cast<const ResCtx*>(rc_bytes);  // (travels as bytes between the units: the same struct in each -- same headers, same flags)
        void* args[] = {&rc};
        // XCD-local: every JSLP_XL_SPREAD-th block of the grid works (all of them on one XCD), the others return at once
        *le = (int)hipLaunchCooperativeKernel((const void*)k_simplex_resident<T, C, R, UNR, LEAN, OPT, CHK, XL>, dim3(XL ? JSLP_XL_SPREAD * grid : grid), dim3(T), args, 0, s);
        return true;
    }
}
// THE table.  Lean rows: unrestricted variables x cycle check; optional objectives (no unrestricted variables) where the lane has the registers for
// three more rows: <1024, 2, 8> and <512, 4, 16>; a general build (what a lean solve whose cycle-check history outgrew LDS is handed to) of the 8-row
// geometries only: on the tall / wide ones it spilled ~0.5 KB per lane and lost to the streaming kernels.
// (the rows' order is the order the compiler instantiates the kernels in, and their code can depend on it: a new row goes where tools/asm_digest.py
//  shows every kernel's assembly unchanged)
static int resident_dispatch(const int* key, unsigned grid, const void* rc, hipStream_t s) {
    int le = -1;
    (void)(launch<512, 2, 32, false, true, false, true, true>(key, grid, rc, s, &le) ||
           launch<512, 2, 32, false, true, false, false, true>(key, grid, rc, s, &le) ||
           launch<1024, 2, 8, false, true, true, true, false>(key, grid, rc, s, &le) ||
           launch<1024, 2, 8, false, true, true, false, false>(key, grid, rc, s, &le) ||
           launch<1024, 2, 8, true, true, false, true, false>(key, grid, rc, s, &le) ||
           launch<1024, 2, 8, true, true, false, false, false>(key, grid, rc, s, &le) ||
           launch<1024, 2, 8, false, true, false, true, false>(key, grid, rc, s, &le) ||
           launch<1024, 2, 8, false, true, false, false, false>(key, grid, rc, s, &le) ||
           launch<1024, 2, 8, true, false, false, true, false>(key, grid, rc, s, &le) ||
           launch<1024, 2, 8, false, false, false, true, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 8, true, true, false, true, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 8, true, true, false, false, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 8, false, true, false, true, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 8, false, true, false, false, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 8, true, false, false, true, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 8, false, false, false, true, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 16, false, true, true, true, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 16, false, true, true, false, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 16, true, true, false, true, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 16, true, true, false, false, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 16, false, true, false, true, false>(key, grid, rc, s, &le) ||
           launch<512, 4, 16, false, true, false, false, false>(key, grid, rc, s, &le) ||
           launch<512, 6, 12, true, true, false, true, false>(key, grid, rc, s, &le) ||
           launch<512, 6, 12, true, true, false, false, false>(key, grid, rc, s, &le) ||
           launch<512, 6, 12, false, true, false, true, false>(key, grid, rc, s, &le) ||
           launch<512, 6, 12, false, true, false, false, false>(key, grid, rc, s, &le) ||
           launch<512, 8, 8, true, true, false, true, false>(key, grid, rc, s, &le) ||
           launch<512, 8, 8, true, true, false, false, false>(key, grid, rc, s, &le) ||
           launch<512, 8, 8, false, true, false, true, false>(key, grid, rc, s, &le) ||
           launch<512, 8, 8, false, true, false, false, false>(key, grid, rc, s, &le));
    return le;
}
#else
// the product's main unit: the rows live in jslp_tu_resident.hip, whose two parts export this same dispatch over their share of the rows each
extern "C" __attribute__((visibility("hidden"))) int jslpx_resident_launch_1(const int* key, unsigned grid, const void* rc, void* stream);
extern "C" __attribute__((visibility("hidden"))) int jslpx_resident_launch_2(const int* key, unsigned grid, const void* rc, void* stream);
static int resident_dispatch(const int* key, unsigned grid, const void* rc, hipStream_t s) {
    const int le = jslpx_resident_launch_1(key, grid, rc, s);
    return le != -1 ? le : jslpx_resident_launch_2(key, grid, rc, s);
}
#endif
