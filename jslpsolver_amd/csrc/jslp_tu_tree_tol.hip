// jslp_tu_tree_tol.hip -- the TOL builds of k_tree_packed (include/jslpg_tree_tolerance.h: every build's twin for the LPs with options.tolerance)
// as a translation unit of their own, compiled in two parts (-DJSLP_TOL_PART=1: the plain, OPT and MIR twins; 2: the ENH and INC twins), so
// that the units of the other pack kernels (jslp_tu_packed.hip, jslp_tu_tree_mir.hip, jslp_tu_tree_enh.hip, jslp_tu_tree_inc.hip) compile
// what they compiled before -- instruction for instruction: an LP without a tolerance pays nothing for the option -- and all run side by side
// (__graft_entry__.build()).
//
// As there, the kernel headers are included inside a namespace of the unit's own, so every kernel and helper has internal linkage and the
// units never meet at link time; each part exports ONE hidden function that launches the build a thread count names, its arguments
// travelling as bytes (PackLaunch, jslp_packed.hip.h: the same struct in every unit).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stddef.h>
#include <string.h>

#ifndef JSLP_TOL_PART
#error "compile with -DJSLP_TOL_PART=1 or 2"
#endif

namespace {
#include "jslp_kernels.hip.h"
#define JSLP_PACKED_KERNELS 1
#define JSLP_PACK_TOL 1
#define JSLP_PACK_BIG 0  // (the large builds, include/jslpb_big_lds.h: jslp_tu_packed_big.hip)
#if JSLP_TOL_PART == 1
#define JSLP_PACK_BUILDS 0x07
#else
#define JSLP_PACK_BUILDS 0x18
#endif
#include "jslp_packed.hip.h"
#include "jslp_tree.hip.h"
}  // namespace

#if JSLP_TOL_PART == 1
extern "C" __attribute__((visibility("hidden"))) int jslpg_tree_tol1_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream) {
#else
extern "C" __attribute__((visibility("hidden"))) int jslpg_tree_tol2_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream) {
#endif
    return pack_dispatch(threads, grid, lds, args, stream);
}
