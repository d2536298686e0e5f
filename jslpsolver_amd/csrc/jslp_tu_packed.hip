// jslp_tu_packed.hip -- the builds of k_simplex_packed and k_tree_packed (include/jslpp_packed.h, jslpt_tree.h, jslps_soft.h: 64 or 256
// threads, each with or without optional objectives) as a translation unit of their own.
//
// The product build compiles this file next to jslp_hip.hip (-DJSLP_SPLIT_TU), the two parts of jslp_tu_resident.hip and jslp_tu_mir.hip
// (__graft_entry__.build()).  As there, the kernel headers are included inside a namespace of the unit's own, so every kernel and helper
// has internal linkage and the units never meet at link time; the unit exports ONE hidden function that launches the build a thread count
// names, its arguments travelling as bytes (PackLaunch, jslp_packed.hip.h: the same struct in every unit).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stddef.h>
#include <string.h>

namespace {
#include "jslp_kernels.hip.h"
#define JSLP_PACKED_KERNELS 1
#define JSLP_PACK_TOL 0  // (the TOL twins of these builds: jslp_tu_tree_tol.hip)
#define JSLP_PACK_BIG 0  // (the large builds, include/jslpb_big_lds.h: jslp_tu_packed_big.hip)
#define JSLP_PACK_BUILDS 0x03  // (the MIR, ENH and INC builds of k_tree_packed: jslp_tu_tree_mir.hip, jslp_tu_tree_enh.hip, jslp_tu_tree_inc.hip)
#include "jslp_packed.hip.h"
#include "jslp_tree.hip.h"  // k_tree_packed (include/jslpt_tree.h): the same LDS layout, the loop as pk_simplex
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int jslpp_packed_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream) {
    return pack_dispatch(threads, grid, lds, args, stream);
}
