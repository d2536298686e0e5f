// jslp_tu_tree_enh.hip -- the ENH builds of k_tree_packed (include/jslpe_tree_enhanced.h: 64 or 256 threads) as a translation unit of their
// own, so that the units of the other pack kernels (jslp_tu_packed.hip, jslp_tu_tree_mir.hip) compile what they compiled before and the
// three run side by side (__graft_entry__.build()).
//
// As there, the kernel headers are included inside a namespace of the unit's own, so every kernel and helper has internal linkage and the
// units never meet at link time; the unit exports ONE hidden function that launches the build a thread count names, its arguments
// travelling as bytes (PackLaunch, jslp_packed.hip.h: the same struct in every unit).
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
#define JSLP_PACK_BUILDS 0x08  // pk_simplex alone: k_simplex_packed is jslp_tu_packed.hip's, and so are the plain and OPT builds of k_tree_packed
#include "jslp_packed.hip.h"
#include "jslp_tree.hip.h"
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int jslpe_tree_enh_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream) {
    return pack_dispatch(threads, grid, lds, args, stream);
}
