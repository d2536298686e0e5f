// jslp_tu_packed_big.hip -- the LARGE builds of k_simplex_packed and k_tree_packed (include/jslpb_big_lds.h): the LPs whose LDS image lies
// between 64 KiB and the 156 KiB a workgroup with a compute unit to itself can have, at ONE thread count (JSLP_PACK_BIG_THREADS,
// jslp_packed.hip.h), each kernel plain and with optional objectives, as a translation unit of their own -- so that the units of the other
// pack kernels compile what they compiled before, instruction for instruction.
//
// The kernels are the templates of jslp_packed.hip.h and jslp_tree.hip.h at that thread count, not a second text: every loop there strides by
// THREADS, the row update's CW x RP grid covers any power of two, the reductions meet in Smem's sixteen wave slots (block_reduce reads
// blockDim), and the DevState copy is one wave's whatever the workgroup's size.
//
// As in the other units, the kernel headers are included inside a namespace of the unit's own, so every kernel and helper has internal
// linkage and the units never meet at link time; the unit exports ONE hidden function that launches the build a thread count names, its
// arguments travelling as bytes (PackLaunch, jslp_packed.hip.h: the same struct in every unit).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stddef.h>
#include <string.h>

namespace {
#include "jslp_kernels.hip.h"
#define JSLP_PACKED_KERNELS 1
#define JSLP_PACK_TOL 0        // (no large build has a TOL twin)
#define JSLP_PACK_BIG 1        // the large builds alone
#define JSLP_PACK_BUILDS 0x03  // k_simplex_packed and the default service's k_tree_packed, plain and OPT
#include "jslp_packed.hip.h"
#include "jslp_tree.hip.h"
// what the kernels declare as static __shared__ objects (k_simplex_packed: PackSmem; k_tree_packed: TreeSmem, which holds one, and TreeMirSm,
// which only a MIR build keeps) stays within the reserve between JSLPB_LDS_LIMIT and the compute unit's 160 KiB
static_assert(sizeof(PackSmem) + sizeof(TreeSmem) + sizeof(TreeMirSm) <= PACK_CU_LDS - PACK_BIG_LDS, "the kernels' static LDS fits the 4 KiB reserve");
static_assert(JSLP_PACK_BIG_THREADS / 64 <= (int)(sizeof(Smem::wave) / sizeof(Cand)), "block_reduce has a slot per wave");
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int jslpb_packed_big_launch_tu(int threads, unsigned grid, size_t lds, const void* args, void* stream) {
    return pack_dispatch(threads, grid, lds, args, stream);
}
