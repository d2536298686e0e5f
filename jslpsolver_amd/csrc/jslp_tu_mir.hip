// jslp_tu_mir.hip -- the MIR builds of the LDS node kernels and k_fractional_volume (include/jslpr_mir.h) as a translation unit of their own.
//
// The product build compiles this file next to jslp_hip.hip (-DJSLP_SPLIT_TU) and the two parts of jslp_tu_resident.hip
// (__graft_entry__.build()).  As there, the kernel headers are included inside a namespace of the unit's own, so every kernel and helper
// has internal linkage and the units never meet at link time; the unit exports ONE hidden function that launches the kernel a number
// names, its arguments travelling as bytes (MirLaunch, jslp_mir_kernels.hip.h: the same struct in every unit).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stddef.h>
#include <string.h>

namespace {
#include "jslp_kernels.hip.h"
#include "jslp_mir_kernels.hip.h"
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int jslpr_mir_launch_tu(int which, unsigned grid, size_t lds, const void* args, void* stream) {
    return mir_launch_impl(which, grid, lds, args, static_cast<hipStream_t>(stream));
}
