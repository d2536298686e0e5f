// jslp_tu_resident.hip -- the register-resident kernel's INSTANCES as translation units of their own (round 6).
//
// jslp_hip.hip used to be one translation unit with ~90 kernel instantiations, 30 of them k_simplex_resident<...> (7-15 k instructions each):
// 2.5 minutes per library whatever was edited.  The product build compiles jslp_hip.hip with -DJSLP_SPLIT_TU -- host code, the small
// kernels, the node kernels, the fused pipeline; no resident instance -- and this file twice, -DJSLP_TU_PART=1 (the 1024-lane geometries and
// <512,4,8>) and -DJSLP_TU_PART=2 (the tall / wide 512-lane geometries, the XCD-local build of the test library), all three side by side
// (__graft_entry__.build()).  A part exports ONE hidden function that launches the instance a key names, or says "not mine": the dispatch of
// jslp_resident_table.hip.h -- THE table of instances, the same text in every build flavour -- compiled here over the part's share of its rows.
// The kernel headers are included inside a namespace of the part's own: every kernel and every helper gets internal linkage, so the parts and
// the main unit never meet at link time; ResCtx travels as bytes (the same struct in every unit: same headers, same flags).
// (A single-unit build -- `hipcc jslp_hip.hip` without -DJSLP_SPLIT_TU, what tools/kernel_resources.py / isa_mix.py and the development
//  builds use -- is still whole: same kernels, same instances.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stddef.h>
#include <string.h>

#ifndef JSLP_TU_PART
#error "compile with -DJSLP_TU_PART=1 or 2"
#endif
#if defined(JSLP_CHAOS_BUILD) && !defined(JSLP_WITH_XL)
#define JSLP_WITH_XL 1
#endif

namespace {
#include "jslp_kernels.hip.h"
#include "jslp_resident_table.hip.h"
}  // namespace

#if JSLP_TU_PART == 1
extern "C" __attribute__((visibility("hidden"))) int jslpx_resident_launch_1(const int* key, unsigned grid, const void* rc, void* stream) {
#else
extern "C" __attribute__((visibility("hidden"))) int jslpx_resident_launch_2(const int* key, unsigned grid, const void* rc, void* stream) {
#endif
    return resident_dispatch(key, grid, rc, static_cast<hipStream_t>(stream));
}
