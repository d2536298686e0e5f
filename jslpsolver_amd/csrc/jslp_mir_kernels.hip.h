// jslp_mir_kernels.hip.h -- the MIR builds of the LDS node kernels (include/jslpr_mir.h) and k_fractional_volume, with the one function
// that launches them.  Included behind jslp_kernels.hip.h by jslp_tu_mir.hip -- the product: a translation unit of their own, because
// the order of instantiation changes the register allocation of OTHER kernels (see the node-kernel table of jslp_hip.hip) -- and by
// jslp_hip.hip itself in a single-unit build.
//
// k_node_lds_mir / k_node_queue_mir are k_node_lds / k_node_queue (jslp_wglds.hip.h) with eager slots, no optional objectives and
// node_lds_run's MIR build: kernels of their own rather than one more template parameter of those two, whose symbols -- what
// tools/asm_digest.py keys its table by -- stay as they are.
#pragma once

template <int THREADS>
__global__ void __launch_bounds__(THREADS, THREADS == 512 ? JSLP_NODE512_WAVES : 4) k_node_lds_mir(Slots s, Snapshot snap, Cuts cuts, MirJob mj, int first_node,
                                                      int check_cycles, int iters_cap, int cap_rows, double* rhs_out, int32_t* rows_out,
                                                      DevState* state_out, int out_stride, int first_out,
                                                      unsigned* done_flag, unsigned done_seq, int* done_count) {
    extern __shared__ __attribute__((aligned(16))) double lds_dyn[];
    __shared__ SmemL sm;
    const WgLds L = wglds_carve(lds_dyn, s.ld, cap_rows);
    node_lds_run<THREADS, false, false, true>(s, snap, cuts, sm, L, blockIdx.x, first_node + blockIdx.x, first_out + blockIdx.x, check_cycles,
                                              iters_cap, cap_rows, rhs_out, rows_out, state_out, out_stride, &mj);
    if (done_flag) {  // the completion flag of k_node_lds: one node, or the last workgroup of a small batch
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
            bool last = true;
            if (done_count) {
                last = atomicAdd(done_count, 1) == (int)gridDim.x - 1;
                if (last) { *done_count = 0; __threadfence_system(); }
            }
            if (last) __hip_atomic_store(done_flag, done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS, THREADS == 512 ? JSLP_NODE512_WAVES : 4) k_node_queue_mir(Slots s, Snapshot snap, Cuts cuts, MirJob mj, int n_nodes,
                                                      const int32_t* order, int* queue, int check_cycles, int iters_cap, int cap_rows,
                                                      double* rhs_out, int32_t* rows_out, DevState* state_out, int out_stride) {
    extern __shared__ __attribute__((aligned(16))) double lds_dyn[];
    __shared__ SmemL sm;
    __shared__ int q_next;
    const WgLds L = wglds_carve(lds_dyn, s.ld, cap_rows);
    for (;;) {
        if (threadIdx.x == 0) q_next = atomicAdd(queue, 1);
        __syncthreads();
        const int k = q_next;
        __syncthreads();
        if (k >= n_nodes) break;
        const int node = order ? order[k] : k;
        int slot = blockIdx.x;
        asm volatile("" : "+s"(slot));  // opaque per iteration, as in k_node_queue
        node_lds_run<THREADS, false, false, true>(s, snap, cuts, sm, L, slot, node, node, check_cycles, iters_cap, cap_rows, rhs_out, rows_out, state_out,
                                                  out_stride, &mj);
        __syncthreads();
    }
}

// computeFractionalVolume(true) of the live tableau (slot 0) for the shapes whose MIR loop the host sequences launch by launch: one
// workgroup, the contributing rows compacted in row order into the slot's pivot-column vector (free between two simplexes), one
// lane multiplies.  Only the 8-byte result crosses to the host.
__global__ void __launch_bounds__(256) k_fractional_volume(Slots s, const uint8_t* is_int, double* out) {
    __shared__ MirSm ms;
    const int H = s.st->H;
    int base = 0;
    for (int r0 = 1; r0 < H; r0 += 256) {
        const int r = r0 + (int)threadIdx.x;
        bool ok = false;
        double distance = 0.0;
        if (r < H) {
            const int v = s.vibr[r];
            if (v >= 0 && is_int[v]) {
                distance = fabs(s.A[(long long)r * s.ld]);
                const double a = distance - floor(distance), b = floor(distance + 1);
                const bool nan = a != a || b != b;
                ok = nan || !((a < b ? a : b) < s.precision);
            }
        }
        int total;
        const int before = mir_rank(ok, ms, &total);
        if (ok) s.pcol[base + before] = distance;
        base += total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double volume = -1.0;
        for (int i = 0; i < base; i++) volume = volume == -1.0 ? s.pcol[i] : volume * s.pcol[i];
        *out = volume == -1.0 ? 0.0 : volume;
    }
}

// launches kernel `which` (MIR_K_*); returns the hipError_t of the launch, or -1 for an unknown kernel.  The error is PEEKED at, not taken:
// the caller's hipGetLastError (launch_node_kernel, device_volume) still sees it and reports it
static int mir_launch_impl(int which, unsigned grid, size_t lds, const void* bytes, hipStream_t st) {
    const MirLaunch a = *static_cast<const MirLaunch*>(bytes);
    switch (which) {
        case MIR_K_NODE_LDS_1024:
            hipLaunchKernelGGL(k_node_lds_mir<1024>, dim3(grid), dim3(1024), lds, st, a.s, a.sn, a.cu, a.mj, a.first, a.check_cycles, a.iters_cap, a.cap_rows, a.rhs,
                               a.rows, a.states, a.out_stride, a.first, a.done_flag, a.done_seq, a.done_count);
            break;
        case MIR_K_NODE_LDS_512:
            hipLaunchKernelGGL(k_node_lds_mir<512>, dim3(grid), dim3(512), lds, st, a.s, a.sn, a.cu, a.mj, a.first, a.check_cycles, a.iters_cap, a.cap_rows, a.rhs,
                               a.rows, a.states, a.out_stride, a.first, a.done_flag, a.done_seq, a.done_count);
            break;
        case MIR_K_NODE_QUEUE_512:
            hipLaunchKernelGGL(k_node_queue_mir<512>, dim3(grid), dim3(512), lds, st, a.s, a.sn, a.cu, a.mj, a.n_nodes, a.order, a.queue, a.check_cycles, a.iters_cap,
                               a.cap_rows, a.rhs, a.rows, a.states, a.out_stride);
            break;
        case MIR_K_VOLUME:
            hipLaunchKernelGGL(k_fractional_volume, dim3(1), dim3(256), 0, st, a.s, a.mj.is_int, a.volume_out);
            break;
        default:
            return -1;
    }
    return (int)hipPeekAtLastError();
}
