// part_adjhelp16.hip (part 8 of the former rmx_kernels.hip) -- the adjoint forward sweep of trees of <= 16 nodes with a second wavefront per rollout that
// forms and stores M, D (k_adjoint_fwd HELP).  Two wavefronts per workgroup: RMX_SYNC is wave-local ordering, the hand-over has its
// own workgroup barrier.
#define RMX_NP 16
#ifndef RMX_SYNC
#define RMX_SYNC() rmx_lane_sync()      // (see rmx_lane_sync)
#endif
#include "rmx_kernels.h"

void launch_adjoint_help_16(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a, bool fullchain) {
    const dim3 grid(b->B);
    const size_t smem_bytes = m->smem_bytes + sizeof(double) * adj_hand_doubles(RMX_NP);
    if (integ == INTEG_BDF1 && fullchain) {      // (configs[3]: the full 16-link chain)
        RMX_LAUNCH((k_adjoint_fwd<RMX_NP, 1, true, true>), grid, dim3(128), smem_bytes, b->stream, m->dm, o, a);
        k_adjoint_bwd<RMX_NP, 1, true><<<grid, dim3(64), 0, b->stream>>>(m->dm, o, a);
    } else if (fullchain) {
        RMX_LAUNCH((k_adjoint_fwd<RMX_NP, 2, true, true>), grid, dim3(128), smem_bytes, b->stream, m->dm, o, a);
        k_adjoint_bwd<RMX_NP, 2, true><<<grid, dim3(64), 0, b->stream>>>(m->dm, o, a);
    } else if (integ == INTEG_BDF1) {
        RMX_LAUNCH((k_adjoint_fwd<RMX_NP, 1, true>), grid, dim3(128), smem_bytes, b->stream, m->dm, o, a);
        k_adjoint_bwd<RMX_NP, 1><<<grid, dim3(64), 0, b->stream>>>(m->dm, o, a);
    } else {
        RMX_LAUNCH((k_adjoint_fwd<RMX_NP, 2, true>), grid, dim3(128), smem_bytes, b->stream, m->dm, o, a);
        k_adjoint_bwd<RMX_NP, 2><<<grid, dim3(64), 0, b->stream>>>(m->dm, o, a);
    }
}
