// part_adjhelp16.hip (part 8 of the former rmx_kernels.hip) -- the adjoint forward sweep of trees of <= 16 nodes with a second wavefront per rollout that
// forms and stores M, D (k_adjoint_fwd HELP).  Two wavefronts per workgroup: RMX_SYNC is wave-local ordering, the hand-over has its
// own workgroup barrier.
#define RMX_NP 16
#ifndef RMX_SYNC
#define RMX_SYNC() rmx_lane_sync()      // (see rmx_lane_sync)
#endif
#include "rmx_kernels.h"

// (MODE: the integrator, + ADJ_CTL per-step controls, where a null a.dPdu asks for the forward sweep alone, + ADJ_TRK the tracking
// objective, whose kept iterate lies behind the hand-over buffers)
template <int MODE, bool FC>
static void adjoint_help_pair(const rmx_model* m, const rmx_batch* b, const DevOpts& o, const AdjArgs& a) {
    const dim3 grid(b->B);
    const size_t smem_bytes = m->smem_bytes + sizeof(double) * (adj_hand_doubles(RMX_NP) + ((MODE & ADJ_TRK) ? adj_trk_doubles(RMX_NP) : 0));
    RMX_LAUNCH((k_adjoint_fwd<RMX_NP, MODE, true, FC>), grid, dim3(128), smem_bytes, b->stream, m->dm, o, a);
    if (!(MODE & ADJ_CTL) || a.dPdu) k_adjoint_bwd<RMX_NP, MODE, FC><<<grid, dim3(64), 0, b->stream>>>(m->dm, o, a);
}
// rmx_rollout_tape / rmx_rollout_vjp: the two kernels of the TAPE instantiation, one per call (a.tape: 1 forward, 2 backward; BDF1)
template <bool FC>
static void adjoint_help_tape(const rmx_model* m, const rmx_batch* b, const DevOpts& o, const AdjArgs& a) {
    const dim3 grid(b->B);
    const size_t smem_bytes = m->smem_bytes + sizeof(double) * adj_hand_doubles(RMX_NP);
    if (a.tape == 1) RMX_LAUNCH((k_adjoint_fwd<RMX_NP, 1 | ADJ_CTL | ADJ_TAPE, true, FC>), grid, dim3(128), smem_bytes, b->stream, m->dm, o, a);
    else k_adjoint_bwd<RMX_NP, 1 | ADJ_CTL | ADJ_TAPE, FC><<<grid, dim3(64), 0, b->stream>>>(m->dm, o, a);
}
template <bool FC>
static void adjoint_help_pairs(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a) {
    if (a.tape) {
        adjoint_help_tape<FC>(m, b, o, a);
    } else if (integ == INTEG_BDF1) {
        if (a.trk) adjoint_help_pair<1 | ADJ_CTL | ADJ_TRK, FC>(m, b, o, a);
        else if (a.u) adjoint_help_pair<1 | ADJ_CTL, FC>(m, b, o, a);
        else adjoint_help_pair<1, FC>(m, b, o, a);
    } else {
        if (a.trk) adjoint_help_pair<2 | ADJ_CTL | ADJ_TRK, FC>(m, b, o, a);
        else if (a.u) adjoint_help_pair<2 | ADJ_CTL, FC>(m, b, o, a);
        else adjoint_help_pair<2, FC>(m, b, o, a);
    }
}

void launch_adjoint_help_16(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a, bool fullchain) {
    if (fullchain) adjoint_help_pairs<true>(m, b, integ, o, a);      // (configs[3]: the full 16-link chain)
    else adjoint_help_pairs<false>(m, b, integ, o, a);
}
