// part_ct.hip (part 1 of the former rmx_kernels.hip) -- the extended (CT) instantiations of eval / step / energy / mfd for ONE padded tree size RMX_NP:
// scenes with ForceGroundCuboid or JointSpherical.
#include "rmx_kernels.h"

void RMX_CAT(launch_eval_ct_, RMX_NP)(const rmx_model* m, const rmx_batch* b, bool wantH, double eta, double* dg, double* dH) {
    const dim3 grid(b->B), block(64);
    if (wantH) RMX_LAUNCH((k_eval<RMX_NP, true, true>), grid, block, m->smem_bytes, b->stream, m->dm, b->B, b->tmpA, b->tmpB, b->tmpC, eta, dg, dH, b->chart);
    else RMX_LAUNCH((k_eval<RMX_NP, false, true>), grid, block, m->smem_bytes, b->stream, m->dm, b->B, b->tmpA, b->tmpB, b->tmpC, eta, dg, dH, b->chart);
}
void RMX_CAT(launch_mfd_ct_, RMX_NP)(const rmx_model* m, const rmx_batch* b, double* dM, double* df, double* dD) {
    const dim3 grid(b->B), block(64);
    RMX_LAUNCH((k_eval_mfd<RMX_NP, true>), grid, block, m->smem_bytes, b->stream, m->dm, b->B, b->tmpA, b->tmpB, dM, df, dD, b->chart);
}
// contact_pass false: the lean launch alone (scenes without ForceGroundCuboid; serial chains of <= 32 nodes, whose steps with the
// contact terms part_ground32.hip's launch_step_pair_32 takes)
void RMX_CAT(launch_step_ct_, RMX_NP)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a, bool contact_pass) {
    const dim3 grid(b->B), block(64);
    // every trajectory as far as it stays clear of the ground (all the way in scenes without ForceGroundCuboid) ...
    if (integ == INTEG_BDF1) RMX_LAUNCH((k_step_bdf1<RMX_NP, true, true>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
    else RMX_LAUNCH((k_step_bdf2<RMX_NP, true, true>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
    if (!contact_pass) return;
    // ... and the rest of its steps with the contact terms
    if (integ == INTEG_BDF1) RMX_LAUNCH((k_step_bdf1<RMX_NP, true>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
    else RMX_LAUNCH((k_step_bdf2<RMX_NP, true>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
}
void RMX_CAT(launch_energy_ct_, RMX_NP)(const rmx_model* m, const rmx_batch* b, double* dT, double* dV) {
    const dim3 grid(b->B), block(64);
    RMX_LAUNCH((k_energy<RMX_NP, true>), grid, block, m->smem_bytes, b->stream, m->dm, b->B, b->q, b->qd, dT, dV, b->chart);
}
