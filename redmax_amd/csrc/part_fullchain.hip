// part_fullchain.hip (part 2 of the former rmx_kernels.hip) -- the FULLCHAIN instantiations of the plain step kernels for ONE padded tree size RMX_NP
// (16, 32, 64), and the 64-slot tree that fills every node slot.
#include "rmx_kernels.h"

void RMX_CAT(launch_step_fullchain_, RMX_NP)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a) {
    const dim3 grid(b->B), block(64);
    if (integ == INTEG_BDF1) RMX_LAUNCH((k_step_bdf1<RMX_NP, false, false, true>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
    else RMX_LAUNCH((k_step_bdf2<RMX_NP, false, false, true>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
}
#if RMX_NP == 64
// a tree that fills all 64 node slots (n == NP at compile time; LDS-resident constants)
void launch_step_fulln_64(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a) {
    const dim3 grid(b->B), block(64);
    if (integ == INTEG_BDF1) RMX_LAUNCH((k_step_bdf1<RMX_NP, false, false, false, TAG_FULLN>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
    else RMX_LAUNCH((k_step_bdf2<RMX_NP, false, false, false, TAG_FULLN>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
}
#endif
