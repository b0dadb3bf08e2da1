// part_gconst64.hip (part 3 of the former rmx_kernels.hip) -- the 64-lane plain step kernels with the per-node constants in global memory
// (RMX_GLOBAL_CONSTS): four wavefronts per CU.
#define RMX_NP 64
#define RMX_GLOBAL_CONSTS
#include "rmx_kernels.h"

void RMX_CAT(launch_step_gconst_, RMX_NP)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a, bool fulln) {
    const dim3 grid(b->B), block(64);
    const size_t bytes = sizeof(double) * (size_t)acc_doubles(m->n, RMX_NP);
    if (fulln) {          // every node slot in use: the n == NP instantiation
        if (integ == INTEG_BDF1) RMX_LAUNCH((k_step_bdf1<RMX_NP, false, false, false, TAG_FULLN + 1>), grid, block, bytes, b->stream, m->dm, o, a);
        else RMX_LAUNCH((k_step_bdf2<RMX_NP, false, false, false, TAG_FULLN + 1>), grid, block, bytes, b->stream, m->dm, o, a);
        return;
    }
    if (integ == INTEG_BDF1) RMX_LAUNCH((k_step_bdf1<RMX_NP, false, false, false, 3>), grid, block, bytes, b->stream, m->dm, o, a);
    else RMX_LAUNCH((k_step_bdf2<RMX_NP, false, false, false, 3>), grid, block, bytes, b->stream, m->dm, o, a);
}
