// part_w2_chain32.hip (part 6 of the former rmx_kernels.hip) -- full 32-link serial chains, BDF1, two wavefronts per rollout (RMX_W2): the second one
// evaluates the point that may end a solve.
#define RMX_NP 32
#define RMX_W2 1
#ifndef RMX_SYNC
#define RMX_SYNC() rmx_wave_sync()
#endif
#ifndef RMX_CONSTS
#define RMX_CONSTS(sAcc, n, NP) (rmx_smem_base() + acc_doubles((n), (NP)))
#endif
#include "rmx_kernels.h"

void launch_step_w2c_32(const rmx_model* m, const rmx_batch* b, const DevOpts& o, const StepArgs& a) {
    const dim3 grid(b->B), block(128);
    const size_t smem_bytes = m->smem_bytes + ((sizeof(double) * W2C_HELP_DOUBLES + 15) & ~(size_t)15);      // + the helper wave's own area
    RMX_LAUNCH((k_step_bdf1<RMX_NP, false, false, true, TAG_W2>), grid, block, smem_bytes, b->stream, m->dm, o, a);
}
