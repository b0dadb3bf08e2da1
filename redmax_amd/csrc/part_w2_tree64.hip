// part_w2_tree64.hip (part 5 of the former rmx_kernels.hip) -- 64-node trees, two wavefronts per rollout (RMX_W2; RMX_SYNC is wave-local ordering there):
// batches of up to one rollout per two SIMDs.
#define RMX_NP 64
#define RMX_W2 1
#ifndef RMX_SYNC
#define RMX_SYNC() rmx_wave_sync()
#endif
#ifndef RMX_CONSTS
#define RMX_CONSTS(sAcc, n, NP) (rmx_smem_base() + acc_doubles((n), (NP)))
#endif
#include "rmx_kernels.h"

void launch_step_w2_64(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a, bool fullchain, bool fulln, bool energy) {
    const dim3 grid(b->B), block(128);
    const size_t smem_bytes = m->smem_bytes + ((sizeof(double) * W2_HELP_DOUBLES + 15) & ~(size_t)15);      // + the helper wave's own area
    if (fullchain) {      // a serial chain that fills every node slot: FULLCHAIN (no tree paths in the front)
        if (integ == INTEG_BDF1) RMX_LAUNCH((k_step_bdf1<RMX_NP, false, false, true, TAG_W2>), grid, block, smem_bytes, b->stream, m->dm, o, a);
        else RMX_LAUNCH((k_step_bdf2<RMX_NP, false, false, true, TAG_W2>), grid, block, smem_bytes, b->stream, m->dm, o, a);
        return;
    }
    if (fulln) {          // every node slot in use: the n == NP instantiation
        // (BDF1 without an energy record - the benchmark's launch -: the instantiation that does not carry the last evaluation's energies)
        if (!energy) RMX_LAUNCH((k_step_bdf1<RMX_NP, false, false, false, TAG_W2_NOE>), grid, block, smem_bytes, b->stream, m->dm, o, a);
        else if (integ == INTEG_BDF1) RMX_LAUNCH((k_step_bdf1<RMX_NP, false, false, false, TAG_W2>), grid, block, smem_bytes, b->stream, m->dm, o, a);
        else RMX_LAUNCH((k_step_bdf2<RMX_NP, false, false, false, TAG_W2>), grid, block, smem_bytes, b->stream, m->dm, o, a);
        return;
    }
    if (integ == INTEG_BDF1) RMX_LAUNCH((k_step_bdf1<RMX_NP, false, false, false, TAG_W2 + 1>), grid, block, smem_bytes, b->stream, m->dm, o, a);
    else RMX_LAUNCH((k_step_bdf2<RMX_NP, false, false, false, TAG_W2 + 1>), grid, block, smem_bytes, b->stream, m->dm, o, a);
}
