// part_plain.hip (part 0 of the former rmx_kernels.hip) -- the plain kernels for ONE padded tree size RMX_NP (every scene without ForceGroundCuboid /
// JointSpherical) plus Euler, adjoint, phase timing.
#include "rmx_kernels.h"
#include "rmx_linearize.h"
#include "rmx_jvp.h"
#include "rmx_params.h"
#include "rmx_jvp_params.h"
#include "rmx_cost.h"
#if RMX_NP <= 32
#include "rmx_lqr.h"
#include "rmx_search.h"
#endif

void RMX_CAT(launch_eval_, RMX_NP)(const rmx_model* m, const rmx_batch* b, bool wantH, double eta, double* dg, double* dH) {
    const dim3 grid(b->B), block(64);
    if (wantH) RMX_LAUNCH((k_eval<RMX_NP, true, false>), grid, block, m->smem_bytes, b->stream, m->dm, b->B, b->tmpA, b->tmpB, b->tmpC, eta, dg, dH, nullptr);
    else RMX_LAUNCH((k_eval<RMX_NP, false, false>), grid, block, m->smem_bytes, b->stream, m->dm, b->B, b->tmpA, b->tmpB, b->tmpC, eta, dg, dH, nullptr);
}

void RMX_CAT(launch_step_plain_, RMX_NP)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a) {
    const dim3 grid(b->B), block(64);
    if (integ == INTEG_BDF1) RMX_LAUNCH((k_step_bdf1<RMX_NP, false>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
    else RMX_LAUNCH((k_step_bdf2<RMX_NP, false>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
}

void RMX_CAT(launch_euler_, RMX_NP)(const rmx_model* m, const rmx_batch* b, double h, const StepArgs& a) {
    const dim3 grid(b->B), block(64);
    RMX_LAUNCH((k_step_euler<RMX_NP>), grid, block, m->smem_bytes, b->stream, m->dm, h, a);
}

void RMX_CAT(launch_energy_, RMX_NP)(const rmx_model* m, const rmx_batch* b, double* dT, double* dV) {
    const dim3 grid(b->B), block(64);
    RMX_LAUNCH((k_energy<RMX_NP, false>), grid, block, m->smem_bytes, b->stream, m->dm, b->B, b->q, b->qd, dT, dV, nullptr);
}

// the adjoint pair of one instantiation (MODE: the integrator, + ADJ_CTL per-step controls, where a null a.dPdu asks for the forward sweep alone,
// + ADJ_TRK the tracking objective, whose forward kernel keeps an iterate in an LDS area of its own behind the constants)
template <int MODE, bool FC>
static void adjoint_pair(const rmx_model* m, const rmx_batch* b, const DevOpts& o, const AdjArgs& a) {
    const dim3 grid(b->B), block(64);
    const size_t smem_bytes = m->smem_bytes + ((MODE & ADJ_TRK) ? sizeof(double) * adj_trk_doubles(RMX_NP) : 0);
    RMX_LAUNCH((k_adjoint_fwd<RMX_NP, MODE, false, FC>), grid, block, smem_bytes, b->stream, m->dm, o, a);
    if (!(MODE & ADJ_CTL) || a.dPdu) k_adjoint_bwd<RMX_NP, MODE, FC><<<grid, block, 0, b->stream>>>(m->dm, o, a);
}
// rmx_rollout_tape / rmx_rollout_tape_bdf2 / rmx_rollout_vjp: the two kernels of the TAPE instantiation, one per call (a.tape: 1 forward,
// 2 backward).  The BDF2 tape (nsteps + 1 slots per rollout) has a backward kernel of its own.
template <bool FC>
static void adjoint_tape(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a) {
    const dim3 grid(b->B), block(64);
    if (integ == INTEG_BDF1) {
        if (a.tape == 1) RMX_LAUNCH((k_adjoint_fwd<RMX_NP, 1 | ADJ_CTL | ADJ_TAPE, false, FC>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
        else k_adjoint_bwd<RMX_NP, 1 | ADJ_CTL | ADJ_TAPE, FC><<<grid, block, 0, b->stream>>>(m->dm, o, a);
    } else {
        if (a.tape == 1) RMX_LAUNCH((k_adjoint_fwd<RMX_NP, 2 | ADJ_CTL | ADJ_TAPE, false, FC>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
        else k_rollout_bwd_bdf2<RMX_NP, FC><<<grid, block, 0, b->stream>>>(m->dm, o, a);
    }
}
template <bool FC>
static void adjoint_pairs(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a) {
    if (a.tape) {
        adjoint_tape<FC>(m, b, integ, o, a);
    } else if (integ == INTEG_BDF1) {
        if (a.trk) adjoint_pair<1 | ADJ_CTL | ADJ_TRK, FC>(m, b, o, a);
        else if (a.u) adjoint_pair<1 | ADJ_CTL, FC>(m, b, o, a);
        else adjoint_pair<1, FC>(m, b, o, a);
    } else {
        if (a.trk) adjoint_pair<2 | ADJ_CTL | ADJ_TRK, FC>(m, b, o, a);
        else if (a.u) adjoint_pair<2 | ADJ_CTL, FC>(m, b, o, a);
        else adjoint_pair<2, FC>(m, b, o, a);
    }
}

void RMX_CAT(launch_adjoint_, RMX_NP)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a) {
    adjoint_pairs<false>(m, b, integ, o, a);
}
#if RMX_NP == 16
// the full 16-link chain: the instantiation part_adjhelp16.hip runs with its helper wave
void launch_adjoint_fullchain_16(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a) {
    adjoint_pairs<true>(m, b, integ, o, a);
}
#endif

// rmx_rollout_tape_feedback: the forward sweep of the tape under per-step affine state feedback (ADJ_FB, rmx_feedback.h).  Always this
// generic one-wavefront kernel (rmx_select.h select_rollout_feedback); the backward sweeps that read its tape are adjoint_tape's
void RMX_CAT(launch_rollout_feedback_, RMX_NP)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a) {
    const dim3 grid(b->B), block(64);
    if (integ == INTEG_BDF1) RMX_LAUNCH((k_adjoint_fwd<RMX_NP, 1 | ADJ_CTL | ADJ_TAPE | ADJ_FB, false, false>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
    else RMX_LAUNCH((k_adjoint_fwd<RMX_NP, 2 | ADJ_CTL | ADJ_TAPE | ADJ_FB, false, false>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
}

// rmx_rollout_vjp_feedback: the closed-loop backward sweep of the tape (rmx_feedback_bwd.h).  Always this generic one-wavefront kernel
// (rmx_select.h select_rollout_vjp_feedback)
void RMX_CAT(launch_vjp_feedback_, RMX_NP)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a) {
    const dim3 grid(b->B), block(64);
    if (integ == INTEG_BDF1) k_rollout_bwd_fb<RMX_NP, 1><<<grid, block, 0, b->stream>>>(m->dm, o, a);
    else k_rollout_bwd_fb<RMX_NP, 2><<<grid, block, 0, b->stream>>>(m->dm, o, a);
}

// rmx_rollout_linearize: every slot of the tape at once
void RMX_CAT(launch_linearize_, RMX_NP)(const rmx_model* m, const rmx_batch* b, const LinArgs& a) {
    const dim3 grid((unsigned)((size_t)b->B * a.nslots)), block(64);
    k_rollout_linearize<RMX_NP><<<grid, block, 0, b->stream>>>(m->dm, a);
}

#if RMX_NP <= 32
// rmx_rollout_lqr: one workgroup per rollout, the whole sweep in LDS (rmx_select.h select_rollout_lqr: the sizes it exists for, its LDS)
void RMX_CAT(launch_lqr_, RMX_NP)(const rmx_model* m, const rmx_batch* b, const LqrArgs& a, size_t lds_bytes) {
    const dim3 grid(b->B), block(LQR_THREADS);
    RMX_LAUNCH((k_rollout_lqr<RMX_NP>), grid, block, lds_bytes, b->stream, m->dm, a);
}
// rmx_rollout_lqr_box: the same sweep with the box QP in the place of the solve (select_rollout_lqr_box: its LDS)
void RMX_CAT(launch_lqr_box_, RMX_NP)(const rmx_model* m, const rmx_batch* b, const LqrArgs& a, size_t lds_bytes) {
    const dim3 grid(b->B), block(LQR_THREADS);
    RMX_LAUNCH((k_rollout_lqr<RMX_NP, true>), grid, block, lds_bytes, b->stream, m->dm, a);
}
// rmx_rollout_search: one wavefront per rollout, every trial pass and the nominal pass in the one launch (select_rollout_search)
void RMX_CAT(launch_search_, RMX_NP)(const rmx_model* m, const rmx_batch* b, const DevOpts& o, const SearchArgs& a, int threads) {
    const dim3 grid(b->B), block(threads);      // (SearchPlan::block: one wavefront per rollout)
    RMX_LAUNCH((k_rollout_search<RMX_NP>), grid, block, m->smem_bytes, b->stream, m->dm, o, a);
}
#endif

// rmx_rollout_jvp: one wavefront per rollout and chunk of tangent directions
void RMX_CAT(launch_jvp_, RMX_NP)(const rmx_model* m, const rmx_batch* b, const JvpArgs& a) {
    const dim3 grid((unsigned)((size_t)b->B * a.nchunks)), block(64);
    k_rollout_jvp<RMX_NP><<<grid, block, 0, b->stream>>>(m->dm, a);
}

// rmx_rollout_jvp_params: r = (dg/dtheta) ttheta of every (rollout, slot, direction), then the sweep that subtracts it
void RMX_CAT(launch_jvp_params_, RMX_NP)(const rmx_model* m, const rmx_batch* b, const ParamRhsArgs& p, const JvpArgs& a) {
    const dim3 rgrid((unsigned)((size_t)b->B * p.nslots)), grid((unsigned)((size_t)b->B * a.nchunks)), block(64);
    RMX_LAUNCH((k_rollout_param_rhs<RMX_NP>), rgrid, block, m->smem_bytes, b->stream, m->dm, p);
    k_rollout_jvp<RMX_NP, true><<<grid, block, 0, b->stream>>>(m->dm, a);
}

// rmx_rollout_points / rmx_rollout_cost, and with `frames` rmx_rollout_frames / rmx_rollout_cost_frames: one wavefront per (rollout,
// step) of the record (rmx_select.h select_rollout_cost)
void RMX_CAT(launch_cost_, RMX_NP)(const rmx_model* m, const rmx_batch* b, const TaskArgs& a, bool frames) {
    const dim3 grid((unsigned)((size_t)b->B * a.nsteps)), block(64);
    if (frames) k_rollout_cost<RMX_NP, true><<<grid, block, 0, b->stream>>>(m->dm, a);
    else k_rollout_cost<RMX_NP, false><<<grid, block, 0, b->stream>>>(m->dm, a);
}

// rmx_rollout_vjp_params: the backward sweep of the tape's integrator in its ADJ_ZS instantiation (du, dq0, dqd0 as rmx_rollout_vjp's
// kernel, and z of every slot to a.zs), then the contraction over the slots.  fullchain: the instantiation rmx_rollout_vjp's plan runs
// for the full 16-link chain.
template <bool FC>
static void vjp_zs(const rmx_batch* b, const rmx_model* m, int integ, const DevOpts& o, const AdjArgs& a) {
    const dim3 grid(b->B), block(64);
    if (integ == INTEG_BDF1) k_adjoint_bwd<RMX_NP, 1 | ADJ_CTL | ADJ_TAPE | ADJ_ZS, FC><<<grid, block, 0, b->stream>>>(m->dm, o, a);
    else k_rollout_bwd_bdf2_zs<RMX_NP, FC><<<grid, block, 0, b->stream>>>(m->dm, o, a);
}
void RMX_CAT(launch_vjp_zs_, RMX_NP)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a, bool fullchain) {
#if RMX_NP == 16
    if (fullchain) {
        vjp_zs<true>(b, m, integ, o, a);
        return;
    }
#endif
    (void)fullchain;
    vjp_zs<false>(b, m, integ, o, a);
}
void RMX_CAT(launch_param_grad_, RMX_NP)(const rmx_model* m, const rmx_batch* b, const ParamArgs& a) {
    const dim3 grid(b->B), block(64);
    RMX_LAUNCH((k_rollout_param_grad<RMX_NP>), grid, block, m->smem_bytes, b->stream, m->dm, a);
}

void RMX_CAT(launch_mfd_, RMX_NP)(const rmx_model* m, const rmx_batch* b, double* dM, double* df, double* dD) {
    const dim3 grid(b->B), block(64);
    RMX_LAUNCH((k_eval_mfd<RMX_NP>), grid, block, m->smem_bytes, b->stream, m->dm, b->B, b->tmpA, b->tmpB, dM, df, dD, b->chart);
}

#if RMX_NP == 64
void launch_stage_consts_64(const rmx_model* m, double* dst, hipStream_t stream) {
    k_stage_consts<64><<<dim3(1), dim3(64), 0, stream>>>(m->dm, dst);
}
#endif

void RMX_CAT(launch_phase_, RMX_NP)(const rmx_model* m, const rmx_batch* b, int reps, double h, unsigned long long* d) {
    const dim3 grid(b->B), block(64);
    RMX_LAUNCH((k_phase_time<RMX_NP>), grid, block, m->smem_bytes, b->stream, m->dm, reps, b->q, b->qd, h, d);
}
