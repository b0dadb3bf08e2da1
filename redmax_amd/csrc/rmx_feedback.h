// rmx_feedback.h -- rmx_rollout_tape_feedback (include/redmax_hip.h): the torque of one step of a taped rollout under time-varying
// affine state feedback,
//     us_i = uff_i + sum_j Kq[i][j] (q_j - qref_j) + sum_j Kv[i][j] (qd_j - qdref_j),
// formed from the state the rollout itself has reached, at the top of the step loop of k_adjoint_fwd's ADJ_FB instantiations.
// Included from rmx_kernels.h alone.
//
// Lane = node; the lane's row is i = M.idx[lane] (`id`, -1 for a node without a DOF and for the lanes past the tree).  The state
// differences are formed per lane and broadcast lane by lane with readlane_d, the lane a compile-time constant; the column a node
// stands for is its reduced index, read out of `id` the same way (wave-uniform), and a node without a DOF has no column: it
// contributes nothing.  One step's table holds du_i/dx_j at j*nr + i, j in 0 .. 2nr-1 over x = (q, qdot) - the ABI's column-major
// convention -, so the loads of one column are contiguous across the lanes where the reduced order follows the node order.
// The sum runs in ONE fixed order - nodes ascending over the q block, then over the qdot block, every term one fused multiply-add
// into the running sum, which is added to uff last - and reads nothing but the rollout's own registers and tables: the result of a
// rollout does not depend on its position in the batch or on the size of the batch.
// The loads of FB_CHUNK columns are issued together and unconditionally (column index clamped, the term selected afterwards: see
// adj_block), not one dependent round trip per column.
//
// What is not here but in rmx_feedback_bwd.h: gradients through the feedback law.  The tape a feedback rollout leaves is the open-loop tape under the applied
// torques uapp, and rmx_rollout_vjp / _linearize / _jvp / _vjp_params differentiate that open-loop rollout - what iLQR re-linearises
// around.  dL/dK, dL/dxref and the closed-loop dL/duff are formed by rmx_rollout_vjp_feedback: rmx_feedback_bwd.h.
#pragma once

constexpr int FB_CHUNK = 16;      // columns in flight at a time

// one block (q or qdot) of the sum: Kb this block's nr x nr table (column-major), dx this lane's state difference
template <int NP>
__device__ __forceinline__ double feedback_block(double acc, const double* __restrict__ Kb, const int nr, const int n, const int id,
                                                 const double dx) {
    constexpr int CH = NP < FB_CHUNK ? NP : FB_CHUNK;
    const double* row = Kb + (id >= 0 ? id : 0);
#pragma unroll
    for (int b = 0; b < NP; b += CH) {
        if (b < n) {                               // (wave-uniform: the chunks past the tree hold no column)
            double kv[CH];
            int col[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                col[c] = __builtin_amdgcn_readlane(id, b + c);
                kv[c] = row[(size_t)(col[c] >= 0 ? col[c] : 0) * nr];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const double dxj = readlane_d(dx, b + c);
                if (col[c] >= 0) acc = fma(kv[c], dxj, acc);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    return acc;
}

// the applied torque of this lane's joint.  Ks: the step's gain table [2 nr][nr]; xr: the step's reference row (q, qdot), or null: zero
template <int NP>
__device__ __forceinline__ double feedback_torque(const double uff, const double* __restrict__ Ks, const double* __restrict__ xr,
                                                  const int nr, const int n, const int id, const double q, const double qd) {
    const bool dof = id >= 0;
    const double dq = dof ? q - (xr ? xr[id] : 0.0) : 0.0;
    const double dqd = dof ? qd - (xr ? xr[nr + id] : 0.0) : 0.0;
    double fb = 0.0;
    fb = feedback_block<NP>(fb, Ks, nr, n, id, dq);
    fb = feedback_block<NP>(fb, Ks + (size_t)nr * nr, nr, n, id, dqd);
    return dof ? uff + fb : 0.0;
}
