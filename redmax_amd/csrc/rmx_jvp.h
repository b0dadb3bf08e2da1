// rmx_jvp.h -- rmx_rollout_jvp (include/redmax_hip.h): the forward sweep over the tape.  Tangents of the controls and of the initial
// state go in, the tangents of the whole trajectory come out; every taped solve is the implicit function x(qA, qB, u) of
// rmx_rollout_linearize, so
//     H dx = M dqB - eta D dqA + eta^2 pscale du ,   dv = (dx - dqA)/eta
// slot after slot in the order the forward rollout took them.  Included and instantiated from part_plain.hip alone.
//
// One wavefront per (rollout, chunk of JVP_TW tangent directions), lane = node = row.  The wave carries this lane's entry of dq, dqd
// (under BDF2 of the previous step as well) of each of its directions in registers.  At a slot it forms this lane's row of the
// right-hand block, JVP_TW columns - M and D rows streamed in column chunks of LIN_CHUNK with lin_load_block's unconditional,
// index-clamped loads, the tangent entries broadcast with readlane_d from a constant lane -, loads its row of H (lin_load_H) and
// eliminates ONCE for all its columns with lin_eliminate<NP, JVP_TW, 1>: Gauss-Jordan, lu_solve_neg's partial-pivot rule, the pivot
// row by readlane_d, no DPP broadcast sequence (the note at tape_solve_bwd).  The pivots and multipliers depend on H alone and the
// columns never mix, so a direction has the same bits whatever stands beside it.  The lane that pivoted at step r holds row r; it goes
// to lane r through the wave's own LDS (store at [r], read at [lane]).
//
// Registers at NP = 64: 64 doubles of H, JVP_TW = 8 columns, the carried entries (4 x 8 under BDF2) and dqA; the two LIN_CHUNK load
// buffers are dead before H is loaded - the right-hand block is formed first.  One loop over the slots holds ONE copy of the
// elimination: the SDIRK2 start solves of a BDF2 tape are its first two turns, told apart by wave-uniform branches.  A tail chunk
// carries zero directions under a wave-uniform count (their loads clamped onto the chunk's first direction, nothing of them stored).
#pragma once
#include "rmx_linearize.h"   /* lin_load_H, lin_load_block, lin_eliminate */
#include "rmx_host.h"        /* JvpArgs */

constexpr int JVP_TW = JVP_CHUNK;     // (rmx_host.h: the host sizes the grid by it)

// R[t] += sum_j M(lane, j) dqB[t]_j - eta sum_j D(lane, j) dqA[t]_j, column chunk after column chunk
template <int NP, int TW>
__device__ __forceinline__ void jvp_rhs(double (&R)[TW], const double (&dqA)[TW], const double (&dqB)[TW], const double* __restrict__ Mj,
                                        const double* __restrict__ Dj, const int n, const int lane, const bool dof, const double eta) {
    constexpr int CH = NP < LIN_CHUNK ? NP : LIN_CHUNK;
#pragma unroll
    for (int c0 = 0; c0 < NP; c0 += CH) {
        double mv[CH], dv[CH];
        lin_load_block<CH>(mv, LIN_M, c0, Mj, Dj, n, lane, dof, eta, 0.0);
        lin_load_block<CH>(dv, LIN_D, c0, Mj, Dj, n, lane, dof, eta, 0.0);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            // (the broadcasts of one column ahead of its FMAs, later columns' kept behind: lin_update's discipline)
            double pb[TW], pa[TW];
#pragma unroll
            for (int t = 0; t < TW; ++t) {
                pb[t] = readlane_d(dqB[t], c0 + c);
                pa[t] = readlane_d(dqA[t], c0 + c);
            }
#pragma unroll
            for (int t = 0; t < TW; ++t) R[t] = fma(dv[c], pa[t], fma(mv[c], pb[t], R[t]));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// RHS (rmx_rollout_jvp_params, rmx_jvp_params.h): the right-hand side of every slot loses this lane's entry of a.r, the parameter
// term (dg/dtheta) ttheta that k_rollout_param_rhs formed, [B][ntan][nslots][n] in node order.  The instantiation without it is the
// kernel of rmx_rollout_jvp, text for text.
template <int NP, bool RHS = false>
__global__ void __launch_bounds__(64) k_rollout_jvp(const DevModel M, const JvpArgs a) {
    constexpr int TW = JVP_TW;
    __shared__ double xs[TW][64];
    const int lane = threadIdx.x, n = M.n, nr = M.nr, N = a.nsteps;
    const int traj = blockIdx.x / a.nchunks, t0 = (blockIdx.x - traj * a.nchunks) * TW;
    const int cnt = a.ntan - t0 < TW ? a.ntan - t0 : TW;      // directions of this chunk (wave-uniform, >= 1)
    const size_t nn = (size_t)n * n;
    const double* Hb = a.Hs + (size_t)traj * a.nslots * nn;
    const double* Mb = a.Ms + (size_t)traj * a.nslots * nn;
    const double* Db = a.Ds + (size_t)traj * a.nslots * nn;
    const int id = (lane < n) ? M.idx[lane] : -1;
    const bool dof = id >= 0;
    const int idc = dof ? id : 0;
    const double h = a.h, al = (2.0 - sqrt(2.0)) / 2.0;
    // this lane's entry of direction t: (traj * ntan + t0 + t) rows of [nr] (the initial state) or of [nsteps][nr]
    size_t dir[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t) dir[t] = (size_t)traj * a.ntan + t0 + (t < cnt ? t : 0);
    double q[TW], v[TW], pq[TW], pv[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t) {
        // (unconditional loads at clamped indices; lanes without a DOF and the directions of a tail chunk selected to zero afterwards)
        const double q0 = a.tq0 ? a.tq0[dir[t] * nr + idc] : 0.0;
        const double v0 = a.tqd0 ? a.tqd0[dir[t] * nr + idc] : 0.0;
        q[t] = (dof && t < cnt) ? q0 : 0.0;
        v[t] = (dof && t < cnt) ? v0 : 0.0;
        pq[t] = 0.0;
        pv[t] = 0.0;
    }
    // The turns of the loop in the order of the recursion.  BDF1: turn s is slot s, step s + 1.  BDF2: turn 0 is the SDIRK2a solve (slot
    // N; its dqd stays in pv, nothing is stored), turn 1 the SDIRK2b solve (slot 0, step 1), turn s >= 2 the BDF2 solve of slot s - 1,
    // step s.
#pragma unroll 1
    for (int s = 0; s < a.nslots; ++s) {
        const int stage = a.bdf2 ? (s < 2 ? s + 1 : 3) : 0;      // 0 BDF1, 1 SDIRK2a, 2 SDIRK2b, 3 BDF2
        const int slot = a.bdf2 ? (s == 0 ? N : s - 1) : s;
        const int step = a.bdf2 ? (s == 0 ? 1 : s) : s + 1;
        const double eta = a.bdf2 ? (s < 2 ? al * h : (2.0 / 3.0) * h) : h;
        const double e2p = eta * eta * a.pscale;
        double dqA[TW], dqB[TW], R[TW];
#pragma unroll
        for (int t = 0; t < TW; ++t) {
            const double tu = a.tu ? a.tu[(dir[t] * N + (step - 1)) * nr + idc] : 0.0;
            if (stage == 0) {
                dqA[t] = q[t];
                dqB[t] = q[t] + h * v[t];
            } else if (stage == 1) {
                dqA[t] = q[t];
                dqB[t] = q[t] + al * h * v[t];
            } else if (stage == 2) {
                dqA[t] = q[t] + (1.0 - al) * h * pv[t];
                dqB[t] = q[t] + (2.0 * al - 1.0) * h * v[t] + 2.0 * (1.0 - al) * h * pv[t];
            } else {
                dqA[t] = (4.0 / 3.0) * q[t] - (1.0 / 3.0) * pq[t];
                dqB[t] = dqA[t] + (8.0 / 9.0) * h * v[t] - (2.0 / 9.0) * h * pv[t];
            }
            R[t] = (dof && t < cnt) ? e2p * tu : 0.0;
            if constexpr (RHS) {      // (an unconditional load: lanes beyond the tree read node 0's entry and drop it)
                const double rr = a.r[(dir[t] * a.nslots + slot) * n + (lane < n ? lane : 0)];
                R[t] = (dof && t < cnt) ? e2p * tu - rr : 0.0;
            }
        }
        jvp_rhs<NP, TW>(R, dqA, dqB, Mb + (size_t)slot * nn, Db + (size_t)slot * nn, n, lane, dof, eta);
        double Hrow[NP], rinv = 0.0;
        lin_load_H<NP>(Hrow, Hb + (size_t)slot * nn, n, lane);
        int r = (lane < NP) ? -1 : (NP + 1);
        lin_eliminate<NP, TW, 1>(lane, Hrow, R, R, R, true, false, false, r, rinv);
        // row r of H^-1 R back to lane r
        if (r >= 0 && r < NP) {
#pragma unroll
            for (int t = 0; t < TW; ++t) xs[t][r] = R[t] * rinv;
        }
        __syncthreads();
        const size_t row = (size_t)(step - 1) * nr + idc;
#pragma unroll
        for (int t = 0; t < TW; ++t) {
            const double dx = dof ? xs[t][lane] : 0.0;
            const double dv = dof ? (dx - dqA[t]) / eta : 0.0;
            if (stage == 1) {
                pv[t] = dv;
            } else {
                pq[t] = q[t];
                pv[t] = v[t];
                q[t] = dx;
                v[t] = dv;
                if (dof && t < cnt) {
                    a.tq[dir[t] * N * nr + row] = dx;
                    a.tqd[dir[t] * N * nr + row] = dv;
                }
            }
        }
        __syncthreads();
    }
}
