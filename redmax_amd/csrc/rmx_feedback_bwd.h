// rmx_feedback_bwd.h -- rmx_rollout_vjp_feedback (include/redmax_hip.h): the backward sweep of a taped rollout that ran in closed
// loop, uapp_k = uff_k + K_k (x_{k-1} - xref_{k-1}) (rmx_rollout_tape_feedback, rmx_feedback.h).  The tape is the open-loop tape
// under uapp; what the closed loop adds is one term per step: the cotangent ubar_k of the applied torque goes back into the cotangent
// of the state the step started from, through K_k'.  That makes the sweep another recursion than rmx_rollout_vjp's - the cotangent of
// x_{k-1} must be complete, K term included, before the solve of step k-1 reads it - and so a kernel of its own; the open-loop
// backward kernels keep their code (the note at k_rollout_bwd_bdf2_zs).  Included from rmx_kernels.h alone.
//
// One wavefront per rollout, lane = node, both integrators on tape_solve_bwd as it stands (its comment says why 17 to 64 nodes take
// the pivoted solve).  With (A, Bq, z) = solve_bwd(slot, eta; qbar, vbar) and gu the caller's cotangent of uapp (or null: zero):
//   BDF1, k = N .. 1 (slot k-1, eta = h):
//       ubar_k = h^2 pscale z + gu_k ;  qbar[k-1] += A + Bq + Kq_k' ubar_k ;  vbar[k-1] += h Bq + Kv_k' ubar_k
//   BDF2: the recursion of k_rollout_bwd_bdf2, with ubar_{k+1} = (2h/3)^2 pscale z + gu_{k+1} going into qbar[k], vbar[k] through
//       K_{k+1}' behind the solve of step k+1, and ubar_1 = (al h)^2 pscale (za + zb) + gu_1 into qbar[0], vbar[0] behind the start step.
//   duff_k = ubar_k ;  dxref_{k-1} = -(Kq_k' ubar_k, Kv_k' ubar_k) ;  dK_k[j nr + i] = (x_{k-1} - xref_{k-1})_j ubar_{k,i}
//
// K' ubar is the mirror of feedback_block: the lane with reduced index j owns COLUMN j of the step's table, nr contiguous doubles
// (entry j*nr + i is du_i/dx_j), ubar is broadcast node by node with readlane_d from a compile-time lane, and the row a node stands
// for is read wave-uniformly out of `id`; a node without a DOF contributes nothing and receives zero.  The loads of FB_CHUNK rows are
// issued together and unconditionally (row clamped, the term selected afterwards: adj_block).  ONE fixed order - nodes ascending,
// every term one fused multiply-add -, and nothing is read but the rollout's own tables: a rollout's result does not depend on its
// place in the batch, on the batch size or on which outputs are asked for.
// dK, where asked for, is written by the same lane: its two columns (q and qdot block), dx_j times the broadcast ubar_i.
#pragma once

// (Kq' ubar, Kv' ubar) of this lane's two columns.  Ks: the step's table [2 nr][nr]
template <int NP>
__device__ __forceinline__ void feedback_block_t(double& kq, double& kv, const double* __restrict__ Ks, const int nr, const int n, const int id,
                                                 const double ubar) {
    constexpr int CH = NP < FB_CHUNK ? NP : FB_CHUNK;
    const double* cq = Ks + (size_t)(id >= 0 ? id : 0) * nr;
    const double* cv = cq + (size_t)nr * nr;
    kq = 0.0;
    kv = 0.0;
#pragma unroll
    for (int b = 0; b < NP; b += CH) {
        if (b < n) {                               // (wave-uniform: the chunks past the tree hold no row)
            double eq[CH], ev[CH];
            int row[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                row[c] = __builtin_amdgcn_readlane(id, b + c);
                eq[c] = cq[row[c] >= 0 ? row[c] : 0];
                ev[c] = cv[row[c] >= 0 ? row[c] : 0];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const double ui = readlane_d(ubar, b + c);
                if (row[c] >= 0) {
                    kq = fma(eq[c], ui, kq);
                    kv = fma(ev[c], ui, kv);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (id < 0) {
        kq = 0.0;
        kv = 0.0;
    }
}

// this lane's two columns of one step's dK table: dKs[id nr + i] = dq ubar_i, dKs[(nr + id) nr + i] = dqd ubar_i
template <int NP>
__device__ __forceinline__ void feedback_dK(double* __restrict__ dKs, const int nr, const int n, const int id, const double dq,
                                            const double dqd, const double ubar) {
    double* cq = dKs + (size_t)(id >= 0 ? id : 0) * nr;
    double* cv = cq + (size_t)nr * nr;
#pragma unroll
    for (int m = 0; m < NP; ++m) {
        if (m < n) {
            const int row = __builtin_amdgcn_readlane(id, m);
            const double ui = readlane_d(ubar, m);
            if (row >= 0 && id >= 0) {
                cq[row] = dq * ui;
                cv[row] = dqd * ui;
            }
        }
    }
}

// what one step does with its ubar: duff, the K term (kq, kv: what goes into qbar, vbar of the state the step started from), dxref, dK.
// step: k (1-based); the state at its start is (q0, qd0) for k = 1 and row k-2 of the tape's trajectory otherwise.
template <int NP>
__device__ __forceinline__ void feedback_step_bwd(const AdjArgs& a, const int nr, const int n, const int id, const int traj, const int k,
                                                  const double ubar, double& kq, double& kv) {
    const bool dof = id >= 0;
    const size_t urow = (size_t)traj * a.nsteps + (size_t)(k - 1);
    if (a.dPdu && dof) a.dPdu[urow * nr + id] = ubar;
    kq = 0.0;
    kv = 0.0;
    if (!a.fbK) return;                            // (wave-uniform: no gains, no K term, and dK / dxref are refused on the host)
    const size_t row = (size_t)traj * a.fb_stride + (size_t)(k - 1);
    feedback_block_t<NP>(kq, kv, a.fbK + row * ((size_t)2 * nr * nr), nr, n, id, ubar);
    if (a.dxref && dof) {
        a.dxref[urow * ((size_t)2 * nr) + id] = -kq;
        a.dxref[urow * ((size_t)2 * nr) + nr + id] = -kv;
    }
    if (a.dK) {
        const size_t lid = dof ? id : 0;
        const double* xq = k >= 2 ? a.fqt + ((size_t)traj * a.nsteps + (size_t)(k - 2)) * nr : a.fq0 + (size_t)traj * nr;
        const double* xv = k >= 2 ? a.fqdt + ((size_t)traj * a.nsteps + (size_t)(k - 2)) * nr : a.fqd0 + (size_t)traj * nr;
        const double q = xq[lid], qd = xv[lid];
        const double rq = a.fbx ? a.fbx[row * ((size_t)2 * nr) + lid] : 0.0;
        const double rv = a.fbx ? a.fbx[row * ((size_t)2 * nr) + nr + lid] : 0.0;
        feedback_dK<NP>(a.dK + urow * ((size_t)2 * nr * nr), nr, n, id, q - rq, qd - rv, ubar);
    }
}

template <int NP, int INTEG>
__global__ void __launch_bounds__(64) k_rollout_bwd_fb(const DevModel Min, const DevOpts o, const AdjArgs a) {
    static_assert(INTEG == 1 || INTEG == 2, "BDF1 or BDF2");
    const DevModel M = model_view<NP, false>(Min);
    const int lane = threadIdx.x, traj = blockIdx.x, n = M.n, N = a.nsteps, nr = M.nr;
    const int id = (lane < n) ? M.idx[lane] : -1;
    const bool dof = id >= 0;
    const size_t nn = (size_t)n * n;
    const double h = o.h;
    const int col = lane < n ? lane : 0;
    const size_t row0 = (size_t)traj * N * nr + (dof ? id : 0);      // this lane's entry of row 0 (step 1) of gq, gqd, gu
    // (the cotangent loads unconditional, the row clamped, lanes without a DOF and rows that do not exist selected to zero afterwards)
    const double* gup = a.gu ? a.gu : a.gq;                           // (a null gu: a valid address, the value selected to zero)
    const bool hasgu = a.gu != nullptr;
    if constexpr (INTEG == 1) {
        const double* Hb = a.Hs + (size_t)traj * N * nn;
        const double* Mb = a.Ms + (size_t)traj * N * nn;
        const double* Db = a.Ds + (size_t)traj * N * nn;
        const double gqN = a.gq[row0 + (size_t)(N - 1) * nr], gdN = a.gqd[row0 + (size_t)(N - 1) * nr];
        double qb1 = dof ? gqN : 0.0, vb1 = dof ? gdN : 0.0;      // step k
        for (int k = N; k >= 1; --k) {
            const size_t rowm = row0 + (size_t)(k >= 2 ? k - 2 : 0) * nr;      // step k-1, in flight across the solve
            const double gqm = a.gq[rowm], gdm = a.gqd[rowm];
            const double guk = gup[row0 + (size_t)(k - 1) * nr];
            double A, Bq, z;
            tape_solve_bwd<NP>(Hb + (size_t)(k - 1) * nn, Mb + (size_t)(k - 1) * nn, Db + (size_t)(k - 1) * nn, n, lane, col, dof, h, qb1, vb1, A, Bq, z);
            const double ubar = dof ? h * h * a.pscale * z + (hasgu ? guk : 0.0) : 0.0;
            double kq, kv;
            feedback_step_bwd<NP>(a, nr, n, id, traj, k, ubar, kq, kv);
            qb1 = ((dof && k >= 2) ? gqm : 0.0) + (A + Bq) + kq;
            vb1 = ((dof && k >= 2) ? gdm : 0.0) + h * Bq + kv;
        }
        if (dof && a.dq0) {
            const size_t off = (size_t)traj * nr + id;
            a.dq0[off] = qb1;
            a.dqd0[off] = vb1;
        }
    } else {
        const double al = (2.0 - sqrt(2.0)) / 2.0;
        const double* Hb = a.Hs + (size_t)traj * (N + 1) * nn;
        const double* Mb = a.Ms + (size_t)traj * (N + 1) * nn;
        const double* Db = a.Ds + (size_t)traj * (N + 1) * nn;
        const double gqN = a.gq[row0 + (size_t)(N - 1) * nr], gdN = a.gqd[row0 + (size_t)(N - 1) * nr];
        const double gqP = a.gq[row0 + (size_t)(N >= 2 ? N - 2 : 0) * nr], gdP = a.gqd[row0 + (size_t)(N >= 2 ? N - 2 : 0) * nr];
        double qb1 = dof ? gqN : 0.0, vb1 = dof ? gdN : 0.0;                        // step k+1
        double qb0 = (dof && N >= 2) ? gqP : 0.0, vb0 = (dof && N >= 2) ? gdP : 0.0;      // step k (step 0 has no cotangent of its own)
        const double eta = (2.0 / 3.0) * h;
        for (int k = N - 1; k >= 1; --k) {
            const size_t rowm = row0 + (size_t)(k >= 2 ? k - 2 : 0) * nr;          // step k-1, in flight across the solve
            const double gqm = a.gq[rowm], gdm = a.gqd[rowm];
            const double guk = gup[row0 + (size_t)k * nr];                         // step k+1
            double A, Bq, z;
            tape_solve_bwd<NP>(Hb + (size_t)k * nn, Mb + (size_t)k * nn, Db + (size_t)k * nn, n, lane, col, dof, eta, qb1, vb1, A, Bq, z);
            const double ubar = dof ? eta * eta * a.pscale * z + (hasgu ? guk : 0.0) : 0.0;
            double kq, kv;
            feedback_step_bwd<NP>(a, nr, n, id, traj, k + 1, ubar, kq, kv);
            const double s = A + Bq;
            qb0 += (4.0 / 3.0) * s + kq;
            vb0 += (8.0 / 9.0) * h * Bq + kv;
            qb1 = qb0;
            vb1 = vb0;
            qb0 = ((dof && k >= 2) ? gqm : 0.0) - (1.0 / 3.0) * s;
            vb0 = ((dof && k >= 2) ? gdm : 0.0) - (2.0 / 9.0) * h * Bq;
        }
        // the start step: qb1, vb1 are the cotangents of step 1, qb0, vb0 of the initial state
        const double gu1 = gup[row0];
        const double etas = al * h;
        double A, Bq, zb, A2, B2, za;
        tape_solve_bwd<NP>(Hb, Mb, Db, n, lane, col, dof, etas, qb1, vb1, A, Bq, zb);                   // SDIRK2b
        qb0 += A + Bq;
        vb0 += (2.0 * al - 1.0) * h * Bq;
        const double qdab = (1.0 - al) * h * A + 2.0 * (1.0 - al) * h * Bq;
        tape_solve_bwd<NP>(Hb + (size_t)N * nn, Mb + (size_t)N * nn, Db + (size_t)N * nn, n, lane, col, dof, etas, 0.0, qdab, A2, B2, za);      // SDIRK2a
        qb0 += A2 + B2;
        vb0 += al * h * B2;
        const double ubar = dof ? etas * etas * a.pscale * (za + zb) + (hasgu ? gu1 : 0.0) : 0.0;
        double kq, kv;
        feedback_step_bwd<NP>(a, nr, n, id, traj, 1, ubar, kq, kv);
        qb0 += kq;
        vb0 += kv;
        if (dof && a.dq0) {
            const size_t off = (size_t)traj * nr + id;
            a.dq0[off] = qb0;
            a.dqd0[off] = vb0;
        }
    }
}
