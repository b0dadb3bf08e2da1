// rmx_force_params.h -- rmx_rollout_vjp_forces (include/redmax_hip.h): the gradient of the caller's loss with respect to the
// constants of the body-to-body forces (stiffness, damping, rest length of every row of the force table), from the tape of a model
// whose tape carries them (rmx_tape_pf.h).  The rule is rmx_params.h's,
//     dL/dtheta = - sum over the slots s of the tape   z_s' dg_s/dtheta ,
// and the forces' share of g is the dg of pf_apply (rmx_pf.h; dA_j = A_{j+1} - A_j per segment, u_j the segment's unit vector,
// lam(a) = sum_j u_j . dA_j(a), l and ldot the total length and its rate, e2 = eta^2).  Per slot and force:
//   point-point           zA = sum_a z_a dA(a)  (a 3-vector):  d(z'g)/dks = e2 zA . dx     d(z'g)/dkd = e2 zA . dv     no L: +0.0
//   spring / taut cable   zl = sum_a z_a lam(a):               d(z'g)/dks = e2 zl (l - L)/L     d(z'g)/dkd = e2 zl ldot/L
//                                                              d(z'g)/dL  = -e2 zl (ks l + kd ldot)/L^2
//   cable, !(strain > 0)  nothing in any of the three (the branch rule of pf_apply and pf_damp)
// tests/proto_rollout_force_params.py holds the numpy twin and checks it against central differences of whole rollouts.
//
// One wavefront per rollout, lane = node, over the slots in the order of k_rollout_param_grad (the slot's x, qA, qB, eta are formed
// statement for statement as there, the rebuilt SDIRK2a state of a BDF2 tape included): one front and the point stage of every force
// per slot, no Hessian, no solve.  zA and zl are wave sums, so every term is wave-uniform; lane f carries the three sums of force f
// (RMX_PF_MAX_FORCES <= 64), updated by a select on lane == f: the order of the sum is the order of the slots, repeated calls give
// the same bits, there are no atomics and no register array indexed at run time.  A NULL output is neither summed nor stored,
// through wave-uniform flags; the three never mix, so an output has the same bits whichever others are asked for.
// Compiled into part_pf.hip's objects, one per padded size, behind rmx_tape_pf.h and under its guard.
#pragma once
#include "rmx_kernels.h"
#if RMX_NP == 64 && !defined(RMX_DPP_SETTLE)
#error "rmx_force_params.h at 64 lanes: RMX_DPP_SETTLE must be defined ahead of rmx_kernels.h"
#endif
static_assert(PF_MAX_FORCES <= 64, "lane f carries the sums of force f");

template <int NP>
__global__ void __launch_bounds__(64) k_rollout_force_grad(const DevModel M, const ForceArgs a, const PfTable* __restrict__ pf) {
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const PfTable& T = *pf;
    const int lane = threadIdx.x, traj = blockIdx.x, n = M.n, nr = M.nr, N = a.nsteps;
    const bool act = lane < n;
    const int id = act ? M.idx[lane] : -1;
    const bool dof = id >= 0;
    const bool wK = a.stiffness != nullptr, wD = a.damping != nullptr, wL = a.L != nullptr;      // (wave-uniform)
    const double h = a.h, al = (2.0 - sqrt(2.0)) / 2.0;
    // this lane's column of the recorded states (unconditional loads, the column clamped, lanes without a DOF selected to zero)
    const size_t c0 = (size_t)traj * nr + (dof ? id : 0);
    const double* qt = a.qt + (size_t)traj * N * nr + (dof ? id : 0);
    const double* qdt = a.qdt + (size_t)traj * N * nr + (dof ? id : 0);
    const double* zs = a.zs + (size_t)traj * a.nslots * n + (act ? lane : 0);
    const double q0l = a.q0[c0], qd0l = a.qd0[c0], q1l = qt[0], qd1l = qdt[0];
    const double q0 = dof ? q0l : 0.0, qd0 = dof ? qd0l : 0.0, q1 = dof ? q1l : 0.0, qd1 = dof ? qd1l : 0.0;
    const double qda = (q1 - (al * h) * qd1 - q0) / ((1.0 - al) * h);      // BDF2 tapes: SDIRK2a's result, rebuilt
    const double qa = q0 + (al * h) * qda;
    double qm = 0.0, qdm = 0.0, qc = q0, qdc = qd0;      // the states of steps k-1 and k
    double gk = 0.0, gd = 0.0, gL = 0.0;                  // lane f: the sums of force f
    const int nf = T.nf;
    for (int it = 0; it < a.nslots; ++it) {
        // the slot of this pass, its eta, qA, qB and its solution x
        int slot, row;          // row: the row of qt / qdt that holds x and the state the solve leaves (-1: SDIRK2a, none)
        double eta, qA, qB;
        if (!a.bdf2) {
            slot = it; row = it;
            eta = h; qA = qc; qB = qc + h * qdc;
        } else if (it == 0) {       // SDIRK2a
            slot = N; row = -1;
            eta = al * h; qA = q0; qB = q0 + (al * h) * qd0;
        } else if (it == 1) {       // SDIRK2b
            slot = 0; row = 0;
            eta = al * h;
            qA = q0 + (1.0 - al) * h * qda;
            qB = q0 + (2.0 * al - 1.0) * h * qd0 + 2.0 * (1.0 - al) * h * qda;
        } else {                    // the BDF2 step it (slot it - 1) from steps it - 1 and it - 2
            slot = it - 1; row = it - 1;
            eta = (2.0 / 3.0) * h;
            qA = (4.0 / 3.0) * qc - (1.0 / 3.0) * qm;
            qB = qA + (8.0 / 9.0) * h * qdc - (2.0 / 9.0) * h * qdm;
        }
        const int rowc = row >= 0 ? row : 0;
        const double xl = qt[(size_t)rowc * nr], xdl = qdt[(size_t)rowc * nr], zl_ = zs[(size_t)slot * n];
        const double x = row >= 0 ? (dof ? xl : 0.0) : qa;
        const double z = dof ? zl_ : 0.0;
        const double v = (x - qA) / eta, e2 = eta * eta, ieta = 1.0 / eta;
        FrontState fs;
        NodeOut e;
        eval_front_e2<NP, false>(M, sAcc, lane, x, v, x - qB, eta, e2, e, fs);
        for (int f = 0; f < nf; ++f) {
            const int k0 = T.first[f], k1 = T.first[f + 1], kind = T.kind[f];
            const double ks = T.ks[f], kd = T.kd[f], L = T.L[f];
            const bool pp = kind == RMX_PF_POINTPOINT;
            // the point stage over the segments: point-point keeps dx, dv and this lane's dA of its one segment, the others the
            // total length, its rate and this lane's lam
            double l = 0.0, ldot = 0.0, lam = 0.0;
            double dx[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0}, dA[3] = {0.0, 0.0, 0.0};
            double xp[3], vp[3], Ap[3], Bp[3];
            bool onp;
            pf_point(T, k0, fs, lane, ieta, xp, vp, Ap, Bp, onp);
            for (int k = k0 + 1; k < k1; ++k) {
                double xk[3], vk[3], A[3], B[3];
                bool on;
                pf_point(T, k, fs, lane, ieta, xk, vk, A, B, on);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    dx[c] = xk[c] - xp[c];
                    dv[c] = vk[c] - vp[c];
                    dA[c] = A[c] - Ap[c];
                    xp[c] = xk[c];
                    vp[c] = vk[c];
                    Ap[c] = A[c];
                }
                if (!pp) {
                    const double ln = sqrt(dot3(dx, dx)), il = 1.0 / ln;
                    const double u[3] = {dx[0] * il, dx[1] * il, dx[2] * il};
                    l += ln;
                    ldot += dot3(u, dv);
                    lam += dot3(u, dA);
                }
            }
            double tk, td, tL;      // d(z'g)/d(ks, kd, L) of this slot and force (wave-uniform)
            if (pp) {
                const double zA[3] = {wave_sum(z * dA[0]), wave_sum(z * dA[1]), wave_sum(z * dA[2])};
                tk = e2 * dot3(zA, dx);
                td = e2 * dot3(zA, dv);
                tL = 0.0;
            } else {
                const double strain = (l - L) / L;
                if (kind == RMX_PF_CABLE && !(strain > 0.0)) continue;      // a slack cable: nothing (wave-uniform)
                const double zl = wave_sum(z * lam);
                tk = e2 * zl * strain;
                td = e2 * zl * (ldot / L);
                tL = -(e2 * zl) * ((ks * l + kd * ldot) / (L * L));
            }
            const bool mine = lane == f;
            if (wK) gk -= mine ? tk : 0.0;
            if (wD) gd -= mine ? td : 0.0;
            if (wL) gL -= mine ? tL : 0.0;
        }
        if (row >= 0) {      // the state this solve leaves
            qm = qc; qdm = qdc;
            qc = x; qdc = dof ? xdl : 0.0;
        }
    }
    if (lane < nf) {
        const size_t off = (size_t)traj * nf + lane;
        if (wK) a.stiffness[off] = gk;
        if (wD) a.damping[off] = gd;
        if (wL) a.L[off] = gL;
    }
}

void RMX_CAT(launch_force_grad_, RMX_NP)(const rmx_model* m, const rmx_batch* b, const ForceArgs& a) {
    const dim3 grid(b->B), block(64);
    RMX_LAUNCH((k_rollout_force_grad<RMX_NP>), grid, block, m->smem_bytes, b->stream, m->dm, a, (const PfTable*)m->dpf);
}
