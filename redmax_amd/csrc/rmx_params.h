// rmx_params.h -- rmx_rollout_vjp_params (include/redmax_hip.h): the gradient of the caller's loss with respect to the model's
// parameters, from the tape.  Every taped solve is g(x; qA, qB, u, theta) = 0 with adjoint vector z (H' z = ...), so
//     dL/dtheta = - sum over the slots s of the tape   z_s' dg_s/dtheta
// and g is linear in joint stiffness, damping and rest position, in the body inertia and in gravity: dg/dtheta is one pass of the
// front (eval_front_e2: world frames, phi = J v, beta = J (x - qB) + eta^2 Jdot v) at the slot's x, qA, qB, plus w = J z, which is
// propagated down the tree as phi is.  Included and instantiated from part_plain.hip alone.
//
// With v = (x - qA)/eta and, per body, everything rotated into the body frame, where the inertia is diag(I[0..5]):
//     d(z'g)/dk_j     =  eta^2 z_j (x_j - qRest_j)            d(z'g)/dd_j = eta^2 z_j v_j            d(z'g)/dqRest_j = -eta^2 k_j z_j
//     d(z'g)/dI_i[c]  =  w_c beta_c - eta^2 (ad(phi) w)_c phi_c   ( - eta^2 w_lin . R_i' grav   for c = 3 )
//     d(z'g)/dgrav    = -eta^2 sum_i m_i (w_lin + w_ang x p_i)       (world frame: the velocity w gives body i's origin)
// (beta carries a = J (x - qB) and c~ = Jdot v together: w_c a_c + eta^2 w_c c~_c = w_c beta_c.  The weight of a body is
// I_i[3] * R_i' grav - the reference reads the mass from that entry alone, Body.m:104-109 -, so the whole gravity term belongs to
// c = 3; the three entries 3..5 must be equal anyway, and the gradient of the mass is their sum.)
//
// One wavefront per rollout, lane = node, looping over the slots of its tape with the sums in registers: the order of the sum is
// the order of the slots, so repeated calls give the same bits, and there are no atomics.  Under BDF2 the slots are taken in time
// order (SDIRK2a = slot nsteps first, then SDIRK2b = slot 0, then the BDF2 steps).  The SDIRK2a result qa is not on the tape; it is
// rebuilt from what is: SDIRK2b has qA = q0 + (1 - al) h qda and qd1 = (q1 - qA)/(al h), so
//     qda = (q1 - al h qd1 - q0) / ((1 - al) h) ,   qa = q0 + al h qda.
// A NULL output is neither formed nor stored, through wave-uniform flags; the groups never mix, so an output has the same bits
// whichever others are asked for.
#pragma once
#include "rmx_kernels.h"

// world-frame twist (tw, tv: angular part, velocity of the point at the world origin) -> the frame of the body at (R, p)
__device__ __forceinline__ void twist_to_body(const double (&R)[9], const double (&p)[3], const double (&tw)[3], const double (&tv)[3],
                                              double (&ow)[3], double (&ov)[3]) {
    double t[3], u[3];
    cross3(tw, p, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = tv[c] + t[c];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ow[k] = R[k] * tw[0] + R[3 + k] * tw[1] + R[6 + k] * tw[2];      // R' tw
        ov[k] = R[k] * u[0] + R[3 + k] * u[1] + R[6 + k] * u[2];
    }
}

template <int NP>
__global__ void __launch_bounds__(64) k_rollout_param_grad(const DevModel M, const ParamArgs a) {
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const int lane = threadIdx.x, traj = blockIdx.x, n = M.n, nr = M.nr, N = a.nsteps;
    const bool act = lane < n;
    const int id = act ? M.idx[lane] : -1;
    const bool dof = id >= 0;
    constexpr int CS = cstride(NP);
    const int jc = (CS > NP && lane >= NP) ? NP : lane;
    const double* cK = RMX_CONSTS(sAcc, n, NP);      // (the layout of eval_front_e2)
    const double* cI4 = cK + 42 * CS;
    const double* cPrm = cI4 + 4 * CS;
    const double* cAnc = cPrm + 8 * CS + 3 * CS;
    const double stiff = cPrm[1 * CS + jc], qRest = cPrm[3 * CS + jc], ms = cI4[3 * CS + jc];
    const bool wJ = a.stiffness || a.damping || a.qrest, wI = a.inertia != nullptr, wG = a.grav != nullptr;      // (wave-uniform)
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
    double gk = 0.0, gd = 0.0, gr = 0.0, gI[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gg[3] = {0.0, 0.0, 0.0};
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
        const double xl = qt[(size_t)rowc * nr], xdl = qdt[(size_t)rowc * nr], zl = zs[(size_t)slot * n];
        const double x = row >= 0 ? (dof ? xl : 0.0) : qa;
        const double z = dof ? zl : 0.0;
        const double v = (x - qA) / eta, e2 = eta * eta;
        FrontState fs;
        NodeOut e;
        eval_front_e2<NP, false>(M, sAcc, lane, x, v, x - qB, eta, e2, e, fs);
        if (wJ) {
            gk -= e2 * z * (x - qRest);
            gd -= e2 * z * v;
            gr += e2 * stiff * z;
        }
        if (wI || wG) {
            // w = (J z)_j = sum over the ancestors-or-self a of s_a z_a, as phi is propagated
            double ww[3], wv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ww[c] = fs.sw[c] * z;
                wv[c] = fs.sv[c] * z;
            }
            if (M.is_chain) {
                chain_scan_sum6<NP>(lane, ww, wv);
            } else {
                for (int r = 0; r < M.rounds; ++r) {
                    const int an = (int)cAnc[r * CS + jc];
                    const int src = an >= 0 ? an : lane;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double tw = shfl_d(ww[c], src), tv = shfl_d(wv[c], src);
                        if (an >= 0) {
                            ww[c] += tw;
                            wv[c] += tv;
                        }
                    }
                }
            }
            if (wG) {       // m (w_lin + w_ang x p): idle lanes carry no mass
                double t[3];
                cross3(ww, fs.pw, t);
#pragma unroll
                for (int c = 0; c < 3; ++c) gg[c] += act ? e2 * ms * (wv[c] + t[c]) : 0.0;
            }
            if (wI) {
                double wbw[3], wbv[3], pbw[3], pbv[3], bbw[3], bbv[3], aw[3], av[3], t[3];
                twist_to_body(fs.Rw, fs.pw, ww, wv, wbw, wbv);
                twist_to_body(fs.Rw, fs.pw, fs.phw, fs.phv, pbw, pbv);
                twist_to_body(fs.Rw, fs.pw, fs.bw, fs.bv, bbw, bbv);
                cross3(pbw, wbw, aw);      // ad(phi) w = (phi_w x w_w, phi_v x w_w + phi_w x w_v)
                cross3(pbv, wbw, av);
                cross3(pbw, wbv, t);
                double wg = 0.0;     // w_lin . R' grav
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    av[c] += t[c];
                    wg += wbv[c] * (fs.Rw[c] * M.grav[0] + fs.Rw[3 + c] * M.grav[1] + fs.Rw[6 + c] * M.grav[2]);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double da = wbw[c] * bbw[c] - e2 * (aw[c] * pbw[c]);
                    const double dl = wbv[c] * bbv[c] - e2 * (av[c] * pbv[c] + (c == 0 ? wg : 0.0));
                    gI[c] -= act ? da : 0.0;      // (idle lanes of a chain carry the last node's prefix sums)
                    gI[3 + c] -= act ? dl : 0.0;
                }
            }
        }
        if (row >= 0) {      // the state this solve leaves
            qm = qc; qdm = qdc;
            qc = x; qdc = dof ? xdl : 0.0;
        }
    }
    if (dof) {
        const size_t off = (size_t)traj * nr + id;
        if (a.stiffness) a.stiffness[off] = gk;
        if (a.damping) a.damping[off] = gd;
        if (a.qrest) a.qrest[off] = gr;
    }
    if (wI) {
        const int li = act ? (int)a.lst[lane] : -1;
        if (li >= 0) {
            double* o = a.inertia + ((size_t)traj * a.njoints + li) * 6;
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] = gI[c];
        }
    }
    if (wG) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double s = wave_sum(gg[c]);
            if (lane == 0) a.grav[(size_t)traj * 3 + c] = s;
        }
    }
}
