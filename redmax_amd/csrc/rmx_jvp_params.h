// rmx_jvp_params.h -- rmx_rollout_jvp_params (include/redmax_hip.h): forward-mode tangents of the taped rollout with respect to the
// model's parameters.  Every taped solve is g(x; qA, qB, u, theta) = 0, so the recursion of rmx_jvp.h gains one term on the right:
//     H dx = M dqB - eta D dqA + eta^2 pscale du - (dg/dtheta) ttheta ,   dv = (dx - dqA)/eta
// with dg/dtheta taken at the slot's recorded x, qA, qB and eta.  Two launches: k_rollout_param_rhs forms r = (dg/dtheta) ttheta for
// every (rollout, slot, direction) - the slots are independent, every state is on the record -, and k_rollout_jvp<NP, true> (rmx_jvp.h)
// subtracts its lane's entry of r where it initialises its right-hand side.  Included and instantiated from part_plain.hip alone.
//
// r is the transpose of the rows at the head of rmx_params.h: those contract dg/dtheta with z through w = J z; here the direction
// ttheta is applied and what remains is a vector over the nodes.  With v = (x - qA)/eta, e2 = eta^2, per node j and body i:
//     joint part      e2 (tk_j (x_j - qRest_j) + td_j v_j - k_j tqrest_j)                          on lanes with a DOF
//     body part       s_j . W_j ,  W_j = the sum over the subtree of j of the world wrenches about the origin of
//         body frame:  f = tI o beta - e2 ad(phi)'(tI o phi) - e2 (0 ; tI[3] R'grav)       (o: entry by entry, diag(I) in the body frame)
//         carried to the world, the dual of twist_to_body:   (R f_ang + p x R f_lin ; R f_lin)
//         gravity:     - e2 m_i (p_i x tg ; tg)
// (z' r is then exactly sum over the groups of d(z'g)/dtheta . ttheta of rmx_params.h: w . f = sum_c tI_c d(z'g)/dI_c because
// (ad(phi) w) . h = w . ad(phi)' h, and (w_ang, w_lin) . (p x tg ; tg) = tg . (w_lin + w_ang x p).)
//
// One wavefront per (rollout, slot), lane = node.  The front runs once (eval_front_e2<NP, false> at x, v, x - qB, as
// k_rollout_param_grad calls it); then the directions follow one after the other, each with one subtree sum of its 6 numbers
// (chain_suffix_sum<NP, 6> on chains, lds_subtree_sum<NP, 6> on trees).  Every direction runs through the same instructions, so a
// direction has the same bits whatever stands beside it.  A NULL group is neither read nor formed, through wave-uniform flags.
// Plain vector loads and stores, no atomics; idle lanes carry zero mass, zero tangents and store nothing.
#pragma once
#include "rmx_params.h"      /* twist_to_body */
#include "rmx_host.h"        /* ParamRhsArgs */

template <int NP>
__global__ void __launch_bounds__(64) k_rollout_param_rhs(const DevModel M, const ParamRhsArgs a) {
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const int lane = threadIdx.x, n = M.n, nr = M.nr, N = a.nsteps;
    const int traj = blockIdx.x / a.nslots, slot = blockIdx.x - traj * a.nslots;
    const bool act = lane < n;
    const int id = act ? M.idx[lane] : -1;
    const bool dof = id >= 0;
    const int idc = dof ? id : 0;
    constexpr int CS = cstride(NP);
    const int jc = (CS > NP && lane >= NP) ? NP : lane;
    const double* cK = RMX_CONSTS(sAcc, n, NP);      // (the layout of eval_front_e2)
    const double* cI4 = cK + 42 * CS;
    const double* cPrm = cI4 + 4 * CS;
    const double* cAnc = cPrm + 8 * CS + 3 * CS;
    const double* cEnd = cAnc + MAXROUNDS * CS;
    const double stiff = cPrm[1 * CS + jc], qRest = cPrm[3 * CS + jc], ms = cI4[3 * CS + jc];
    const bool wK = a.stiffness != nullptr, wD = a.damping != nullptr, wR = a.qrest != nullptr;      // (wave-uniform)
    const bool wI = a.inertia != nullptr, wG = a.grav != nullptr;
    const double h = a.h, al = (2.0 - sqrt(2.0)) / 2.0;
    // this lane's column of the recorded states: state k is (q0, qd0) for k = 0, row k - 1 of (qt, qdt) otherwise (unconditional loads,
    // the column and the row clamped, lanes without a DOF selected to zero)
    const double* q0p = a.q0 + (size_t)traj * nr + idc;
    const double* qd0p = a.qd0 + (size_t)traj * nr + idc;
    const double* qtp = a.qt + (size_t)traj * N * nr + idc;
    const double* qdtp = a.qdt + (size_t)traj * N * nr + idc;
    const double q0 = dof ? q0p[0] : 0.0, qd0 = dof ? qd0p[0] : 0.0;
    // the slot's eta, qA, qB and its solution x (the cases of k_rollout_param_grad)
    double eta, qA, qB, x;
    if (!a.bdf2 || (slot >= 1 && slot < N)) {
        // BDF1 step slot + 1 from state slot; BDF2 step slot + 1 from the states slot and slot - 1
        const int kc = slot, km = slot >= 1 ? slot - 1 : 0;
        const double qcl = qtp[(size_t)(kc >= 1 ? kc - 1 : 0) * nr], qdcl = qdtp[(size_t)(kc >= 1 ? kc - 1 : 0) * nr];
        const double qml = qtp[(size_t)(km >= 1 ? km - 1 : 0) * nr], qdml = qdtp[(size_t)(km >= 1 ? km - 1 : 0) * nr];
        const double xl = qtp[(size_t)slot * nr];
        const double qc = kc >= 1 ? (dof ? qcl : 0.0) : q0, qdc = kc >= 1 ? (dof ? qdcl : 0.0) : qd0;
        const double qm = km >= 1 ? (dof ? qml : 0.0) : q0, qdm = km >= 1 ? (dof ? qdml : 0.0) : qd0;
        x = dof ? xl : 0.0;
        if (!a.bdf2) {
            eta = h; qA = qc; qB = qc + h * qdc;
        } else {
            eta = (2.0 / 3.0) * h;
            qA = (4.0 / 3.0) * qc - (1.0 / 3.0) * qm;
            qB = qA + (8.0 / 9.0) * h * qdc - (2.0 / 9.0) * h * qdm;
        }
    } else {
        // the SDIRK2 start of a BDF2 tape; SDIRK2a's result qa is rebuilt as rmx_params.h rebuilds it
        const double q1l = qtp[0], qd1l = qdtp[0];
        const double q1 = dof ? q1l : 0.0, qd1 = dof ? qd1l : 0.0;
        const double qda = (q1 - (al * h) * qd1 - q0) / ((1.0 - al) * h);
        const double qa = q0 + (al * h) * qda;
        eta = al * h;
        if (slot == N) {      // SDIRK2a
            qA = q0; qB = q0 + (al * h) * qd0;
            x = qa;
        } else {              // SDIRK2b
            qA = q0 + (1.0 - al) * h * qda;
            qB = q0 + (2.0 * al - 1.0) * h * qd0 + 2.0 * (1.0 - al) * h * qda;
            x = q1;
        }
    }
    const double v = (x - qA) / eta, e2 = eta * eta;
    FrontState fs;
    NodeOut e;
    eval_front_e2<NP, false>(M, sAcc, lane, x, v, x - qB, eta, e2, e, fs);
    // phi, beta and gravity in the body frame, once for all directions
    double pbw[3], pbv[3], bbw[3], bbv[3], rg[3];
    twist_to_body(fs.Rw, fs.pw, fs.phw, fs.phv, pbw, pbv);
    twist_to_body(fs.Rw, fs.pw, fs.bw, fs.bv, bbw, bbv);
#pragma unroll
    for (int c = 0; c < 3; ++c) rg[c] = fs.Rw[c] * M.grav[0] + fs.Rw[3 + c] * M.grav[1] + fs.Rw[6 + c] * M.grav[2];
    const int li = act ? (int)a.lst[lane] : -1;
    const int lic = li >= 0 ? li : 0;
    const int jj = act ? lane : 0;
    // One direction per turn of a loop that is NOT unrolled: every direction runs through the same instructions, so its bits cannot
    // depend on where it stands in the call.  (Four directions unrolled around one shared subtree sum did not keep that on trees: the
    // copies of the body need not be compiled alike, and a direction at the second place differed in the last bits from the same
    // direction at the first.)
#pragma unroll 1
    for (int t = 0; t < a.ntan; ++t) {
        const size_t dir = (size_t)traj * a.ntan + t;
        // joint part
        double r = 0.0;
        if (wK) r += a.stiffness[dir * nr + idc] * (x - qRest);
        if (wD) r += a.damping[dir * nr + idc] * v;
        if (wR) r -= stiff * a.qrest[dir * nr + idc];
        const double rj = dof ? e2 * r : 0.0;
        // body part: the world wrench of this node's body about the origin
        double S[NACC];
        double Wt[3] = {0.0, 0.0, 0.0}, Wf[3] = {0.0, 0.0, 0.0};
        if (wI) {
            const double* ti = a.inertia + (dir * a.njoints + lic) * 6;
            double tI[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const double l = ti[c];
                tI[c] = li >= 0 ? l : 0.0;
            }
            double ht[3], hf[3], a3[3], b3[3], c3[3], ft[3], ff[3], F[3], T[3], t3[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ht[c] = tI[c] * pbw[c];
                hf[c] = tI[3 + c] * pbv[c];
            }
            cross3(pbw, ht, a3);      // ad(phi)' h = (-phi_w x h_t - phi_v x h_f ; -phi_w x h_f)
            cross3(pbv, hf, b3);
            cross3(pbw, hf, c3);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ft[c] = tI[c] * bbw[c] + e2 * (a3[c] + b3[c]);
                ff[c] = tI[3 + c] * bbv[c] + e2 * (c3[c] - tI[3] * rg[c]);
            }
            mat3v(fs.Rw, ft, T);
            mat3v(fs.Rw, ff, F);
            cross3(fs.pw, F, t3);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Wt[c] += T[c] + t3[c];
                Wf[c] += F[c];
            }
        }
        if (wG) {
            const double* tgp = a.grav + dir * 3;
            const double tg[3] = {tgp[0], tgp[1], tgp[2]};
            double t3[3];
            cross3(fs.pw, tg, t3);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Wt[c] -= e2 * ms * t3[c];
                Wf[c] -= e2 * ms * tg[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {      // (idle lanes of a chain carry the last node's prefix sums in phi, beta: nothing of them enters)
            S[c] = act ? Wt[c] : 0.0;
            S[3 + c] = act ? Wf[c] : 0.0;
        }
        double rb = 0.0;
        if (wI || wG) {
            if (M.is_chain) chain_suffix_sum<NP, 6>(lane, S);
            else lds_subtree_sum<NP, 6>(M, sAcc, cEnd, lane, act, jj, S);
            rb = dot3(fs.sw, &S[0]) + dot3(fs.sv, &S[3]);
        }
        if (act) a.r[(dir * a.nslots + slot) * n + lane] = dof ? rb + rj : 0.0;
    }
}
