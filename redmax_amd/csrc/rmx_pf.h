// rmx_pf.h -- body-to-body forces (ForcePointPoint.m, ForceSpringDamper.m / ForceSpringGeneric.m, ForceCable.m /
// ForceSpringMultiPointGeneric.m of the reference) for the one-wavefront kernels: the point stage behind eval_front, the dense
// update of the Hessian rows behind eval_hess, and the Newton loop around them.  part_pf.hip instantiates the
// kernels; nothing here is reached by a model without a force table.
//
// Point k of a force sits on node b_k at the local position xl_k: x_k = R xl_k + p, Gw_k = [-[x_k], I], v_k = Gw_k phi_{b_k}.
// Its Jacobian column for joint a is  A_k(a) = Gw_k s_a = w_a x x_k + v_a  for a in anc*(b_k) and 0 otherwise (s_a = (w_a, v_a): the
// world screw of joint a), and under qdot = (q - qA)/eta the point velocity changes with q_i by
//     B_k(i) = A_k(i)/eta + w_i x (v_k - Gw_k phi_i) + om_i x A_k(i)          (phi_i = (om_i, .): world twist of body i).
// A force is a sum over the SEGMENTS j = (point j, point j+1) of its polyline, dA_j = A_{j+1} - A_j, dB_j = B_{j+1} - B_j:
//     g(a)   += eta^2 sum_j dA_j(a) . F_j
//     H(a,i) += sum_j dA_j(a) . C_j(i)  -  eta^2 sum_k F_k . dA_k(a)/dq_i
//   point-point   F = ks dx + kd dv                      C(i)   = eta^2 (ks dA(i) + kd dB(i))
//   spring/cable  F_j = fs u_j, u_j = dx_j/|dx_j|         C_j(i) = eta^2 (fs P_j dA_j(i)/l_j + u_j mu(i)),  P_j = I - u_j u_j'
//                 fs = k (l - L)/L + d ldot/L             mu(i)  = (k/L) sum_j u_j.dA_j(i) + (d/L) sum_j (dv_j.P_j dA_j(i)/l_j + u_j.dB_j(i))
//                 (a cable has fs = mu = 0 while l <= L)
// The last term of H - the net force F_k on point k held fixed while the column of the point Jacobian moves - couples only joints
// on the path to b_k:  dA_k(a)/dq_i = w_i x A_k(a) (i ancestor-or-self of a), w_a x A_k(i) (a strict ancestor of i).  The segment
// terms couple a in anc*(b_k) with i in anc*(b_l) on DIFFERENT branches: H is dense, the solve takes the dense elimination order.
// tests/proto_point_forces.py holds the same algebra in numpy and checks it against the reference's literal J'(fm, Km, Dm)J form.
//
// Lane = node.  The points' positions, velocities, lengths and the tension are wave-uniform (the owning node's transform and twist
// are fetched with v_readlane from a uniform lane index); the Jacobian columns A, B, the sums over them and the rows of H are per
// lane; the column-side vectors of the H update are broadcast with v_readlane of a constant lane.
#pragma once

namespace rmx {

constexpr int PF_MAX_FORCES = RMX_PF_MAX_FORCES;      // (include/redmax_hip.h)
constexpr int PF_MAX_POINTS = RMX_PF_MAX_POINTS;      // points of one force
constexpr int PF_MAX_TOTAL = RMX_PF_MAX_TOTAL;        // points of all forces of a model
// The force table of a model, shared by the batch (global memory; every lane reads it at wave-uniform addresses).
struct PfTable {
    int nf;
    int first[PF_MAX_FORCES + 1];      // points first[f] .. first[f + 1] - 1 belong to force f
    int kind[PF_MAX_FORCES];           // RMX_PF_POINTPOINT / SPRINGDAMPER / CABLE
    double ks[PF_MAX_FORCES], kd[PF_MAX_FORCES], L[PF_MAX_FORCES];
    int node[PF_MAX_TOTAL];            // node of each point, -1: the world
    double xl[PF_MAX_TOTAL][3];        // local position
};

#ifdef __HIPCC__
// Point k at the state the front left behind: x, v (wave-uniform), this lane's columns A, B (zero unless the lane's node is an
// ancestor-or-self of the point's node: `on`).  Returns the node.
__device__ __forceinline__ int pf_point(const PfTable& T, const int k, const FrontState& fs, const int lane, const double ieta,
                                        double (&x)[3], double (&v)[3], double (&A)[3], double (&B)[3], bool& on) {
    const int b = __builtin_amdgcn_readfirstlane(T.node[k]);
    const double xl[3] = {T.xl[k][0], T.xl[k][1], T.xl[k][2]};
    if (b < 0) {                       // the world: a fixed point
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = xl[c];
            v[c] = A[c] = B[c] = 0.0;
        }
        on = false;
        return b;
    }
    double R[9], p[3], ow[3], ov[3], t[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) R[c] = readlane_d(fs.Rw[c], b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        p[c] = readlane_d(fs.pw[c], b);
        ow[c] = readlane_d(fs.phw[c], b);
        ov[c] = readlane_d(fs.phv[c], b);
    }
    mat3v(R, xl, x);
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] += p[c];
    cross3(ow, x, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ov[c] + t[c];
    on = lane == b || ((fs.desc_m >> b) & 1ull) != 0ull;
    double a3[3], d3[3], b3[3];
    cross3(fs.sw, x, a3);
    cross3(fs.phw, x, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a3[c] += fs.sv[c];
        d3[c] = v[c] - (fs.phv[c] + t[c]);       // the point's velocity relative to this lane's body
    }
    cross3(fs.sw, d3, b3);
    cross3(fs.phw, a3, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        A[c] = on ? a3[c] : 0.0;
        B[c] = on ? (a3[c] * ieta + b3[c] + t[c]) : 0.0;
    }
    return b;
}

// H(lane, i) += dA(lane) . C(i) for every column node i
template <int NP>
__device__ __forceinline__ void pf_seg_update(double (&Hrow)[NP], const double (&dA)[3], const double (&C)[3]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const double c0 = readlane_d(C[0], i), c1 = readlane_d(C[1], i), c2 = readlane_d(C[2], i);
        Hrow[i] += dA[0] * c0 + dA[1] * c1 + dA[2] * c2;
    }
}

// H(lane, i) -= eta^2 F . dA_k(lane)/dq_i  with  F . (w_i x A(a)) = A(a) . (F x w_i)  and  F . (w_a x A(i)) = A(i) . (F x w_a)
template <int NP>
__device__ __forceinline__ void pf_geom_update(double (&Hrow)[NP], const double (&A)[3], const bool on, const double (&F)[3],
                                               const FrontState& fs, const int lane, const double e2) {
    double G[3];
    cross3(F, fs.sw, G);
#pragma unroll
    for (int c = 0; c < 3; ++c) G[c] = on ? e2 * G[c] : 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const double a0 = readlane_d(A[0], i), a1 = readlane_d(A[1], i), a2 = readlane_d(A[2], i);
        const double g0 = readlane_d(G[0], i), g1 = readlane_d(G[1], i), g2 = readlane_d(G[2], i);
        const bool up = i == lane || ((fs.anc_m >> i) & 1ull) != 0ull;      // column node i is an ancestor-or-self of this row's node
        const bool dn = ((fs.desc_m >> i) & 1ull) != 0ull;                  // ... a strict descendant
        const double t1 = A[0] * g0 + A[1] * g1 + A[2] * g2, t2 = G[0] * a0 + G[1] * a1 + G[2] * a2;
        Hrow[i] -= (up ? t1 : 0.0) + (dn ? t2 : 0.0);
    }
}

// The point forces at the state of `fs`: their share of the residual and of the potential energy is added to `out`, and (HESS)
// their share of this lane's row of H to Hrow.  Residual-only evaluations (line search, energies) run it without the blocks.
template <int NP, bool HESS>
__device__ __forceinline__ void pf_apply(const PfTable& T, const FrontState& fs, const int lane, NodeOut& out, double (&Hrow)[NP]) {
    const double eta = fs.eta, e2 = eta * eta, ieta = 1.0 / eta;
    double dg = 0.0, V = 0.0;
    const int nf = T.nf;
    for (int f = 0; f < nf; ++f) {
        const int k0 = T.first[f], k1 = T.first[f + 1], kind = T.kind[f];
        const double ks = T.ks[f], kd = T.kd[f], L = T.L[f];
        const bool pp = kind == RMX_PF_POINTPOINT;
        double tens = 0.0, mu = 0.0;      // the scalar tension (wave-uniform) and this lane's entry of its derivative
        if (!pp) {
            // first pass: total length and its rate, lambda(lane) = dl/dq and nu(lane) = dldot/dq
            double l = 0.0, ldot = 0.0, lam = 0.0, nu = 0.0;
            double xp[3], vp[3], Ap[3], Bp[3];
            bool onp;
            pf_point(T, k0, fs, lane, ieta, xp, vp, Ap, Bp, onp);
            for (int k = k0 + 1; k < k1; ++k) {
                double x[3], v[3], A[3], B[3];
                bool on;
                pf_point(T, k, fs, lane, ieta, x, v, A, B, on);
                double dx[3], dv[3], dA[3], dB[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    dx[c] = x[c] - xp[c];
                    dv[c] = v[c] - vp[c];
                    dA[c] = A[c] - Ap[c];
                    dB[c] = B[c] - Bp[c];
                    xp[c] = x[c];
                    vp[c] = v[c];
                    Ap[c] = A[c];
                    Bp[c] = B[c];
                }
                const double ln = sqrt(dot3(dx, dx)), il = 1.0 / ln;
                const double u[3] = {dx[0] * il, dx[1] * il, dx[2] * il};
                const double udv = dot3(u, dv), uA = dot3(u, dA);
                l += ln;
                ldot += udv;
                lam += uA;
                if (HESS) nu += (dot3(dv, dA) - udv * uA) * il + dot3(u, dB);
            }
            const double strain = (l - L) / L;
            if (kind == RMX_PF_CABLE && !(strain > 0.0)) continue;      // a slack cable: no force, no energy, no blocks
            tens = ks * strain + kd * (ldot / L);
            V += 0.5 * ks * strain * strain * L;
            dg += e2 * tens * lam;
            if (!HESS) continue;
            mu = (ks / L) * lam + (kd / L) * nu;
        }
        // second pass: the segments' column vectors and forces (point-point: also the residual and the energy)
        double xp[3], vp[3], Ap[3], Bp[3], Fp[3] = {0.0, 0.0, 0.0};
        bool onp;
        int bp = pf_point(T, k0, fs, lane, ieta, xp, vp, Ap, Bp, onp);
        for (int k = k0 + 1; k < k1; ++k) {
            double x[3], v[3], A[3], B[3];
            bool on;
            const int b = pf_point(T, k, fs, lane, ieta, x, v, A, B, on);
            double dx[3], dv[3], dA[3], dB[3], F[3], C[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dx[c] = x[c] - xp[c];
                dv[c] = v[c] - vp[c];
                dA[c] = A[c] - Ap[c];
                dB[c] = B[c] - Bp[c];
            }
            if (pp) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    F[c] = ks * dx[c] + kd * dv[c];
                    C[c] = e2 * (ks * dA[c] + kd * dB[c]);
                }
                dg += e2 * dot3(dA, F);
                V += 0.5 * ks * dot3(dx, dx);
            } else {
                const double ln = sqrt(dot3(dx, dx)), il = 1.0 / ln;
                const double u[3] = {dx[0] * il, dx[1] * il, dx[2] * il};
                const double uA = dot3(u, dA);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    F[c] = tens * u[c];
                    C[c] = e2 * (tens * il * (dA[c] - u[c] * uA) + u[c] * mu);
                }
            }
            if constexpr (HESS) {
                pf_seg_update<NP>(Hrow, dA, C);
                if (bp >= 0) {          // the net force on the previous point is complete
                    const double Fn[3] = {F[0] - Fp[0], F[1] - Fp[1], F[2] - Fp[2]};
                    pf_geom_update<NP>(Hrow, Ap, onp, Fn, fs, lane, e2);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                xp[c] = x[c];
                vp[c] = v[c];
                Ap[c] = A[c];
                Bp[c] = B[c];
                Fp[c] = F[c];
            }
            onp = on;
            bp = b;
        }
        if constexpr (HESS) {
            if (bp >= 0) {
                const double Fn[3] = {-Fp[0], -Fp[1], -Fp[2]};
                pf_geom_update<NP>(Hrow, Ap, onp, Fn, fs, lane, e2);
            }
        }
    }
    out.g += dg;                       // (lanes without a DOF have zero columns: dg = 0)
    if (lane == 0) out.eV += V;
}

// The point forces' share of D = df/dqdot at the state of `fs`, added to this lane's row (the taped rollouts: part_tape_pf.hip).
// pf_apply never forms it on its own - it folds the damping into H through B = A/eta + ... -; it is the coefficient of 1/eta in C,
// divided by eta, without the geometric terms:
//   point-point          D(a,i) -= kd dA(a) . dA(i)
//   spring / taut cable  D(a,i) -= (kd/L) lam(a) lam(i),   lam(a) = sum_j u_j . dA_j(a)   (the lam of pf_apply's first pass)
//   slack cable          nothing
// Same point stage, same broadcasts and same cable switch as pf_apply, force by force (tests/proto_rollout_pf.py holds the numpy
// twin and checks it against the reference's literal J' Dm J).
template <int NP>
__device__ __forceinline__ void pf_damp(const PfTable& T, const FrontState& fs, const int lane, double (&Drow)[NP]) {
    const double ieta = 1.0 / fs.eta;
    const int nf = T.nf;
    for (int f = 0; f < nf; ++f) {
        const int k0 = T.first[f], k1 = T.first[f + 1], kind = T.kind[f];
        const double kd = T.kd[f], L = T.L[f];
        const bool pp = kind == RMX_PF_POINTPOINT;
        double l = 0.0, lam = 0.0;
        double xp[3], vp[3], Ap[3], Bp[3];
        bool onp;
        pf_point(T, k0, fs, lane, ieta, xp, vp, Ap, Bp, onp);
        for (int k = k0 + 1; k < k1; ++k) {
            double x[3], v[3], A[3], B[3];
            bool on;
            pf_point(T, k, fs, lane, ieta, x, v, A, B, on);
            double dx[3], dA[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dx[c] = x[c] - xp[c];
                dA[c] = A[c] - Ap[c];
                xp[c] = x[c];
                Ap[c] = A[c];
            }
            if (pp) {
                const double C[3] = {-kd * dA[0], -kd * dA[1], -kd * dA[2]};
                pf_seg_update<NP>(Drow, dA, C);
            } else {
                const double ln = sqrt(dot3(dx, dx)), il = 1.0 / ln;
                const double u[3] = {dx[0] * il, dx[1] * il, dx[2] * il};
                l += ln;
                lam += dot3(u, dA);
            }
        }
        if (pp) continue;
        const double strain = (l - L) / L;
        if (kind == RMX_PF_CABLE && !(strain > 0.0)) continue;      // a slack cable: no block
        const double cl = (kd / L) * lam;
#pragma unroll
        for (int i = 0; i < NP; ++i) Drow[i] -= cl * readlane_d(lam, i);
    }
}

// H(lane, lane) of a row held in registers (the scale of the row for the solver's growth guard)
template <int NP>
__device__ __forceinline__ double pf_diag(const double (&Hrow)[NP], const int lane, double d) {
#pragma unroll
    for (int i = 0; i < NP; ++i) d = (i == lane) ? Hrow[i] : d;
    return d;
}

// One evaluation with the point forces (parity hook, energies)
template <int NP, bool WANT_H>
__device__ __forceinline__ void eval_node_pf(const DevModel& M, const PfTable& T, double* __restrict__ sAcc, const int lane, const double xq,
                                             const double xqd, const double xv, const double eta, NodeOut& out, double (&Hrow)[NP]) {
    FrontState fs;
    eval_front<NP, WANT_H>(M, sAcc, lane, xq, xqd, xv, eta, out, fs);
    if (WANT_H) eval_hess<NP>(M, lane, fs, Hrow, nullptr, sAcc);
    pf_apply<NP, WANT_H>(T, fs, lane, out, Hrow);
}

// The guarded solve on rows held in registers (diagonal pivots in node order under the growth guard; H is dense here, so neither the
// tree solve nor a staged layout that the Hessian stage would have filled applies)
template <int NP>
__device__ __forceinline__ double pf_solve_guarded(const DevModel& M, const int lane, double* sAcc, double (&Hrow)[NP], const double g, bool& ok) {
    if constexpr (NP == 64) return lu_solve_neg_diag64(M.n, lane, sAcc, Hrow, g, ok);
    else return lu_solve_neg_diag<NP>(lane, Hrow, g, pf_diag<NP>(Hrow, lane, 1.0), ok);
}

// newton() of driverRedMaxBDF1.m:94-157 for a model with point forces: newton_impl's loop (same decisions in the same order, the
// compensated iterate, the stall shortcut) with the point stage behind every evaluation of the front and the dense update behind
// every Hessian.  Solve policy as newton_policy: guarded diagonal pivots, a tripped solve redone with partial pivoting
// (RMX_ST_PIVOTED), whole steps of pivoting while the guard keeps tripping.
template <int NP>
__device__ __forceinline__ double newton_pf(const DevModel& M, const PfTable& T, const DevOpts& o, double* sAcc, const int lane, double x,
                                            const double qA, const double qB, const double eta, NodeOut& last, int& iters, int& halvings,
                                            int& status, PivotPolicy& piv, double& xlo) {
    const bool pivot_only = o.lu_mode != 0 || piv.hold > 0;      // wave-uniform
    if (piv.hold > 0) --piv.hold;
    double Hrow[NP];
    FrontState fs;
    NodeOut e;
    double lo = 0.0;
    eval_front<NP, true>(M, sAcc, lane, x, (x - qA) / eta, x - qB, eta, e, fs);
    pf_apply<NP, false>(T, fs, lane, e, Hrow);
    int iter = 1, lsfail = 0;
    double gcarry = -1.0;
    while (true) {
        NodeOut eh = e;                  // (the Hessian pass adds the forces' residual share again: to a copy)
        eval_hess<NP>(M, lane, fs, Hrow, nullptr, sAcc);
        pf_apply<NP, true>(T, fs, lane, eh, Hrow);
        const NodeOut e0 = e;
        last = e;
        ++iters;
        double dx = 0.0;
        bool lu_ok = false;
        if (!pivot_only) {
            dx = pf_solve_guarded<NP>(M, lane, sAcc, Hrow, e.g, lu_ok);
            if (lu_ok) {
                piv.streak = 0;
            } else {                     // growth guard tripped: H was destroyed in place, form it again
                ++piv.streak;
                status |= 16;
                eval_hess<NP>(M, lane, fs, Hrow, nullptr, sAcc);
                eh = e;
                pf_apply<NP, true>(T, fs, lane, eh, Hrow);
            }
        }
        if (!lu_ok) dx = lu_solve_neg<NP>(M.n, lane, Hrow, e.g);
        const double dxn2 = wave_sum(dx * dx);
        if (!(dxn2 == dxn2)) {
            status |= 4;
            break;
        }
        if (sqrt(dxn2) > o.dxMax) {
            status |= 1;
            break;
        }
        double alpha = 1.0;
        const double g0n2 = gcarry >= 0.0 ? gcarry : wave_sum(e.g * e.g);
        const double f0 = 0.5 * g0n2;
        const double x0 = x, lo0 = lo;
        int iterLs = 1;
        double gn2 = g0n2;
        bool stalled = false;
        while (true) {
            two_sum(x0, fma(alpha, dx, lo0), x, lo);
            lo *= o.comp;
            if (__all(x == x0 && lo == lo0)) {      // see newton_impl: every further halving re-evaluates g(x0)
                stalled = true;
                iterLs = o.iterLsMax;
                e = e0;
                break;
            }
            eval_front<NP, true>(M, sAcc, lane, x, ((x - qA) + lo) / eta, (x - qB) + lo, eta, e, fs);
            pf_apply<NP, false>(T, fs, lane, e, Hrow);
            gn2 = wave_sum(e.g * e.g);
            if (0.5 * gn2 < f0) break;
            if (iterLs >= o.iterLsMax) break;
            alpha *= 0.5;
            ++iterLs;
        }
        last = e;
        halvings += iterLs - 1;
        if (stalled) {
            if (!(sqrt(g0n2) < o.tol)) status |= 2 | 8;
            break;
        }
        gcarry = gn2;
        if (sqrt(gn2) < o.tol) break;
        if (iter >= o.iterMax) {
            status |= 2;
            break;
        }
        lsfail += (0.5 * gn2 < f0) ? 0 : 1;
        if (o.lsFailLimit > 0 && lsfail >= o.lsFailLimit) {
            status |= 2 | ST_LS_CUT;
            break;
        }
        ++iter;
    }
    if (!pivot_only) pivot_policy_update(piv);
    xlo = lo;
    return x;
}
#endif  // __HIPCC__

}  // namespace rmx
