// rmx_cost.h -- rmx_rollout_points / rmx_rollout_cost (include/redmax_hip.h): world positions of body points along a state record,
// the pull-back of cotangents through them, and the second-order model of a joint-space quadratic plus point targets that the
// Riccati sweep (rmx_lqr.h) takes.  Included and instantiated from part_plain.hip alone, for every padded size.
//
// One wavefront per (rollout, step), lane = node, as rmx_rollout_linearize: every row of the record is independent, so the grid is
// B * nsteps.  No LDS and no barrier: a wavefront evaluates the kinematics ONCE, so the per-node constants are read straight from the
// model's arrays (coalesced over the lanes) and not staged as the step kernels stage them.
//
// The front (cost_front) is the kinematic part of eval_front_e2 alone - the joint transform, the world frames Rw, pw by the chain scan
// or the pointer jumping of the tree, the world joint screws sw, sv - without velocities, wrenches, energies or subtree scans.  A step
// that owns no term skips it through a wave-uniform branch: its rows are the joint-space part alone (zeros for gq).
//
// For a term t on node n_t with local point xl:   p_t = Rw[n_t] xl + pw[n_t], and the column of its Jacobian that belongs to the DOF
// of node j is   sv_j + sw_j x p_t   where j == n_t or j is an ancestor of n_t (bit j of n_t's ancestor mask), an exact zero
// elsewhere.  This is the Jacobian AT THE GIVEN STATE q[b][k-1] - not at the last evaluated Newton iterate, which is what the TRK
// branch of k_adjoint_fwd (rmx_kernels.h) reproduces from the reference: lx is the exact gradient of Jk at the state it is given.
//
// With x = (q, qdot), dx = x - xgoal, r_t = p_t - xtarget_t over the terms of the step, in the caller's order:
//     Jk   = 1/2 dx'Q dx + sum_t 1/2 w_t |r_t|^2
//     lx   = Q dx + (sum_t w_t Jp_t'r_t ; 0)
//     Qout = Q + [sum_t w_t Jp_t'Jp_t, 0; 0, 0]        Gauss-Newton: the term sum_t w_t r_t . d2p_t/dq2 is dropped
//     gq   = sum_t Jp_t'gx_t                            (rmx_rollout_points)
// Every sum runs in one order: the joint-space part first (columns ascending, one FMA each), then the terms in the caller's order,
// the three Cartesian components in order inside a term.  Every product is an explicit fma or a lone multiplication, so no
// contraction is left to the compiler: entry (i, j) of Qout is Q(i, j) + sum_t w_t (J_i . J_j), formed in the lane of node i from its
// own column and the broadcast column of node j - the same numbers in the same order as entry (j, i), hence Qout is symmetric bit for
// bit whenever Q is.  A structural zero adds nothing (a select, not a product with 0.0): the qdot rows and columns, the rows of steps
// without terms and the off-path entries are the input's bits.
//
// Q and xgoal absent: the same arithmetic on 0.0 in their place (no loads), so a NULL table has the bits of a table of zeros.  A
// NULL output drops its stores alone.  Q traffic: every entry of the input row is read once and every entry of the output row written
// once, through plain vector stores, coalesced along the column-major rows (the reduced indices of the lanes are a permutation of
// 0 .. nr-1); nothing of it is staged in LDS.
#pragma once
#include "rmx_host.h"      /* CostArgs */

struct CostFront {
    double Rw[9], pw[3];      // world frame of this lane's body
    double sw[3], sv[3];      // world joint screw
    unsigned long long anc_m; // bit i: node i is a strict ancestor of this node
};

// a x b and a . b with every product spelled out (see the header: nothing here may be contracted one way in one place and another way
// in another)
__device__ __forceinline__ void cost_cross(const double a[3], const double b[3], double c[3]) {
    c[0] = fma(a[1], b[2], -(a[2] * b[1]));
    c[1] = fma(a[2], b[0], -(a[0] * b[2]));
    c[2] = fma(a[0], b[1], -(a[1] * b[0]));
}
__device__ __forceinline__ double cost_dot(const double a[3], const double b[3]) { return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0])); }

// the kinematic part of eval_front_e2: frames and screws of every node at q (zero on lanes without a DOF)
template <int NP>
__device__ __forceinline__ void cost_front(const DevModel& M, const int lane, const double q, CostFront& f) {
    const bool act = lane < M.n;
    const int jj = act ? lane : 0;
    const int type = act ? M.type[jj] : 0;
    f.anc_m = act ? M.rel[jj] : 0ull;
    double u = 0.0, w = 0.0;
    if (type == 1) {
        sincos(q, &u, &w);
    } else if (type == 2) {
        u = q;
    }
    // T_j(q) = K0 + u K1 + w K2; lanes past the tree hold the identity, so they are neutral in the chain scan
    double R[9], p[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        const double k0 = M.K[c * MAXN + jj], k1 = M.K[(12 + c) * MAXN + jj], k2 = M.K[(24 + c) * MAXN + jj];
        R[c] = act ? fma(w, k2, fma(u, k1, k0)) : ((c % 4 == 0) ? 1.0 : 0.0);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double k0 = M.K[(9 + c) * MAXN + jj], k1 = M.K[(21 + c) * MAXN + jj], k2 = M.K[(33 + c) * MAXN + jj];
        p[c] = act ? fma(w, k2, fma(u, k1, k0)) : 0.0;
    }
    if (M.is_chain) {
        chain_scan_transform<NP>(lane, R, p);
    } else {      // pointer jumping over the ancestors, as eval_front_e2
        for (int r = 0; r < M.rounds; ++r) {
            const int a = act ? M.anc[r * MAXN + jj] : -1;
            const int src = a >= 0 ? a : lane;
            double Ra[9], pa[3];
#pragma unroll
            for (int c = 0; c < 9; ++c) Ra[c] = shfl_d(R[c], src);
#pragma unroll
            for (int c = 0; c < 3; ++c) pa[c] = shfl_d(p[c], src);
            if (a >= 0) {
                double Rn[9], pn[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) Rn[3 * i + k] = Ra[3 * i] * R[k] + Ra[3 * i + 1] * R[3 + k] + Ra[3 * i + 2] * R[6 + k];
                    pn[i] = Ra[3 * i] * p[0] + Ra[3 * i + 1] * p[1] + Ra[3 * i + 2] * p[2] + pa[i];
                }
#pragma unroll
                for (int c = 0; c < 9; ++c) R[c] = Rn[c];
#pragma unroll
                for (int c = 0; c < 3; ++c) p[c] = pn[c];
            }
        }
    }
    // s_j = Ad(E_w,j) (A0_ij S): sw = R sb_w, sv = R sb_v + p x sw
    double sbw[3], sbv[3], t3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        sbw[c] = act ? M.sb[c * MAXN + jj] : 0.0;
        sbv[c] = act ? M.sb[(3 + c) * MAXN + jj] : 0.0;
    }
    mat3v(R, sbw, f.sw);
    mat3v(R, sbv, f.sv);
    cross3(p, f.sw, t3);
#pragma unroll
    for (int c = 0; c < 3; ++c) f.sv[c] += t3[c];
#pragma unroll
    for (int c = 0; c < 9; ++c) f.Rw[c] = R[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) f.pw[c] = p[c];
}

// One term at this wavefront's state: the point p (wave-uniform) and this lane's column J of its Jacobian; returns whether the lane's
// node is on the path (J is zero off it).  One function, so that every use forms p and J by the same instructions.
__device__ __forceinline__ bool cost_term(const CostFront& f, const rmx_track::DevTerm& T, const int lane, const bool dof, double p[3], double J[3]) {
    const int node = __builtin_amdgcn_readfirstlane(T.node);
    const double xl[3] = {T.xl[0], T.xl[1], T.xl[2]};
    double Rb[9], pb[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) Rb[c] = readlane_d(f.Rw[c], node);
#pragma unroll
    for (int c = 0; c < 3; ++c) pb[c] = readlane_d(f.pw[c], node);
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = fma(Rb[3 * c + 2], xl[2], fma(Rb[3 * c + 1], xl[1], fma(Rb[3 * c], xl[0], pb[c])));
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(f.anc_m & 0xffffffffull), node);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(f.anc_m >> 32), node);
    const unsigned long long path = (((unsigned long long)hi << 32) | lo) | (1ull << node);      // the node and its strict ancestors
    const bool on = dof && ((path >> lane) & 1ull) != 0;
    double t3[3];
    cost_cross(f.sw, p, t3);
#pragma unroll
    for (int c = 0; c < 3; ++c) J[c] = on ? f.sv[c] + t3[c] : 0.0;
    return on;
}

template <int NP>
__global__ void __launch_bounds__(64) k_rollout_cost(const DevModel M, const CostArgs a) {
    const int lane = threadIdx.x, n = M.n, nr = M.nr, d2 = 2 * nr;
    const int traj = blockIdx.x / a.nsteps, s = blockIdx.x - traj * a.nsteps;      // row s: the state after step s + 1
    const size_t row = (size_t)traj * a.nsteps + s;
    const int id = lane < n ? M.idx[lane] : -1;
    const bool dof = id >= 0;
    const int tb = a.trk_begin ? a.trk_begin[s] : 0, te = a.trk_begin ? a.trk_begin[s + 1] : 0;
    const bool front = te > tb;      // (wave-uniform)
    const double qj = dof ? a.q[row * nr + id] : 0.0;
    CostFront f;
    if (front) cost_front<NP>(M, lane, qj, f);

    // ---- rmx_rollout_points: the points, and the pull-back of their cotangents
    if (a.x) {
        for (int t = tb; t < te; ++t) {
            const rmx_track::DevTerm& T = a.trk[t];
            double p[3], J[3];
            cost_term(f, T, lane, dof, p, J);
            if (lane < 3) a.x[((size_t)traj * a.nterms + T.orig) * 3 + lane] = lane == 0 ? p[0] : (lane == 1 ? p[1] : p[2]);
        }
    }
    if (a.gq) {
        double acc = 0.0;
        for (int t = tb; t < te; ++t) {
            const rmx_track::DevTerm& T = a.trk[t];
            const double* gx = a.gx + ((size_t)traj * a.nterms + T.orig) * 3;
            const double g3[3] = {gx[0], gx[1], gx[2]};
            double p[3], J[3];
            if (cost_term(f, T, lane, dof, p, J)) acc += cost_dot(J, g3);
        }
        if (dof) a.gq[row * nr + id] = acc;
    }
    if (!a.Jk && !a.lx && !a.Qout) return;

    // ---- rmx_rollout_cost.  The joint-space part: this lane holds rows id and nr + id of Q, the columns in ascending order
    const double* Qs = a.Qin ? a.Qin + (size_t)traj * a.q_stride + (size_t)s * d2 * d2 : nullptr;
    const double* xg = a.xgoal ? a.xgoal + (size_t)traj * a.goal_stride + (size_t)s * d2 : nullptr;
    double* Qo = a.Qout ? a.Qout + row * (size_t)d2 * d2 : nullptr;
    const int ii = dof ? id : 0;
    const double dxq = dof ? qj - (xg ? xg[ii] : 0.0) : 0.0;
    const double dxv = dof ? a.qd[row * nr + ii] - (xg ? xg[nr + ii] : 0.0) : 0.0;
    double a1 = 0.0, a2 = 0.0;      // rows id, nr + id of Q dx
    // the first term of the step (most steps own one) is formed once, ahead of the columns; cost_term is the same instructions on the
    // same numbers wherever it runs, so the later terms, formed again per column, see no difference
    double J0[3] = {0.0, 0.0, 0.0}, w0 = 0.0;
    bool on0 = false;
    if (front && Qo) {
        double p[3];
        on0 = cost_term(f, a.trk[tb], lane, dof, p, J0);
        w0 = a.trk[tb].wpos;
    }
    for (int col = 0; col < nr; ++col) {
        const unsigned long long mk = __ballot(id == col);
        const int c = __builtin_amdgcn_readfirstlane(mk ? (int)__builtin_ctzll(mk) : 0);      // the node of reduced DOF col
        const double dxc = readlane_d(dxq, c);
        const double q1 = (Qs && dof) ? Qs[(size_t)col * d2 + ii] : 0.0, q2 = (Qs && dof) ? Qs[(size_t)col * d2 + nr + ii] : 0.0;
        a1 = fma(q1, dxc, a1);
        a2 = fma(q2, dxc, a2);
        if (Qo) {
            double g = q1;      // Q(id, col), then the terms of the step
            for (int t = tb; t < te; ++t) {
                double p[3], J[3] = {J0[0], J0[1], J0[2]}, w = w0;
                bool on = on0;
                if (t > tb) {
                    on = cost_term(f, a.trk[t], lane, dof, p, J);
                    w = a.trk[t].wpos;
                }
                const double Jc[3] = {readlane_d(J[0], c), readlane_d(J[1], c), readlane_d(J[2], c)};
                const bool on_c = ((__ballot(on) >> c) & 1ull) != 0;      // (wave-uniform: is the column's node on the path)
                const double sd = cost_dot(J, Jc);
                g = (on && on_c) ? fma(w, sd, g) : g;
            }
            if (dof) {
                Qo[(size_t)col * d2 + ii] = g;
                Qo[(size_t)col * d2 + nr + ii] = q2;
            }
        }
    }
    for (int col = 0; col < nr; ++col) {
        const unsigned long long mk = __ballot(id == col);
        const int c = __builtin_amdgcn_readfirstlane(mk ? (int)__builtin_ctzll(mk) : 0);
        const double dxc = readlane_d(dxv, c);
        const double q1 = (Qs && dof) ? Qs[(size_t)(nr + col) * d2 + ii] : 0.0, q2 = (Qs && dof) ? Qs[(size_t)(nr + col) * d2 + nr + ii] : 0.0;
        a1 = fma(q1, dxc, a1);
        a2 = fma(q2, dxc, a2);
        if (Qo && dof) {
            Qo[(size_t)(nr + col) * d2 + ii] = q1;
            Qo[(size_t)(nr + col) * d2 + nr + ii] = q2;
        }
    }
    // ---- the value and the gradient: the joint-space part, then the terms
    double Jk = 0.5 * wave_sum(fma(dxv, a2, dxq * a1));
    double lq = a1;
    for (int t = tb; t < te; ++t) {
        const rmx_track::DevTerm& T = a.trk[t];
        const double* xt = a.xt + (size_t)traj * a.xt_stride + (size_t)3 * T.orig;
        double p[3], J[3];
        const bool on = cost_term(f, T, lane, dof, p, J);
        const double r3[3] = {p[0] - xt[0], p[1] - xt[1], p[2] - xt[2]};
        Jk = fma(0.5 * T.wpos, cost_dot(r3, r3), Jk);
        lq = on ? fma(T.wpos, cost_dot(J, r3), lq) : lq;
    }
    if (a.Jk && lane == 0) a.Jk[row] = Jk;
    if (a.lx && dof) {
        a.lx[row * d2 + ii] = lq;
        a.lx[row * d2 + nr + ii] = a2;
    }
}
