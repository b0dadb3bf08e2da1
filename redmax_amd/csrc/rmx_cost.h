// rmx_cost.h -- the task-space cost kernel, k_rollout_cost<NP, FRAMES>, behind rmx_rollout_points / rmx_rollout_cost (FRAMES = false)
// and rmx_rollout_frames / rmx_rollout_cost_frames (FRAMES = true) of include/redmax_hip.h: position - and with FRAMES point velocity
// and orientation - of body frames along a state record, the pull-back of cotangents through them, and the second-order model of a
// joint-space quadratic plus targets on them that the Riccati sweep (rmx_lqr.h) takes.  Included and instantiated from part_plain.hip
// alone, for every padded size.  Everything about velocity and rotation sits under `if constexpr (FRAMES)`: the point instantiation
// is the same text with those parts compiled out, so a frame step whose terms weigh position alone executes the point
// instantiation's instructions on its numbers and writes its bits (and the point instantiation stays the lighter kernel).
//
// One wavefront per (rollout, step), lane = node, as rmx_rollout_linearize: every row of the record is independent, so the grid is
// B * nsteps.  No LDS and no barrier: a wavefront evaluates the kinematics ONCE, so the per-node constants are read straight from the
// model's arrays (coalesced over the lanes) and not staged as the step kernels stage them.
//
// The front (cost_front) is the kinematic part of eval_front_e2 alone - the joint transform, the world frames Rw, pw by the chain scan
// or the pointer jumping of the tree, the world joint screws sw, sv - without velocities, wrenches, energies or subtree scans.  The
// velocity front (frame_twists, FRAMES) forms the node twists  om_i = sum_{j in anc*(i)} sw_j qdot_j,  V_i = sum_{j in anc*(i)} sv_j
// qdot_j (i included) from the ancestor masks cost_front already holds: every lane adds the broadcast share of node j = 0 .. n-1
// where bit j of its mask is set, in ascending j - one loop for chains and trees, one order of summation.  It runs only in a step
// that owns a term with wvel > 0 (rmx_rollout_frames: only where v, gv or gqd is asked for).  A step that owns no term skips both
// fronts through a wave-uniform branch: its rows are the joint-space part alone (zeros for gq, gqd).
//
// For a term t on node n with local point xl:   p = Rw[n] xl + pw[n], and the column of its Jacobian that belongs to the DOF of node
// i is   J_i = sv_i + sw_i x p   where i == n or i is an ancestor of n (bit i of n's ancestor mask), an exact zero elsewhere.  This
// is the Jacobian AT THE GIVEN STATE q[b][k-1] - not at the last evaluated Newton iterate, which is what the TRK branch of
// k_adjoint_fwd (rmx_kernels.h) reproduces from the reference: lx is the exact gradient of Jk at the state it is given.  With FRAMES,
// for lane i on the path:
//     v   = V_n + om_n x p                                           ( = Jp qdot; wave-uniform)
//     G_i = sw_i x (v - (V_i + om_i x p)) + om_i x J_i               dv/dq_i      (dv/dqdot_i = J_i)
//     W_i = sw_i                                                     the angular column
//     e_w = 1/2 a(R Rtarget'),  a(M) = (M32 - M23, M13 - M31, M21 - M12)
// With x = (q, qdot), dx = x - xgoal, r = p - xtarget, rv = v - vtarget over the terms of the step, in the caller's order (a point
// term is a frame term with wvel = wrot = 0):
//     Jk   = 1/2 dx'Q dx + sum_t wpos/2 |r|^2 + wvel/2 |rv|^2 + wrot/4 |R - Rtarget|_F^2
//     lx   = Q dx + sum_t ( wpos J'r + wvel G'rv + wrot W'e_w ; wvel J'rv )
//     Qout = Q + sum_t [ wpos J'J + wvel G'G + wrot W'W, wvel G'J ; wvel J'G, wvel J'J ]       Gauss-Newton: the curvature of p, v
//                                                                                             and R is dropped
//     gq   = sum_t J'gx + G'gv + W'a(gR R'),   gqd = sum_t J'gv                                (rmx_rollout_points / _frames)
// Every sum runs in one order: the joint-space part first (columns ascending, one FMA each), then the terms in the caller's order,
// inside a term position, velocity, rotation, the three Cartesian components in order.  Every product is an explicit fma or a lone
// multiplication, so no contraction is left to the compiler: entry (i, j) of Qout is formed in the lane of node i from its own
// columns and the broadcast columns of node j, and cost_dot commutes bit for bit - the same numbers in the same order as entry
// (j, i), the cross blocks included, hence Qout is symmetric bit for bit whenever Q is.  A structural zero adds nothing (a select,
// not a product with 0.0): off the path, where wvel or wrot is zero, in the rows of steps without terms and - for point terms - in
// the qdot rows and columns the accumulators keep the input's bits.
//
// Q and xgoal absent: the same arithmetic on 0.0 in their place (no loads), so a NULL table has the bits of a table of zeros.  A
// NULL output drops its stores alone.  Q traffic: every entry of the input row is read once and every entry of the output row written
// once, through plain vector stores, coalesced along the column-major rows (the reduced indices of the lanes are a permutation of
// 0 .. nr-1); nothing of it is staged in LDS.  Matrices in memory are column-major, CostFront::Rw is row-major.
#pragma once
#include "rmx_host.h"      /* TaskArgs */

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

struct FrameTwist {
    double om[3], V[3];      // angular and linear part of this lane's node twist
};

__device__ __forceinline__ void frame_twists(const CostFront& f, const int n, const int lane, const bool dof, const double qd, FrameTwist& w) {
    double sh[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        sh[c] = dof ? f.sw[c] * qd : 0.0;
        sh[3 + c] = dof ? f.sv[c] * qd : 0.0;
    }
    const unsigned long long mine = f.anc_m | (lane < n ? 1ull << lane : 0ull);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < n; ++j) {
        const bool in = ((mine >> j) & 1ull) != 0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double s = readlane_d(sh[c], j);
            acc[c] = in ? acc[c] + s : acc[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        w.om[c] = acc[c];
        w.V[c] = acc[3 + c];
    }
}

// One term at this wavefront's state: the point p (wave-uniform) and this lane's column J of its Jacobian; with FRAMES and vel
// (wave-uniform) the point's velocity v (wave-uniform) and this lane's column G of dv/dq - v and G are zero without vel, and not
// written at all without FRAMES.  Returns whether the lane's node is on the path (J and G are zero off it).  One function, so that
// every use forms p, J, v and G by the same instructions.
template <bool FRAMES>
__device__ __forceinline__ bool cost_term(const CostFront& f, const FrameTwist& w, const bool vel, const rmx_track::DevTerm& T, const int lane,
                                          const bool dof, double p[3], double v[3], double J[3], double G[3]) {
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
    if constexpr (FRAMES) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = G[c] = 0.0;
        if (vel) {
            double omn[3], Vn[3], d3[3], g1[3], g2[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                omn[c] = readlane_d(w.om[c], node);
                Vn[c] = readlane_d(w.V[c], node);
            }
            cost_cross(omn, p, t3);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = Vn[c] + t3[c];
            cost_cross(w.om, p, t3);
#pragma unroll
            for (int c = 0; c < 3; ++c) d3[c] = v[c] - (w.V[c] + t3[c]);
            cost_cross(f.sw, d3, g1);
            cost_cross(w.om, J, g2);
#pragma unroll
            for (int c = 0; c < 3; ++c) G[c] = on ? g1[c] + g2[c] : 0.0;
        }
    }
    return on;
}

// the world frame of a term's body (wave-uniform, row-major)
__device__ __forceinline__ void frame_rot(const CostFront& f, const rmx_track::DevTerm& T, double Rb[9]) {
    const int node = __builtin_amdgcn_readfirstlane(T.node);
#pragma unroll
    for (int c = 0; c < 9; ++c) Rb[c] = readlane_d(f.Rw[c], node);
}

// a(A B') for A column-major (memory) and B row-major (a frame): (A B')(i, j) = sum_k A(i, k) B(j, k)
__device__ __forceinline__ void frame_a_cm_rm(const double A[9], const double Bm[9], double o[3]) {
    double Mx[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Mx[3 * i + j] = fma(A[6 + i], Bm[3 * j + 2], fma(A[3 + i], Bm[3 * j + 1], A[i] * Bm[3 * j]));
    o[0] = Mx[7] - Mx[5];
    o[1] = Mx[2] - Mx[6];
    o[2] = Mx[3] - Mx[1];
}

template <int NP, bool FRAMES>
__global__ void __launch_bounds__(64) k_rollout_cost(const DevModel M, const TaskArgs a) {
    const int lane = threadIdx.x, n = M.n, nr = M.nr, d2 = 2 * nr;
    const int traj = blockIdx.x / a.nsteps, s = blockIdx.x - traj * a.nsteps;      // row s: the state after step s + 1
    const size_t row = (size_t)traj * a.nsteps + s;
    const int id = lane < n ? M.idx[lane] : -1;
    const bool dof = id >= 0;
    const int tb = a.trk_begin ? a.trk_begin[s] : 0, te = a.trk_begin ? a.trk_begin[s + 1] : 0;
    const bool front = te > tb;      // (wave-uniform)
    const bool model = a.Jk || a.lx || a.Qout;
    const double qj = dof ? a.q[row * nr + id] : 0.0;
    CostFront f;
    FrameTwist w;
    if (front) cost_front<NP>(M, lane, qj, f);
    bool vel = false;      // (wave-uniform) the step needs the velocity front
    if constexpr (FRAMES) {
        vel = front && !model && (a.v || a.gv || a.gqd);
        if (model)
            for (int t = tb; t < te; ++t) vel = vel || a.trk[t].wvel > 0.0;
        const double qdj = (dof && a.qd) ? a.qd[row * nr + id] : 0.0;
        if (vel) frame_twists(f, n, lane, dof, qdj, w);
    }

    // ---- rmx_rollout_points / rmx_rollout_frames: the frames, and the pull-back of their cotangents
    if (a.x || (FRAMES && (a.v || a.R))) {
        for (int t = tb; t < te; ++t) {
            const rmx_track::DevTerm& T = a.trk[t].t;
            double p[3], v[3], J[3], G[3];
            cost_term<FRAMES>(f, w, vel, T, lane, dof, p, v, J, G);
            const size_t at = (size_t)traj * a.nterms + T.orig;
            if (a.x && lane < 3) a.x[at * 3 + lane] = lane == 0 ? p[0] : (lane == 1 ? p[1] : p[2]);
            if constexpr (FRAMES) {
                if (a.v && lane < 3) a.v[at * 3 + lane] = lane == 0 ? v[0] : (lane == 1 ? v[1] : v[2]);
                if (a.R) {
                    double Rb[9];
                    frame_rot(f, T, Rb);
                    const int e = 3 * (lane % 3) + lane / 3;      // the row-major place of slot `lane` of the column-major output
                    double val = Rb[0];
#pragma unroll
                    for (int c = 1; c < 9; ++c) val = e == c ? Rb[c] : val;
                    if (lane < 9) a.R[at * 9 + lane] = val;
                }
            }
        }
    }
    if (a.gq || (FRAMES && a.gqd)) {
        double acc = 0.0, accd = 0.0;
        for (int t = tb; t < te; ++t) {
            const rmx_track::DevTerm& T = a.trk[t].t;
            const size_t at = (size_t)traj * a.nterms + T.orig;
            double p[3], v[3], J[3], G[3];
            const bool on = cost_term<FRAMES>(f, w, vel, T, lane, dof, p, v, J, G);
            if (a.gx) {
                const double* gx = a.gx + at * 3;
                const double g3[3] = {gx[0], gx[1], gx[2]};
                if (on) acc += cost_dot(J, g3);
            }
            if constexpr (FRAMES) {
                if (a.gv) {
                    const double* gv = a.gv + at * 3;
                    const double g3[3] = {gv[0], gv[1], gv[2]};
                    if (on) {
                        acc += cost_dot(G, g3);
                        accd += cost_dot(J, g3);
                    }
                }
                if (a.gR) {
                    const double* gR = a.gR + at * 9;
                    double A[9], Rb[9], m3[3];
#pragma unroll
                    for (int c = 0; c < 9; ++c) A[c] = gR[c];
                    frame_rot(f, T, Rb);
                    frame_a_cm_rm(A, Rb, m3);
                    if (on) acc += cost_dot(f.sw, m3);
                }
            }
        }
        if (dof) {
            if (a.gq) a.gq[row * nr + id] = acc;
            if constexpr (FRAMES)
                if (a.gqd) a.gqd[row * nr + id] = accd;
        }
    }
    if (!model) return;

    // ---- rmx_rollout_cost / rmx_rollout_cost_frames.  The joint-space part: this lane holds rows id and nr + id of Q, the columns in
    // ascending order
    const double* Qs = a.Qin ? a.Qin + (size_t)traj * a.q_stride + (size_t)s * d2 * d2 : nullptr;
    const double* xg = a.xgoal ? a.xgoal + (size_t)traj * a.goal_stride + (size_t)s * d2 : nullptr;
    double* Qo = a.Qout ? a.Qout + row * (size_t)d2 * d2 : nullptr;
    const int ii = dof ? id : 0;
    const double dxq = dof ? qj - (xg ? xg[ii] : 0.0) : 0.0;
    const double dxv = dof ? a.qd[row * nr + ii] - (xg ? xg[nr + ii] : 0.0) : 0.0;
    double a1 = 0.0, a2 = 0.0;      // rows id, nr + id of Q dx
    // the first term of the step (most steps own one) is formed once, ahead of the columns; cost_term is the same instructions on the
    // same numbers wherever it runs, so the later terms, formed again per column, see no difference
    double J0[3] = {0.0, 0.0, 0.0}, G0[3] = {0.0, 0.0, 0.0}, wp0 = 0.0, wv0 = 0.0, wr0 = 0.0;
    bool on0 = false;
    if (front && Qo) {
        double p[3], v[3];
        on0 = cost_term<FRAMES>(f, w, vel, a.trk[tb].t, lane, dof, p, v, J0, G0);
        wp0 = a.trk[tb].t.wpos;
        if constexpr (FRAMES) {
            wv0 = a.trk[tb].wvel;
            wr0 = a.trk[tb].wrot;
        }
    }
    for (int col = 0; col < nr; ++col) {
        const unsigned long long mk = __ballot(id == col);
        const int c = __builtin_amdgcn_readfirstlane(mk ? (int)__builtin_ctzll(mk) : 0);      // the node of reduced DOF col
        const double dxc = readlane_d(dxq, c);
        const double q1 = (Qs && dof) ? Qs[(size_t)col * d2 + ii] : 0.0, q2 = (Qs && dof) ? Qs[(size_t)col * d2 + nr + ii] : 0.0;
        a1 = fma(q1, dxc, a1);
        a2 = fma(q2, dxc, a2);
        if (Qo) {
            double g = q1, h = q2;      // Q(id, col) and Q(nr + id, col), then the terms of the step
            for (int t = tb; t < te; ++t) {
                double p[3], v[3], J[3] = {J0[0], J0[1], J0[2]}, G[3] = {G0[0], G0[1], G0[2]}, wp = wp0, wv = wv0, wr = wr0;
                bool on = on0;
                if (t > tb) {
                    on = cost_term<FRAMES>(f, w, vel, a.trk[t].t, lane, dof, p, v, J, G);
                    wp = a.trk[t].t.wpos;
                    if constexpr (FRAMES) {
                        wv = a.trk[t].wvel;
                        wr = a.trk[t].wrot;
                    }
                }
                const double Jc[3] = {readlane_d(J[0], c), readlane_d(J[1], c), readlane_d(J[2], c)};
                const bool on_c = ((__ballot(on) >> c) & 1ull) != 0;      // (wave-uniform: is the column's node on the path)
                const double sd = cost_dot(J, Jc);
                g = (on && on_c) ? fma(wp, sd, g) : g;
                if constexpr (FRAMES) {
                    if (wv > 0.0) {      // (wave-uniform)
                        const double Gc[3] = {readlane_d(G[0], c), readlane_d(G[1], c), readlane_d(G[2], c)};
                        const double gg = cost_dot(G, Gc), jg = cost_dot(J, Gc);
                        g = (on && on_c) ? fma(wv, gg, g) : g;
                        h = (on && on_c) ? fma(wv, jg, h) : h;
                    }
                    if (wr > 0.0) {
                        const double Wc[3] = {readlane_d(f.sw[0], c), readlane_d(f.sw[1], c), readlane_d(f.sw[2], c)};
                        const double ww = cost_dot(f.sw, Wc);
                        g = (on && on_c) ? fma(wr, ww, g) : g;
                    }
                }
            }
            if (dof) {
                Qo[(size_t)col * d2 + ii] = g;
                Qo[(size_t)col * d2 + nr + ii] = h;
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
        if (Qo) {
            double g = q1, h = q2;      // Q(id, nr + col) and Q(nr + id, nr + col): the velocity terms alone add to them
            if constexpr (FRAMES) {
                if (vel) {
                    for (int t = tb; t < te; ++t) {
                        double p[3], v[3], J[3] = {J0[0], J0[1], J0[2]}, G[3] = {G0[0], G0[1], G0[2]}, wv = wv0;
                        bool on = on0;
                        if (t > tb) {
                            on = cost_term<FRAMES>(f, w, vel, a.trk[t].t, lane, dof, p, v, J, G);
                            wv = a.trk[t].wvel;
                        }
                        if (wv > 0.0) {
                            const double Jc[3] = {readlane_d(J[0], c), readlane_d(J[1], c), readlane_d(J[2], c)};
                            const bool on_c = ((__ballot(on) >> c) & 1ull) != 0;
                            const double gj = cost_dot(G, Jc), jj = cost_dot(J, Jc);
                            g = (on && on_c) ? fma(wv, gj, g) : g;
                            h = (on && on_c) ? fma(wv, jj, h) : h;
                        }
                    }
                }
            }
            if (dof) {
                Qo[(size_t)(nr + col) * d2 + ii] = g;
                Qo[(size_t)(nr + col) * d2 + nr + ii] = h;
            }
        }
    }
    // ---- the value and the gradient: the joint-space part, then the terms
    double Jk = 0.5 * wave_sum(fma(dxv, a2, dxq * a1));
    double lq = a1, lv = a2;
    for (int t = tb; t < te; ++t) {
        const rmx_track::DevTerm& T = a.trk[t].t;
        const size_t at = (size_t)traj * a.t_stride + (size_t)T.orig;
        double p[3], v[3], J[3], G[3];
        const bool on = cost_term<FRAMES>(f, w, vel, T, lane, dof, p, v, J, G);
        // (a weight > 0 has its table: the host refuses the call otherwise; a point call always has xt)
        const double* xt = (FRAMES && !a.xt) ? nullptr : a.xt + at * 3;
        const double r3[3] = {p[0] - (xt ? xt[0] : 0.0), p[1] - (xt ? xt[1] : 0.0), p[2] - (xt ? xt[2] : 0.0)};
        Jk = fma(0.5 * T.wpos, cost_dot(r3, r3), Jk);
        lq = on ? fma(T.wpos, cost_dot(J, r3), lq) : lq;
        if constexpr (FRAMES) {
            const double wv = a.trk[t].wvel, wr = a.trk[t].wrot;
            if (wv > 0.0) {      // (wave-uniform)
                const double* vt = a.vt + at * 3;
                const double rv[3] = {v[0] - vt[0], v[1] - vt[1], v[2] - vt[2]};
                Jk = fma(0.5 * wv, cost_dot(rv, rv), Jk);
                lq = on ? fma(wv, cost_dot(G, rv), lq) : lq;
                lv = on ? fma(wv, cost_dot(J, rv), lv) : lv;
            }
            if (wr > 0.0) {
                const double* Rt = a.Rt + at * 9;
                double A[9], Rb[9], m3[3];
#pragma unroll
                for (int c = 0; c < 9; ++c) A[c] = Rt[c];
                frame_rot(f, T, Rb);
                double fro = 0.0;      // |R - Rtarget|_F^2, the entries in the order of the memory
#pragma unroll
                for (int c = 0; c < 9; ++c) {
                    const double dd = Rb[3 * (c % 3) + c / 3] - A[c];
                    fro = fma(dd, dd, fro);
                }
                // e_w = 1/2 a(R Rtarget') = -1/2 a(Rtarget R')
                frame_a_cm_rm(A, Rb, m3);
                const double ew[3] = {-0.5 * m3[0], -0.5 * m3[1], -0.5 * m3[2]};
                Jk = fma(0.25 * wr, fro, Jk);
                lq = on ? fma(wr, cost_dot(f.sw, ew), lq) : lq;
            }
        }
    }
    if (a.Jk && lane == 0) a.Jk[row] = Jk;
    if (a.lx && dof) {
        a.lx[row * d2 + ii] = lq;
        a.lx[row * d2 + nr + ii] = lv;
    }
}
