// rmx_frames.h -- rmx_rollout_frames / rmx_rollout_cost_frames (include/redmax_hip.h): position, velocity and orientation of body
// frames along a state record, the pull-back of cotangents through them, and the second-order model of a joint-space quadratic plus
// frame targets that the Riccati sweep (rmx_lqr.h) takes.  Included and instantiated from part_plain.hip alone, for every padded size.
//
// k_rollout_cost's shape (rmx_cost.h): one wavefront per (rollout, step), lane = node, grid B * nsteps, no LDS and no barrier.  The
// kinematic front is cost_front and a term's point and Jacobian column are cost_term's, both unchanged: a step whose terms weigh
// position alone executes k_rollout_cost's instructions on k_rollout_cost's numbers and writes its bits.
//
// The velocity front (frame_twists) forms the node twists  om_i = sum_{j in anc*(i)} sw_j qdot_j,  V_i = sum_{j in anc*(i)} sv_j qdot_j
// (i included) from the ancestor masks cost_front already holds: every lane adds the broadcast share of node j = 0 .. n-1 where bit
// j of its mask is set, in ascending j - one loop for chains and trees, one order of summation.  It runs only in a step that owns a
// term with wvel > 0 (rmx_rollout_frames: only where v, gv or gqd is asked for); a step without terms skips both fronts through a
// wave-uniform branch.
//
// For a term on node n with point p and lane i on its path (J_i = sv_i + sw_i x p is cost_term's column):
//     v   = V_n + om_n x p                                           ( = Jp qdot; wave-uniform)
//     G_i = sw_i x (v - (V_i + om_i x p)) + om_i x J_i               dv/dq_i      (dv/dqdot_i = J_i)
//     W_i = sw_i                                                     the angular column
//     e_w = 1/2 a(R Rtarget'),  a(M) = (M32 - M23, M13 - M31, M21 - M12)
// and with r = p - xtarget, rv = v - vtarget:
//     Jk   += wpos/2 |r|^2 + wvel/2 |rv|^2 + wrot/4 |R - Rtarget|_F^2
//     lx   += ( wpos J'r + wvel G'rv + wrot W'e_w ; wvel J'rv )
//     Qout += [ wpos J'J + wvel G'G + wrot W'W, wvel G'J ; wvel J'G, wvel J'J ]       (Gauss-Newton)
//     gq   += J'gx + G'gv + W'a(gR R'),   gqd += J'gv                                  (rmx_rollout_frames)
// Order of every sum: the joint-space part, then the terms in the caller's order, inside a term position, velocity, rotation.  Every
// product is an explicit fma or a lone multiplication; cost_dot commutes bit for bit, so entry (i, j) and entry (j, i) of Qout - the
// cross blocks included - are the same products in the same order.  A structural zero adds nothing (a select): off the path, and
// where wvel or wrot is zero, the accumulators keep their bits.  Matrices in memory are column-major, CostFront::Rw is row-major.
#pragma once
#include "rmx_cost.h"

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

// One term at this wavefront's state: cost_term's p and J, and with vel (wave-uniform) the point's velocity v (wave-uniform) and this
// lane's column G of dv/dq; v and G are zero without vel, G is zero off the path.  One function, as cost_term.
__device__ __forceinline__ bool frame_term(const CostFront& f, const FrameTwist& w, const bool vel, const rmx_track::DevTerm& T, const int lane,
                                           const bool dof, double p[3], double v[3], double J[3], double G[3]) {
    const bool on = cost_term(f, T, lane, dof, p, J);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = G[c] = 0.0;
    if (vel) {
        const int node = __builtin_amdgcn_readfirstlane(T.node);
        double omn[3], Vn[3], t3[3], d3[3], g1[3], g2[3];
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

template <int NP>
__global__ void __launch_bounds__(64) k_rollout_frames(const DevModel M, const FrameArgs a) {
    const int lane = threadIdx.x, n = M.n, nr = M.nr, d2 = 2 * nr;
    const int traj = blockIdx.x / a.nsteps, s = blockIdx.x - traj * a.nsteps;      // row s: the state after step s + 1
    const size_t row = (size_t)traj * a.nsteps + s;
    const int id = lane < n ? M.idx[lane] : -1;
    const bool dof = id >= 0;
    const int tb = a.trk_begin ? a.trk_begin[s] : 0, te = a.trk_begin ? a.trk_begin[s + 1] : 0;
    const bool front = te > tb;      // (wave-uniform)
    const bool model = a.Jk || a.lx || a.Qout;
    bool vel = front && !model && (a.v || a.gv || a.gqd);      // (wave-uniform)
    if (model)
        for (int t = tb; t < te; ++t) vel = vel || a.trk[t].wvel > 0.0;
    const double qj = dof ? a.q[row * nr + id] : 0.0;
    const double qdj = (dof && a.qd) ? a.qd[row * nr + id] : 0.0;
    CostFront f;
    FrameTwist w;
    if (front) cost_front<NP>(M, lane, qj, f);
    if (vel) frame_twists(f, n, lane, dof, qdj, w);

    // ---- rmx_rollout_frames: the frames, and the pull-back of their cotangents
    if (a.x || a.v || a.R) {
        for (int t = tb; t < te; ++t) {
            const rmx_track::DevTerm& T = a.trk[t].t;
            double p[3], v[3], J[3], G[3];
            frame_term(f, w, vel, T, lane, dof, p, v, J, G);
            const size_t at = (size_t)traj * a.nterms + T.orig;
            if (a.x && lane < 3) a.x[at * 3 + lane] = lane == 0 ? p[0] : (lane == 1 ? p[1] : p[2]);
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
    if (a.gq || a.gqd) {
        double acc = 0.0, accd = 0.0;
        for (int t = tb; t < te; ++t) {
            const rmx_track::DevTerm& T = a.trk[t].t;
            const size_t at = (size_t)traj * a.nterms + T.orig;
            double p[3], v[3], J[3], G[3];
            const bool on = frame_term(f, w, vel, T, lane, dof, p, v, J, G);
            if (a.gx) {
                const double* gx = a.gx + at * 3;
                const double g3[3] = {gx[0], gx[1], gx[2]};
                if (on) acc += cost_dot(J, g3);
            }
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
        if (dof) {
            if (a.gq) a.gq[row * nr + id] = acc;
            if (a.gqd) a.gqd[row * nr + id] = accd;
        }
    }
    if (!model) return;

    // ---- rmx_rollout_cost_frames.  The joint-space part: this lane holds rows id and nr + id of Q, the columns in ascending order
    const double* Qs = a.Qin ? a.Qin + (size_t)traj * a.q_stride + (size_t)s * d2 * d2 : nullptr;
    const double* xg = a.xgoal ? a.xgoal + (size_t)traj * a.goal_stride + (size_t)s * d2 : nullptr;
    double* Qo = a.Qout ? a.Qout + row * (size_t)d2 * d2 : nullptr;
    const int ii = dof ? id : 0;
    const double dxq = dof ? qj - (xg ? xg[ii] : 0.0) : 0.0;
    const double dxv = dof ? a.qd[row * nr + ii] - (xg ? xg[nr + ii] : 0.0) : 0.0;
    double a1 = 0.0, a2 = 0.0;      // rows id, nr + id of Q dx
    // the first term of the step is formed once, ahead of the columns; the later ones again per column (as k_rollout_cost)
    double J0[3] = {0.0, 0.0, 0.0}, G0[3] = {0.0, 0.0, 0.0}, wp0 = 0.0, wv0 = 0.0, wr0 = 0.0;
    bool on0 = false;
    if (front && Qo) {
        double p[3], v[3];
        on0 = frame_term(f, w, vel, a.trk[tb].t, lane, dof, p, v, J0, G0);
        wp0 = a.trk[tb].t.wpos;
        wv0 = a.trk[tb].wvel;
        wr0 = a.trk[tb].wrot;
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
                    on = frame_term(f, w, vel, a.trk[t].t, lane, dof, p, v, J, G);
                    wp = a.trk[t].t.wpos;
                    wv = a.trk[t].wvel;
                    wr = a.trk[t].wrot;
                }
                const double Jc[3] = {readlane_d(J[0], c), readlane_d(J[1], c), readlane_d(J[2], c)};
                const bool on_c = ((__ballot(on) >> c) & 1ull) != 0;      // (wave-uniform: is the column's node on the path)
                const double sd = cost_dot(J, Jc);
                g = (on && on_c) ? fma(wp, sd, g) : g;
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
            double g = q1, h = q2;      // Q(id, nr + col) and Q(nr + id, nr + col)
            if (vel) {
                for (int t = tb; t < te; ++t) {
                    double p[3], v[3], J[3] = {J0[0], J0[1], J0[2]}, G[3] = {G0[0], G0[1], G0[2]}, wv = wv0;
                    bool on = on0;
                    if (t > tb) {
                        on = frame_term(f, w, vel, a.trk[t].t, lane, dof, p, v, J, G);
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
        const double wv = a.trk[t].wvel, wr = a.trk[t].wrot;
        const size_t at = (size_t)traj * a.t_stride + (size_t)T.orig;
        double p[3], v[3], J[3], G[3];
        const bool on = frame_term(f, w, vel, T, lane, dof, p, v, J, G);
        const double* xt = a.xt ? a.xt + at * 3 : nullptr;
        const double r3[3] = {p[0] - (xt ? xt[0] : 0.0), p[1] - (xt ? xt[1] : 0.0), p[2] - (xt ? xt[2] : 0.0)};
        Jk = fma(0.5 * T.wpos, cost_dot(r3, r3), Jk);
        lq = on ? fma(T.wpos, cost_dot(J, r3), lq) : lq;
        if (wv > 0.0) {      // (wave-uniform; a weight > 0 has its table: the host refuses the call otherwise)
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
    if (a.Jk && lane == 0) a.Jk[row] = Jk;
    if (a.lx && dof) {
        a.lx[row * d2 + ii] = lq;
        a.lx[row * d2 + nr + ii] = lv;
    }
}
