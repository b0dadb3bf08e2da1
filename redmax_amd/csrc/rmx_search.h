// rmx_search.h -- rmx_rollout_search (include/redmax_hip.h): the backtracking line search of the device iLQR in ONE launch,
// k_rollout_search<NP>.  Included and instantiated from part_plain.hip alone, for the padded sizes the Riccati sweep exists for
// (4 .. 32: rmx_select.h select_rollout_search).  A kernel of its own around the building blocks of k_adjoint_fwd's ADJ_FB
// instantiation, not a mode bit of it: every existing instantiation keeps its text, and so its instruction stream and its bits.
//
// One wavefront per rollout, lane = node.  The wavefront runs PASSES over all the steps, one per trial step length in the caller's
// order and - where none is accepted, or none is given - one nominal pass.  A pass is the closed loop of
// rmx_rollout_tape_feedback_box under BDF1 from the state the batch held at the call (read again from a.q at the top of every pass:
// nothing of it is live across a Newton loop), with the feed-forward torque
//     trial pass:     uff = ubar + alpha * kff      the product rounded, then the sum (search_torque: contraction off) - the bits
//                                                    of the float64 expression a caller forms
//     nominal pass:   uff = ubar                    kff is not read: a non-finite kff cannot reach it
// The choice is a select on the VALUE behind a wave-uniform load; the step body - feedback sum, clamp, uapp store, the Newton loop,
// the H, M, D stores, the record - is one text that every pass executes, so a nominal pass under uff' = ubar + alpha * kff formed
// by the caller returns the bits of the trial pass under alpha.  Every pass overwrites the record, uapp and the tape of the pass
// before it: what the launch leaves belongs to the last pass the rollout ran.
//
// The cost of a pass is formed between two steps (search_step_cost), from the wavefront's own q, qd and applied torque us, so
// nothing of it is live across the Newton loop but the running sum J:
//     J = sum_k [ 1/2 dx_k' Q_k dx_k  +  1/2 u_k' R u_k  +  sum_{t: step_t = k} wpos/2 |r|^2 + wvel/2 |rv|^2 + wrot/4 |R - Rtarget|_F^2 ]
// in one fixed order - steps ascending; within a step the state part (the two rows id, nr + id of Q_k per lane from global memory,
// columns ascending, q block then qdot block, as k_rollout_cost; search_rows: FB_CHUNK columns in flight), the control part (the
// row id of R against the broadcast torques, one wave_sum), the terms in the caller's order (cost_front, frame_twists where a term
// of the step weighs velocity, cost_term: rmx_cost.h, reused, not restated).  Every product is an explicit fma or a lone
// multiplication.  No LDS beyond the step's own.  The map from reduced DOF to node is formed once per launch (search_node_of); per
// step the three vectors the products read are brought into reduced order by one shuffle each (search_reduced).
//
// Acceptance is wave-uniform: J is a sum of readlane results, lane 0's copy is broadcast, and the test - no solve of the pass
// diverged, ran out of iterations or met a NaN (status bits 1, 2, 4), and J < Jbar, false for a NaN - is a scalar branch.
// Plain vector stores throughout.
#pragma once
#include "rmx_cost.h"

// ubar + alpha * kff in two roundings, whatever the contraction mode of the translation unit
__device__ __forceinline__ double search_torque(const double ubar, const double alpha, const double kff) {
#pragma clang fp contract(off)
    const double step = alpha * kff;
    return ubar + step;
}

// acc1 += sum_col T[col * ld] x_col and acc2 += sum_col T[col * ld + off2] x_col over the reduced DOFs col < nr, ascending, one fused
// multiply-add each (T: the table at this lane's row): this lane's two rows of a column-major table against a vector held in REDUCED order (lane col holds
// x_col: search_reduced).  The loads of a chunk of columns are issued together and unconditionally (column clamped, the product
// selected afterwards), as rmx_feedback.h's feedback_block issues its columns - not one dependent round trip per column.  TWO false:
// one row (acc2 and off2 are not used).
template <int NP, bool TWO>
__device__ __forceinline__ void search_rows(double& acc1, double& acc2, const double* __restrict__ T, const size_t ld, const size_t off2, const int nr,
                                            const bool dof, const double xr) {
    constexpr int CH = NP < FB_CHUNK ? NP : FB_CHUNK;
#pragma unroll
    for (int b = 0; b < NP; b += CH) {
        if (b < nr) {      // (wave-uniform: the chunks past the reduced DOFs hold no column)
            double k1[CH], k2[TWO ? CH : 1];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const size_t col = (b + c) < nr ? (size_t)(b + c) : 0;
                k1[c] = T[col * ld];
                if constexpr (TWO) k2[c] = T[col * ld + off2];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const double xc = readlane_d(xr, b + c);
                if (b + c < nr) {
                    acc1 = fma(dof ? k1[c] : 0.0, xc, acc1);
                    if constexpr (TWO) acc2 = fma(dof ? k2[c] : 0.0, xc, acc2);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}
// a per-node value in reduced order: lane col takes the value of the node that carries reduced DOF col (node_of: search_node_of)
__device__ __forceinline__ double search_reduced(const double v, const int node_of) { return shfl_d(v, node_of); }
// lane col (< nr): the node whose reduced index is col.  The map does not change within a launch: formed once, ahead of the passes
__device__ __forceinline__ int search_node_of(const int id, const int nr, const int lane) {
    int node_of = 0;
    for (int col = 0; col < nr; ++col) {
        const unsigned long long mk = __ballot(id == col);
        const int cn = mk ? (int)__builtin_ctzll(mk) : 0;
        node_of = lane == col ? cn : node_of;
    }
    return node_of;
}

// the cost of the state after step `row` + 1 (q, qd) under the applied torque us; wave-uniform
template <int NP>
__device__ __forceinline__ double search_step_cost(const DevModel& M, const SearchArgs& s, const int traj, const int row, const int lane,
                                                   const int id, const int node_of, const double q, const double qd, const double us) {
    const TaskArgs& c = s.c;
    const int n = M.n, nr = M.nr, d2 = 2 * nr;
    const bool dof = id >= 0;
    const int ii = dof ? id : 0;
    double Jk = 0.0;
    if (c.Qin) {      // ---- the joint-space part: this lane holds rows id and nr + id of Q dx, the q columns then the qdot columns
        const double* Qs = c.Qin + (size_t)traj * c.q_stride + (size_t)row * d2 * d2;
        const double* xg = c.xgoal ? c.xgoal + (size_t)traj * c.goal_stride + (size_t)row * d2 : nullptr;
        const double dxq = dof ? q - (xg ? xg[ii] : 0.0) : 0.0;
        const double dxv = dof ? qd - (xg ? xg[nr + ii] : 0.0) : 0.0;
        double a1 = 0.0, a2 = 0.0;
        search_rows<NP, true>(a1, a2, Qs + ii, (size_t)d2, (size_t)nr, nr, dof, search_reduced(dxq, node_of));
        search_rows<NP, true>(a1, a2, Qs + (size_t)nr * d2 + ii, (size_t)d2, (size_t)nr, nr, dof, search_reduced(dxv, node_of));
        Jk = 0.5 * wave_sum(fma(dxv, a2, dxq * a1));
    }
    if (s.R) {      // ---- the control part: row id of R against the torques (us is zero on the lanes without a DOF)
        double ru = 0.0, none = 0.0;
        search_rows<NP, false>(ru, none, s.R + ii, (size_t)nr, 0, nr, dof, search_reduced(us, node_of));
        Jk = fma(0.5, wave_sum(us * ru), Jk);
    }
    const int tb = c.trk_begin ? c.trk_begin[row] : 0, te = c.trk_begin ? c.trk_begin[row + 1] : 0;
    if (te > tb) {      // ---- the terms of the step (wave-uniform), in the caller's order: the value lines of k_rollout_cost<NP, true>
        CostFront f;
        FrameTwist w;
        cost_front<NP>(M, lane, dof ? q : 0.0, f);
        bool vel = false;
        for (int t = tb; t < te; ++t) vel = vel || c.trk[t].wvel > 0.0;
        if (vel) frame_twists(f, n, lane, dof, dof ? qd : 0.0, w);
        for (int t = tb; t < te; ++t) {
            const rmx_track::DevTerm& T = c.trk[t].t;
            const size_t at = (size_t)traj * c.t_stride + (size_t)T.orig;
            double p[3], v[3], Jc[3], G[3];
            cost_term<true>(f, w, vel, T, lane, dof, p, v, Jc, G);
            // (a weight > 0 has its table: the host refuses the call otherwise)
            const double* xt = c.xt ? c.xt + at * 3 : nullptr;
            const double r3[3] = {p[0] - (xt ? xt[0] : 0.0), p[1] - (xt ? xt[1] : 0.0), p[2] - (xt ? xt[2] : 0.0)};
            Jk = fma(0.5 * T.wpos, cost_dot(r3, r3), Jk);
            const double wv = c.trk[t].wvel, wr = c.trk[t].wrot;
            if (wv > 0.0) {
                const double* vt = c.vt + at * 3;
                const double rv[3] = {v[0] - vt[0], v[1] - vt[1], v[2] - vt[2]};
                Jk = fma(0.5 * wv, cost_dot(rv, rv), Jk);
            }
            if (wr > 0.0) {
                const double* Rt = c.Rt + at * 9;
                double Rb[9];
                frame_rot(f, T, Rb);
                double fro = 0.0;      // |R - Rtarget|_F^2, the entries in the order of the memory
#pragma unroll
                for (int e = 0; e < 9; ++e) {
                    const double dd = Rb[3 * (e % 3) + e / 3] - Rt[e];
                    fro = fma(dd, dd, fro);
                }
                Jk = fma(0.25 * wr, fro, Jk);
            }
        }
    }
    return Jk;
}

template <int NP>
__global__ void __launch_bounds__(64) k_rollout_search(const DevModel Min, const DevOpts o, const SearchArgs s) {
    static_assert(NP <= 32, "the search exists where the Riccati sweep that feeds it exists (select_rollout_search)");
    const AdjArgs& a = s.a;
    const DevModel M = model_view<NP, false>(Min);
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const int lane = threadIdx.x, traj = blockIdx.x, n = M.n, nr = M.nr;
    const int id = (lane < n) ? M.idx[lane] : -1;
    const bool dof = id >= 0;
    const size_t off = (size_t)traj * nr + (dof ? id : 0);
    const size_t base = (size_t)traj * a.nsteps * nr + (dof ? id : 0);      // this lane's entry of row 0 of u, kff, uapp and the record
    const size_t nn = (size_t)n * n;
    const double h = o.h;
    const double Jbar = s.nalpha > 0 ? s.Jbar[traj] : 0.0;
    FrontState fs;
    const int node_of = search_node_of(id, nr, lane);
    double q = 0.0, qd = 0.0, J = 0.0, taken = 0.0;
    int iters = 0, status = 0, trials = 0;
    for (int pass = 0; pass <= s.nalpha; ++pass) {
        const bool nominal = pass == s.nalpha;      // (wave-uniform)
        const double alpha = nominal ? 0.0 : s.alphas[pass];
        q = dof ? a.q[off] : 0.0;
        qd = dof ? a.qd[off] : 0.0;
        J = 0.0;
        iters = 0;
        status = 0;
        for (int st = 1; st <= a.nsteps; ++st) {
            const size_t at = base + (size_t)(st - 1) * nr;
            double us = dof ? a.u[at] : 0.0;
            if (!nominal) {
                const double kf = dof ? s.kff[at] : 0.0;
                us = dof ? search_torque(us, alpha, kf) : 0.0;
            }
            // the ADJ_FB stage of k_adjoint_fwd: the feedback sum on the state at the start of the step, the clamp, the uapp store
            if (a.fbK) {
                const size_t row = (size_t)traj * a.fb_stride + (size_t)(st - 1);
                us = feedback_torque<NP>(us, a.fbK + row * ((size_t)2 * nr * nr), a.fbx ? a.fbx + row * ((size_t)2 * nr) : nullptr, nr, n, id, q, qd);
            }
            if (a.ulo && dof) {
                const double lo = a.ulo[id];
                us = us < lo ? lo : us;
            }
            if (a.uhi && dof) {
                const double hi = a.uhi[id];
                us = us > hi ? hi : us;
            }
            if (a.uapp && dof) a.uapp[at] = us;
            fs.tau_add = a.pscale * us;
            double* Hk = a.Hs + ((size_t)traj * a.nsteps + (st - 1)) * nn;
            double* Mk = a.Ms + ((size_t)traj * a.nsteps + (st - 1)) * nn;
            double* Dk = a.Ds + ((size_t)traj * a.nsteps + (st - 1)) * nn;
            // evalBDF1 and the Newton loop of k_adjoint_fwd (BDF1, up to 32 nodes: H rides in registers through the loop, M and D are
            // formed once behind it from the state the last evaluation left in fs)
            const double q0 = q, qd0 = qd;
            const double qA = q0, qB = q0 + h * qd0;
            double x = qB, xlo = 0.0;
            int iter = 1;
            double Hs[NP];
            while (true) {
                NodeOut e;
                double Hrow[NP];
                eval_front<NP, true>(M, sAcc, lane, x, ((x - qA) + xlo) / h, (x - qB) + xlo, h, e, fs);
                const double hdiag = eval_hess<NP>(M, lane, fs, Hrow, nullptr, sAcc);
#pragma unroll
                for (int i = 0; i < NP; ++i) Hs[i] = Hrow[i];
                ++iters;
                bool lu_ok;
                double dx = lu_solve_neg_diag<NP>(lane, Hrow, e.g, hdiag, lu_ok);
                if (!lu_ok) {
#pragma unroll
                    for (int i = 0; i < NP; ++i) Hrow[i] = Hs[i];
                    dx = lu_solve_neg<NP, true>(n, lane, Hrow, e.g);
                    status |= 16;
                }
                const double dxn2 = wave_sum(dx * dx);
                if (!(dxn2 == dxn2)) { status |= 4; break; }
                if (sqrt(dxn2) > o.dxMax) { status |= 1; break; }
                {
                    const double xa = x;
                    two_sum(xa, xlo + dx, x, xlo);
                    xlo *= o.comp;
                }
                if (sqrt(wave_sum(e.g * e.g)) < o.tol) break;
                if (iter >= o.iterMax) { status |= 2; break; }
                ++iter;
            }
            if constexpr (NP == 32 && HESS_MFMA) {
                eval_MD_mfma32_store(M, lane, fs, sAcc, Mk, Dk);
                if (lane < n) {
#pragma unroll
                    for (int i = 0; i < NP; ++i)
                        if (i < n) Hk[(size_t)i * n + lane] = Hs[i];
                }
            } else {
                double Mrow[NP], Drow[NP];
                eval_MD<NP>(M, lane, fs, Mrow, Drow);
                if (lane < n) {
#pragma unroll
                    for (int i = 0; i < NP; ++i)
                        if (i < n) {
                            Hk[(size_t)i * n + lane] = Hs[i];
                            Mk[(size_t)i * n + lane] = Mrow[i];
                            Dk[(size_t)i * n + lane] = Drow[i];
                        }
                }
            }
            qd = ((x - q0) + xlo) / h;
            q = x;
            if (dof) {      // the record: row st-1 is the state after step st
                a.qtraj[at] = q;
                a.qdtraj[at] = qd;
            }
            // the cost of the step, between two steps: steps ascending
            J += search_step_cost<NP>(M, s, traj, st - 1, lane, id, node_of, q, qd, us);
        }
        ++trials;
        if (nominal) break;
        const double Jw = readlane_d(J, 0);
        if ((status & 7) == 0 && Jw < Jbar) {      // (false for a NaN)
            taken = alpha;
            break;
        }
    }
    if (dof) {
        a.q[off] = q;
        a.qd[off] = qd;
    }
    if (lane == 0) {
        s.J[traj] = J;
        if (s.alpha) s.alpha[traj] = taken;
        if (s.trials) s.trials[traj] = trials;
        if (s.sstatus) s.sstatus[traj] = status;
        if (a.it) {
            a.it[traj] = iters;
            a.status[traj] = status;
        }
    }
}
