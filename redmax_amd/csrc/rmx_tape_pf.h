// rmx_tape_pf.h -- the taped rollouts of a model with body-to-body forces (rmx_model_tape_point_forces): the forward sweep of
// rmx_rollout_tape / _tape_bdf2 / _tape_feedback / _tape_feedback_box with the point stage of rmx_pf.h.  A kernel of its own around
// the pieces k_adjoint_fwd's TAPE instantiations are made of: those keep their instruction streams.  The tape it leaves has the
// layout of every other tape, with the forces in H and in D.
// Compiled into part_pf.hip's objects, one per padded size (the build table pins the list of objects): the 64-lane object defines
// RMX_DPP_SETTLE ahead of rmx_kernels.h there, which this kernel needs for the same reason as k_step_pf<64> - H lives in 128
// registers per lane beside the point stage, the kernel spills, and a spill reload directly in front of a row-broadcast FMA is a DPP
// read of a register that the preceding VALU instruction wrote (rmx_device.h).
#pragma once
#include "rmx_kernels.h"
#if RMX_NP == 64 && !defined(RMX_DPP_SETTLE)
#error "rmx_tape_pf.h at 64 lanes: RMX_DPP_SETTLE must be defined ahead of rmx_kernels.h"
#endif

// The step loop, the integrator stages, the feedback stage (FB: rmx_feedback.h, the clamp of the box included) and the line-search-free
// Newton loop of k_adjoint_fwd<NP, INTEG | ADJ_CTL | ADJ_TAPE (| ADJ_FB)>, one wavefront per rollout, with
//   pf_apply<NP, true> behind every eval_hess: the forces' residual enters e.g once per evaluation, their blocks this lane's row of H;
//   the guarded solve on the dense rows (pf_solve_guarded: diagonal pivots in node order, the row's scale from the updated row), a
//     tripped guard redone with partial pivoting on H as it was formed (status bit 16);
//   pf_damp added to the row of D ahead of the one store of M, D per solve.
// M, D come from eval_MD's rows in registers at every size (no matrix-core store: the block is added to the rows).  Every solve of
// the tape has a slot of its own - the SDIRK2a solve of the BDF2 tape too -, so H of the last evaluated iterate is always at hand
// where a tripped guard needs it again: up to 32 lanes a copy in registers, at 64 lanes the slot itself (H with the forces; every
// iterate is stored, the last store wins).
template <int NP, int INTEG, bool FB>
__global__ void __launch_bounds__(64) k_tape_pf(const DevModel M, const DevOpts o, const AdjArgs a, const PfTable* __restrict__ pf) {
    static_assert(INTEG == 1 || INTEG == 2, "BDF1 or BDF2");
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const PfTable& T = *pf;
    const int lane = threadIdx.x, traj = blockIdx.x, n = M.n;
    const int id = (lane < n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    double q = id >= 0 ? a.q[off] : 0.0;
    double qd = id >= 0 ? a.qd[off] : 0.0;
    double qp = 0.0, qdp = 0.0;             // BDF2: the state of step k-1
    const double* uj = a.u + (size_t)traj * a.nsteps * M.nr + (id >= 0 ? id : 0);
    const double h = o.h;
    FrontState fs;
    int iters = 0, status = 0;
    const size_t nn = (size_t)n * n;
    const int nslots = INTEG == 2 ? a.nsteps + 1 : a.nsteps;      // (BDF2: the SDIRK2a solve in slot nsteps)
    const double al = (2.0 - sqrt(2.0)) / 2.0;
    for (int s = 1; s <= a.nsteps; ++s) {
        double us = id >= 0 ? uj[(size_t)(s - 1) * M.nr] : 0.0;      // (under BDF2 step 1's torque holds for both SDIRK2 solves)
        if constexpr (FB) {                  // (q, qd: the state at the start of step s)
            if (a.fbK) {
                const size_t row = (size_t)traj * a.fb_stride + (size_t)(s - 1);
                us = feedback_torque<NP>(us, a.fbK + row * ((size_t)2 * M.nr * M.nr), a.fbx ? a.fbx + row * ((size_t)2 * M.nr) : nullptr,
                                         M.nr, n, id, q, qd);
            }
            if (a.ulo && id >= 0) {
                const double lo = a.ulo[id];
                us = us < lo ? lo : us;
            }
            if (a.uhi && id >= 0) {
                const double hi = a.uhi[id];
                us = us > hi ? hi : us;
            }
            if (a.uapp && id >= 0) a.uapp[((size_t)traj * a.nsteps + (s - 1)) * M.nr + id] = us;
        }
        fs.tau_add = a.pscale * us;
        const double q0 = (INTEG == 2 && s > 1) ? qp : q, qd0 = (INTEG == 2 && s > 1) ? qdp : qd;      // BDF2: step k-1
        const double q1 = q, qd1 = qd;                                                                  // BDF2: step k
        double qa = 0.0, qda = 0.0;                  // SDIRK2a's result
        double x = 0.0, xlo = 0.0;                   // compensated iterate x + xlo
        const int nsolve = (INTEG == 2 && s == 1) ? 2 : 1;
        for (int sv = 0; sv < nsolve; ++sv) {
            double qA, qB, eta;
            if (INTEG == 1) {
                eta = h; qA = q0; qB = q0 + h * qd0; x = qB;
            } else if (s == 1 && sv == 0) {          // SDIRK2a
                eta = al * h; qA = q0; qB = q0 + (al * h) * qd0; x = q0 + al * h * qd0;
            } else if (s == 1) {                     // SDIRK2b
                eta = al * h;
                x = qa + (1.0 - al) * h * qda;
                qA = q0 + (1.0 - al) * h * qda;
                qB = q0 + (2.0 * al - 1.0) * h * qd0 + 2.0 * (1.0 - al) * h * qda;
            } else {                                 // BDF2
                eta = (2.0 / 3.0) * h;
                x = q1 + h * qd1;
                qA = (4.0 / 3.0) * q1 - (1.0 / 3.0) * q0;
                qB = (4.0 / 3.0) * q1 - (1.0 / 3.0) * q0 + (8.0 / 9.0) * h * qd1 - (2.0 / 9.0) * h * qd0;
            }
            xlo = 0.0;
            const size_t slot = (size_t)traj * nslots + ((INTEG == 2 && s == 1 && sv == 0) ? a.nsteps : s - 1);
            double* Hk = a.Hs + slot * nn;
            double* Mk = a.Ms + slot * nn;
            double* Dk = a.Ds + slot * nn;
            int iter = 1;
            constexpr bool STORE_ONCE = NP <= 32;
            double Hs[STORE_ONCE ? NP : 1];
            while (true) {
                NodeOut e;
                double Hrow[NP];
                eval_front<NP, true>(M, sAcc, lane, x, ((x - qA) + xlo) / eta, (x - qB) + xlo, eta, e, fs);
                eval_hess<NP>(M, lane, fs, Hrow, nullptr, sAcc);
                pf_apply<NP, true>(T, fs, lane, e, Hrow);
                if constexpr (STORE_ONCE) {
#pragma unroll
                    for (int i = 0; i < NP; ++i) Hs[i] = Hrow[i];
                } else if (lane < n) {
#pragma unroll
                    for (int i = 0; i < NP; ++i)
                        if (i < n) Hk[(size_t)i * n + lane] = Hrow[i];
                }
                ++iters;
                bool lu_ok;
                double dx = pf_solve_guarded<NP>(M, lane, sAcc, Hrow, e.g, lu_ok);
                if (!lu_ok) {                // the guard tripped: H was destroyed in place
#pragma unroll
                    for (int i = 0; i < NP; ++i) {
                        if constexpr (STORE_ONCE) Hrow[i] = Hs[i];
                        else Hrow[i] = (lane < n && i < n) ? Hk[(size_t)i * n + lane] : ((i == lane) ? 1.0 : 0.0);
                    }
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
            {
                double Mrow[NP], Drow[NP];
                eval_MD<NP>(M, lane, fs, Mrow, Drow);       // fs: the state of the last evaluated iterate
                pf_damp<NP>(T, fs, lane, Drow);
                if (lane < n) {
#pragma unroll
                    for (int i = 0; i < NP; ++i)
                        if (i < n) {
                            if constexpr (STORE_ONCE) Hk[(size_t)i * n + lane] = Hs[i];
                            Mk[(size_t)i * n + lane] = Mrow[i];
                            Dk[(size_t)i * n + lane] = Drow[i];
                        }
                }
            }
            if (INTEG == 2 && s == 1 && sv == 0) {
                qa = x;
                qda = ((x - q0) + xlo) / (al * h);
            }
        }
        if (INTEG == 1) {
            qd = ((x - q0) + xlo) / h;
            q = x;
        } else if (s == 1) {
            qd = (x - q0 - (1.0 - al) * h * qda) / (al * h);
            q = x;
            qp = q0;
            qdp = qd0;
        } else {
            qd = (3.0 / (2.0 * h)) * (x - (4.0 / 3.0) * q1 + (1.0 / 3.0) * q0);
            q = x;
            qp = q1;
            qdp = qd1;
        }
        if (a.qtraj && id >= 0) {             // the record of the rollout: row s-1 is the state after step s, in the layout of u
            const size_t offs = ((size_t)traj * a.nsteps + (s - 1)) * M.nr + id;
            a.qtraj[offs] = q;
            a.qdtraj[offs] = qd;
        }
    }
    if (id >= 0) {
        a.q[off] = q;
        a.qd[off] = qd;
        if (INTEG == 2) {
            a.qp[off] = qp;
            a.qdp[off] = qdp;
        }
    }
    if (lane == 0 && a.it) {
        a.it[traj] = iters;
        a.status[traj] = status;
    }
}

// feedback: the ADJ_FB stage (rmx_rollout_tape_feedback, _feedback_box); rmx_select.h select_rollout_tape_pf chooses nothing else
void RMX_CAT(launch_tape_pf_, RMX_NP)(const rmx_model* m, const rmx_batch* b, int integ, bool feedback, const DevOpts& o, const AdjArgs& a) {
    const dim3 grid(b->B), block(64);
    const PfTable* pf = (const PfTable*)m->dpf;
    if (integ == INTEG_BDF1) {
        if (feedback) RMX_LAUNCH((k_tape_pf<RMX_NP, 1, true>), grid, block, m->smem_bytes, b->stream, m->dm, o, a, pf);
        else RMX_LAUNCH((k_tape_pf<RMX_NP, 1, false>), grid, block, m->smem_bytes, b->stream, m->dm, o, a, pf);
    } else {
        if (feedback) RMX_LAUNCH((k_tape_pf<RMX_NP, 2, true>), grid, block, m->smem_bytes, b->stream, m->dm, o, a, pf);
        else RMX_LAUNCH((k_tape_pf<RMX_NP, 2, false>), grid, block, m->smem_bytes, b->stream, m->dm, o, a, pf);
    }
}
