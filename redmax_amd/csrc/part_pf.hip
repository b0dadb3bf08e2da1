// part_pf.hip (part 9 of the former rmx_kernels.hip) -- models with body-to-body forces (rmx_model_set_point_forces): the kernels around rmx_pf.h, for ONE
// padded tree size RMX_NP (every size).
// 64 lanes: the step kernels spill (H lives in 128 registers per lane beside the point stage), and a spill reload directly in
// front of a row-broadcast FMA is a DPP read of a register that the preceding VALU instruction wrote (rmx_device.h, RMX_DPP_SETTLE)
#if RMX_NP == 64
#define RMX_DPP_SETTLE 1
#endif
#include "rmx_kernels.h"
#include "rmx_tape_pf.h"      /* k_tape_pf and its launcher: the taped rollouts of these models */
#include "rmx_force_params.h" /* k_rollout_force_grad and its launcher: the gradients in the force constants from such a tape */

// simLoop of driverRedMaxBDF1.m:57-91 (INTEG 1) / driverRedMaxBDF2.m:57-125 (INTEG 2: SDIRK2 start step, then BDF2) with the point
// forces: k_step_bdf1 / k_step_bdf2 of the plain kernels around newton_pf, all steps of a rollout in one launch.
template <int NP, int INTEG>
__global__ void __launch_bounds__(64) k_step_pf(const DevModel M, const DevOpts o, const StepArgs a, const PfTable* __restrict__ pf) {
    const unsigned long long tick0 = __builtin_amdgcn_s_memtime();
    const int traj = blockIdx.x;
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const PfTable& T = *pf;
    const int lane = threadIdx.x;
    const double h = o.h;
    const int id = (lane < M.n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    double q = id >= 0 ? a.q[off] : 0.0;
    double qd = id >= 0 ? a.qd[off] : 0.0;
    double qp = 0.0, qdp = 0.0;              // step k-1 (BDF2)
    bool started = true;
    if constexpr (INTEG == INTEG_BDF2) {
        qp = id >= 0 ? a.qp[off] : 0.0;
        qdp = id >= 0 ? a.qdp[off] : 0.0;
        started = (*a.started) != 0;
    }
    int iters = 0, halv = 0, status = 0;
    PivotPolicy piv;
    for (int s = 0; s < a.nsteps; ++s) {
        NodeOut last;
        double xlo;
        if constexpr (INTEG == INTEG_BDF1) {
            const double q0 = q, qd0 = qd;
            const double xg = q0 + h * qd0;          // initial guess (:70) and q0 + h qdot0 of dqtmp (:169)
            const double x = newton_pf<NP>(M, T, o, sAcc, lane, xg, q0, xg, h, last, iters, halv, status, piv, xlo);
            qd = ((x - q0) + xlo) / h;               // (:72), with the low-order part of the iterate the residual was evaluated at
            q = x;
        } else if (s == 0 && !started) {
            const double al = (2.0 - sqrt(2.0)) / 2.0;    // (:74)
            const double q0 = q, qd0 = qd;
            // SDIRK2a (evalSDIRK2a :194-225): eta = a h, qA = q0, qB = q0 + a h qdot0
            const double xa0 = q0 + al * h * qd0;
            const double qa = newton_pf<NP>(M, T, o, sAcc, lane, xa0, q0, q0 + (al * h) * qd0, al * h, last, iters, halv, status, piv, xlo);
            const double qda = (qa - q0) / (al * h);
            // SDIRK2b (evalSDIRK2b :228-260)
            const double x10 = qa + (1.0 - al) * h * qda;
            const double qA = q0 + (1.0 - al) * h * qda;
            const double qB = q0 + (2.0 * al - 1.0) * h * qd0 + 2.0 * (1.0 - al) * h * qda;
            const double q1 = newton_pf<NP>(M, T, o, sAcc, lane, x10, qA, qB, al * h, last, iters, halv, status, piv, xlo);
            qd = (q1 - q0 - (1.0 - al) * h * qda) / (al * h);
            q = q1;
            qp = q0;
            qdp = qd0;
        } else {
            // BDF2 (evalBDF2 :263-293): eta = 2h/3
            const double q0 = qp, qd0 = qdp, q1 = q, qd1 = qd;
            const double x0 = q1 + h * qd1;
            const double qA = (4.0 / 3.0) * q1 - (1.0 / 3.0) * q0;
            const double qB = (4.0 / 3.0) * q1 - (1.0 / 3.0) * q0 + (8.0 / 9.0) * h * qd1 - (2.0 / 9.0) * h * qd0;
            const double q2 = newton_pf<NP>(M, T, o, sAcc, lane, x0, qA, qB, (2.0 / 3.0) * h, last, iters, halv, status, piv, xlo);
            qp = q1;
            qdp = qd1;
            qd = (3.0 / (2.0 * h)) * (q2 - (4.0 / 3.0) * q1 + (1.0 / 3.0) * q0);
            q = q2;
        }
        if (a.histT) {                               // Scene.saveHistory (Scene.m:134-161)
            const double Tk = wave_sum(last.eT), Vk = wave_sum(last.eV);
            if (lane == 0) {
                a.histT[(size_t)s * a.B + traj] = Tk;
                a.histV[(size_t)s * a.B + traj] = Vk;
            }
        }
        if (a.histQ && id >= 0) {
            a.histQ[(size_t)s * a.B * M.nr + off] = q;
            a.histQd[(size_t)s * a.B * M.nr + off] = qd;
        }
    }
    if (id >= 0) {
        a.q[off] = q;
        a.qd[off] = qd;
        if constexpr (INTEG == INTEG_BDF2) {
            a.qp[off] = qp;
            a.qdp[off] = qdp;
        }
    }
    if (lane == 0 && a.it) {
        a.it[traj] += iters;
        a.ls[traj] += halv;
        a.status[traj] |= status;
    }
    if (lane == 0 && a.ticks) a.ticks[traj] += __builtin_amdgcn_s_memtime() - tick0;      // (rmx_step_ticks)
}

// Parity hook (k_eval) with the point forces.
template <int NP, bool WANT_H>
__global__ void __launch_bounds__(64) k_eval_pf(const DevModel M, const int B, const double* __restrict__ q, const double* __restrict__ qA,
                                                const double* __restrict__ qB, const double eta, double* __restrict__ g, double* __restrict__ H,
                                                const PfTable* __restrict__ pf) {
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const int lane = threadIdx.x, traj = blockIdx.x;
    const int id = (lane < M.n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    const double x = id >= 0 ? q[off] : 0.0;
    const double xa = id >= 0 ? qA[off] : 0.0;
    const double xb = id >= 0 ? qB[off] : 0.0;
    NodeOut e;
    double Hrow[NP];
    eval_node_pf<NP, WANT_H>(M, *pf, sAcc, lane, x, (x - xa) / eta, x - xb, eta, e, Hrow);
    if (id >= 0) g[off] = e.g;
    if (WANT_H) {
        double* Ht = H + (size_t)traj * M.nr * M.nr;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            if (i < M.n) {
                const int ci = M.idx[i];
                if (id >= 0 && ci >= 0) Ht[(size_t)ci * M.nr + id] = Hrow[i];   // column-major H(id, ci)
            }
        }
    }
}

// Joint / Body / Force.computeEnergy at the stored state.
template <int NP>
__global__ void __launch_bounds__(64) k_energy_pf(const DevModel M, const int B, const double* __restrict__ q, const double* __restrict__ qd,
                                                  double* __restrict__ T, double* __restrict__ V, const PfTable* __restrict__ pf) {
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const int lane = threadIdx.x, traj = blockIdx.x;
    const int id = (lane < M.n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    NodeOut e;
    double Hrow[NP];
    eval_node_pf<NP, false>(M, *pf, sAcc, lane, id >= 0 ? q[off] : 0.0, id >= 0 ? qd[off] : 0.0, 0.0, 1.0, e, Hrow);
    const double t = wave_sum(e.eT), v = wave_sum(e.eV);
    if (lane == 0) {
        T[traj] = t;
        V[traj] = v;
    }
}

void RMX_CAT(launch_eval_pf_, RMX_NP)(const rmx_model* m, const rmx_batch* b, bool wantH, double eta, double* dg, double* dH) {
    const dim3 grid(b->B), block(64);
    const PfTable* pf = (const PfTable*)m->dpf;
    if (wantH) RMX_LAUNCH((k_eval_pf<RMX_NP, true>), grid, block, m->smem_bytes, b->stream, m->dm, b->B, b->tmpA, b->tmpB, b->tmpC, eta, dg, dH, pf);
    else RMX_LAUNCH((k_eval_pf<RMX_NP, false>), grid, block, m->smem_bytes, b->stream, m->dm, b->B, b->tmpA, b->tmpB, b->tmpC, eta, dg, dH, pf);
}
void RMX_CAT(launch_step_pf_, RMX_NP)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a) {
    const dim3 grid(b->B), block(64);
    const PfTable* pf = (const PfTable*)m->dpf;
    if (integ == INTEG_BDF1) RMX_LAUNCH((k_step_pf<RMX_NP, INTEG_BDF1>), grid, block, m->smem_bytes, b->stream, m->dm, o, a, pf);
    else RMX_LAUNCH((k_step_pf<RMX_NP, INTEG_BDF2>), grid, block, m->smem_bytes, b->stream, m->dm, o, a, pf);
}
void RMX_CAT(launch_energy_pf_, RMX_NP)(const rmx_model* m, const rmx_batch* b, double* dT, double* dV) {
    const dim3 grid(b->B), block(64);
    RMX_LAUNCH((k_energy_pf<RMX_NP>), grid, block, m->smem_bytes, b->stream, m->dm, b->B, b->q, b->qd, dT, dV, (const PfTable*)m->dpf);
}
