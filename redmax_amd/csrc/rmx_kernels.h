// rmx_kernels.h -- what the kernel translation units (the part_*.hip files, one object per part and padded tree size RMX_NP: lanes
// in use per wavefront, 4, 8, 16, 32 or 64) share: the kernel templates from stage_consts to k_phase_time, and RMX_LAUNCH.  A part
// file defines the macros that make it what it is (RMX_NP, RMX_W2, RMX_SYNC, RMX_CONSTS, RMX_GLOBAL_CONSTS) AHEAD of this include;
// the multi-size parts take RMX_NP from the build (__graft_entry__.HIP_UNITS).  Device code: rmx_device.h.
#pragma once
#ifndef RMX_NP
#error "compile with -DRMX_NP=4|8|16|32|64"
#endif
#include <algorithm>
#include <cstdlib>

#include "rmx_host.h"
#include "rmx_feedback.h"

// ============================================================================ kernels



// the per-node constants in the layout the evaluation reads them in, [NCONST][cstride(NP)] (see eval_front_e2): into the wavefront's
// LDS (smem_setup) or, once per model, into a global table (k_stage_consts for the RMX_GLOBAL_CONSTS kernels)
template <int NP>
__device__ __forceinline__ void stage_consts(const DevModel& M, double* __restrict__ dst) {
    constexpr int CS = cstride(NP);
    if (threadIdx.x < CS) {       // column NP (trees padded to < 64 lanes) and the unused node slots n..NP-1: idle defaults
        const int j = threadIdx.x;
        const bool in = j < M.n;
        double* c = dst;
        for (int r = 0; r < 36; ++r) c[r * CS + j] = in ? M.K[r * MAXN + j] : ((r == 0 || r == 4 || r == 8) ? 1.0 : 0.0);   // identity
        c += 36 * CS;
        for (int r = 0; r < 6; ++r) c[r * CS + j] = in ? M.sb[r * MAXN + j] : 0.0;
        c += 6 * CS;
        for (int r = 0; r < 4; ++r) c[r * CS + j] = in ? M.I4[r * MAXN + j] : 0.0;
        c += 4 * CS;
        for (int r = 0; r < 8; ++r) c[r * CS + j] = in ? M.prm[r * MAXN + j] : 0.0;
        c += 8 * CS;
        c[j] = in ? (double)M.type[j] : 0.0;
        c += CS;
        c[j] = in ? __longlong_as_double((long long)M.rel[j]) : 0.0;
        c[CS + j] = in ? __longlong_as_double((long long)M.rel[MAXN + j]) : 0.0;
        c += 2 * CS;
        for (int r = 0; r < MAXROUNDS; ++r) c[r * CS + j] = in ? (double)M.anc[r * MAXN + j] : -1.0;
        c += MAXROUNDS * CS;
        c[j] = in ? (double)M.end[j] : (double)M.n;
        c += CS;
        for (int r = 0; r < 4; ++r) c[r * CS + j] = (in && M.con) ? M.con[r * MAXN + j] : 0.0;
    }
}

template <int NP>
__device__ __forceinline__ void smem_setup(const DevModel& M, double*& sAcc, double*& sCol) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    sAcc = smem;
    if (threadIdx.x < ACC_STRIDE) sAcc[M.n * ACC_STRIDE + threadIdx.x] = 0.0;   // zero row n (end-of-tree suffix)
#ifdef RMX_GLOBAL_CONSTS
    sCol = const_cast<double*>(M.gconst);     // read-only here: the kernels of this translation unit never switch Euler charts
#else
    sCol = smem + acc_doubles(M.n, NP);       // per-node constants, [NCONST][NP] (see eval_front_e2)
    stage_consts<NP>(M, sCol);
#endif
    __syncthreads();
}

// The contact-capable kernels: every body's own ground frame and constants (DevModel::con rows 4..13, GroundC) behind the per-node
// constants.  Ends with a barrier.
template <int NP>
__device__ __forceinline__ void con_setup(const DevModel& M, double* __restrict__ sCol) {
    constexpr int CS = cstride(NP);
    if (M.con && threadIdx.x < CS) {
        const int j = threadIdx.x;
        const bool in = j < M.n;
        for (int r = 0; r < NGROUND; ++r) sCol[(NCONST + r) * CS + j] = in ? M.con[(4 + r) * MAXN + j] : 0.0;
    }
    __syncthreads();
}

template <int NP>
__global__ void __launch_bounds__(64) k_stage_consts(const DevModel M, double* __restrict__ dst) {
    stage_consts<NP>(M, dst);
}

// simLoop (driverRedMaxBDF1.m:57-91): all steps of one trajectory inside one wavefront.
// Contact-capable scenes (CT) take two launches per call.  LEAN: the plain evaluation plus the test that every cuboid is clear of
// the ground; a trajectory that fails it stops at the start of that step and leaves the step index in a.resume.  The second
// launch (CT, not LEAN: the evaluation with the contact terms) takes every trajectory from its a.resume to the end.  In one
// kernel the contact terms' registers (72 accumulators for the K/D blocks on top of the Hessian stage's state) put the whole
// Newton loop into scratch - 34 us per iteration in free flight against 12 us for the plain kernel (tools/ct_overhead.py) -
// and an out-of-line call of the contact solve tripled ITS cost (the model constants arrive as a pointer into scratch).
// FULLCHAIN: an instantiation for serial chains that fill every node slot (is_chain && n == NP, decided by the launcher): the two
// model facts are compile-time constants there, so the tree paths (pointer jumping, relation masks, subtree ranges) and the
// per-row bounds of partly filled sizes are not even compiled in - fewer live masks, a smaller loop body.
// TAG >= TAG_FULLN: a tree (not necessarily a chain) that fills every node slot: n == NP at compile time, so the per-row bounds of partly
// filled sizes go (the 64-joint tree of BASELINE.json configs[2]).
constexpr int TAG_FULLN = 4;
constexpr int TAG_COOP = 8;      // k_step_bdf1/2<32, true, false, false, TAG_COOP>: the cooperative launch (part_ground32.hip)
constexpr int TAG_W2 = 16;       // k_step_bdf1/2<64, false, false, false, TAG_W2>: two wavefronts per 64-node tree (part_w2_tree64.hip, RMX_W2);
                                 // TAG_W2 + 1: the same for trees of 33..63 nodes (n at run time)
constexpr int TAG_W2_NOE = TAG_W2 + 2;      // TAG_W2 for a call that records no energies (the benchmark's launch): the energies of the last
                                             // evaluation are neither copied per Newton iteration nor summed by the helper wave
constexpr bool tag_w2(const int tag) { return tag == TAG_W2 || tag == TAG_W2 + 1 || tag == TAG_W2_NOE; }
constexpr bool tag_w2_full(const int tag) { return tag == TAG_W2 || tag == TAG_W2_NOE; }
template <int NP, bool FULLCHAIN, int TAG = 0>
__device__ __forceinline__ DevModel model_view(const DevModel& Min) {
    DevModel M = Min;
    if constexpr (FULLCHAIN) {
        M.n = NP;
        M.is_chain = 1;
    }
    if constexpr ((TAG >= TAG_FULLN && TAG < TAG_COOP) || tag_w2_full(TAG)) M.n = NP;
    return M;
}

template <int NP>
__device__ __forceinline__ double* w2_help_area(const DevModel& M, double* sAcc) {      // (W2_HELP_*: behind the per-node constants)
    return const_cast<double*>(static_cast<const double*>(RMX_CONSTS(sAcc, M.n, NP))) + (NCONST + NGROUND) * cstride(NP);
}
// RMX_W2: wave 1 of a two-wave workgroup.  It serves wave 0's guarded Newton iterations - the odd columns of the Hessian tiles, its
// share of the block-column elimination - and sleeps at the workgroup barrier in between (eval_hess and lu_solve_neg_diag64_staged
// hold wave 0's side of the same barriers).
template <int NP, bool ENERGY = true>
__device__ __forceinline__ void w2_helper(const DevModel& M, double* __restrict__ sAcc, const int lane) {
    if constexpr (NP == 64 && RMX_W2) {
        constexpr int CS = cstride(NP);
        const double* cRel = RMX_CONSTS(sAcc, M.n, NP) + (36 + 6 + 4 + 8 + 1) * CS;
        double* const hp = w2_help_area<NP>(M, sAcc);
        if (lane < W2_HELP_AS) hp[M.n * W2_HELP_AS + lane] = 0.0;                    // (row n of an accumulation scratch stays zero)
        for (;;) {
            RMX_WG_BAR();
            const int cmd = *w2_cmd();
            if (cmd == 0) break;
            if (cmd == 2) {       // an evaluation that may end wave 0's solve: residual and energies only, on this wave's scratch
                const double x = hp[W2_HELP_ARGS + lane], xqd = hp[W2_HELP_ARGS + 64 + lane], xv = hp[W2_HELP_ARGS + 128 + lane];
                const double eta = hp[W2_HELP_ARGS + 192];
                NodeOut e;
                FrontState f2;
                eval_front_e2<NP, false, false, false, false, W2_HELP_AS>(M, hp, lane, x, xqd, xv, eta, eta * eta, e, f2);
                const double gn2 = wave_sum_np<NP>(e.g * e.g);
                double T = 0.0, V = 0.0;
                if constexpr (ENERGY) {
                    T = wave_sum(e.eT);
                    V = wave_sum(e.eV);
                }
                if (lane == 0) {
                    hp[W2_HELP_RES] = gn2;
                    hp[W2_HELP_RES + 1] = T;
                    hp[W2_HELP_RES + 2] = V;
                }
                RMX_WG_BAR();
                continue;
            }
            double h1[4][2][4];
            hess64_tiles<NP, 1>(lane, sAcc, cRel, h1);
            RMX_WG_BAR();
            w2_store_half<1>(sAcc, lane, h1);
            RMX_WG_BAR();
#if RMX_W2
            if (M.tree_dmax == 0) (void)w2_lu_call();      // (a branching tree's solve runs along the tree, on wave 0 alone: tree_solve64)
#endif
        }
    }
}
// RMX_W2, chains of <= 32 nodes (part_w2_chain32.hip): the helper wave only evaluates - the point wave 0 posts, with the FULL front (see W2C_HELP_*)
template <int NP>
__device__ __forceinline__ void w2c_helper(const DevModel& M, double* __restrict__ sAcc, const int lane) {
    if constexpr (NP == 32 && RMX_W2) {
        double* const hp = w2_help_area<NP>(M, sAcc);
        if (lane < ACC_STRIDE) hp[M.n * ACC_STRIDE + lane] = 0.0;                    // (row n of an accumulation scratch stays zero)
        for (;;) {
            RMX_WG_BAR();
            if (*w2_cmd() == 0) break;
            const double x = hp[W2C_HELP_ARGS + lane], xqd = hp[W2C_HELP_ARGS + 64 + lane], xv = hp[W2C_HELP_ARGS + 128 + lane];
            const double eta = hp[W2C_HELP_ARGS + 192];
            NodeOut e;
            FrontState f2;
            eval_front_e2<NP, true, false, false, false>(M, hp, lane, x, xqd, xv, eta, eta * eta, e, f2);
            const double gn2 = wave_sum_np<NP>(e.g * e.g), T = wave_sum(e.eT), V = wave_sum(e.eV);
            if (lane == 0) {
                hp[W2C_HELP_RES] = gn2;
                hp[W2C_HELP_RES + 1] = T;
                hp[W2C_HELP_RES + 2] = V;
            }
            RMX_WG_BAR();
        }
    }
}

#if RMX_W2
// BDF1 steps s, s + 1, ... of a tree under the guarded Newton (driverRedMaxBDF1.m:57-157), ONE loop around one call site of the front:
// newton_rot<NP, false> and the step epilogue of k_step_bdf1, decision for decision and operation for operation, plus this.  The
// evaluation that ENDS a solve (the accepted line-search trial whose |g| is below tol) is followed by the first evaluation of the NEXT
// step, at a point that depends on the converged iterate alone - known before that last evaluation is run.  When the current Newton
// iteration is the one the previous solve ended at, wave 0 hands the trial point to the helper wave (w2_helper, command 2: a
// residual-only front on a scratch of its own - the same operations, so the same residual) and evaluates the next step's first point
// itself; if the helper's |g|^2 ends the solve, the epilogue of the step runs here and the loop goes on as the next step's solve with
// its first evaluation done; if not, the trial point is evaluated after all (the prediction cost one evaluation).  Returns the number
// of steps finished (>= 1); ends at the first solve that ends on an evaluation of its own.
template <int NP, bool ENERGY = true>
__device__ __forceinline__ int w2_steps_bdf1(const DevModel& M, const DevOpts& o, const StepArgs& a, double* sAcc, const int lane,
                                             const int traj, const int id, const size_t off, int s, double& q, double& qd, int& iters,
                                             int& halvings, int& status, PivotPolicy& piv, int& predict) {
    double Hrow[NP];
    FrontState fs;
    NodeOut e, e0, last;
    double q0 = q;
    double x = q0 + o.h * qd;                    // initial guess (:70) and q0 + h qdot0 of dqtmp (:169)
    double qA = q0, qB = x;
    const double eta = o.h;
    double lo = 0.0, dx = 0.0, alpha = 1.0, f0 = 0.0, g0n2 = 0.0, x0 = x, lo0 = 0.0;
    int iter = 1, lsfail = 0, iterLs = 1, done = 0;
    bool ls = false, spec_failed = false;
    e0.g = e0.eT = e0.eV = 0.0;
    last = e0;
    double* const hp = w2_help_area<NP>(M, sAcc);
    constexpr int HARGS = NP == 64 ? W2_HELP_ARGS : W2C_HELP_ARGS, HRES = NP == 64 ? W2_HELP_RES : W2C_HELP_RES;
    // the epilogue of step s (k_step_bdf1): qdot (:72), q, Scene.saveHistory; T, V: the sums of the last evaluation's energies
    auto finish = [&](const double T, const double V) {
        qd = ((x - q0) + lo) / o.h;
        q = x;
        if (ENERGY && a.histT && lane == 0) {
            a.histT[(size_t)s * a.B + traj] = T;
            a.histV[(size_t)s * a.B + traj] = V;
        }
        if (a.histQ && id >= 0) {
            a.histQ[(size_t)s * a.B * M.nr + off] = q;
            a.histQd[(size_t)s * a.B * M.nr + off] = qd;
        }
        ++s;
        ++done;
    };
    while (true) {
        const bool spec = !spec_failed && ls && iter == predict && piv.streak == 0 && s + 1 < a.nsteps && !a.w2_noahead;      // (wave-uniform)
        // (the run-ahead swaps the next step's point INTO x, lo, qA, qB: the expressions handed to the front stay newton_rot's)
        const double sx = x, slo = lo, sqA = qA, sqB = qB;
        if (spec) {
            hp[HARGS + lane] = x;
            hp[HARGS + 64 + lane] = ((x - qA) + lo) / eta;
            hp[HARGS + 128 + lane] = (x - qB) + lo;
            if (lane == 0) {
                hp[HARGS + 192] = eta;
                *w2_cmd() = 2;
            }
            RMX_WG_BAR();
            const double qn = x, qdn = ((x - q0) + lo) / o.h;      // q, qdot as `finish` forms them
            x = qn + o.h * qdn;
            lo = 0.0;
            qA = qn;
            qB = x;
        }
        eval_front<NP, true, false, false, false>(M, sAcc, lane, x, ((x - qA) + lo) / eta, (x - qB) + lo, eta, e, fs);
        if (spec) {
            RMX_WG_BAR();
            const double gh = hp[HRES], Th = hp[HRES + 1], Vh = hp[HRES + 2];
            const double nx = x;
            x = sx; lo = slo; qA = sqA; qB = sqB;
            if (!((0.5 * gh < f0 || !(iterLs < o.iterLsMax)) && sqrt(gh) < o.tol)) {
                spec_failed = true;              // not the end of this solve: the trial point is evaluated here after all
                continue;
            }
            // the solve of step s ends at x (newton_rot: halvings, pivot policy; then the step's epilogue) ...
            halvings += iterLs - 1;
            predict = iter;
            pivot_policy_update(piv);
            finish(Th, Vh);
            // ... and this is the solve of the next step after its first evaluation
            q0 = q;
            x = nx;
            qA = q0;
            qB = x;
            lo = 0.0; dx = 0.0; alpha = 1.0; f0 = 0.0; g0n2 = 0.0; x0 = x; lo0 = 0.0;
            iter = 1; lsfail = 0; iterLs = 1;
            ls = false;
        }
        spec_failed = false;
        const double gn2 = wave_sum_np<NP>(e.g * e.g);
        if (ls) {                                        // this was a trial point of the line search (:124-138)
            if (!(0.5 * gn2 < f0) && iterLs < o.iterLsMax) {
                alpha *= 0.5;
                ++iterLs;
                two_sum(x0, fma(alpha, dx, lo0), x, lo);
                lo *= o.comp;
                if (__all(x == x0 && lo == lo0)) {        // see newton_impl: every further halving re-evaluates g(x0)
                    if constexpr (ENERGY) last = e0;
                    halvings += o.iterLsMax - 1;
                    if (!(sqrt(g0n2) < o.tol)) status |= 2 | 8;
                    break;
                }
                continue;
            }
            if constexpr (ENERGY) last = e;
            halvings += iterLs - 1;
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
        (void)eval_hess<NP, false, false, false>(M, lane, fs, Hrow, nullptr, sAcc, e.g);
        if constexpr (ENERGY) {
            e0 = e;
            last = e;
        }
        ++iters;
        {
            bool lu_ok;
            if constexpr (NP == 64) {
                if (M.tree_dmax > 0) {   // (a branching tree: along the tree, this wave alone - w2_helper skips the solve)
                    dx = tree_solve64(M, lane, sAcc, lu_ok);
                } else {
                    const W2Lu r = w2_lu_call();
                    dx = r.dx;
                    lu_ok = r.ok != 0;
                }
                RMX_SYNC();             // sAcc goes back to the front, whose subtree scan relies on a zero row n
                if (lane < ACC_STRIDE) sAcc[M.n * ACC_STRIDE + lane] = 0.0;
                RMX_SYNC();
            } else {
                static_assert(NP == 64 || (NP == 32 && LU_SPLIT32), "the sizes newton_rot solves from the staging area");
                dx = lu_solve_neg_diag32(M.n, lane, sAcc, e.g, lu_ok);
            }
            if (lu_ok) {
                piv.streak = 0;
            } else {             // growth guard tripped: redo this solve with partial pivoting (see newton_impl)
                ++piv.streak;
                status |= 16;
                NodeOut e2;
                eval_front<NP, true, false, false, false>(M, sAcc, lane, x, ((x - qA) + lo) / eta, (x - qB) + lo, eta, e2, fs);
                eval_hess<NP, false, false>(M, lane, fs, Hrow, nullptr, sAcc);
                dx = lu_solve_neg<NP>(M.n, lane, Hrow, e.g);
            }
        }
        const double dxn2 = wave_sum_np<NP>(dx * dx);
        if (!(dxn2 == dxn2)) {
            status |= 4;
            break;
        }
        if (sqrt(dxn2) > o.dxMax) {
            status |= 1;
            break;
        }
        alpha = 1.0;
        g0n2 = gn2;
        f0 = 0.5 * g0n2;
        x0 = x;
        lo0 = lo;
        iterLs = 1;
        two_sum(x0, fma(alpha, dx, lo0), x, lo);
        lo *= o.comp;
        if (__all(x == x0 && lo == lo0)) {
            if constexpr (ENERGY) last = e0;
            halvings += o.iterLsMax - 1;
            if (!(sqrt(g0n2) < o.tol)) status |= 2 | 8;
            break;
        }
        ls = true;
    }
    // a solve that ended on an evaluation of its own
    predict = iter;
    pivot_policy_update(piv);
    if constexpr (ENERGY) finish(wave_sum(last.eT), wave_sum(last.eV));
    else finish(0.0, 0.0);
    return done;
}
#endif

__device__ __forceinline__ void w2_release(const int lane) {
    if (lane == 0) *w2_cmd() = 0;
    RMX_WG_BAR();
}

// TAG: keeps the kernel names of a translation unit compiled with other macros (RMX_GLOBAL_CONSTS) distinct (0, 3); TAG_FULLN, TAG_FULLN + 1:
// the n == NP instantiations of the two
template <int NP, bool CT, bool LEAN = false, bool FULLCHAIN = false, int TAG = 0>
__global__ void __launch_bounds__(tag_w2(TAG) ? 128 : 64) k_step_bdf1(const DevModel Min, const DevOpts o, const StepArgs a) {
    static_assert(!LEAN || CT, "the lean launch belongs to the contact-capable kernels");
    constexpr bool COOP = TAG == TAG_COOP;           // the cooperative launch (rmx_device.h CoopCtx): COOP_G workgroups per parked rollout
    static_assert(!COOP || (CT && !LEAN), "the cooperative launch belongs to the kernels with the contact terms");
    constexpr bool PARKS = CT && !LEAN && !COOP;     // the launch with the contact terms may park a rollout for the cooperative one
    const DevModel M = model_view<NP, FULLCHAIN, TAG>(Min);
    unsigned long long tick0 = __builtin_amdgcn_s_memtime();
    int traj = blockIdx.x;
    CoopCtx cx;
    cx.ticks = o.coopTicks;
    int pk = 0, npark = 1, pstride = 1;
    if constexpr (COOP) {
        pk = blockIdx.x / COOP_G;
        cx.member = blockIdx.x % COOP_G;
        cx.words = a.xch + (size_t)pk * COOP_WORDS;
        npark = a.park[0];
        pstride = a.ngroups;
        if (pk >= npark) return;
        traj = a.park[1 + pk];
    }
    const int s0 = (CT && !LEAN && a.resume) ? a.resume[traj] : 0;
    if (!COOP && s0 >= a.nsteps) return;           // the lean launch took this trajectory all the way
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const int lane = threadIdx.x;
    if constexpr (tag_w2(TAG)) {
        if (threadIdx.x >= 64) {
            if constexpr (NP == 64) w2_helper<NP, TAG != TAG_W2_NOE>(M, sAcc, lane - 64);
            else w2c_helper<NP>(M, sAcc, lane - 64);
            return;
        }
    }
    int* const chart0 = (CT && M.nsph) ? a.chart : nullptr;
    if constexpr (CT) con_setup<NP>(M, sCol);
    const bool writer = !COOP || cx.member == 0;     // (members 1.. of a cooperative group compute, member 0 also stores)
    for (; pk < npark; pk += pstride) {              // (one pass unless COOP: group g finishes parked rollouts g, g + ngroups, ...)
    int sfirst = s0;
    if constexpr (COOP) {
        traj = a.park[1 + pk];
        sfirst = a.resume[traj];
        tick0 = __builtin_amdgcn_s_memtime();
    }
    const int id = (lane < M.n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    double q = id >= 0 ? a.q[off] : 0.0;
    double qd = id >= 0 ? a.qd[off] : 0.0;
    int iters = 0, halv = 0, status = 0;
    PivotPolicy piv;
    if constexpr (COOP) {
        const int* pp = a.park + 1 + a.B + 3 * traj;
        piv.hold = pp[0]; piv.len = pp[1]; piv.streak = pp[2];
    }
    int* const chart = chart0 ? chart0 + (size_t)traj * M.nsph : nullptr;
    if constexpr (CT) {
        if (M.nsph) sph_setup<NP>(M, sCol, lane, chart);
    }
    int stop = a.nsteps;
#if RMX_W2
    int w2_predict = 0;                            // (w2_steps_bdf1: the Newton iteration the last solve ended at)
#endif
    for (int s = sfirst; s < a.nsteps; ++s) {
#if RMX_W2
        if constexpr (tag_w2(TAG) && (!FULLCHAIN || NP == 32)) {
            // guarded solves of a tree: the loop that runs ahead into the next step (w2_steps_bdf1); pivoting solves and the 64-lane serial
            // chains (whose residual-only front sums by another scan) keep newton_node.  NP == 32: the chains of part_w2_chain32.hip, whose helper
            // runs the full front
            if ((NP == 32 || !M.is_chain) && o.lu_mode == 0 && piv.hold == 0) {
                s += w2_steps_bdf1<NP, TAG != TAG_W2_NOE>(M, o, a, sAcc, lane, traj, id, off, s, q, qd, iters, halv, status, piv, w2_predict) - 1;
                continue;
            }
        }
#endif
        const double q0 = q, qd0 = qd;
        const double xg = q0 + o.h * qd0;          // initial guess (:70) and q0 + h qdot0 of dqtmp (:169)
        NodeOut last;
        double xlo;
        const int it_in = iters, hv_in = halv, st_in = status;
        const PivotPolicy piv_in = piv;
#if RMX_W2
        // (a full tree gets here for its pivoting solves only - newton_policy's first branch: the guarded loop is w2_steps_bdf1)
        double x;
        if constexpr (tag_w2_full(TAG) && (!FULLCHAIN || NP == 32)) {
            if (piv.hold > 0) --piv.hold;
            xlo = 0.0;
            x = newton_rot<NP, true>(M, o, sAcc, sCol, lane, xg, q0, xg, o.h, last, iters, halv, status, piv, xlo);
        } else {
            x = newton_node<NP, CT, LEAN, COOP>(M, o, sAcc, sCol, lane, xg, q0, xg, o.h, last, iters, halv, status, piv, xlo, cx);
        }
#else
        const double x = newton_node<NP, CT, LEAN, COOP>(M, o, sAcc, sCol, lane, xg, q0, xg, o.h, last, iters, halv, status, piv, xlo, cx);
#endif
        if (LEAN && (status & ST_LEFT_LEAN)) {
            status &= ~ST_LEFT_LEAN;
            stop = s;
            break;
        }
        if (PARKS && (status & ST_PARK)) {         // this step goes to the cooperative launch, from its start: nothing of it is kept
            iters = it_in; halv = hv_in; status = st_in; piv = piv_in;
            stop = s;
            break;
        }
        if (COOP && (status & ST_COOP_FAULT)) break;
        qd = ((x - q0) + xlo) / o.h;               // (:72), with the low-order part of the iterate the residual was evaluated at
        q = x;
        if constexpr (CT) {                        // jroot.reparam() (:78)
            double np0 = 0.0, np1 = 0.0;
            if (M.nsph && sph_reparam<NP, false>(M, sCol, lane, chart, q, qd, np0, np1)) status |= 32;
        }
        if (a.histT && writer) {                   // Scene.saveHistory (Scene.m:134-161)
            const double T = wave_sum(last.eT), V = wave_sum(last.eV);
            if (lane == 0) {
                a.histT[(size_t)s * a.B + traj] = T;
                a.histV[(size_t)s * a.B + traj] = V;
            }
        }
        if (a.histQ && id >= 0 && writer) {
            a.histQ[(size_t)s * a.B * M.nr + off] = q;
            a.histQd[(size_t)s * a.B * M.nr + off] = qd;
        }
        if constexpr (CT) {
            if (a.histC && lane < M.nsph && writer) a.histC[((size_t)s * a.B + traj) * M.nsph + lane] = chart[lane];
        }
    }
    if (id >= 0 && writer) {
        a.q[off] = q;
        a.qd[off] = qd;
    }
    if (LEAN && lane == 0) a.resume[traj] = stop;
    if constexpr (PARKS) {
        if (a.park && lane == 0) {
            a.resume[traj] = stop;
            if (stop < a.nsteps) {
                a.park[1 + atomicAdd(a.park, 1)] = traj;
                int* pp = a.park + 1 + a.B + 3 * traj;
                pp[0] = piv.hold; pp[1] = piv.len; pp[2] = piv.streak;
            }
        }
    }
    if (lane == 0 && a.it && writer) {
        a.it[traj] += iters;
        a.ls[traj] += halv;
        a.status[traj] |= status;
    }
    if (lane == 0 && a.ticks && writer) a.ticks[traj] += __builtin_amdgcn_s_memtime() - tick0;      // this rollout's share of the launch (rmx_step_ticks)
    }
    if constexpr (tag_w2(TAG)) w2_release(lane);
}

// simLoop (driverRedMaxBDF2.m:57-125): SDIRK2 start step (two Newton solves), then BDF2.  CT / LEAN: see k_step_bdf1.
template <int NP, bool CT, bool LEAN = false, bool FULLCHAIN = false, int TAG = 0>
__global__ void __launch_bounds__(tag_w2(TAG) ? 128 : 64) k_step_bdf2(const DevModel Min, const DevOpts o, const StepArgs a) {
    static_assert(!LEAN || CT, "the lean launch belongs to the contact-capable kernels");
    constexpr bool COOP = TAG == TAG_COOP;           // see k_step_bdf1
    static_assert(!COOP || (CT && !LEAN), "the cooperative launch belongs to the kernels with the contact terms");
    constexpr bool PARKS = CT && !LEAN && !COOP;
    const DevModel M = model_view<NP, FULLCHAIN, TAG>(Min);
    unsigned long long tick0 = __builtin_amdgcn_s_memtime();
    int traj = blockIdx.x;
    CoopCtx cx;
    cx.ticks = o.coopTicks;
    int pk = 0, npark = 1, pstride = 1;
    if constexpr (COOP) {
        pk = blockIdx.x / COOP_G;
        cx.member = blockIdx.x % COOP_G;
        cx.words = a.xch + (size_t)pk * COOP_WORDS;
        npark = a.park[0];
        pstride = a.ngroups;
        if (pk >= npark) return;
        traj = a.park[1 + pk];
    }
    const int s0 = (CT && !LEAN && a.resume) ? a.resume[traj] : 0;
    if (!COOP && s0 >= a.nsteps) return;
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const int lane = threadIdx.x;
    if constexpr (tag_w2(TAG)) {
        if (threadIdx.x >= 64) {
            if constexpr (NP == 64) w2_helper<NP>(M, sAcc, lane - 64);
            else w2c_helper<NP>(M, sAcc, lane - 64);
            return;
        }
    }
    int* const chart0 = (CT && M.nsph) ? a.chart : nullptr;
    if constexpr (CT) con_setup<NP>(M, sCol);
    const bool writer = !COOP || cx.member == 0;
    const double h = o.h;
    for (; pk < npark; pk += pstride) {              // (one pass unless COOP)
    int sfirst = s0;
    if constexpr (COOP) {
        traj = a.park[1 + pk];
        sfirst = a.resume[traj];
        tick0 = __builtin_amdgcn_s_memtime();
    }
    const int id = (lane < M.n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    double q = id >= 0 ? a.q[off] : 0.0;
    double qd = id >= 0 ? a.qd[off] : 0.0;
    double qp = id >= 0 ? a.qp[off] : 0.0;       // step k-1 (Joint.q1 / qdot1 in the reference)
    double qdp = id >= 0 ? a.qdp[off] : 0.0;
    const bool started = (*a.started) != 0 || sfirst > 0;    // resumed behind the lean launch: its steps are this call's history
    int iters = 0, halv = 0, status = 0;
    PivotPolicy piv;
    if constexpr (COOP) {
        const int* pp = a.park + 1 + a.B + 3 * traj;
        piv.hold = pp[0]; piv.len = pp[1]; piv.streak = pp[2];
    }
    int* const chart = chart0 ? chart0 + (size_t)traj * M.nsph : nullptr;
    if constexpr (CT) {
        if (M.nsph) sph_setup<NP>(M, sCol, lane, chart);
    }
    int stop = a.nsteps;
    for (int s = sfirst; s < a.nsteps; ++s) {
        NodeOut last;
        double xlo;       // low-order part of the converged iterate: below the rounding of the multistep velocity formulas, not used
        const int it_in = iters, hv_in = halv, st_in = status;
        const PivotPolicy piv_in = piv;
        bool left = false;                         // the step was given up to the next launch (lean -> contact terms -> cooperative)
        if (s == 0 && !started) {
            const double al = (2.0 - sqrt(2.0)) / 2.0;    // (:74)
            const double q0 = q, qd0 = qd;
            // SDIRK2a (evalSDIRK2a :194-225): eta = a h, qA = q0, qB = q0 + a h qdot0
            const double xa0 = q0 + al * h * qd0;
            const double qa = newton_node<NP, CT, LEAN, COOP>(M, o, sAcc, sCol, lane, xa0, q0, q0 + (al * h) * qd0, al * h, last, iters, halv, status, piv, xlo, cx);
            left = (LEAN && (status & ST_LEFT_LEAN)) || (PARKS && (status & ST_PARK)) || (COOP && (status & ST_COOP_FAULT));
            if (!left) {
                const double qda = (qa - q0) / (al * h);
                // SDIRK2b (evalSDIRK2b :228-260)
                const double x10 = qa + (1.0 - al) * h * qda;
                const double qA = q0 + (1.0 - al) * h * qda;
                const double qB = q0 + (2.0 * al - 1.0) * h * qd0 + 2.0 * (1.0 - al) * h * qda;
                const double q1 = newton_node<NP, CT, LEAN, COOP>(M, o, sAcc, sCol, lane, x10, qA, qB, al * h, last, iters, halv, status, piv, xlo, cx);
                left = (LEAN && (status & ST_LEFT_LEAN)) || (PARKS && (status & ST_PARK)) || (COOP && (status & ST_COOP_FAULT));
                if (!left) {
                    qd = (q1 - q0 - (1.0 - al) * h * qda) / (al * h);
                    q = q1;
                    qp = q0;
                    qdp = qd0;
                }
            }
        } else {
            // BDF2 (evalBDF2 :263-293): eta = 2h/3
            const double q0 = qp, qd0 = qdp, q1 = q, qd1 = qd;
            const double x0 = q1 + h * qd1;
            const double qA = (4.0 / 3.0) * q1 - (1.0 / 3.0) * q0;
            const double qB = (4.0 / 3.0) * q1 - (1.0 / 3.0) * q0 + (8.0 / 9.0) * h * qd1 - (2.0 / 9.0) * h * qd0;
            const double q2 = newton_node<NP, CT, LEAN, COOP>(M, o, sAcc, sCol, lane, x0, qA, qB, (2.0 / 3.0) * h, last, iters, halv, status, piv, xlo, cx);
            left = (LEAN && (status & ST_LEFT_LEAN)) || (PARKS && (status & ST_PARK)) || (COOP && (status & ST_COOP_FAULT));
            if (!left) {
                qp = q1;
                qdp = qd1;
                qd = (3.0 / (2.0 * h)) * (q2 - (4.0 / 3.0) * q1 + (1.0 / 3.0) * q0);
                q = q2;
                // the Newton residual was evaluated with qdot = (q2-qA)/eta, identical up to rounding
            }
        }
        if (left) {
            if (COOP) break;                       // (ST_COOP_FAULT stays in the status)
            // nothing of this step is kept: the next launch takes it from its start (a solve of the start step that went through included)
            iters = it_in; halv = hv_in; status = st_in; piv = piv_in;
            stop = s;
            break;
        }
        if constexpr (CT) {                        // jroot.reparam() (:112): q, qdot and the previous step's q1, qdot1
            if (M.nsph && sph_reparam<NP, true>(M, sCol, lane, chart, q, qd, qp, qdp)) status |= 32;
        }
        if (a.histT && writer) {
            const double T = wave_sum(last.eT), V = wave_sum(last.eV);
            if (lane == 0) {
                a.histT[(size_t)s * a.B + traj] = T;
                a.histV[(size_t)s * a.B + traj] = V;
            }
        }
        if (a.histQ && id >= 0 && writer) {
            a.histQ[(size_t)s * a.B * M.nr + off] = q;
            a.histQd[(size_t)s * a.B * M.nr + off] = qd;
        }
        if constexpr (CT) {
            if (a.histC && lane < M.nsph && writer) a.histC[((size_t)s * a.B + traj) * M.nsph + lane] = chart[lane];
        }
    }
    if (id >= 0 && writer) {
        a.q[off] = q;
        a.qd[off] = qd;
        a.qp[off] = qp;
        a.qdp[off] = qdp;
    }
    if (LEAN && lane == 0) a.resume[traj] = stop;
    if constexpr (PARKS) {
        if (a.park && lane == 0) {
            a.resume[traj] = stop;
            if (stop < a.nsteps) {
                a.park[1 + atomicAdd(a.park, 1)] = traj;
                int* pp = a.park + 1 + a.B + 3 * traj;
                pp[0] = piv.hold; pp[1] = piv.len; pp[2] = piv.streak;
            }
        }
    }
    if (lane == 0 && a.it && writer) {
        a.it[traj] += iters;
        a.ls[traj] += halv;
        a.status[traj] |= status;
    }
    if (lane == 0 && a.ticks && writer) a.ticks[traj] += __builtin_amdgcn_s_memtime() - tick0;      // this rollout's share of the launch (rmx_step_ticks)
    }
    if constexpr (tag_w2(TAG)) w2_release(lane);
}

// euler (matlab-simple/testRedMax.m:67-109), BASELINE.json configs[0]: linearly-implicit Euler,
//   Mr = J'MmJ ; (Mr + h Dr - h^2 Kr) qdot1 = Mr qdot0 + h (J'(fm - Mm Jdot qdot0) + fr) ; q1 = q0 + h qdot1
// with the same front as the implicit integrators: the right-hand side is g(v = qdot0, e2 = -h) plus h*damping*qdot0
// (matlab-simple drops the joint damping FORCE, testRedMax.m:84), the matrix is eval_mass + the joint diagonals.
template <int NP>
__global__ void __launch_bounds__(64) k_step_euler(const DevModel M, const double h, const StepArgs a) {
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const int lane = threadIdx.x, traj = blockIdx.x;
    const int id = (lane < M.n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    double q = id >= 0 ? a.q[off] : 0.0;
    double qd = id >= 0 ? a.qd[off] : 0.0;
    for (int s = 0; s < a.nsteps; ++s) {
        FrontState fs;
        NodeOut e;
        double Mrow[NP];
        eval_front_e2<NP, true>(M, sAcc, lane, q, qd, qd, 0.0, -h, e, fs);
        eval_mass<NP>(M, lane, fs, Mrow);
        const double rhs = e.g + h * fs.dd * qd;
#pragma unroll
        for (int i = 0; i < NP; ++i)
            if (i == lane && fs.dof) Mrow[i] += h * fs.dd + h * h * fs.kd;
        const double qd1 = lu_solve_neg<NP, true>(M.n, lane, Mrow, -rhs);
        q = q + h * qd1;
        qd = qd1;
        if (a.histT) {
            eval_front<NP, false>(M, sAcc, lane, q, qd, 0.0, 1.0, e, fs);
            const double T = wave_sum(e.eT), V = wave_sum(e.eV);
            if (lane == 0) {
                a.histT[(size_t)s * a.B + traj] = T;
                a.histV[(size_t)s * a.B + traj] = V;
            }
        }
    }
    if (id >= 0) {
        a.q[off] = q;
        a.qd[off] = qd;
    }
}

// ---------------------------------------------------------------- adjoint BDF1 / BDF2 (BASELINE.json configs[3])
//
// taskObjective of driverRedMaxAdjointBDF1.m:39-62 (TaskBDF1PointPos) and driverRedMaxAdjointBDF2.m:38-62 (TaskBDF2PointPos), batched:
// parameters p[B][nr] are constant joint torques tau = pscale*p (applyStep, TaskBDF1PointPos.m:58-64).  Forward = simLoop (BDF1
// :65-102; BDF2 :65-136 with the SDIRK2a / SDIRK2b start step) with the line-search-free newton (:105-146 / :139-181); per step the
// H, M, D of the LAST EVALUATED iterate of the step's final solve are kept in HBM ([B][nsteps][n*n], column-major over nodes), which
// is what Scene.saveHistory stores (the reference keeps lu(H), the backward kernel re-factors H').  Backward = TaskBDF1.calcFinal
// (TaskBDF1.m:45-81) / TaskBDF2.calcFinal (TaskBDF2.m:45-107).  Every forward solve is the common residual
//     qdot = (x - qA)/eta,  v = x - qB,  g = M v - eta^2 f,  H = dg/dx      (evalBDF1, evalSDIRK2a/b, evalBDF2).

// HELP (part_adjhelp16.hip, trees of <= 16 nodes in batches of at most one rollout per two SIMDs - configs[3]'s 512 rollouts): a workgroup of
// TWO wavefronts per rollout.  M and D of a step do not enter the Newton iteration; forming and storing them is 9.5 % of the launch
// pair (profiles/r05w_adjoint_md_bound.txt).  Wave 0 - the rollout - leaves the 39 numbers per node that eval_MD reads in a
// double-buffered hand-over area of the workgroup's LDS at the end of each step and goes on with the next step; wave 1 forms M, D
// from them and stores them.  One workgroup barrier per step: wave 1 reaches barrier s + 1 after it has finished step s, so it has
// read buffer s & 1 before wave 0 (which writes that buffer again only behind barrier s + 1) can touch it.  Same function on the same
// numbers: M, D are bit-identical to the one-wave kernel's.
constexpr int ADJ_HAND = 40;      // doubles per node and buffer
__host__ __device__ constexpr size_t adj_hand_doubles(const int NP) { return (size_t)2 * ADJ_HAND * NP; }
template <int NP>
__device__ __forceinline__ void adj_hand_put(double* __restrict__ hb, const int lane, const FrontState& fs) {
    if (lane < NP) {
        double* o = hb + lane;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c * NP] = fs.sw[c];
            o[(3 + c) * NP] = fs.sv[c];
            o[(6 + c) * NP] = fs.xiw[c];
            o[(9 + c) * NP] = fs.xiv[c];
        }
#pragma unroll
        for (int c = 6; c < NACC; ++c) o[(12 + c - 6) * NP] = fs.S[c];
        static_assert(12 + NACC - 6 + 5 <= ADJ_HAND, "hand-over rows");
        o[(12 + NACC - 6) * NP] = fs.dd;
        o[(13 + NACC - 6) * NP] = __longlong_as_double((long long)fs.anc_m);
        o[(14 + NACC - 6) * NP] = __longlong_as_double((long long)fs.desc_m);
        o[(15 + NACC - 6) * NP] = fs.act ? 1.0 : 0.0;
        o[(16 + NACC - 6) * NP] = fs.dof ? 1.0 : 0.0;
    }
}
template <int NP>
__device__ __forceinline__ void adj_md_helper(const DevModel& M, const AdjArgs& a, const double* __restrict__ hand, const int lane, const int traj) {
    const int n = M.n;
    const size_t nn = (size_t)n * n;
    const int l = lane < NP ? lane : 0;      // (lanes beyond the tree's DPP row read node 0's numbers: their results are not stored)
    for (int s = 1; s <= a.nsteps; ++s) {
        __syncthreads();
        const double* o = hand + (size_t)(s & 1) * (ADJ_HAND * NP) + l;
        FrontState fs;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            fs.sw[c] = o[c * NP];
            fs.sv[c] = o[(3 + c) * NP];
            fs.xiw[c] = o[(6 + c) * NP];
            fs.xiv[c] = o[(9 + c) * NP];
        }
#pragma unroll
        for (int c = 6; c < NACC; ++c) fs.S[c] = o[(12 + c - 6) * NP];
        fs.dd = o[(12 + NACC - 6) * NP];
        fs.anc_m = (unsigned long long)__double_as_longlong(o[(13 + NACC - 6) * NP]);
        fs.desc_m = (unsigned long long)__double_as_longlong(o[(14 + NACC - 6) * NP]);
        fs.act = lane < NP && o[(15 + NACC - 6) * NP] != 0.0;
        fs.dof = o[(16 + NACC - 6) * NP] != 0.0;
        double Mrow[NP], Drow[NP];
        eval_MD<NP>(M, lane, fs, Mrow, Drow);
        double* Mk = a.Ms + ((size_t)traj * a.nsteps + (s - 1)) * nn;
        double* Dk = a.Ds + ((size_t)traj * a.nsteps + (s - 1)) * nn;
        if (lane < n) {
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (i < n) {
                    Mk[(size_t)i * n + lane] = Mrow[i];
                    Dk[(size_t)i * n + lane] = Drow[i];
                }
        }
    }
}

// FC: a serial chain that fills every node slot (is_chain && n == NP, decided by the launcher): the two model facts as compile-time
// constants (model_view), as in the FULLCHAIN step kernels - no tree paths in the front, no per-row bounds
// CTL (rmx_adjoint_controls): one torque per joint and STEP, a.u[B][nsteps][nr], loaded at the top of every step - applyStep is called
// once per step (TaskBDF1PointPos.m:58-64) - in place of the constant parameters a.p[B][nr]; the backward kernel then stores one row
// of a.dPdu per step.  Compile-time, not a test on a.u, and carried as a bit of the integrator argument (MODE = 1 | 2, + ADJ_CTL): the
// constant-parameter kernels keep their names and their instruction streams, which profiles/roofline_calibration.json is tied to
// (bench.py load_calibration).
constexpr int ADJ_CTL = 4;
// TRK (rmx_adjoint_track, with CTL): the objective is a table of terms - a point of a body, a step, a weight, a target (a.trk, sorted
// by step; a.trk_begin; a.trk_xt, shared or one table per rollout) - in place of the one term of a.task_step / a.task_node.  A step
// that owns terms keeps what J of the last evaluated iterate is made of - every lane's sw, sv, the frames Rw, pw - in an LDS area of
// its own behind the constants (and the helper wave's hand-over), runs the final-state front ONCE and loops over its terms; row
// s-1 of a.dPdq ([B][nsteps][n] here) is their sum, which the backward kernel reads where the step owns terms.  J is formed once per
// measured step from the kept iterate, not at every Newton iterate.  Compile-time like CTL: the other instantiations keep their code.
constexpr int ADJ_TRK = 8;
// TAPE (rmx_rollout_tape / rmx_rollout_vjp, with CTL, never with TRK): no objective at all.  The forward kernel is the CTL
// sweep with a.task_step = 0 - no step is the task step, so no J is formed, no final-state front runs, no dPdq is written - without
// the regulariser and P, and records q, qdot of every step (a.qtraj / a.qdtraj).  The task branches stay COMPILED in it: the sweep has
// to be rmx_adjoint_controls' bit for bit, and with them compiled out the compiler contracts a few products of the front differently
// (1 ulp in q on the 7-joint tree and the 32-link chain, measured; either branch alone restores the bits);
// the backward kernel takes y_k from the caller's cotangents (a.gq / a.gqd), stores du per step and forms the k = 0 row (dL/dq0,
// dL/dqdot0) behind the loop.  The two kernels are launched by different calls (a.tape).  Compile-time like CTL and TRK.
// Under BDF2 (rmx_rollout_tape_bdf2) the tape has nsteps + 1 slots per rollout: step s in slot s-1 as everywhere, and H, M, D of the
// SDIRK2a solve - which the adjoint pairs drop, with the reference - in slot nsteps; its backward sweep is a kernel of its own
// (k_rollout_bwd_bdf2) that differentiates every solve exactly.  One wavefront per rollout, never the helper-wave form.
constexpr int ADJ_TAPE = 16;
// ZS (rmx_rollout_vjp_params, with TAPE; backward kernels only): the backward sweep also stores z of every solve (a.zs), which the
// parameter contraction of rmx_params.h reads.  Compile-time: rmx_rollout_vjp keeps the instantiations it had.
constexpr int ADJ_ZS = 32;
// FB (rmx_rollout_tape_feedback, with CTL and TAPE, never with TRK or the helper wave): the torque of step s is not a.u's row alone
// but a.u's row (the feed-forward uff) plus an affine feedback on the state the rollout has reached at the START of the step - the
// kernel's own q, qd registers, the bits of row s-2 of the record - formed at the top of the step loop (rmx_feedback.h) and stored to
// a.uapp.  Nothing else of the sweep changes, and the tape it leaves is the open-loop tape under a.uapp.  A null a.fbK is no
// feedback: the applied torque is a.u's bit for bit.  Compile-time like the others: every other instantiation keeps its code.
constexpr int ADJ_FB = 64;
constexpr int ADJ_TRK_ROWS = 18;      // sw[3], sv[3], Rw[9], pw[3], one column per node
__host__ __device__ constexpr size_t adj_trk_doubles(const int NP) { return (size_t)ADJ_TRK_ROWS * NP; }
template <int NP, int MODE, bool HELP = false, bool FC = false>
__global__ void __launch_bounds__(HELP ? 128 : 64) k_adjoint_fwd(const DevModel Min, const DevOpts o, const AdjArgs a) {
    constexpr int INTEG = MODE & 3;
    constexpr bool CTL = (MODE & ADJ_CTL) != 0;
    constexpr bool TRK = (MODE & ADJ_TRK) != 0;
    constexpr bool TAPE = (MODE & ADJ_TAPE) != 0;
    static_assert(INTEG == 1 || INTEG == 2, "BDF1 or BDF2");
    static_assert(!TRK || CTL, "the tracking objective comes with per-step controls");
    static_assert(!TAPE || (CTL && !TRK), "the taped rollout: per-step controls, no objective");
    constexpr bool TAPE2 = TAPE && INTEG == 2;       // the BDF2 tape: H, M, D of the SDIRK2a solve too, in a slot of its own
    static_assert(!TAPE2 || !HELP, "the BDF2 tape runs one wavefront per rollout (two hand-overs in step 1 only: see select_rollout_tape)");
    constexpr bool FB = (MODE & ADJ_FB) != 0;
    static_assert(!FB || (TAPE && !HELP), "state feedback: the taped rollout, one wavefront per rollout (select_rollout_feedback)");
    static_assert(!HELP || NP <= 16, "the helper-wave form: trees of one DPP row");
    const DevModel M = model_view<NP, FC>(Min);
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    double* hand = nullptr;
    // TRK: the kept iterate, behind the wave's scratch, the constants and (HELP) the hand-over buffers
    double* const kept = TRK ? sAcc + acc_doubles(M.n, NP) + (size_t)(NCONST + NGROUND) * cstride(NP) + (HELP ? adj_hand_doubles(NP) : 0) : nullptr;
    if constexpr (HELP) {
        hand = sAcc + acc_doubles(M.n, NP) + (size_t)(NCONST + NGROUND) * cstride(NP);      // behind the wave's scratch and the constants
        if (threadIdx.x >= 64) {
            adj_md_helper<NP>(M, a, hand, (int)threadIdx.x - 64, (int)blockIdx.x);
            return;
        }
    }
    const int lane = threadIdx.x, traj = blockIdx.x, n = M.n;
    const int id = (lane < n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    double q = id >= 0 ? a.q[off] : 0.0;
    double qd = id >= 0 ? a.qd[off] : 0.0;
    double qp = 0.0, qdp = 0.0;             // BDF2: the state of step k-1 (Joint.q1 / qdot1)
    const double pj = (id >= 0 && !CTL) ? a.p[off] : 0.0;
    const double* uj = CTL ? a.u + (size_t)traj * a.nsteps * M.nr + (id >= 0 ? id : 0) : nullptr;
    double ureg = 0.0;                      // CTL: this lane's sum of u^2 over the steps
    const double h = o.h;
    FrontState fs;
    fs.tau_add = a.pscale * pj;
    // does the task body hang below (or at) this lane's joint?  (rows of J(idxM_body, :) that are non-zero)
    const bool on_path = !TRK && lane < n && (lane == a.task_node || ((M.rel[MAXN + lane] >> a.task_node) & 1ull));
    int iters = 0, status = 0;
    double Ptask = 0.0;
    const size_t nn = (size_t)n * n;
    const double al = (2.0 - sqrt(2.0)) / 2.0;       // SDIRK2 (driverRedMaxAdjointBDF2.m:80)
    for (int s = 1; s <= a.nsteps; ++s) {
        if constexpr (CTL) {                 // (under BDF2 step 1's torque holds for both SDIRK2 solves)
            double us = id >= 0 ? uj[(size_t)(s - 1) * M.nr] : 0.0;
            if constexpr (FB) {              // (q, qd: the state at the start of step s)
                if (a.fbK) {
                    const size_t row = (size_t)traj * a.fb_stride + (size_t)(s - 1);
                    us = feedback_torque<NP>(us, a.fbK + row * ((size_t)2 * M.nr * M.nr), a.fbx ? a.fbx + row * ((size_t)2 * M.nr) : nullptr,
                                             M.nr, n, id, q, qd);
                }
                // rmx_rollout_tape_feedback_box: the actuator saturates - behind the feedback sum, and with a null K too.  The tests
                // on the pointers are wave-uniform; two selects on the lane's own value (a NaN torque stays one)
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
            if constexpr (!TAPE) ureg += us * us;
        }
        double* Hk = a.Hs + ((size_t)traj * a.nsteps + (s - 1)) * nn;
        double* Mk = a.Ms + ((size_t)traj * a.nsteps + (s - 1)) * nn;
        double* Dk = a.Ds + ((size_t)traj * a.nsteps + (s - 1)) * nn;
        double Jw[3] = {0.0, 0.0, 0.0}, Jv[3] = {0.0, 0.0, 0.0};   // J(idxM_body, this joint) of the last evaluated iterate
        int tb = 0, te = 0;                          // TRK: the terms this step owns
        if constexpr (TRK) {
            tb = a.trk_begin[s - 1];
            te = a.trk_begin[s];
        }
        const bool measured = te > tb;
        const double q0 = (INTEG == 2 && s > 1) ? qp : q, qd0 = (INTEG == 2 && s > 1) ? qdp : qd;      // BDF2: step k-1
        const double q1 = q, qd1 = qd;                                                                  // BDF2: step k
        double qa = 0.0, qda = 0.0;                  // SDIRK2a's result
        double x = 0.0, xlo = 0.0;                   // compensated iterate x + xlo (newton_impl in rmx_device.h)
        const int nsolve = (INTEG == 2 && s == 1) ? 2 : 1;
        for (int sv = 0; sv < nsolve; ++sv) {
            double qA, qB, eta;
            if (INTEG == 1) {                        // evalBDF1 :160-176
                eta = h; qA = q0; qB = q0 + h * qd0; x = qB;
            } else if (s == 1 && sv == 0) {          // SDIRK2a :78-84, evalSDIRK2a :184-216
                eta = al * h; qA = q0; qB = q0 + (al * h) * qd0; x = q0 + al * h * qd0;
            } else if (s == 1) {                     // SDIRK2b :89-92, evalSDIRK2b :219-252
                eta = al * h;
                x = qa + (1.0 - al) * h * qda;
                qA = q0 + (1.0 - al) * h * qda;
                qB = q0 + (2.0 * al - 1.0) * h * qd0 + 2.0 * (1.0 - al) * h * qda;
            } else {                                 // BDF2 :103-113, evalBDF2 :255-287
                eta = (2.0 / 3.0) * h;
                x = q1 + h * qd1;
                qA = (4.0 / 3.0) * q1 - (1.0 / 3.0) * q0;
                qB = (4.0 / 3.0) * q1 - (1.0 / 3.0) * q0 + (8.0 / 9.0) * h * qd1 - (2.0 / 9.0) * h * qd0;
            }
            xlo = 0.0;
            if constexpr (TAPE2) {      // nsteps + 1 slots per rollout: step s in slot s-1, the SDIRK2a solve in slot nsteps
                const size_t slot = (size_t)traj * (a.nsteps + 1) + ((s == 1 && sv == 0) ? a.nsteps : s - 1);
                Hk = a.Hs + slot * nn;
                Mk = a.Ms + slot * nn;
                Dk = a.Ds + slot * nn;
            }
            // the SDIRK2a solve leaves nothing in the history - but on the BDF2 tape, where it has a slot of its own: there every use
            // below is a store to the slot (no step is the task step, no terms, no helper wave)
            const bool last_solve = TAPE2 || sv + 1 == nsolve;
            int iter = 1;
            // Scene.saveHistory keeps H, M, D of the LAST evaluated iterate of the step (driverRedMaxAdjointBDF1.m:100, 127).  Up to 32
            // nodes H rides in registers through the Newton loop (the solve destroys its working copy) and M, D are formed ONCE, after
            // the loop, from the state the last evaluation left behind (fs) - they do not enter the Newton iteration itself; all three
            // go to HBM once per step.  Larger trees store H at every iterate (the last store wins) and form M, D once per step as well.
            constexpr bool STORE_ONCE = NP <= 32;
            double Hs[STORE_ONCE ? NP : 1];
            while (true) {
                NodeOut e;
                double Hrow[NP];
                eval_front<NP, true>(M, sAcc, lane, x, ((x - qA) + xlo) / eta, (x - qB) + xlo, eta, e, fs);
                const double hdiag = eval_hess<NP>(M, lane, fs, Hrow, nullptr, sAcc);
                if constexpr (STORE_ONCE) {
#pragma unroll
                    for (int i = 0; i < NP; ++i) Hs[i] = Hrow[i];
                } else if (last_solve) {
                    // the solve destroys its copy and 64 more doubles per lane do not fit next to it: H of every iterate goes to HBM, the
                    // last store wins.  M and D do not enter the Newton iteration: they are formed once, after the loop, from fs
                    if (lane < n) {
#pragma unroll
                        for (int i = 0; i < NP; ++i)
                            if (i < n) Hk[(size_t)i * n + lane] = Hrow[i];
                    }
                }
                if constexpr (TRK) {
                    // the frames of the last evaluated iterate go to the kept area at every iterate of a measured step (the last store
                    // wins), so that they are not live across the solve; sw, sv follow after the loop, where eval_MD has them anyway.
                    // One store of all 18 rows after the loop instead: scratch per lane 180 -> 276 bytes in <16, 14>, 188 -> 288 in
                    // <32, 14>, 2104 -> 2200 / 3832 -> 3960 in the 64-lane pair - more than the CTL siblings take (228, 244, 2156, 3880)
                    if (measured && last_solve && lane < NP) {
#pragma unroll
                        for (int c = 0; c < 9; ++c) kept[(6 + c) * NP + lane] = fs.Rw[c];
#pragma unroll
                        for (int c = 0; c < 3; ++c) kept[(15 + c) * NP + lane] = fs.pw[c];
                    }
                }
                if (!TRK && s == a.task_step && last_solve) {   // J(body rows, joint) = Ad(E_body^-1) s_joint : body-frame twist of the task body per unit qdot
                    double Rb[9], pb[3], t3[3], d3[3];
#pragma unroll
                    for (int c = 0; c < 9; ++c) Rb[c] = readlane_d(fs.Rw[c], a.task_node);
#pragma unroll
                    for (int c = 0; c < 3; ++c) pb[c] = readlane_d(fs.pw[c], a.task_node);
                    cross3(pb, fs.sw, t3);
#pragma unroll
                    for (int c = 0; c < 3; ++c) d3[c] = fs.sv[c] - t3[c];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {   // R' (.)
                        Jw[c] = on_path ? (Rb[c] * fs.sw[0] + Rb[3 + c] * fs.sw[1] + Rb[6 + c] * fs.sw[2]) : 0.0;
                        Jv[c] = on_path ? (Rb[c] * d3[0] + Rb[3 + c] * d3[1] + Rb[6 + c] * d3[2]) : 0.0;
                    }
                }
                ++iters;
                // [Hl,Hu,Hp] = lu(H,'vector'); dx = -(Hu\(Hl\g(Hp)))  :127-128.  As in the step kernels the solve takes diagonal pivots
                // under the growth guard first (a third of the instructions of the pivot search) and falls back to partial pivoting
                // on the saved copy of H when the guard trips; the factors themselves are not kept (the backward pass re-solves).
                double dx;
                if constexpr (STORE_ONCE) {
                    bool lu_ok;
                    dx = lu_solve_neg_diag<NP>(lane, Hrow, e.g, hdiag, lu_ok);
                    if (!lu_ok) {
#pragma unroll
                        for (int i = 0; i < NP; ++i) Hrow[i] = Hs[i];
                        dx = lu_solve_neg<NP, true>(n, lane, Hrow, e.g);
                        status |= 16;
                    }
                } else if constexpr (NP == 64 && LU_SPLIT64) {
                    // 33..64 nodes: the guarded block-column solve of the step kernels (lu_solve_neg_diag64: H through the front's scratch,
                    // every update one DPP-fused FMA; a third of the instructions of the pivoted solve); H of this iterate is in the
                    // history already, so a tripped guard reloads it from there and pivots
                    (void)hdiag;
                    bool lu_ok;
                    dx = lu_solve_neg_diag64(n, lane, sAcc, Hrow, e.g, lu_ok);
                    if (!lu_ok) {
                        if (last_solve) {
#pragma unroll
                            for (int i = 0; i < NP; ++i) Hrow[i] = (lane < n && i < n) ? Hk[(size_t)i * n + lane] : ((i == lane) ? 1.0 : 0.0);
                        } else {             // (the SDIRK2a solve leaves nothing in the history: evaluate again)
                            NodeOut e2;
                            eval_front<NP, true>(M, sAcc, lane, x, ((x - qA) + xlo) / eta, (x - qB) + xlo, eta, e2, fs);
                            eval_hess<NP>(M, lane, fs, Hrow, nullptr, sAcc);
                        }
                        dx = lu_solve_neg<NP, true>(n, lane, Hrow, e.g);
                        status |= 16;
                    }
                } else {
                    (void)hdiag;
                    dx = lu_solve_neg<NP, true>(n, lane, Hrow, e.g);
                }
                const double dxn2 = wave_sum(dx * dx);
                if (!(dxn2 == dxn2)) { status |= 4; break; }
                if (sqrt(dxn2) > o.dxMax) { status |= 1; break; }            // :129-132
                {                                                             // x = x + dx, :134, before the convergence test
                    const double xa = x;
                    two_sum(xa, xlo + dx, x, xlo);
                    xlo *= o.comp;
                }
                if (sqrt(wave_sum(e.g * e.g)) < o.tol) break;                 // :135-138
                if (iter >= o.iterMax) { status |= 2; break; }                // :139-142
                ++iter;
            }
            if constexpr (NP == 32 && HESS_MFMA) {
                if (last_solve) {           // M, D on the matrix cores, stored from the MFMA layout (eval_MD_mfma32_store); H from its rows
                    eval_MD_mfma32_store(M, lane, fs, sAcc, Mk, Dk);
                    if (lane < n) {
#pragma unroll
                        for (int i = 0; i < NP; ++i)
                            if (i < n) Hk[(size_t)i * n + lane] = Hs[i];
                    }
                }
            } else if (HELP && last_solve) {
                adj_hand_put<NP>(hand + (size_t)(s & 1) * (ADJ_HAND * NP), lane, fs);      // fs: the state of the last evaluated iterate
                __syncthreads();                                                            // (the one barrier of the step: see above)
                if (lane < n) {
#pragma unroll
                    for (int i = 0; i < NP; ++i)
                        if (i < n) Hk[(size_t)i * n + lane] = Hs[i];
                }
            } else if (last_solve) {
                double Mrow[NP], Drow[NP];
                eval_MD<NP>(M, lane, fs, Mrow, Drow);       // fs: the state of the last evaluated iterate
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
            if (INTEG == 2 && s == 1 && sv == 0) {   // :85-87
                qa = x;
                qda = ((x - q0) + xlo) / (al * h);
            }
        }
        if (INTEG == 1) {
            qd = ((x - q0) + xlo) / h;
            q = x;
        } else if (s == 1) {                         // :93-98: setQ(q1, qdot1), setQ1(q0, qdot0)
            qd = (x - q0 - (1.0 - al) * h * qda) / (al * h);
            q = x;
            qp = q0;
            qdp = qd0;
        } else {                                     // :114-117
            qd = (3.0 / (2.0 * h)) * (x - (4.0 / 3.0) * q1 + (1.0 / 3.0) * q0);
            q = x;
            qp = q1;
            qdp = qd1;
        }
        if constexpr (TAPE) {             // the record of the rollout: row s-1 is the state after step s, in the layout of u
            if (a.qtraj && id >= 0) {
                const size_t offs = ((size_t)traj * a.nsteps + (s - 1)) * M.nr + id;
                a.qtraj[offs] = q;
                a.qdtraj[offs] = qd;
            }
        }
        if constexpr (TRK) {
            if (measured) {      // this step owns terms: calcStep of each of them, their sum in row s-1 of dPdq
                // fs is still the state of the last evaluated iterate: keep what J needs of it before the final-state front overwrites it
                // (the frames are in the area already)
                if (lane < NP) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        kept[c * NP + lane] = fs.sw[c];
                        kept[(3 + c) * NP + lane] = fs.sv[c];
                    }
                }
                RMX_SYNC();
                NodeOut e;
                eval_front<NP, false>(M, sAcc, lane, q, qd, 0.0, 1.0, e, fs);
                const int l = lane < NP ? lane : 0;      // (lanes past the tree: node 0's numbers, never on a path)
                double swk[3], svk[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    swk[c] = kept[c * NP + l];
                    svk[c] = kept[(3 + c) * NP + l];
                }
                double ysum = 0.0;
                for (int t = tb; t < te; ++t) {
                    const rmx_track::DevTerm& T = a.trk[t];
                    const int node = __builtin_amdgcn_readfirstlane(T.node);      // (wave-uniform: the frame reads stay v_readlane)
                    const double* xt = a.trk_xt + (size_t)traj * a.trk_xt_stride + (size_t)3 * (size_t)T.orig;
                    const double xl[3] = {T.xl[0], T.xl[1], T.xl[2]}, wp = T.wpos;
                    // M.rel's descendant mask of this lane as smem_setup staged it: the final-state eval_front above has just reloaded
                    // fs.desc_m from there (the staged rows mirror M.rel[MAXN + lane]), so this relies on that call coming first
                    const bool on = lane < n && (lane == node || ((fs.desc_m >> node) & 1ull));
                    double Rb[9], pb[3], dxw[3], vl[3], t3[3], d3[3], Jw[3], Jv[3];
#pragma unroll
                    for (int c = 0; c < 9; ++c) Rb[c] = readlane_d(fs.Rw[c], node);
#pragma unroll
                    for (int c = 0; c < 3; ++c) pb[c] = readlane_d(fs.pw[c], node);
#pragma unroll
                    for (int c = 0; c < 3; ++c) dxw[c] = Rb[3 * c] * xl[0] + Rb[3 * c + 1] * xl[1] + Rb[3 * c + 2] * xl[2] + pb[c] - xt[c];
                    Ptask += wp * 0.5 * dot3(dxw, dxw);
                    // J(body rows, joint) of the kept iterate = Ad(E_body^-1) s_joint, as the single-term kernels form it per iterate
                    double Rk[9], pk[3];
#pragma unroll
                    for (int c = 0; c < 9; ++c) Rk[c] = kept[(6 + c) * NP + node];
#pragma unroll
                    for (int c = 0; c < 3; ++c) pk[c] = kept[(15 + c) * NP + node];
                    cross3(pk, swk, t3);
#pragma unroll
                    for (int c = 0; c < 3; ++c) d3[c] = svk[c] - t3[c];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {   // R' (.)
                        Jw[c] = on ? (Rk[c] * swk[0] + Rk[3 + c] * swk[1] + Rk[6 + c] * swk[2]) : 0.0;
                        Jv[c] = on ? (Rk[c] * d3[0] + Rk[3 + c] * d3[1] + Rk[6 + c] * d3[2]) : 0.0;
                    }
                    cross3(Jw, xl, t3);
#pragma unroll
                    for (int c = 0; c < 3; ++c) vl[c] = Jv[c] + t3[c];
                    double g3[3];
                    mat3v(Rb, vl, g3);
                    ysum += wp * dot3(g3, dxw);
                }
                if (lane < n) a.dPdq[((size_t)traj * a.nsteps + (s - 1)) * n + lane] = ysum;
                RMX_SYNC();      // (the kept iterate is read out before a later step writes the area again)
            }
        } else if (s == a.task_step) {    // TaskBDF1PointPos.calcStep :67-107 (TaskBDF2PointPos.calcStep is the same) at the final state of this step
            NodeOut e;
            eval_front<NP, false>(M, sAcc, lane, q, qd, 0.0, 1.0, e, fs);
            double Rb[9], pb[3], dxw[3], vl[3], t3[3];
#pragma unroll
            for (int c = 0; c < 9; ++c) Rb[c] = readlane_d(fs.Rw[c], a.task_node);
#pragma unroll
            for (int c = 0; c < 3; ++c) pb[c] = readlane_d(fs.pw[c], a.task_node);
#pragma unroll
            for (int c = 0; c < 3; ++c) dxw[c] = Rb[3 * c] * a.xl[0] + Rb[3 * c + 1] * a.xl[1] + Rb[3 * c + 2] * a.xl[2] + pb[c] - a.xt[c];
            Ptask += a.wpos * 0.5 * dot3(dxw, dxw);
            // dPdq = J' * (R*Gamma(xlocal))' * dx * wp ,  Gamma = [brac(xlocal)', I]  =>  R (v + w x xlocal) . dx * wp
            const double xl[3] = {a.xl[0], a.xl[1], a.xl[2]};
            cross3(Jw, xl, t3);
#pragma unroll
            for (int c = 0; c < 3; ++c) vl[c] = Jv[c] + t3[c];
            double g3[3];
            mat3v(Rb, vl, g3);
            if (lane < n) a.dPdq[(size_t)traj * n + lane] = a.wpos * dot3(g3, dxw);
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
    const double preg = wave_sum(CTL ? ureg : pj * pj);
    if (lane == 0) {
        if constexpr (!TAPE) a.P[traj] = Ptask + a.wreg * 0.5 * preg;      // TaskBDF1.calcFinal :49 / TaskBDF2.calcFinal :49
        if (a.it) {
            a.it[traj] = iters;
            a.status[traj] = status;
        }
    }
}

// yk -= (cm M_j + cd h D_j)' z_j : one off-diagonal block of the backward sweep; this lane's entry = column `col` of the block . z
template <int NP>
__device__ __forceinline__ void adj_block(double& y, const double* __restrict__ Mj, const double* __restrict__ Dj, const int n, const int lane,
                                          const int col, const double cm, const double cdh, const double z) {
    const double* Mc = Mj + (size_t)col * n;
    const double* Dc = Dj + (size_t)col * n;
    // Every load of the column before its first use, none of them under a lane condition (index and column clamped into the block,
    // the padding selected afterwards): guarded by `j < n && lane < n` each load sat in its own exec-masked block with a full wait
    // behind it - 32 dependent round trips per block and step, most of the backward kernel's time.
    double mc[NP], dc[NP];
    const bool withD = cdh != 0.0;
#pragma unroll
    for (int j = 0; j < NP; ++j) mc[j] = Mc[j < n ? j : 0];
    if (withD) {
#pragma unroll
        for (int j = 0; j < NP; ++j) dc[j] = Dc[j < n ? j : 0];
    } else {
#pragma unroll
        for (int j = 0; j < NP; ++j) dc[j] = 0.0;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        double blk = 0.0;
        if (j < n && lane < n) blk = withD ? (cm * mc[j] + cdh * dc[j]) : cm * mc[j];
        y -= blk * readlane_d(z, j);
    }
}

template <int NP, int MODE, bool FC = false>
__global__ void __launch_bounds__(64) k_adjoint_bwd(const DevModel Min, const DevOpts o, const AdjArgs a) {
    constexpr int INTEG = MODE & 3;              // (MODE: as k_adjoint_fwd)
    constexpr bool CTL = (MODE & ADJ_CTL) != 0;
    constexpr bool TRK = (MODE & ADJ_TRK) != 0;      // y_k: row k of dPdq where step k owns terms
    constexpr bool TAPE = (MODE & ADJ_TAPE) != 0;    // y_k: the caller's cotangents; du per step; the k = 0 row behind the loop
    constexpr bool ZS = (MODE & ADJ_ZS) != 0;        // z_k of every step to a.zs as well
    static_assert(!TAPE || (CTL && !TRK && INTEG == 1), "the taped rollout: per-step controls, no objective, BDF1");
    static_assert(!ZS || TAPE, "z per slot: the taped rollout");
    const DevModel M = model_view<NP, FC>(Min);
    const int lane = threadIdx.x, traj = blockIdx.x, n = M.n;
    const int id = (lane < n) ? M.idx[lane] : -1;
    const size_t nn = (size_t)n * n;
    const double h = o.h;
    const int col = lane < n ? lane : 0;
    const double al = (2.0 - sqrt(2.0)) / 2.0;
    double z1 = 0.0, z2 = 0.0, z3 = 0.0, z4 = 0.0, zs = 0.0;      // z of steps k+1 .. k+4
    const double* Mb = a.Ms + (size_t)traj * a.nsteps * nn;
    const double* Db = a.Ds + (size_t)traj * a.nsteps * nn;
    double gdn = 0.0;                                // TAPE: dL/dqdot of step k+1
    for (int k = a.nsteps; k >= 1; --k) {
        double y;
        if constexpr (TAPE) {
            // y_k = dL/dq_k + (dL/dqdot_k - dL/dqdot_{k+1}) / h, from qdot_k = (q_k - q_{k-1}) / h; mapped through M.idx as u is, zero on
            // lanes without a DOF (the loads unconditional, the index clamped: see adj_block)
            const size_t offk = ((size_t)traj * a.nsteps + (k - 1)) * M.nr + (id >= 0 ? id : 0);
            const double gqk = a.gq[offk], gdk = a.gqd[offk];
            y = id >= 0 ? gqk + (gdk - gdn) / h : 0.0;
            gdn = gdk;
        } else if constexpr (TRK) y = (a.trk_begin[k] > a.trk_begin[k - 1] && lane < n) ? a.dPdq[((size_t)traj * a.nsteps + (k - 1)) * n + lane] : 0.0;
        else y = (k == a.task_step && lane < n) ? a.dPdq[(size_t)traj * n + lane] : 0.0;
        if (INTEG == 1) {
            // yk -= (-2 M_{k+1} + h D_{k+1})' z_{k+1}   TaskBDF1.m:58-64 ;   yk -= M_{k+2}' z_{k+2}   :65-70
            if (k < a.nsteps) adj_block<NP>(y, Mb + (size_t)k * nn, Db + (size_t)k * nn, n, lane, col, -2.0, h, z1);
            if (k < a.nsteps - 1) adj_block<NP>(y, Mb + (size_t)(k + 1) * nn, Db + (size_t)(k + 1) * nn, n, lane, col, 1.0, 0.0, z2);
        } else {
            // TaskBDF2.m:66-96: blocks of steps k+1 .. k+4; the k == 1 variants carry the SDIRK2 start step's coefficients
            if (k < a.nsteps)
                adj_block<NP>(y, Mb + (size_t)k * nn, Db + (size_t)k * nn, n, lane, col, k == 1 ? -((8.0 / (9.0 * al)) + (4.0 / 3.0)) : -(8.0 / 3.0),
                              (8.0 / 9.0) * h, z1);
            if (k < a.nsteps - 1)
                adj_block<NP>(y, Mb + (size_t)(k + 1) * nn, Db + (size_t)(k + 1) * nn, n, lane, col, k == 1 ? ((2.0 / (9.0 * al)) + (19.0 / 9.0)) : (22.0 / 9.0),
                              -(2.0 / 9.0) * h, z2);
            if (k < a.nsteps - 2) adj_block<NP>(y, Mb + (size_t)(k + 2) * nn, Db + (size_t)(k + 2) * nn, n, lane, col, -(8.0 / 9.0), 0.0, z3);
            if (k < a.nsteps - 3) adj_block<NP>(y, Mb + (size_t)(k + 3) * nn, Db + (size_t)(k + 3) * nn, n, lane, col, 1.0 / 9.0, 0.0, z4);
        }
        // z_k = H_k'^-1 y_k  (zkk0(Hp) = Hl'\(Hu'\yk) :76): this lane's "row" of H' is column `lane` of H
        double Hrow[NP];
        const double* Hc = a.Hs + ((size_t)traj * a.nsteps + (k - 1)) * nn + (size_t)col * n;
        {   // (unconditional loads, all in flight together: see adj_block)
            double hv[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) hv[i] = Hc[i < n ? i : 0];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < NP; ++i) Hrow[i] = (i < n && lane < n) ? hv[i] : ((i == lane) ? 1.0 : 0.0);
        }
        double z;
        if constexpr (NP <= 32) {
            // as in the forward sweep: diagonal pivots under the growth guard first (a third of the instructions of the pivot search; H'
            // is as close to symmetric positive definite as H), partial pivoting on a fresh copy of the rows when the guard trips
            const double hdl = Hc[col];
            const double hd = lane < n ? hdl : 1.0;
            bool lu_ok;
            z = lu_solve_neg_diag<NP>(lane, Hrow, -y, hd, lu_ok);
            if (!lu_ok) {
#pragma unroll
                for (int i = 0; i < NP; ++i) Hrow[i] = (i < n && lane < n) ? Hc[i] : ((i == lane) ? 1.0 : 0.0);
                z = lu_solve_neg<NP, true>(n, lane, Hrow, -y);
            }
        } else {
            z = lu_solve_neg<NP, true>(n, lane, Hrow, -y);
        }
        if constexpr (TAPE) {   // du_k = -z_k' dg_k/du_k, dg_k/du_k = -h^2 pscale I
            if (id >= 0) a.dPdu[((size_t)traj * a.nsteps + (k - 1)) * M.nr + id] = h * h * a.pscale * z;
            if constexpr (ZS) {
                if (lane < n) a.zs[((size_t)traj * a.nsteps + (k - 1)) * n + lane] = z;      // (nodes without a DOF: an identity row, z = 0)
            }
        } else if constexpr (CTL) {    // the constant-parameter formula below before its sum over the steps, one row per step
            if (id >= 0) {
                const size_t offk = ((size_t)traj * a.nsteps + (k - 1)) * M.nr + id;
                a.dPdu[offk] = a.wreg * a.u[offk] + (INTEG == 1 ? h * h : (4.0 / 9.0) * h * h) * a.pscale * z;
            }
        } else {
            zs += z;
        }
        z4 = z3;
        z3 = z2;
        z2 = z1;
        z1 = z;
    }
    if constexpr (TAPE) {
        // the k = 0 row.  g_1 = M (q_1 - q_0 - h qdot_0) - h^2 f(q_1, (q_1 - q_0) / h): dg_1/dq_0 = -M_1 + h D_1 (where the recursion has
        // -2 M: nothing precedes q_0), dg_1/dqdot_0 = -h M_1, dg_2/dq_0 = M_2; and qdot_1 = (q_1 - q_0) / h reads q_0 directly.
        // z1, z2 are z of steps 1 and 2 here, gdn is dL/dqdot_1.
        if (a.dq0) {
            double y0 = id >= 0 ? -gdn / h : 0.0, yd0 = 0.0;
            adj_block<NP>(y0, Mb, Db, n, lane, col, -1.0, h, z1);
            if (a.nsteps > 1) adj_block<NP>(y0, Mb + nn, Db + nn, n, lane, col, 1.0, 0.0, z2);
            adj_block<NP>(yd0, Mb, Db, n, lane, col, -h, 0.0, z1);      // dL/dqdot_0 = h M_1' z_1
            if (id >= 0) {
                const size_t off = (size_t)traj * M.nr + id;
                a.dq0[off] = y0;
                a.dqd0[off] = yd0;
            }
        }
    }
    if (id >= 0 && !CTL) {   // dPdp = wreg*p' - z'*dgdp, dgdp(kk,:) = -eta^2*pscale*I with eta^2 = h^2 (TaskBDF1PointPos.m:104-105) or (4/9) h^2 for
        const size_t off = (size_t)traj * M.nr + id;                 // EVERY step (TaskBDF2PointPos.m:97-106)
        const double e2 = INTEG == 1 ? h * h : (4.0 / 9.0) * h * h;
        a.dPdp[off] = a.wreg * a.p[off] + e2 * a.pscale * zs;
    }
}

// The backward sweep of the BDF2 tape (rmx_rollout_tape_bdf2 / rmx_rollout_vjp; the recursion is in include/redmax_hip.h).  Every solve
// of the BDF2 loop is x(qA, qB, u): g = M(x)(x - qB) - eta^2 (f(x, (x - qA)/eta) + pscale u) = 0 with v = (x - qA)/eta, and with H,
// M, D of the tape dg/dqB = -M, dg/dqA = eta D, dg/du = -eta^2 pscale.  Cotangents (xbar, vbar) on (x, v) go back through
//     H' z = xbar + vbar/eta,   qAbar = -vbar/eta - eta D' z,   qBbar = M' z,   ubar = eta^2 pscale z.

// (M' z, D' z) of one slot, from one pass over column `col` of M and of D (this lane's entries).  The load discipline of adj_block:
// every load before the first use, none under a lane condition, index and column clamped into the block, the padding selected afterwards.
template <int NP>
__device__ __forceinline__ void adj_block_md(double& mz, double& dz, const double* __restrict__ Mj, const double* __restrict__ Dj, const int n,
                                             const int lane, const int col, const double z) {
    const double* Mc = Mj + (size_t)col * n;
    const double* Dc = Dj + (size_t)col * n;
    double mc[NP], dc[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) mc[j] = Mc[j < n ? j : 0];
#pragma unroll
    for (int j = 0; j < NP; ++j) dc[j] = Dc[j < n ? j : 0];
    __builtin_amdgcn_sched_barrier(0);
    mz = 0.0;
    dz = 0.0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const bool in = j < n && lane < n;
        const double zj = readlane_d(z, j);
        mz += (in ? mc[j] : 0.0) * zj;
        dz += (in ? dc[j] : 0.0) * zj;
    }
}

// one taped solve backwards: z, and the cotangents A of qA and Bq of qB.  Lanes without a DOF carry zeros.
template <int NP>
__device__ __forceinline__ void tape_solve_bwd(const double* __restrict__ Hj, const double* __restrict__ Mj, const double* __restrict__ Dj, const int n,
                                               const int lane, const int col, const bool dof, const double eta, const double xbar,
                                               const double vbar, double& A, double& Bq, double& z) {
    const double y = dof ? xbar + vbar / eta : 0.0;
    // z = H'^-1 y: this lane's "row" of H' is column `lane` of H (as k_adjoint_bwd: unconditional loads, all in flight together)
    double Hrow[NP];
    const double* Hc = Hj + (size_t)col * n;
    {
        double hv[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) hv[i] = Hc[i < n ? i : 0];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NP; ++i) Hrow[i] = (i < n && lane < n) ? hv[i] : ((i == lane) ? 1.0 : 0.0);
    }
    // Up to 16 nodes: diagonal pivots under the growth guard first, partial pivoting on a fresh copy when it trips (k_adjoint_bwd's
    // policy).  At 16 lanes that solve is lu_diag_tail from its first pivot on: its DPP broadcasts read Hrow[] and the right-hand side
    // straight away, so both are materialised and two wait states pass first (dpp_settle; the hazard note at fmsub_rowbcast).
    // From 17 nodes on the pivoted solve, which has no DPP sequence: at 32 lanes the guarded solve gave wrong results in the two
    // start-step solves of this kernel - zero cotangents came back as a non-zero du_1 on an MI355X, the loop's solve being right -,
    // which fits a broadcast that reads a register too soon after its write; the offending pair was not isolated.
    if constexpr (NP <= 16) {
        double yv = y;
        if constexpr (NP == 16) {
            asm volatile("" : "+v"(yv));
            dpp_settle(Hrow);
        }
        const double hdl = Hc[col];
        const double hd = lane < n ? hdl : 1.0;
        bool lu_ok;
        z = lu_solve_neg_diag<NP>(lane, Hrow, -yv, hd, lu_ok);
        if (!lu_ok) {
#pragma unroll
            for (int i = 0; i < NP; ++i) Hrow[i] = (i < n && lane < n) ? Hc[i] : ((i == lane) ? 1.0 : 0.0);
            z = lu_solve_neg<NP, true>(n, lane, Hrow, -y);
        }
    } else {
        z = lu_solve_neg<NP, true>(n, lane, Hrow, -y);
    }
    double mz, dz;
    adj_block_md<NP>(mz, dz, Mj, Dj, n, lane, col, z);
    A = dof ? -vbar / eta - eta * dz : 0.0;
    Bq = dof ? mz : 0.0;
}

// One wavefront per rollout, lane = node.  qbar, vbar of steps k+1 (complete) and k (still collecting) ride in registers; the solve that
// produced step k+1 (slot k; eta = 2h/3, qA = 4/3 q_k - 1/3 q_{k-1}, qB = qA + 8/9 h qd_k - 2/9 h qd_{k-1}) feeds steps k and k-1.  H, M,
// D are read once each per step.  The SDIRK2 start step runs behind the loop: stage b (slot 0) reads q0, qd0 and qda, stage a (slot
// nsteps) is read through qda alone; step 1's torque holds for both.
template <int NP, bool FC = false>
__global__ void __launch_bounds__(64) k_rollout_bwd_bdf2(const DevModel Min, const DevOpts o, const AdjArgs a) {
    const DevModel M = model_view<NP, FC>(Min);
    const int lane = threadIdx.x, traj = blockIdx.x, n = M.n, N = a.nsteps;
    const int id = (lane < n) ? M.idx[lane] : -1;
    const bool dof = id >= 0;
    const size_t nn = (size_t)n * n;
    const double h = o.h;
    const int col = lane < n ? lane : 0;
    const double al = (2.0 - sqrt(2.0)) / 2.0;
    const double* Hb = a.Hs + (size_t)traj * (N + 1) * nn;
    const double* Mb = a.Ms + (size_t)traj * (N + 1) * nn;
    const double* Db = a.Ds + (size_t)traj * (N + 1) * nn;
    const size_t row0 = (size_t)traj * N * M.nr + (dof ? id : 0);      // this lane's entry of row 0 (step 1) of gq, gqd, du
    // (the cotangent loads unconditional, the row clamped, lanes without a DOF and rows that do not exist selected to zero afterwards)
    const double gqN = a.gq[row0 + (size_t)(N - 1) * M.nr], gdN = a.gqd[row0 + (size_t)(N - 1) * M.nr];
    const double gqP = a.gq[row0 + (size_t)(N >= 2 ? N - 2 : 0) * M.nr], gdP = a.gqd[row0 + (size_t)(N >= 2 ? N - 2 : 0) * M.nr];
    double qb1 = dof ? gqN : 0.0, vb1 = dof ? gdN : 0.0;                        // step k+1
    double qb0 = (dof && N >= 2) ? gqP : 0.0, vb0 = (dof && N >= 2) ? gdP : 0.0;      // step k (step 0 has no cotangent of its own)
    const double eta = (2.0 / 3.0) * h;
    for (int k = N - 1; k >= 1; --k) {
        const size_t rowm = row0 + (size_t)(k >= 2 ? k - 2 : 0) * M.nr;          // step k-1, in flight across the solve
        const double gqm = a.gq[rowm], gdm = a.gqd[rowm];
        double A, Bq, z;
        tape_solve_bwd<NP>(Hb + (size_t)k * nn, Mb + (size_t)k * nn, Db + (size_t)k * nn, n, lane, col, dof, eta, qb1, vb1, A, Bq, z);
        if (dof) a.dPdu[row0 + (size_t)k * M.nr] = eta * eta * a.pscale * z;
        const double s = A + Bq;
        qb0 += (4.0 / 3.0) * s;
        vb0 += (8.0 / 9.0) * h * Bq;
        qb1 = qb0;
        vb1 = vb0;
        qb0 = ((dof && k >= 2) ? gqm : 0.0) - (1.0 / 3.0) * s;
        vb0 = ((dof && k >= 2) ? gdm : 0.0) - (2.0 / 9.0) * h * Bq;
    }
    // the start step: qb1, vb1 are the cotangents of step 1, qb0, vb0 of the initial state
    const double etas = al * h;
    double A, Bq, zb, A2, B2, za;
    tape_solve_bwd<NP>(Hb, Mb, Db, n, lane, col, dof, etas, qb1, vb1, A, Bq, zb);                   // SDIRK2b
    qb0 += A + Bq;
    vb0 += (2.0 * al - 1.0) * h * Bq;
    const double qdab = (1.0 - al) * h * A + 2.0 * (1.0 - al) * h * Bq;
    tape_solve_bwd<NP>(Hb + (size_t)N * nn, Mb + (size_t)N * nn, Db + (size_t)N * nn, n, lane, col, dof, etas, 0.0, qdab, A2, B2, za);      // SDIRK2a
    qb0 += A2 + B2;
    vb0 += al * h * B2;
    if (dof) {
        a.dPdu[row0] = etas * etas * a.pscale * (za + zb);
        if (a.dq0) {
            const size_t off = (size_t)traj * M.nr + id;
            a.dq0[off] = qb0;
            a.dqd0[off] = vb0;
        }
    }
}

// k_rollout_bwd_bdf2 with z of every solve stored as well - a.zs, [B][nsteps + 1][n] in the tape's slots (zb in slot 0, za in slot
// nsteps): the kernel of rmx_rollout_vjp_params.  A kernel of its own, statement for statement the one above plus the three stores:
// as a flag of a shared body the compiler scheduled rmx_rollout_vjp's instantiation differently (other code, if the same results),
// and that kernel keeps its code.
template <int NP, bool FC = false>
__global__ void __launch_bounds__(64) k_rollout_bwd_bdf2_zs(const DevModel Min, const DevOpts o, const AdjArgs a) {
    const DevModel M = model_view<NP, FC>(Min);
    const int lane = threadIdx.x, traj = blockIdx.x, n = M.n, N = a.nsteps;
    const int id = (lane < n) ? M.idx[lane] : -1;
    const bool dof = id >= 0;
    const size_t nn = (size_t)n * n;
    const double h = o.h;
    const int col = lane < n ? lane : 0;
    const double al = (2.0 - sqrt(2.0)) / 2.0;
    const double* Hb = a.Hs + (size_t)traj * (N + 1) * nn;
    const double* Mb = a.Ms + (size_t)traj * (N + 1) * nn;
    const double* Db = a.Ds + (size_t)traj * (N + 1) * nn;
    const size_t row0 = (size_t)traj * N * M.nr + (dof ? id : 0);      // this lane's entry of row 0 (step 1) of gq, gqd, du
    // (the cotangent loads unconditional, the row clamped, lanes without a DOF and rows that do not exist selected to zero afterwards)
    const double gqN = a.gq[row0 + (size_t)(N - 1) * M.nr], gdN = a.gqd[row0 + (size_t)(N - 1) * M.nr];
    const double gqP = a.gq[row0 + (size_t)(N >= 2 ? N - 2 : 0) * M.nr], gdP = a.gqd[row0 + (size_t)(N >= 2 ? N - 2 : 0) * M.nr];
    double qb1 = dof ? gqN : 0.0, vb1 = dof ? gdN : 0.0;                        // step k+1
    double qb0 = (dof && N >= 2) ? gqP : 0.0, vb0 = (dof && N >= 2) ? gdP : 0.0;      // step k (step 0 has no cotangent of its own)
    const double eta = (2.0 / 3.0) * h;
    for (int k = N - 1; k >= 1; --k) {
        const size_t rowm = row0 + (size_t)(k >= 2 ? k - 2 : 0) * M.nr;          // step k-1, in flight across the solve
        const double gqm = a.gq[rowm], gdm = a.gqd[rowm];
        double A, Bq, z;
        tape_solve_bwd<NP>(Hb + (size_t)k * nn, Mb + (size_t)k * nn, Db + (size_t)k * nn, n, lane, col, dof, eta, qb1, vb1, A, Bq, z);
        if (dof) a.dPdu[row0 + (size_t)k * M.nr] = eta * eta * a.pscale * z;
        if (lane < n) a.zs[((size_t)traj * (N + 1) + k) * n + lane] = z;
        const double s = A + Bq;
        qb0 += (4.0 / 3.0) * s;
        vb0 += (8.0 / 9.0) * h * Bq;
        qb1 = qb0;
        vb1 = vb0;
        qb0 = ((dof && k >= 2) ? gqm : 0.0) - (1.0 / 3.0) * s;
        vb0 = ((dof && k >= 2) ? gdm : 0.0) - (2.0 / 9.0) * h * Bq;
    }
    // the start step: qb1, vb1 are the cotangents of step 1, qb0, vb0 of the initial state
    const double etas = al * h;
    double A, Bq, zb, A2, B2, za;
    tape_solve_bwd<NP>(Hb, Mb, Db, n, lane, col, dof, etas, qb1, vb1, A, Bq, zb);                   // SDIRK2b
    qb0 += A + Bq;
    vb0 += (2.0 * al - 1.0) * h * Bq;
    const double qdab = (1.0 - al) * h * A + 2.0 * (1.0 - al) * h * Bq;
    tape_solve_bwd<NP>(Hb + (size_t)N * nn, Mb + (size_t)N * nn, Db + (size_t)N * nn, n, lane, col, dof, etas, 0.0, qdab, A2, B2, za);      // SDIRK2a
    qb0 += A2 + B2;
    vb0 += al * h * B2;
    if (dof) {
        a.dPdu[row0] = etas * etas * a.pscale * (za + zb);
        if (a.dq0) {
            const size_t off = (size_t)traj * M.nr + id;
            a.dq0[off] = qb0;
            a.dqd0[off] = vb0;
        }
    }
    if (lane < n) {
        a.zs[(size_t)traj * (N + 1) * n + lane] = zb;
        a.zs[((size_t)traj * (N + 1) + N) * n + lane] = za;
    }
}

#include "rmx_feedback_bwd.h"      /* k_rollout_bwd_fb: the closed-loop backward sweep, on tape_solve_bwd above */

// Parity hook: one residual (+Hessian) evaluation per trajectory, results to HBM.
template <int NP, bool WANT_H, bool CT>
__global__ void __launch_bounds__(64) k_eval(const DevModel M, const int B, const double* __restrict__ q,
                                             const double* __restrict__ qA, const double* __restrict__ qB, const double eta,
                                             double* __restrict__ g, double* __restrict__ H, const int* __restrict__ chart) {
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const int lane = threadIdx.x, traj = blockIdx.x;
    if constexpr (CT) {
        con_setup<NP>(M, sCol);
        if (M.nsph) sph_setup<NP>(M, sCol, lane, chart + (size_t)traj * M.nsph);
    }
    const int id = (lane < M.n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    const double x = id >= 0 ? q[off] : 0.0;
    const double xa = id >= 0 ? qA[off] : 0.0;
    const double xb = id >= 0 ? qB[off] : 0.0;
    NodeOut e;
    double Hrow[NP];
    eval_node<NP, WANT_H, false, CT>(M, sAcc, sCol, lane, x, (x - xa) / eta, x - xb, eta, e, Hrow);
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

// Parity hook for computeValues itself (driverRedMaxBDF1.m:190-243): M = J'MmJ (:212), f = fr + J'(fm - Mm Jdot qdot) (:215-216)
// and D = df/dqdot (:227-237) at (q, qdot), results to HBM (column-major per trajectory).  f is the residual with v = 0 and
// e2 = 1 (g = M v - e2 f = -f); M and D rows come from the subtree sums the same front pass leaves behind (eval_MD).
template <int NP, bool CT = false>
__global__ void __launch_bounds__(64) k_eval_mfd(const DevModel M, const int B, const double* __restrict__ q, const double* __restrict__ qd,
                                                 double* __restrict__ Mo, double* __restrict__ fo, double* __restrict__ Do,
                                                 const int* __restrict__ chart) {
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    // JointSpherical / JointFree3D: the group's three revolute nodes about the axes of the trajectory's Euler chart ARE the joint in
    // the chart's coordinates (S = T of JointSpherical.m:298-303), so M, f, D come out in those coordinates with no further term
    if constexpr (CT) con_setup<NP>(M, sCol);
    if (M.nsph) sph_setup<NP>(M, sCol, threadIdx.x, chart + (size_t)blockIdx.x * M.nsph);
    const int lane = threadIdx.x, traj = blockIdx.x;
    const int id = (lane < M.n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    FrontState fs;
    NodeOut e;
    eval_front_e2<NP, true, false, CT>(M, sAcc, lane, id >= 0 ? q[off] : 0.0, id >= 0 ? qd[off] : 0.0, 0.0, 1.0, 1.0, e, fs);
    double Mrow[NP], Drow[NP];
    if constexpr (CT) {       // ForceGroundCuboid: its wrench is in f (the front), its damping blocks go into D here
        double yc[6];
        contact_damping_fold<NP>(M, sAcc, lane, fs, yc);
        eval_MD<NP, true>(M, lane, fs, Mrow, Drow, yc);
    } else {
        eval_MD<NP>(M, lane, fs, Mrow, Drow);
    }
    if (id >= 0) fo[off] = -e.g;
    double* Mt = Mo + (size_t)traj * M.nr * M.nr;
    double* Dt = Do + (size_t)traj * M.nr * M.nr;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (i < M.n) {
            const int ci = M.idx[i];
            if (id >= 0 && ci >= 0) {
                Mt[(size_t)ci * M.nr + id] = Mrow[i];
                Dt[(size_t)ci * M.nr + id] = Drow[i];
            }
        }
    }
}

// Joint.computeEnergies / Body.computeEnergies at the stored state.
template <int NP, bool CT>
__global__ void __launch_bounds__(64) k_energy(const DevModel M, const int B, const double* __restrict__ q,
                                               const double* __restrict__ qd, double* __restrict__ T, double* __restrict__ V,
                                               const int* __restrict__ chart) {
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    if constexpr (CT) {
        con_setup<NP>(M, sCol);
        if (M.nsph) sph_setup<NP>(M, sCol, threadIdx.x, chart + (size_t)blockIdx.x * M.nsph);
    }
    const int lane = threadIdx.x, traj = blockIdx.x;
    const int id = (lane < M.n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    NodeOut e;
    double Hrow[NP];
    eval_node<NP, false, false, CT>(M, sAcc, sCol, lane, id >= 0 ? q[off] : 0.0, id >= 0 ? qd[off] : 0.0, 0.0, 1.0, e, Hrow);
    const double t = wave_sum(e.eT), v = wave_sum(e.eV);
    if (lane == 0) {
        T[traj] = t;
        V[traj] = v;
    }
}

// Profiling hook: shader-clock cycles (s_memtime) of the phases of one Newton iteration with the GENERIC device functions (eval_node,
// the pivoting solve / the 64-row guarded solve) at the production occupancy (one wavefront per trajectory).  The full 32-link chain
// is timed by k_phase_time_pair32 instead (the functions its step kernel runs).
template <int NP>
__global__ void __launch_bounds__(64) k_phase_time(const DevModel M, const int reps, const double* __restrict__ q,
                                                   const double* __restrict__ qd, const double h, unsigned long long* __restrict__ out) {
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const int lane = threadIdx.x, traj = blockIdx.x;
    const int id = (lane < M.n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    const double q0 = id >= 0 ? q[off] : 0.0, qd0 = id >= 0 ? qd[off] : 0.0;
    double x = q0 + h * qd0;
    unsigned long long tg = 0, tH = 0, tLU = 0, tred = 0;
    unsigned long long stamps[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double sink = 0.0;
    for (int r = 0; r < reps; ++r) {
        NodeOut e;
        double Hrow[NP];
        unsigned long long t0 = __builtin_amdgcn_s_memtime();
        eval_node<NP, false>(M, sAcc, sCol, lane, x, (x - q0) / h, x - (q0 + h * qd0), h, e, Hrow);
        sink += e.g;
        unsigned long long t1 = __builtin_amdgcn_s_memtime();
        bool staged = false;
        if constexpr (NP == 64 && LU_SPLIT64 && HESS_MFMA64) {
            if (M.tree_dmax > 0) {                    // a branching tree: the Hessian stage as the step kernels run it (operands staged for tree_solve64)
                FrontState fs;
                eval_front<NP, true, true, false>(M, sAcc, lane, x, (x - q0) / h, x - (q0 + h * qd0), h, e, fs, stamps);
                (void)eval_hess<NP, false, false, false>(M, lane, fs, Hrow, nullptr, sAcc, e.g);
                staged = true;
            }
        }
        if (!staged) eval_node<NP, true, true>(M, sAcc, sCol, lane, x, (x - q0) / h, x - (q0 + h * qd0), h, e, Hrow, stamps);
        unsigned long long t2 = __builtin_amdgcn_s_memtime();
        double dx;
        if constexpr (NP == 64 && LU_SPLIT64) {      // the guarded solve the step kernels run (33..64 rows)
            bool lu_ok;
            if (M.tree_dmax > 0) {                    // a branching tree: along the tree
                dx = solve64_staged(M, lane, sAcc, lu_ok);
            } else {
                dx = lu_solve_neg_diag64(M.n, lane, sAcc, Hrow, e.g, lu_ok);
            }
            sink += lu_ok ? 0.0 : 1.0;
        } else {
            dx = lu_solve_neg<NP, true>(M.n, lane, Hrow, e.g);
        }
        unsigned long long t3 = __builtin_amdgcn_s_memtime();
        const double s1 = wave_sum(dx * dx) + wave_sum(e.g * e.g);
        unsigned long long t4 = __builtin_amdgcn_s_memtime();
        sink += s1;
        x += 1e-3 * dx;   // keep the iterations data dependent
        tg += t1 - t0; tH += t2 - t1; tLU += t3 - t2; tred += t4 - t3;
    }
    if (lane == 0) {
        out[16 * traj + 0] = tg; out[16 * traj + 1] = tH; out[16 * traj + 2] = tLU; out[16 * traj + 3] = tred;
        for (int k = 0; k < 12; ++k) out[16 * traj + 4 + k] = stamps[k];
    }
    if (sink == 1.2345e301) out[0] = 0;   // keep the results live
}

// ============================================================================ launchers (declared in rmx_host.h)
//
// The launchers of the part files decide nothing: rmx_select.h picks the kernel family and the instantiation, the host unit calls the
// launcher of that family with the plan's flags.  An instantiation stays in the part it is launched from (the parts differ in macros
// and scheduling flags).  One object per part and size, so the builds run in parallel.

// More than 64 KiB of dynamic LDS (trees of 33..64 nodes: 34 KiB of per-node constants + H row-major for the block-column solve)
// is an opt-in per kernel and device; it costs microseconds, so it is set at every launch rather than cached (a process may
// drive several devices from several threads).
#define RMX_LAUNCH(kernel, grid, block, bytes, stream, ...)                                                                         \
    do {                                                                                                                            \
        if ((bytes) > 64 * 1024)                                                                                                    \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)); \
        kernel<<<grid, block, bytes, stream>>>(__VA_ARGS__);                                                                        \
    } while (0)
