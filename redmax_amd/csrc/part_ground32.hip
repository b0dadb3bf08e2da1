// part_ground32.hip (part 4 of the former rmx_kernels.hip) -- serial chains of <= 32 nodes with ForceGroundCuboid: the step kernels around newton_pair
// (rmx_ct32.h).  One wavefront per workgroup in every kernel of the part: LDS hand-overs ordered by wavefront-scope fences.
#define RMX_NP 32
#ifndef RMX_SYNC
#define RMX_SYNC() rmx_lane_sync()      // (see rmx_lane_sync)
#endif
#include "rmx_kernels.h"
#include "rmx_ct32.h"

// simLoop of driverRedMaxBDF1.m:57-91 / driverRedMaxBDF2.m:57-125 (integ, wave-uniform) for one rollout of a chain of <= 32 nodes with
// ground contact, steps sfirst .. nsteps - 1.  ONE call site of newton_pair for every stage of every integrator: the SDIRK2 start step
// is two passes of the stage loop, everything else one.
// Returns the step at which the rollout was handed on (nsteps: it is complete).  One Newton flavour per instantiation:
// RUN_LEAN: free flight - the lean solve (newton_node<32, true, true>: the plain evaluation plus the test that every cuboid is clear of
//   the ground, under which the contact terms vanish identically); the rollout is handed on at the start of the first STEP in which an
//   evaluation fails that test (what the lean launch of launch_step_ct_32 does).
// RUN_PAIR: newton_pair, one wavefront; a solve whose line searches keep running out their trials hands the rollout on, at the start
//   of that step, to a cooperative group (DevOpts::parkHalv).
// RUN_COOP: this wavefront is a member of the group that finishes a parked rollout.
enum { RUN_LEAN = 0, RUN_PAIR = 1, RUN_COOP = 2 };
template <int MODE>
__device__ __forceinline__ int run_rollout(const DevModel& M, const DevOpts& o, const StepArgs& a, const int integ, double* sAcc, double* sCol,
                                           const int lane, const int traj, const int sfirst, CoopCtx& cx, const CoopPub& pb,
                                           const unsigned long long tick0) {
    constexpr int NP = 32;
    constexpr bool COOP = MODE == RUN_COOP;
    const bool writer = !COOP || cx.member == 0;     // (members 1.. of a cooperative group compute, member 0 also stores)
    const double h = o.h;
    const bool bdf2 = integ == INTEG_BDF2;
    const int id = (lane < M.n) ? M.idx[lane] : -1;
    const size_t off = (size_t)traj * M.nr + (id >= 0 ? id : 0);
    double q = id >= 0 ? a.q[off] : 0.0;
    double qd = id >= 0 ? a.qd[off] : 0.0;
    double qp = (bdf2 && id >= 0) ? a.qp[off] : 0.0;       // step k-1 (Joint.q1 / qdot1 in the reference)
    double qdp = (bdf2 && id >= 0) ? a.qdp[off] : 0.0;
    const bool started = (*a.started) != 0 || sfirst > 0;    // resumed behind earlier steps of this call: they are its history
    int iters = 0, halv = 0, status = 0;
    PivotPolicy piv;
    if constexpr (COOP) {
        const int* pp = a.park + 1 + a.B + 3 * traj;
        piv.hold = pp[0]; piv.len = pp[1]; piv.streak = pp[2];
    }
    int stop = a.nsteps;
    for (int s = sfirst; s < a.nsteps; ++s) {
        NodeOut last;
        last.g = last.eT = last.eV = 0.0;
        double xlo = 0.0;
        const int it_in = iters, hv_in = halv, st_in = status;
        const PivotPolicy piv_in = piv;
        const bool start2 = bdf2 && s == 0 && !started;       // SDIRK2 start step (driverRedMaxBDF2.m:64-88): two solves
        const double al = (2.0 - sqrt(2.0)) / 2.0;            // (:74)
        const double q0 = (bdf2 && !start2) ? qp : q, qd0 = (bdf2 && !start2) ? qdp : qd, q1 = q, qd1 = qd;
        double qa = 0.0, qda = 0.0, xsol = 0.0;
        bool left = false;
        for (int stage = 0; stage < (start2 ? 2 : 1) && !left; ++stage) {
            double xi, qA, qB, eta;
            if (!bdf2) {                       // BDF1 (evalBDF1 :160-187): eta = h, qA = q0, qB = q0 + h qdot0 = the initial guess (:70)
                xi = q0 + h * qd0; qA = q0; qB = xi; eta = h;
            } else if (!start2) {              // BDF2 (evalBDF2 :263-293): eta = 2h/3
                xi = q1 + h * qd1;
                qA = (4.0 / 3.0) * q1 - (1.0 / 3.0) * q0;
                qB = (4.0 / 3.0) * q1 - (1.0 / 3.0) * q0 + (8.0 / 9.0) * h * qd1 - (2.0 / 9.0) * h * qd0;
                eta = (2.0 / 3.0) * h;
            } else if (stage == 0) {           // SDIRK2a (evalSDIRK2a :194-225): eta = a h, qA = q0, qB = q0 + a h qdot0
                xi = q0 + al * h * qd0; qA = q0; qB = q0 + (al * h) * qd0; eta = al * h;
            } else {                           // SDIRK2b (evalSDIRK2b :228-260)
                xi = qa + (1.0 - al) * h * qda;
                qA = q0 + (1.0 - al) * h * qda;
                qB = q0 + (2.0 * al - 1.0) * h * qd0 + 2.0 * (1.0 - al) * h * qda;
                eta = al * h;
            }
            if constexpr (MODE == RUN_LEAN) {
                xsol = newton_node<NP, true, true, false>(M, o, sAcc, sCol, lane, xi, qA, qB, eta, last, iters, halv, status, piv, xlo, cx);
                left = (status & ST_LEFT_LEAN) != 0;   // a cuboid comes near the ground: nothing of this step is kept
            } else {
                // the pivot policy of newton_policy (rmx_device.h): a hold after three tripped solves in a row
                const bool pivot_all = o.lu_mode != 0 || piv.hold > 0;
                if (piv.hold > 0) --piv.hold;
                xsol = newton_pair<COOP>(M, o, sAcc, lane, xi, qA, qB, eta, last, iters, halv, status, piv, pivot_all, xlo, cx, pb);
                if (!pivot_all) pivot_policy_update(piv);
                left = (MODE == RUN_PAIR && (status & ST_PARK)) || (COOP && (status & ST_COOP_FAULT));
            }
            if (start2 && stage == 0 && !left) {
                qa = xsol;
                qda = (qa - q0) / (al * h);
            }
        }
        if (left) {
            if (COOP) break;                   // (ST_COOP_FAULT stays in the status)
            // nothing of this step is kept: whoever takes the rollout on starts the step again (a solve of the start step that went through included)
            iters = it_in; halv = hv_in; status = st_in & ~(ST_PARK | ST_LEFT_LEAN); piv = piv_in;
            stop = s;
            break;
        }
        if (!bdf2) {
            qd = ((xsol - q0) + xlo) / h;      // (:72), with the low-order part of the iterate the residual was evaluated at
            q = xsol;
        } else if (start2) {
            qd = (xsol - q0 - (1.0 - al) * h * qda) / (al * h);
            q = xsol;
            qp = q0;
            qdp = qd0;
        } else {
            qp = q1;
            qdp = qd1;
            qd = (3.0 / (2.0 * h)) * (xsol - (4.0 / 3.0) * q1 + (1.0 / 3.0) * q0);
            q = xsol;
        }
        if (a.histT && writer) {               // Scene.saveHistory (Scene.m:134-161)
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
    }
    if (id >= 0 && writer) {
        a.q[off] = q;
        a.qd[off] = qd;
        if (bdf2) {
            a.qp[off] = qp;
            a.qdp[off] = qdp;
        }
    }
    if constexpr (COOP) {
        // a parked rollout a group has taken to its end: k_park_audit tells it from one nobody picked up by this
        if (lane == 0 && writer && !(status & ST_COOP_FAULT)) a.resume[traj] = a.nsteps;
    }
    if constexpr (!COOP) {
        if (lane == 0) {
            a.resume[traj] = stop;
            if (MODE == RUN_PAIR && a.park && stop < a.nsteps) {
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
#ifdef RMX_TICK_PHASE
    if (lane == 0 && a.ticks && writer) a.ticks[traj] += cx.phase;
    cx.phase = 0;
#else
    if (lane == 0 && a.ticks && writer) a.ticks[traj] += __builtin_amdgcn_s_memtime() - tick0;      // this rollout's share of the launch (rmx_step_ticks)
#endif
    return stop;
}

// Three launches (RMX_GROUND_FUSED=0, and whenever the cooperative groups are switched off): the lean launch of launch_step_ct_32, then
// COOP = false for every rollout from its a.resume, then COOP = true: group g finishes the parked rollouts g, g + ngroups, ...
template <bool COOP>
__global__ void __launch_bounds__(64) k_step_pair(const DevModel M, const DevOpts o, const StepArgs a, const int integ) {
    constexpr int NP = 32;
    unsigned long long tick0 = __builtin_amdgcn_s_memtime();
    int traj = blockIdx.x;
    CoopCtx cx;
    cx.ticks = o.coopTicks;
    CoopPub pb;
    int pk = 0, npark = 1, pstride = 1;
    if constexpr (COOP) {
#ifdef RMX_COOP_MAP_AID      // measurement builds: RMX_COOP_MAP=1 scatters the members of a group over the launch (member-major mapping)
        pk = a.coop_map ? blockIdx.x % a.ngroups : blockIdx.x / COOP_G;
        cx.member = a.coop_map ? blockIdx.x / a.ngroups : blockIdx.x % COOP_G;
#else
        pk = blockIdx.x / COOP_G;
        cx.member = blockIdx.x % COOP_G;
#endif
        cx.words = a.xch + (size_t)pk * COOP_WORDS;
        pb.rec = a.xrec + (size_t)pk * 2 * COOP_REC;
        npark = a.park[0];
        pstride = a.ngroups;
        if (pk >= npark) return;
        traj = a.park[1 + pk] - 1;
    }
    const int s0 = a.resume ? a.resume[traj] : 0;
    if (!COOP && s0 >= a.nsteps) return;           // the lean launch took this trajectory all the way
    double *sAcc, *sCol;
    smem_setup<NP>(M, sAcc, sCol);
    const int lane = threadIdx.x;
    con_setup<NP>(M, sCol);
    for (; pk < npark; pk += pstride) {              // (one pass unless COOP)
        int sfirst = s0;
        if constexpr (COOP) {
            traj = a.park[1 + pk] - 1;
            sfirst = a.resume[traj];
            tick0 = __builtin_amdgcn_s_memtime();
        }
        const int stop = run_rollout<COOP ? RUN_COOP : RUN_PAIR>(M, o, a, integ, sAcc, sCol, lane, traj, sfirst, cx, pb, tick0);
        if constexpr (!COOP) {
            if (lane == 0 && a.park && stop < a.nsteps) a.park[1 + atomicAdd(a.park, 1)] = traj + 1;
        }
    }
}

// ONE launch for the whole call: workgroups 0 .. B - 1 are the rollouts (lean solve, then newton_pair from the step that comes near the
// ground, until the end or until a solve parks the rollout), workgroups B .. are the members of the cooperative groups - workgroups are
// dispatched in index order (per XCD), so they take the SIMDs that finished rollouts leave - and pick the parked rollouts up as they
// appear: group g the g-th, (g + ngroups)-th ... entry of the list.  No launch boundary anywhere: a rollout that leaves free flight
// early is not held back by the last one to do so, and a parked rollout does not wait for the last unparked one.
// The list: a.park[1 + e] = rollout + 1 (zero before the launch), published with release semantics after the rollout's state;
// a.park[1 + 4 B] counts the rollout workgroups that have finished (the groups leave when all have and the list is exhausted).
// The three roles are OUT-OF-LINE functions: inlined into one kernel their three Newton loops share one register allocation (688 bytes
// of scratch, 860 spilled SGPRs, every loop slower than in a kernel of its own).  They take the launch's arguments as a pointer
// into global memory (scalar loads, as kernel arguments are) and name the LDS array themselves: a generic pointer into LDS handed
// to an out-of-line function loses its address space.
struct GroundArgs {
    DevModel M;
    DevOpts o;
    StepArgs a;
    int integ;
    int coop_only;      // measurement aid (RMX_GROUND_FUSED=3): every workgroup of this launch is a member of a cooperative group
};
__device__ __forceinline__ void role_smem(const DevModel& M, double*& sAcc, double*& sCol) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    sAcc = smem;
    sCol = smem + acc_doubles(M.n, 32);
}
// (the arguments are copied into locals once: read through the pointer, every field would be loaded again behind every store and
// every scheduling pin of the Newton loop - the compiler cannot know that nothing writes them)
__device__ __attribute__((noinline)) int role_lean(const GroundArgs* __restrict__ g, const int traj) {
    const DevModel M = g->M;
    const DevOpts o = g->o;
    const StepArgs a = g->a;
    const int integ = g->integ;
    double *sAcc, *sCol;
    role_smem(M, sAcc, sCol);
    CoopCtx cx;
    cx.ticks = o.coopTicks;
    CoopPub pb;
    return run_rollout<RUN_LEAN>(M, o, a, integ, sAcc, sCol, threadIdx.x, traj, 0, cx, pb, __builtin_amdgcn_s_memtime());
}
__device__ __attribute__((noinline)) int role_pair(const GroundArgs* __restrict__ g, const int traj, const int sfirst) {
    const DevModel M = g->M;
    const DevOpts o = g->o;
    const StepArgs a = g->a;
    const int integ = g->integ;
    double *sAcc, *sCol;
    role_smem(M, sAcc, sCol);
    CoopCtx cx;
    cx.ticks = o.coopTicks;
    CoopPub pb;
    return run_rollout<RUN_PAIR>(M, o, a, integ, sAcc, sCol, threadIdx.x, traj, sfirst, cx, pb, __builtin_amdgcn_s_memtime());
}
__device__ __forceinline__ void role_coop(const GroundArgs* __restrict__ g, const int grp, const int member) {
    const DevModel M = g->M;
    const DevOpts o = g->o;
    const StepArgs a = g->a;
    const int integ = g->integ;
    double *sAcc, *sCol;
    role_smem(M, sAcc, sCol);
    const int lane = threadIdx.x;
    CoopCtx cx;
    cx.ticks = o.coopTicks;
    CoopPub pb;
    cx.member = member;
    cx.words = a.xch + (size_t)grp * COOP_WORDS;
    pb.rec = a.xrec + (size_t)grp * 2 * COOP_REC;
    int* const done = a.park + 1 + 4 * a.B;
    for (int e = grp; e < a.B; e += a.ngroups) {
        int v = 0;
        // (the wait below ends when the rollout workgroups have all finished or parked.  It relies on their being dispatched - nothing
        // in the programming model promises that workgroups start in index order -, so it is bounded: a group that has seen no entry and
        // no end for 16 x the group timeout leaves, and k_park_audit marks whatever stays unfinished RMX_ST_COOP_FAULT)
        const unsigned long long tw0 = __builtin_amdgcn_s_memtime();
        while (true) {
            // (relaxed polls: an agent-scope ACQUIRE invalidates this XCD's L2 under every wavefront that lives in it, hundreds of
            // times per microsecond with ~500 idle members polling; the one fence below, after the entry has been seen, is what orders
            // the reads of the rollout's state)
            if (lane == 0) v = __hip_atomic_load(a.park + 1 + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v = __builtin_amdgcn_readfirstlane(v);
            if (v != 0) break;
            int d = 0, cnt = 0;
            if (lane == 0) {
                d = __hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                cnt = __hip_atomic_load(a.park, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            d = __builtin_amdgcn_readfirstlane(d);
            cnt = __builtin_amdgcn_readfirstlane(cnt);
            // every rollout has finished or parked (its list entry is written BEFORE it is counted, both by the same lane with release
            // semantics), and the count of entries, read after the count of finished rollouts, does not reach this one
            if (d >= a.B && cnt <= e) return;
            if (__builtin_amdgcn_s_memtime() - tw0 > 16ull * cx.ticks) return;
            __builtin_amdgcn_s_sleep(127);
        }
        __threadfence();                                 // acquire
        const int traj = v - 1;
        const int sfirst = __hip_atomic_load(a.resume + traj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        run_rollout<RUN_COOP>(M, o, a, integ, sAcc, sCol, lane, traj, sfirst, cx, pb, __builtin_amdgcn_s_memtime());
    }
}
__global__ void __launch_bounds__(64) k_ground32(const GroundArgs* __restrict__ g) {
    constexpr int NP = 32;
    {
        double *sAcc, *sCol;
        smem_setup<NP>(g->M, sAcc, sCol);
        con_setup<NP>(g->M, sCol);
    }
    const int B = g->coop_only ? 0 : g->a.B, nsteps = g->a.nsteps;
    if ((int)blockIdx.x >= B) {
        role_coop(g, ((int)blockIdx.x - B) / COOP_G, ((int)blockIdx.x - B) % COOP_G);
        return;
    }
    const int traj = blockIdx.x;
    int stop = role_lean(g, traj);
    if (stop < nsteps) stop = role_pair(g, traj, stop);
    int* const park = g->a.park;
    if (!park) return;                                   // (no cooperative groups in this call: nothing parks, nobody waits)
    __threadfence();                                     // release: this rollout's state, counters and pivot policy before its list entry
    if (threadIdx.x == 0) {
        if (stop < nsteps) {
            const int e = atomicAdd(park, 1);
            __hip_atomic_store(park + 1 + e, traj + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
        __hip_atomic_fetch_add(park + 1 + 4 * B, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the steps with the contact terms of a chain of <= 32 nodes: fused (one launch for everything) or behind the lean launch of launch_step_ct_32
// After the launches of a call that may park rollouts: a rollout that was parked and that no group took to its end (a group that gave
// up waiting, see role_coop; never observed) must not pass for a result - RMX_ST_COOP_FAULT | RMX_ST_NAN and a NaN state, as for a rollout
// whose group faulted.
__global__ void __launch_bounds__(256) k_park_audit(const StepArgs a, const int nr) {
    const int traj = blockIdx.x * blockDim.x + threadIdx.x;
    if (traj >= a.B || a.resume[traj] >= a.nsteps) return;
    if (a.status) a.status[traj] |= ST_COOP_FAULT | 4;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = 0; i < nr; ++i) {
        a.q[(size_t)traj * nr + i] = nan;
        a.qd[(size_t)traj * nr + i] = nan;
    }
}
// (a.park is set exactly where the call parks: StepPlan::parks)
static void park_audit(const rmx_model* m, const rmx_batch* b, const StepArgs& a) {
    if (a.park) k_park_audit<<<dim3((b->B + 255) / 256), dim3(256), 0, b->stream>>>(a, m->nr);
}
// a.fused 1: rollouts and cooperative groups in one launch; 2: the rollouts (free flight + contact terms) in one launch, the groups in a second
static void ground32_launches(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a) {
    const int inline_groups = a.fused == 1 ? a.ngroups : 0;
    GroundArgs ga;
    ga.M = m->dm; ga.o = o; ga.a = a; ga.integ = integ;
    ga.a.ngroups = inline_groups;
    ga.coop_only = 0;
    static_assert(2 * sizeof(GroundArgs) <= RMX_GARGS_BYTES, "rmx_batch::gargs");
    // (pageable source: staged before the call returns; a failed copy must not be followed by a launch that reads the block - the
    // sticky error surfaces in the caller's hipGetLastError)
    if (hipMemcpyAsync(b->gargs, &ga, sizeof ga, hipMemcpyHostToDevice, b->stream) != hipSuccess) return;
    RMX_LAUNCH(k_ground32, dim3(b->B + inline_groups * COOP_G), dim3(64), m->smem_bytes, b->stream, (const GroundArgs*)b->gargs);
    if (a.fused == 3 && a.park) {      // measurement aid: the groups as a second launch of the SAME kernel (its out-of-line role)
        ga.a.ngroups = a.ngroups;
        ga.coop_only = 1;
        GroundArgs* g2 = (GroundArgs*)b->gargs + 1;
        if (hipMemcpyAsync(g2, &ga, sizeof ga, hipMemcpyHostToDevice, b->stream) != hipSuccess) return;
        RMX_LAUNCH(k_ground32, dim3(a.ngroups * COOP_G), dim3(64), m->smem_bytes, b->stream, (const GroundArgs*)g2);
        return;
    }
    if (a.fused != 1 && a.park) RMX_LAUNCH((k_step_pair<true>), dim3(a.ngroups * COOP_G), dim3(64), m->smem_bytes, b->stream, m->dm, o, a, integ);
}
void launch_step_ground_32(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a) {
    ground32_launches(m, b, integ, o, a);
    park_audit(m, b, a);
}
void launch_step_pair_32(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a) {
    RMX_LAUNCH((k_step_pair<false>), dim3(b->B), dim3(64), m->smem_bytes, b->stream, m->dm, o, a, integ);
    // group g = workgroups COOP_G g .. COOP_G g + COOP_G - 1, all of them resident at once
    if (a.park) RMX_LAUNCH((k_step_pair<true>), dim3(a.ngroups * COOP_G), dim3(64), m->smem_bytes, b->stream, m->dm, o, a, integ);
    park_audit(m, b, a);
}
