// rmx_host.h -- what the host translation unit (redmax_hip.hip: the C ABI) and the kernel translation units
// (the part_*.hip files around rmx_kernels.h, one object per part and padded tree size RMX_NP in {4,8,16,32,64} so the builds run in
// parallel; rmx_big.hip) share:
// launch argument blocks, the model / batch objects and the per-size launcher entry points.
// Which step / adjoint kernel a call runs is decided in rmx_select.h (select_step / select_adjoint) and nowhere else: the host unit
// executes the plan through the step and adjoint launchers below, each of which launches one kernel family and takes the choice of
// instantiation as an argument.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "redmax_hip_profile.h"   /* redmax_hip.h + the measurement hooks */
#include "rmx_device.h"
#include "rmx_pf.h"
#include "rmx_select.h"
#include "rmx_track.h"

using namespace rmx;

enum { INTEG_BDF1 = 1, INTEG_BDF2 = 2 };
constexpr size_t RMX_GARGS_BYTES = 2048;

struct StepArgs {
    int B, nsteps;
    double* q;        // [B][nr] state (in/out)
    double* qd;
    double* qp;       // [B][nr] state of step k-1 (BDF2)
    double* qdp;
    int* started;     // [1] device flag: 0 => BDF2 must take the SDIRK2 start step first
    int* it;          // [B] stats (accumulated) or null
    int* ls;
    int* status;
    double* histT;    // [nsteps][B] or null
    double* histV;
    int* chart;       // [B][nsph] Euler charts of the spherical joints (in/out) or null
    double* histQ;    // [nsteps][B][nr] or null: q, qdot after every step (Scene.saveHistory, Scene.m:134-161)
    double* histQd;
    int* histC;       // [nsteps][B][nsph] or null: Euler charts after every step
    int* resume;      // [B] contact-capable kernels: first step the lean launch left to the launch with the contact terms
    unsigned long long* ticks;   // [B] or null: s_memtime ticks each rollout's wavefront spent in the launch(es) of this call (accumulated)
    // park and relaunch (rmx_device.h CoopCtx; null / 0: off): rollouts the launch with the contact terms gave up at the start of a step
    int* park;        // [1 + B + 3 B + 1]: [0] their number, [1 .. ] their indices + 1 in the order they parked (0: no entry yet),
                      // [1 + B + 3 traj ..] their pivot policy, [1 + 4 B] rollout workgroups that have finished (k_ground32)
    unsigned* xch;    // [ngroups][COOP_WORDS] exchange words of the cooperative groups (zero before the cooperative launch)
    int ngroups;      // cooperative groups in flight: group g finishes parked rollouts g, g + ngroups, ... one after the other
    int coop_map;     // measurement aid (RMX_COOP_MAP): 1 = member-major mapping of the cooperative launch's workgroups onto (group, member)
    int fused;        // the whole call in one launch (part_ground32.hip k_ground32): rollouts and cooperative groups side by side
    unsigned long long* xrec;   // [ngroups][2 COOP_REC] what the winner of a line search publishes to its group (rmx_ct32.h CoopPub; zero before the launch)
    int w2_noahead;   // two-wave tree kernels (rmx_kernels.h w2_steps_bdf1): 1 = no evaluation is run ahead (RMX_W2_RUNAHEAD=0; tests)
    int pairc;        // the full 32-link chain under BDF1: 1 = the two-point kernel of rmx_pair32.h (default), 0 = the one-point kernel (RMX_PAIRC=0; tests)
};

struct AdjArgs {
    int B, nsteps, task_step, task_node;
    double xl[3], xt[3], pscale, wreg, wpos;
    double *q, *qd;
    double *qp, *qdp;         // BDF2: state of step k-1 after the rollout (out)
    const double* p;
    double *Hs, *Ms, *Ds;     // [B][nsteps][n*n]
    double* dPdq;             // [B][n]   dP/dq of the task step
    double* P;                // [B]
    double* dPdp;             // [B][nr]
    int *it, *status;
    // rmx_adjoint_controls (the CTL instantiations; behind the members the constant-parameter kernels read, whose offsets stay)
    const double* u;          // [B][nsteps][nr] one torque per step, or null: the constant parameters p
    double* dPdu;             // [B][nsteps][nr] (with u), or null: with u the forward sweep alone
    // rmx_adjoint_track (the TRK instantiations; dPdq is [B][nsteps][n] there, row k written and read only where step k owns terms)
    const rmx_track::DevTerm* trk;   // [nterms] the terms sorted by step (rmx_track.h)
    const int* trk_begin;     // [nsteps + 1] step k owns terms trk_begin[k-1] .. trk_begin[k]-1
    const double* trk_xt;     // targets, [nterms][3] or [B][nterms][3], indexed by the term's position in the caller's array
    size_t trk_xt_stride;     // doubles from one rollout's target table to the next (0: one table for the batch)
    // rmx_rollout_tape / rmx_rollout_vjp (the TAPE instantiations: u as above, dPdu is du; no task, no P, no dPdq)
    int tape;                 // 0: an adjoint pair; 1: the forward sweep alone (rmx_rollout_tape); 2: the backward sweep alone (rmx_rollout_vjp)
    double *qtraj, *qdtraj;   // [B][nsteps][nr] q, qdot after every step (out), or null together
    const double *gq, *gqd;   // [B][nsteps][nr] the cotangents dL/dq_k, dL/dqdot_k
    double *dq0, *dqd0;       // [B][nr] dL/dq0, dL/dqdot0 (out), or null together
    // rmx_rollout_vjp_params (the ADJ_ZS instantiations of the two backward kernels, launched by that entry alone)
    double* zs;               // [B][nslots][n] the adjoint vector z of every taped solve, lane = node (out); slots as the tape's
    // rmx_rollout_tape_feedback (the ADJ_FB instantiations of the forward kernel; u is the feed-forward uff there)
    const double* fbK;        // [nsteps][2 nr nr] or [B][..]: du_i/dx_j of step k at row k-1, entry j*nr + i, x = (q, qdot); null: no feedback
    const double* fbx;        // [nsteps][2 nr] or [B][..]: row k-1 the reference (q, qdot) for the state at the start of step k; null: zero
    size_t fb_stride;         // rows (steps) from one rollout's tables to the next: nsteps, or 0 for tables the batch shares
    double* uapp;             // [B][nsteps][nr] the torque applied in every step (out), or null
    // rmx_rollout_vjp_feedback (k_rollout_bwd_fb, rmx_feedback_bwd.h: fbK, fbx, fb_stride as above; dPdu is duff and may be null there)
    const double* gu;         // [B][nsteps][nr] the cotangent of the applied torque, or null: zero
    double* dK;               // [B][nsteps][2 nr nr] one table per rollout (out), or null
    double* dxref;            // [B][nsteps][2 nr] one row per rollout (out), or null
    const double *fq0, *fqd0; // [B][nr] the state the tape started from (its parts Q0, QD0 of rmx_tape.h): read for dK alone
    const double *fqt, *fqdt; // [B][nsteps][nr] the tape's trajectory (parts QT, QDT): read for dK alone
    // rmx_rollout_tape_feedback_box (the ADJ_FB instantiations of the forward kernel alone read these)
    const double *ulo, *uhi;  // [nr] the torque limits the applied torque is clamped into, or null: that side is skipped
};

// rmx_rollout_vjp_params (rmx_params.h): one wavefront per rollout walks the slots of its tape
struct ParamArgs {
    int nsteps, nslots;       // nslots per rollout: nsteps (BDF1) or nsteps + 1 (BDF2: slot nsteps holds the SDIRK2a solve)
    int bdf2;                 // the tape's integrator
    int njoints;              // joints / bodies in the caller's listing (the rows of `inertia`)
    double h;                 // the tape's
    const double *q0, *qd0;   // [B][nr] the state the tape started from
    const double *qt, *qdt;   // [B][nsteps][nr] q, qdot after every step
    const double* zs;         // [B][nslots][n] z of every slot (AdjArgs::zs)
    double *stiffness, *damping, *qrest;   // [B][nr] reduced DOF order; null: not wanted
    double* inertia;          // [B][njoints][6] listing order; null: not wanted
    double* grav;             // [B][3]; null: not wanted
    short lst[MAXN];          // listing index of the body each node carries, -1: none (the inner nodes of a lowered multi-DOF joint)
};

// rmx_rollout_vjp_forces (rmx_force_params.h): one wavefront per rollout walks the slots of its tape, as above
struct ForceArgs {
    int nsteps, nslots;       // nslots per rollout: nsteps (BDF1) or nsteps + 1 (BDF2: slot nsteps holds the SDIRK2a solve)
    int bdf2;                 // the tape's integrator
    double h;                 // the tape's
    const double *q0, *qd0;   // [B][nr] the state the tape started from
    const double *qt, *qdt;   // [B][nsteps][nr] q, qdot after every step
    const double* zs;         // [B][nslots][n] z of every slot (AdjArgs::zs)
    double *stiffness, *damping, *L;   // [B][nforces] in the order of the force table; null: not wanted
};

// rmx_rollout_linearize (rmx_linearize.h): one wavefront per (rollout, slot) of the tape
struct LinArgs {
    int nslots;               // per rollout: nsteps (BDF1) or nsteps + 1 (BDF2: slot nsteps holds the SDIRK2a solve)
    int bdf2;                 // the tape's integrator: eta per slot
    double h, pscale;         // the tape's
    const double *Hs, *Ms, *Ds;   // [B][nslots][n*n], entry (row r, column c) at c*n + r
    double *XA, *XB, *XU;     // [B][nslots][nr*nr], entry j*nr + i = dx_i/d(.)_j in reduced order; null: not wanted
};

// rmx_rollout_jvp (rmx_jvp.h): one wavefront per (rollout, chunk of JVP_CHUNK tangent directions) walks the slots of the tape forwards
constexpr int JVP_CHUNK = 8;     // tangent directions per wavefront (rmx_jvp.h JVP_TW: the register budget at 64 lanes)
struct JvpArgs {
    int nsteps, nslots;       // nslots per rollout: nsteps (BDF1) or nsteps + 1 (BDF2: slot nsteps holds the SDIRK2a solve)
    int bdf2;                 // the tape's integrator
    int ntan, nchunks;        // tangent directions per rollout, and the chunks of JVP_CHUNK they make: the grid is B * nchunks
    double h, pscale;         // the tape's
    const double *Hs, *Ms, *Ds;   // [B][nslots][n*n], entry (row r, column c) at c*n + r
    const double* tu;         // [B][ntan][nsteps][nr], or null: zero
    const double *tq0, *tqd0; // [B][ntan][nr], or null: zero
    double *tq, *tqd;         // [B][ntan][nsteps][nr] (out)
    const double* r;          // rmx_rollout_jvp_params (the RHS instantiation alone reads it): [B][ntan][nslots][n], node order
};

// rmx_rollout_jvp_params (rmx_jvp_params.h): one wavefront per (rollout, slot) of the tape forms r = (dg/dtheta) ttheta of every direction
struct ParamRhsArgs {
    int nsteps, nslots;       // nslots per rollout: nsteps (BDF1) or nsteps + 1 (BDF2: slot nsteps holds the SDIRK2a solve)
    int bdf2;                 // the tape's integrator
    int njoints;              // joints / bodies in the caller's listing (the rows of `inertia`)
    int ntan;                 // tangent directions per rollout
    double h;                 // the tape's
    const double *q0, *qd0;   // [B][nr] the state the tape started from
    const double *qt, *qdt;   // [B][nsteps][nr] q, qdot after every step
    const double *stiffness, *damping, *qrest;   // [B][ntan][nr] reduced DOF order; null: zero
    const double* inertia;    // [B][ntan][njoints][6] listing order; null: zero
    const double* grav;       // [B][ntan][3]; null: zero
    double* r;                // [B][ntan][nslots][n] (out), node order
    short lst[MAXN];          // as ParamArgs::lst
};

// rmx_rollout_lqr (rmx_lqr.h): one workgroup per rollout walks the slots of its BDF1 tape backwards
struct LqrArgs {
    int nsteps;               // of the tape (BDF1: one slot per step)
    double h, pscale;         // the tape's
    double mu;                // the regulariser of Quu where mu_b is null
    const double *Hs, *Ms, *Ds;   // [B][nsteps][n*n], entry (row r, column c) at c*n + r
    const double *lx, *lu;    // [B][nsteps][2 nr], [B][nsteps][nr]
    const double* Q;          // [nsteps][2nr * 2nr] or [B][..], column-major
    size_t q_stride;          // doubles from one rollout's Q table to the next (0: one table for the batch)
    const double* R;          // [nr * nr]
    const double* mu_b;       // [B] or null
    double *kff, *K;          // [B][nsteps][nr], [B][nsteps][2 nr nr] (entry j*nr + i of a row: du_i/dx_j)
    double* expected;         // [B] or null
    int* status;              // [B] or null
    // rmx_rollout_lqr_box (the BOX instantiations alone read these)
    const double *ulo, *uhi;  // [nr] the torque limits, or null: that side is unbounded
    const double* ubar;       // [B][nsteps][nr] the nominal applied torques: the QP of step k is over ulo - ubar_k <= x <= uhi - ubar_k
    int max_iter;             // >= 1: the cap on the QP iterations of a step
    unsigned* clamped;        // [B][nsteps] or null: bit i of row k-1 is set where DOF i of step k ended on a bound
};

// rmx_rollout_points / rmx_rollout_cost / rmx_rollout_frames / rmx_rollout_cost_frames (rmx_cost.h): one wavefront per (rollout,
// step) of a state record.  A point term is a frame term with wvel = wrot = 0; the point instantiation reads neither them nor the
// arrays marked (frames).
struct FrameDevTerm {
    rmx_track::DevTerm t;     // the point, its node, wpos and the term's position in the caller's array
    double wvel, wrot;
};
static_assert(sizeof(FrameDevTerm) == 56, "FrameDevTerm: a DevTerm and two doubles, no padding");
struct TaskArgs {
    int nsteps, nterms;
    const double *q, *qd;     // [B][nsteps][nr] the record (qd may be null where no velocity is asked for)
    const FrameDevTerm* trk;  // [nterms] the terms sorted by step (rmx_track.h), or null: no terms
    const int* trk_begin;     // [nsteps + 1] step k owns terms trk_begin[k-1] .. trk_begin[k]-1, or null
    const double *xt, *vt, *Rt;   // targets [nterms][3], [nterms][3], [nterms][9] (column-major) or [B][..], indexed by the term's position
                              // in the caller's array; null: no term weighs it (vt, Rt: frames)
    size_t t_stride;          // TERMS from one rollout's target tables to the next (0: one table for the batch)
    const double* Qin;        // [nsteps][2nr * 2nr] or [B][..], column-major, or null: zero
    size_t q_stride;          // doubles from one rollout's Q table to the next (0: one table for the batch)
    const double* xgoal;      // [nsteps][2nr] or [B][..], or null: zero
    size_t goal_stride;
    double *Jk, *lx, *Qout;   // [B][nsteps], [B][nsteps][2nr], [B][nsteps][2nr * 2nr]; null: not wanted
    double *x, *v, *R;        // [B][nterms][3], [B][nterms][3], [B][nterms][9] (rmx_rollout_points: x; rmx_rollout_frames), or null
    const double *gx, *gv, *gR;   // their cotangents, or null: zero (gv, gR: frames)
    double *gq, *gqd;         // [B][nsteps][nr], or null (gqd: frames)
};

// rmx_rollout_search (rmx_search.h): one wavefront per rollout runs the trial passes and the nominal pass of the line search
struct SearchArgs {
    AdjArgs a;                // the closed-loop sweep's, as rmx_rollout_tape_feedback_box fills it: u is the nominal torque ubar; qtraj and
                              // qdtraj are never null here (without a caller's record: the tape's own rows)
    const double* kff;        // [B][nsteps][nr] the search direction, or null with nalpha == 0
    const double* Jbar;       // [B] the cost a trial has to beat, or null with nalpha == 0
    int nalpha;               // 0 .. RMX_SEARCH_MAX_ALPHAS
    double alphas[RMX_SEARCH_MAX_ALPHAS];
    TaskArgs c;               // the cost: trk, trk_begin, xt, vt, Rt, t_stride, Qin, q_stride, xgoal, goal_stride (no record, no outputs)
    const double* R;          // [nr * nr] or null: no control cost
    double *J, *alpha;        // [B]; alpha may be null
    int *trials, *sstatus;    // [B], or null
};

struct rmx_model {
    int device = 0;
    int n = 0, nr = 0, nm = 0, NP = 0;   // n: 1-DOF nodes on the device (after lowering multi-DOF joints)
    int nlist = 0;                      // joints/bodies in the caller's listing
    std::vector<int> idx_listing;   // reduced index per LISTED joint (-1 fixed)
    std::vector<int> node_of_listing;   // depth-first node index of each LISTED joint/body
    void* dbuf = nullptr;           // one device allocation holding all constant arrays
    void* dcon = nullptr;           // contact flags + cuboid sides (rmx_model_set_ground_contact)
    void* dsph = nullptr;           // axis variants of the spherical group nodes
    DevModel dm{};
    size_t smem_bytes = 0;
    int n_simd = 0;                 // SIMDs of the device (4 per CU)
    unsigned long long coop_ticks = 5000000000ull;   // ~2 s in s_memtime ticks of this device (DevOpts::coopTicks): measured at model creation
    int lds_limit = 0;              // LDS bytes one workgroup may hold (hipDeviceProp_t::sharedMemPerBlock); RMX_BIG_LDS_LIMIT overrides
    void* dgconst = nullptr;        // 64-lane plain models: the staged per-node constants in global memory (DevModel::gconst)
    int gconst_min_batch = 0;       // batches of at least this many rollouts run the global-constants kernels (0: never)
    int w2_max_batch = 0;           // 33..64-node trees / the full 32-link chain: batches of up to this many rollouts take two wavefronts each (0: never; RMX_W2_MAX)
    int adj_help_max_batch = 0;     // trees of <= 16 nodes: adjoint batches of up to this many rollouts take a second wavefront each for M, D (part_adjhelp16.hip; 0: never)
    int w2_min_batch = 0;           // the full 32-link chain: ... and of at least this many (RMX_W2C_MIN; smaller batches keep the one-wave kernel every test pins)
    void* dpf = nullptr;            // body-to-body forces (rmx_model_set_point_forces): the PfTable of rmx_pf.h on the device, or null
    int npf = 0;                    // ... and the number of its rows (the rows of rmx_force_grads)
    bool tape_pf = false;           // rmx_model_tape_point_forces: the four tape entries take the model while it has a force table
    bool big = false;               // more than 64 nodes: the one-workgroup-per-tree kernels of rmx_big.hip
    std::vector<struct rmx_batch*> batches;   // live batches of this model (rmx_model_set_ground_contact drains their streams only)
};

struct rmx_batch {
    rmx_model* m = nullptr;
    int B = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double *q = nullptr, *qd = nullptr, *qp = nullptr, *qdp = nullptr;
    double *tmpA = nullptr, *tmpB = nullptr, *tmpC = nullptr;   // [B][nr] scratch for rmx_eval inputs
    int* started = nullptr;
    int* chart = nullptr;           // [B][nsph] current Euler chart of every spherical joint (JointSpherical.chart), 1..12
    int *it = nullptr, *ls = nullptr, *status = nullptr;
    int* resume = nullptr;          // [B] see StepArgs.resume
    int started_host = -1;          // what the device flag `started` holds (-1: not known): a step call rewrites it only when it changes
    int* park = nullptr;            // see StepArgs.park / xch (allocated for models whose steps can park: rmx_model::coop)
    unsigned* xch = nullptr;
    unsigned long long* xrec = nullptr;
    void* gargs = nullptr;          // RMX_GARGS_BYTES: the arguments of the fused ground launch (part_ground32.hip GroundArgs)
    int ngroups = 0;
    unsigned long long* ticks = nullptr;   // [B] see StepArgs.ticks (rmx_step_ticks)
    double* bigws = nullptr;        // trees of more than 64 nodes: per-rollout workspace of the rmx_big.hip kernels
    size_t bigws_stride = 0;        // doubles per rollout
    void* adjws = nullptr;          // rmx_adjoint_*: H, M, D of every step and rollout, dP/dq, P, dP/dp - one allocation that is kept
    size_t adjws_bytes = 0;         // between calls and only ever grows (hipMalloc + hipFree of 3 x 20 MB cost more than the kernels)
    int tape_nsteps = 0;           // rmx_rollout_tape: steps of the tape H, M, D in adjws hold (0: none - every rmx_adjoint_* call rewrites them)
    int tape_integ = 0;             // ... the integrator that recorded it (INTEG_BDF2: nsteps + 1 slots per rollout, rmx_rollout_tape_bdf2)
    double tape_h = 0.0, tape_pscale = 0.0;   // ... and the step size and torque scale it was recorded with
    bool tape_pf = false;           // ... and whether its H and D carry point forces (rmx_tape_pf.h): rmx_rollout_vjp_params refuses it then
    double last_ms = 0.0;
    const char* last_kernel = "";   // label of the step kernel the last step call launched (rmx_last_step_kernel; StepPlan::label)
    bool async_pending = false;     // an rmx_step_*_async launch nobody has waited for yet (see pending_error_check)
    // per-step record of the last step call (Scene.saveHistory): device buffers, kept until the next step call so that an
    // asynchronous launch can be read back after rmx_sync (rmx_history_read)
    struct Hist {
        double *T = nullptr, *V = nullptr;      // [nsteps][B]
        double *Q = nullptr, *Qd = nullptr;     // [nsteps][B][nr]
        int* C = nullptr;                       // [nsteps][B][nsph]
        int nsteps = 0;
    } hist;                                     // the record of the last step call: null = that part was not recorded
    // The device buffers behind `hist` live on the batch and only grow: no hipFree (device-synchronising) sits between the launches
    // of shards that share a device, and a step call never pulls a buffer from under a launch still in flight.
    struct HistPool {
        double *T = nullptr, *V = nullptr, *Q = nullptr, *Qd = nullptr;
        int* C = nullptr;
        size_t capH = 0, capQ = 0, capC = 0;    // elements
    } hpool;
    // rmx_rollout_points / rmx_rollout_cost: the term table and its step offsets on the device - an allocation of its own that only
    // grows (the adjoint workspace holds the tape, which these calls must leave alone)
    void* costws = nullptr;
    size_t costws_bytes = 0;
};

// launchers defined by the multi-size parts (part_plain / part_ct / part_fullchain / part_pf / part_tape_pf .hip) for one RMX_NP each
#define RMX_CAT_(a, b) a##b
#define RMX_CAT(a, b) RMX_CAT_(a, b)
#define RMX_DECLARE_LAUNCHERS(NPV) \
    void RMX_CAT(launch_eval_, NPV)(const rmx_model* m, const rmx_batch* b, bool wantH, double eta, double* dg, double* dH); \
    void RMX_CAT(launch_step_plain_, NPV)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a); \
    void RMX_CAT(launch_euler_, NPV)(const rmx_model* m, const rmx_batch* b, double h, const StepArgs& a); \
    void RMX_CAT(launch_energy_, NPV)(const rmx_model* m, const rmx_batch* b, double* dT, double* dV); \
    void RMX_CAT(launch_adjoint_, NPV)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a); \
    void RMX_CAT(launch_rollout_feedback_, NPV)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a); \
    void RMX_CAT(launch_vjp_feedback_, NPV)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a); \
    void RMX_CAT(launch_linearize_, NPV)(const rmx_model* m, const rmx_batch* b, const LinArgs& a); \
    void RMX_CAT(launch_jvp_, NPV)(const rmx_model* m, const rmx_batch* b, const JvpArgs& a); \
    void RMX_CAT(launch_jvp_params_, NPV)(const rmx_model* m, const rmx_batch* b, const ParamRhsArgs& p, const JvpArgs& a); \
    void RMX_CAT(launch_cost_, NPV)(const rmx_model* m, const rmx_batch* b, const TaskArgs& a, bool frames); \
    void RMX_CAT(launch_vjp_zs_, NPV)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a, bool fullchain); \
    void RMX_CAT(launch_param_grad_, NPV)(const rmx_model* m, const rmx_batch* b, const ParamArgs& a); \
    void RMX_CAT(launch_phase_, NPV)(const rmx_model* m, const rmx_batch* b, int reps, double h, unsigned long long* d); \
    void RMX_CAT(launch_mfd_, NPV)(const rmx_model* m, const rmx_batch* b, double* dM, double* df, double* dD); \
    void RMX_CAT(launch_mfd_ct_, NPV)(const rmx_model* m, const rmx_batch* b, double* dM, double* df, double* dD); \
    void RMX_CAT(launch_eval_ct_, NPV)(const rmx_model* m, const rmx_batch* b, bool wantH, double eta, double* dg, double* dH); \
    void RMX_CAT(launch_step_ct_, NPV)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a, bool contact_pass); \
    void RMX_CAT(launch_energy_ct_, NPV)(const rmx_model* m, const rmx_batch* b, double* dT, double* dV); \
    void RMX_CAT(launch_step_fullchain_, NPV)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a); \
    void RMX_CAT(launch_eval_pf_, NPV)(const rmx_model* m, const rmx_batch* b, bool wantH, double eta, double* dg, double* dH); \
    void RMX_CAT(launch_step_pf_, NPV)(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a); \
    void RMX_CAT(launch_energy_pf_, NPV)(const rmx_model* m, const rmx_batch* b, double* dT, double* dV); \
    void RMX_CAT(launch_tape_pf_, NPV)(const rmx_model* m, const rmx_batch* b, int integ, bool feedback, const DevOpts& o, const AdjArgs& a); \
    void RMX_CAT(launch_force_grad_, NPV)(const rmx_model* m, const rmx_batch* b, const ForceArgs& a);
// The one-size step launchers (StepKernel of rmx_select.h; the bools are StepPlan's instantiation flags)
// part_gconst64.hip: 64-lane plain step kernels reading the per-node constants from global memory, and the staging kernel (part_plain.hip)
void launch_step_gconst_64(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a, bool fulln);
void launch_stage_consts_64(const rmx_model* m, double* dst, hipStream_t stream);
// part_fullchain.hip: a tree that fills all 64 node slots
void launch_step_fulln_64(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a);
// part_w2_tree64.hip / part_w2_chain32.hip: two wavefronts per rollout - 33..64-node trees, the full 32-link chain under BDF1
void launch_step_w2_64(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a, bool fullchain, bool fulln, bool energy);
void launch_step_w2c_32(const rmx_model* m, const rmx_batch* b, const DevOpts& o, const StepArgs& a);
// part_pair32.hip: the full 32-link chain, BDF1, two points per evaluation (rmx_pair32.h)
void launch_step_pairchain_32(const rmx_model* m, const rmx_batch* b, const DevOpts& o, const StepArgs& a, bool energy);
void launch_phase_pairchain_32(const rmx_model* m, const rmx_batch* b, int reps, double h, unsigned long long* d);
// part_ground32.hip (32 lanes): serial chains with ground contact, the kernels around newton_pair (rmx_ct32.h).  ground: the whole call in
// k_ground32 (StepArgs::fused 1, 2, 3); pair: the steps with the contact terms behind the lean launch of launch_step_ct_32 (fused 0).
// Both end with the cooperative launch that finishes the rollouts they parked, where the call parks (StepArgs::park).
void launch_step_ground_32(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a);
void launch_step_pair_32(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a);
// the adjoint pair for trees of <= 16 nodes: part_adjhelp16.hip (a second wavefront per rollout for M, D), and part_plain.hip's full 16-link chain
void launch_adjoint_help_16(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a, bool fullchain);
void launch_adjoint_fullchain_16(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const AdjArgs& a);
// rmx_big.hip: trees of 65..BIG_MAXN nodes, one workgroup per rollout
size_t big_ws_doubles(const rmx_model* m);
void launch_big_step(const rmx_model* m, const rmx_batch* b, int integ, const DevOpts& o, const StepArgs& a);
void launch_big_eval(const rmx_model* m, const rmx_batch* b, bool wantH, double eta, double* dg, double* dH);
void launch_big_energy(const rmx_model* m, const rmx_batch* b, double* dT, double* dV);
// part_plain.hip: the Riccati sweep over the tape (rmx_lqr.h), the padded sizes its LDS-resident kernel exists for (select_rollout_lqr)
void launch_lqr_4(const rmx_model* m, const rmx_batch* b, const LqrArgs& a, size_t lds_bytes);
void launch_lqr_8(const rmx_model* m, const rmx_batch* b, const LqrArgs& a, size_t lds_bytes);
void launch_lqr_16(const rmx_model* m, const rmx_batch* b, const LqrArgs& a, size_t lds_bytes);
void launch_lqr_32(const rmx_model* m, const rmx_batch* b, const LqrArgs& a, size_t lds_bytes);
// ... and its box-constrained form (k_rollout_lqr<NP, true>; select_rollout_lqr_box)
void launch_lqr_box_4(const rmx_model* m, const rmx_batch* b, const LqrArgs& a, size_t lds_bytes);
void launch_lqr_box_8(const rmx_model* m, const rmx_batch* b, const LqrArgs& a, size_t lds_bytes);
void launch_lqr_box_16(const rmx_model* m, const rmx_batch* b, const LqrArgs& a, size_t lds_bytes);
void launch_lqr_box_32(const rmx_model* m, const rmx_batch* b, const LqrArgs& a, size_t lds_bytes);
// ... and the line search that follows it (k_rollout_search<NP>, rmx_search.h; select_rollout_search: the same sizes)
void launch_search_4(const rmx_model* m, const rmx_batch* b, const DevOpts& o, const SearchArgs& a, int block);
void launch_search_8(const rmx_model* m, const rmx_batch* b, const DevOpts& o, const SearchArgs& a, int block);
void launch_search_16(const rmx_model* m, const rmx_batch* b, const DevOpts& o, const SearchArgs& a, int block);
void launch_search_32(const rmx_model* m, const rmx_batch* b, const DevOpts& o, const SearchArgs& a, int block);
RMX_DECLARE_LAUNCHERS(4)
RMX_DECLARE_LAUNCHERS(8)
RMX_DECLARE_LAUNCHERS(16)
RMX_DECLARE_LAUNCHERS(32)
RMX_DECLARE_LAUNCHERS(64)
