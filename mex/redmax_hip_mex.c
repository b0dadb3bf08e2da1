/*
 * redmax_hip_mex.c -- MATLAB MEX gateway onto the C ABI of include/redmax_hip.h.
 *
 * The reference (sueda/redmax, matlab-diff) runs simLoop / newton / evalBDF1 / computeValues inside the MATLAB
 * interpreter (driverRedMaxBDF1.m:57-243).  This gateway is the thin layer BASELINE.json's north_star names: MATLAB keeps the
 * +redmax Scene/Joint/Body classes and the driverRedMaxBDF1(sceneID,batch) entry point, and the body of simLoop becomes
 * calls into libredmax_hip.so.  The MATLAB callers are matlab/+redmax/HipSim.m (handle wrapper), matlab/+redmax/flattenScene.m
 * (Scene -> rmx_model_desc arrays) and matlab/driverRedMaxBDF1.m / driverRedMaxBDF2.m.
 *
 *   mex -I../include redmax_hip_mex.c -L../redmax_amd -lredmax_hip          (inside MATLAB, R2018a+ for the C matrix API used)
 *
 * MATLAB is not available in the build environment: the file is compiled and EXECUTED against mex/stub/ (a minimal
 * implementation of the mx and mex functions used here) by tests/test_mex_gateway.py.
 *
 * Commands (first argument is the command string).  Array shapes are MATLAB's; the ABI's row-major [batch][nr] is the
 * column-major nr x batch MATLAB matrix, [nsteps][batch] is batch x nsteps, [nsteps][batch][nr] is nr x batch x nsteps, 4x4
 * transforms are column-major on both sides, so no transposition happens anywhere.
 *
 *   v            = redmax_hip_mex('version')
 *   n            = redmax_hip_mex('devices')
 *   h            = redmax_hip_mex('create', desc, batch [, devices])    desc: struct, see cmd_create() below.  devices: a device index
 *                  or a VECTOR of them (default 0).  The batch is split into one contiguous shard per listed device (sizes differ by at
 *                  most one; a device may be listed twice); every array below is the WHOLE batch, the gateway scatters / gathers
 *                  (rmx_group_*).  BASELINE.json north_star: "the batch axis shards across GPUs", host = MATLAB.
 *                  redmax_hip_mex('destroy', h)
 *   info         = redmax_hip_mex('info', h)                            struct nr, nm, nsph, batch, idxR (0-based, -1 fixed),
 *                                                                       nshards, devices, shard_first (0-based), shard_count
 *                  redmax_hip_mex('set', h, q, qdot)                     nr x B each          Joint.setQ   (Joint.m:231-292)
 *   [q, qdot]    = redmax_hip_mex('get', h)                                                   Joint.getQ   (Joint.m:173-229)
 *   [T,V,st,Q,Qd,C]= redmax_hip_mex('step', h, itype, hstep, nsteps [, opts])
 *                  itype 1: simLoop of driverRedMaxBDF1.m:57-91, 2: of driverRedMaxBDF2.m:57-125.  T, V: B x nsteps
 *                  (Scene.saveHistory energies); st: B x 3 int32 [newton iterations, line-search halvings, RMX_ST_* bits];
 *                  Q, Qd (only when requested): nr x B x nsteps, the full Scene.saveHistory record (Scene.m:134-161);
 *                  C (only when requested): nsph x B x nsteps int32, the Euler chart of every spherical joint after each step.
 *                  opts: struct with any of tol, dxMax, iterMaxPerDof, iterLsMax, lu_mode, compensated, ls_fail_limit (driverRedMaxBDF1.m:95-98).
 *                  All shards' kernels are launched before the first one is waited for: N devices run concurrently.
 *                  redmax_hip_mex('step_async', h, itype, hstep, nsteps [, opts [, record]])
 *                  the same launch without the wait: MATLAB gets control back while the devices step (several handles can be in
 *                  flight).  record: bit mask of what Scene.saveHistory keeps on the device, 1 = T, V (default), 2 = Q, Qdot, 4 = C.
 *   [T,V,st,Q,Qd,C]= redmax_hip_mex('sync', h)
 *                  waits for the launches of the last 'step_async' and gathers; outputs beyond what `record` asked for are an error.
 *   [wall,k,t0,t1] = redmax_hip_mex('timing', h)                         rmx_group_timing of the last step: wall clock ms, and per shard
 *                  (1 x nshards) kernel ms, start and end of its launch relative to the first shard on the same device
 *   [T, V]       = redmax_hip_mex('euler', h, hstep, nsteps)             matlab-simple/testRedMax.m:67-109
 *   [g, H]       = redmax_hip_mex('eval', h, q, qA, qB, eta)             evalBDF1 & co (driverRedMaxBDF1.m:160-187); H: nr x nr x B
 *   [T, V]       = redmax_hip_mex('energy', h)                           Joint/Body.computeEnergies
 *   c            = redmax_hip_mex('getcharts', h)                        nsph x B int32, JointSpherical.chart
 *                  redmax_hip_mex('setcharts', h, c)
 *   [P,dPdp,st]  = redmax_hip_mex('adjoint', h, hstep, nsteps, task, p [, integrator])  taskObjective of
 *                  driverRedMaxAdjointBDF1.m:39-62 (integrator 1, default) or driverRedMaxAdjointBDF2.m:38-62 (integrator 2);
 *                  task: struct body (1-based listing index), xlocal, xtarget, step, pscale, wreg, wpos; p: nr x B;
 *                  st: B x 2 int32 [newton iterations, status]
 *   [P,dPdu,st]  = redmax_hip_mex('adjoint_controls', h, hstep, nsteps, task, u [, integrator])  rmx_adjoint_controls: one torque
 *                  per joint and step.  u, dPdu: nr x nsteps x B (the ABI's [B][nsteps][nr]); task, integrator, st as 'adjoint'.
 *                  With one output the forward sweep runs alone (P of a controlled rollout, no gradient).
 *   [P,dPdu,st]  = redmax_hip_mex('adjoint_track', h, hstep, nsteps, task, u [, integrator])  rmx_adjoint_track: the same with point
 *                  targets on several bodies at several steps.  task: struct terms (struct array: body 1-based, xlocal, step, wpos),
 *                  xtarget (3 x nterms, or 3 x nterms x B: one target table per rollout), pscale, wreg; u, dPdu, st, the one-output
 *                  form as 'adjoint_controls'.
 *   [qtraj,qdtraj,st] = redmax_hip_mex('rollout_tape', h, hstep, nsteps, pscale, u [, integrator])  rmx_rollout_tape: a controlled BDF1
 *                  rollout from the current state under the torques tau + pscale*u(:,k,b) that records its trajectory and keeps the
 *                  tape 'rollout_vjp' reads.  u, qtraj, qdtraj: nr x nsteps x B; column k is the state after step k; st as 'adjoint'.
 *                  integrator (default 1) 2: rmx_rollout_tape_bdf2, the BDF2 rollout, self-started with SDIRK2 (step 1).
 *   [qtraj,qdtraj,uapp,st] = redmax_hip_mex('rollout_feedback', h, hstep, nsteps, pscale, uff, K, xref [, integrator])
 *                  rmx_rollout_tape_feedback: 'rollout_tape' in closed loop - the torque of step k is uapp(:,k,b) = uff(:,k,b) +
 *                  K(:,:,k)*(x - xref(:,k)) with x = [q; qdot] at the START of step k, formed on the device.  uff: nr x nsteps x B.
 *                  K: nr x 2nr x nsteps (shared) or nr x 2nr x nsteps x B, K(i,j,k) = du_i/dx_j; xref: 2nr x nsteps [x B]; [] for
 *                  either: no feedback / a zero reference.  uapp: the applied torques.  The tape is the open-loop tape under uapp.
 *   [du,dq0,dqd0] = redmax_hip_mex('rollout_vjp', h, nsteps, gq, gqd)  rmx_rollout_vjp on the tape of the last 'rollout_tape': gq, gqd
 *                  (nr x nsteps x B) are dL/dq and dL/dqdot of every step; du (nr x nsteps x B), dq0, dqd0 (nr x B) are dL/du,
 *                  dL/dq0, dL/dqdot0.  May be repeated with other cotangents; any 'adjoint*' command ends the tape.
 *   [XA,XB,XU] = redmax_hip_mex('rollout_linearize', h, nsteps)  rmx_rollout_linearize on the tape of the last 'rollout_tape': the
 *                  sensitivities dx/dqA, dx/dqB, dx/du of every taped solve, nr x nr x nslots x B with (i,j,s,b) = dx_i/d(.)_j of slot s
 *                  (nslots = nsteps, or nsteps + 1 after a BDF2 'rollout_tape': the last slot is the SDIRK2a solve).  Outputs that are
 *                  not asked for are not computed.  include/redmax_hip.h has the assembly of A_k, B_k from them.
 *   [du,dq0,dqd0,dk,dd,dqrest,dI,dgrav] = redmax_hip_mex('rollout_vjp_params', h, nsteps, gq, gqd)  rmx_rollout_vjp_params on the tape
 *                  of the last 'rollout_tape': 'rollout_vjp' (the same du, dq0, dqd0) and the gradient of the loss with respect to
 *                  the model's parameters, one column per rollout: joint stiffness dk, damping dd and rest position dqrest (nr x B,
 *                  reduced DOF order), body inertia dI (6 x njoints x B, the layout of desc.I_i) and gravity dgrav (3 x B).  The
 *                  gradient of a parameter the rollouts share is the sum over B.
 *   [du,dq0,dqd0,dks,dkd,dL,dk,dd,dqrest,dI,dgrav] = redmax_hip_mex('rollout_vjp_forces', h, nsteps, gq, gqd, nforces)
 *                  rmx_rollout_vjp_forces on a tape that carries point forces ('tape_point_forces'): 'rollout_vjp' (the same du, dq0,
 *                  dqd0), the gradient with respect to the stiffness dks, damping dkd and rest length dL of every force (nforces x B,
 *                  the order of the force table; nforces: its rows) and, where more than six outputs are asked for, the five arrays
 *                  of 'rollout_vjp_params' on such a tape.  The library refuses a tape without point forces.
 *   [tq,tqd] = redmax_hip_mex('rollout_jvp', h, nsteps, tu, tq0, tqd0)  rmx_rollout_jvp on the tape of the last 'rollout_tape': the
 *                  tangents of the whole trajectory, tq, tqd (nr x nsteps x ntan x B), for tangents of the controls tu (nr x nsteps x
 *                  ntan x B) and of the initial state tq0, tqd0 (nr x ntan x B); ntan directions per rollout, taken from the arrays'
 *                  sizes.  [] for any of the three: zero (not all three).
 *   [tq,tqd] = redmax_hip_mex('rollout_jvp_params', h, nsteps, tk, td, tqrest, tI, tgrav, tu, tq0, tqd0)  rmx_rollout_jvp_params on
 *                  the same tape: 'rollout_jvp' with tangents of the model's parameters - tk, td, tqrest (nr x ntan x B: stiffness,
 *                  damping, rest position per reduced DOF), tI (6 x njoints x ntan x B, the layout of desc.I_i) and tgrav (3 x ntan
 *                  x B).  [] for any of the eight: zero (not all five parameter arrays); ntan from the first non-empty array.
 *   [kff,K,expected,notpd] = redmax_hip_mex('rollout_lqr', h, nsteps, lx, lu, Q, R [, mu])  rmx_rollout_lqr on the BDF1 tape of the
 *                  last 'rollout_tape' / 'rollout_feedback': the Riccati sweep of iLQR.  lx (2nr x nsteps x B), lu (nr x nsteps x B):
 *                  the cost's gradients at the nominal; Q: 2nr x 2nr x nsteps (shared) or 2nr x 2nr x nsteps x B, R: nr x nr, both
 *                  symmetric; mu (default 0) regularises Quu.  kff: nr x nsteps x B; K: nr x 2nr x nsteps x B, K(i,j,k,b) = du_i/dx_j -
 *                  what 'rollout_feedback' takes; expected, notpd: 1 x B (notpd 1: Quu + mu I was not positive definite, zero gains).
 *   [qtraj,qdtraj,uapp,st] = redmax_hip_mex('rollout_feedback_box', h, hstep, nsteps, pscale, uff, K, xref, ulo, uhi [, integrator])
 *                  rmx_rollout_tape_feedback_box: 'rollout_feedback' with uapp clamped into ulo <= u <= uhi behind the feedback sum
 *                  (with K = [] too).  ulo, uhi: nr elements, or []: that side is unbounded.
 *   [kff,K,expected,status,clamped] = redmax_hip_mex('rollout_lqr_box', h, nsteps, lx, lu, Q, R, ubar, ulo, uhi [, mu [, max_iter]])
 *                  rmx_rollout_lqr_box: 'rollout_lqr' with the box QP of control-limited DDP at every step.  ubar (nr x nsteps x B):
 *                  the nominal applied torques; max_iter (default 0: 64) caps the QP iterations of a step.  status 1 x B: 0, 1 (a
 *                  pivot not > 0), 2 (a QP did not terminate); clamped nsteps x B: bit i set where DOF i ended on a bound.
 *   [x,gq] = redmax_hip_mex('rollout_points', h, nsteps, q, terms [, gx])  rmx_rollout_points: the world positions of body points
 *                  along a state record q (nr x nsteps x B, any record - typically a qtraj), x 3 x nterms x B, and with gx (3 x
 *                  nterms x B) the pull-back gq (nr x nsteps x B) = sum over the terms of a step of Jp'*gx.  terms: struct array
 *                  body (1-based), xlocal, step, as task.terms of 'adjoint_track' (a wpos is not read).  Needs no tape.
 *   [Jk,lx,Q] = redmax_hip_mex('rollout_cost', h, nsteps, q, qdot, Qin, xgoal, terms, xtarget)  rmx_rollout_cost: the cost of a
 *                  state record and its second-order model for 'rollout_lqr' - the joint-space quadratic Qin (2nr x 2nr x nsteps
 *                  [x B], symmetric) about xgoal (2nr x nsteps [x B]) plus point targets: terms (struct array body, xlocal, step,
 *                  wpos >= 0) and xtarget (3 x nterms [x B]).  [] for Qin, xgoal: zero; [] for terms: no targets.  Jk: nsteps x B;
 *                  lx: 2nr x nsteps x B, the exact gradient; Q: 2nr x 2nr x nsteps x B, Qin + sum w Jp'*Jp in the q block
 *                  (Gauss-Newton).  Outputs that are not asked for are not computed.  Needs no tape.
 *   [x,v,R,gq,gqd] = redmax_hip_mex('rollout_frames', h, nsteps, q, qdot, terms [, gx, gv, gR])  rmx_rollout_frames: position x and
 *                  point velocity v (3 x nterms x B) and orientation R (3 x 3 x nterms x B) of body frames along a state record
 *                  q, qdot (nr x nsteps x B), and with cotangents gx, gv (3 x nterms x B), gR (3 x 3 x nterms x B), [] for zero, the
 *                  pull-back gq = sum_t Jp'*gx + G'*gv + Jw'*a(gR*R'), gqd = sum_t Jp'*gv (nr x nsteps x B).  terms: struct array
 *                  body (1-based), xlocal, step (weights are not read).  Needs no tape.
 *   [qtraj,qdtraj,uapp,J,alpha,st] = redmax_hip_mex('rollout_search', h, hstep, nsteps, pscale, ubar, kff, K, xref, alphas, Jbar, cost [, ulo, uhi])
 *                  rmx_rollout_search: the backtracking line search of iLQR in one launch (BDF1) - every rollout runs the closed loop
 *                  of 'rollout_feedback' under ubar + a*kff for a in alphas, in order, keeps the first pass whose cost is below its
 *                  Jbar, else its nominal (uff = ubar).  alphas [] (then kff, Jbar may be []): the nominal pass alone.  cost: a struct
 *                  with the fields Q, xgoal, terms, xtarget, vtarget, Rtarget as 'rollout_cost_frames' takes them and R (nr x nr), each
 *                  optional.  J, alpha: 1 x B (alpha 0: none accepted); the record, uapp, st and the tape belong to the pass kept.
 *   [Jk,lx,Q] = redmax_hip_mex('rollout_cost_frames', h, nsteps, q, qdot, Qin, xgoal, terms, xtarget, vtarget, Rtarget)
 *                  rmx_rollout_cost_frames: 'rollout_cost' with frame terms - struct array body, xlocal, step and the weights wpos,
 *                  wvel, wrot >= 0 (a missing one is 0) - and the targets xtarget, vtarget (3 x nterms [x B]) and Rtarget (3 x 3 x
 *                  nterms [x B]); [] for a table no term weighs.  Per term wpos/2 |p - xtarget|^2 + wvel/2 |v - vtarget|^2 +
 *                  wrot/4 |R - Rtarget|_F^2; lx is the exact gradient, Q the Gauss-Newton table with the velocity terms' cross blocks.
 *   on = redmax_hip_mex('tape_point_forces', h, enable)  rmx_model_tape_point_forces on the model of every shard: enable 1, 'rollout_tape'
 *                  and 'rollout_feedback[_box]' take a model with point forces and leave a tape whose H and D carry them; 0 (the
 *                  default) restores their refusal.  A model without a force table is not affected.  on: the switch as read back.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "mex.h"
#include "redmax_hip.h"
#include "redmax_hip_profile.h"   /* 'timing' / 'ticks': measurement hooks, not part of the host-facing ABI */

typedef struct {
    uint64_t magic;
    rmx_group* g;          /* one model + batch per listed device */
    int nshards;
    int nr, nm, nsph, B, njoints;
    int pending_nsteps;    /* 'step_async' in flight: its nsteps and record mask ('sync' shapes its outputs from them) */
    int pending_record;
    int pending;
    int tape_integ;        /* the integrator of the last 'rollout_tape' (2: its tape has nsteps + 1 slots; 'rollout_linearize' shapes its outputs) */
} handle_t;

#define HANDLE_MAGIC 0x726d78686970ull /* "rmxhip" */
/* live handles: a handle value that MATLAB passes back is only dereferenced when it is in this table, so a stale or
 * made-up uint64 is an error message, not a crash */
#define MAX_LIVE 256
#define MAX_SHARDS 64
static handle_t* g_live[MAX_LIVE];
static int live_slot(const handle_t* h) {
    for (int i = 0; i < MAX_LIVE; ++i)
        if (g_live[i] == h) return i;
    return -1;
}

static void die_rmx(const char* what) { mexErrMsgIdAndTxt("redmax:hip", "%s: %s", what, rmx_last_error()); }
static void die(const char* msg) { mexErrMsgIdAndTxt("redmax:hip", "%s", msg); }

static const mxArray* field(const mxArray* s, const char* k, int required) {
    const mxArray* f = mxIsStruct(s) ? mxGetField(s, 0, k) : NULL;
    if ((!f || mxIsEmpty(f)) && required) mexErrMsgIdAndTxt("redmax:hip", "desc.%s is required", k);
    return (f && !mxIsEmpty(f)) ? f : NULL;
}
/* double array field with exactly `count` elements (NULL when optional and absent) */
static const double* f64(const mxArray* s, const char* k, size_t count, int required) {
    const mxArray* f = field(s, k, required);
    if (!f) return NULL;
    if (!mxIsDouble(f) || mxIsComplex(f)) mexErrMsgIdAndTxt("redmax:hip", "desc.%s must be a real double array", k);
    if (mxGetNumberOfElements(f) != count) mexErrMsgIdAndTxt("redmax:hip", "desc.%s must have %d elements", k, (int)count);
    return mxGetPr(f);
}
static const int* i32(const mxArray* s, const char* k, size_t count, int required) {
    const mxArray* f = field(s, k, required);
    if (!f) return NULL;
    if (!mxIsInt32(f)) mexErrMsgIdAndTxt("redmax:hip", "desc.%s must be an int32 array", k);
    if (mxGetNumberOfElements(f) != count) mexErrMsgIdAndTxt("redmax:hip", "desc.%s must have %d elements", k, (int)count);
    return (const int*)mxGetData(f);
}
static double scalar_field(const mxArray* s, const char* k, double dflt) {
    const mxArray* f = field(s, k, 0);
    return f ? mxGetScalar(f) : dflt;
}

static handle_t* get_handle(int nrhs, const mxArray* prhs[]) {
    if (nrhs < 2 || !mxIsUint64(prhs[1]) || mxGetNumberOfElements(prhs[1]) != 1) die("second argument must be the uint64 handle");
    handle_t* h = (handle_t*)(uintptr_t)(*(const uint64_t*)mxGetData(prhs[1]));
    if (!h || live_slot(h) < 0 || h->magic != HANDLE_MAGIC) die("stale or invalid handle");
    return h;
}
static const double* state_arg(const mxArray* a, const handle_t* h, const char* name) {
    if (!mxIsDouble(a) || mxIsComplex(a) || mxGetNumberOfElements(a) != (size_t)h->nr * (size_t)h->B)
        mexErrMsgIdAndTxt("redmax:hip", "%s must be a real double nr x batch (%d x %d) array", name, h->nr, h->B);
    return mxGetPr(a);
}
static mxArray* new_i32(size_t r, size_t c) { return mxCreateNumericMatrix(r, c, mxINT32_CLASS, mxREAL); }
/* the hooks without a group form run shard by shard, every array advanced to the shard's first trajectory */
static rmx_batch* shard(const handle_t* h, int s, size_t* first) {
    int f = 0;
    if (rmx_group_shard(h->g, s, NULL, &f, NULL)) die_rmx("rmx_group_shard");
    *first = (size_t)f;
    return rmx_group_shard_batch(h->g, s);
}
/* the rmx_stats of the shard that begins at rollout f: its rows of the B x 2 int32 output st = [newton iterations, status] */
static rmx_stats shard_stats(mxArray* st, const handle_t* h, size_t f) {
    int* sp = (int*)mxGetData(st);
    rmx_stats s;
    s.newton_iters = sp + f;
    s.ls_halvings = NULL;
    s.status = sp + h->B + f;
    return s;
}
/* the part of the shard that begins at rollout f of a table that is NULL, shared by the batch, or holds `per` doubles per rollout */
static const double* table_at(const double* t, int per_rollout, size_t f, size_t per) { return (t && per_rollout) ? t + f * per : t; }
/* the tail of a command: out[0] is returned always, out[i] where the caller asked for it, else destroyed (NULL: never made) */
static void give(int nlhs, mxArray* plhs[], mxArray* const out[], int n) {
    plhs[0] = out[0];
    for (int i = 1; i < n; ++i) {
        if (nlhs > i) plhs[i] = out[i];
        else if (out[i]) mxDestroyArray(out[i]);
    }
}

/* Scene.init() (Scene.m:59-119) -> rmx_model_create.  desc fields, joints in the scene's listing order (N = njoints):
 *   njoints; parent int32 1xN (0-based, -1 root); type int32 1xN (RMX_JOINT_*); axis 3xN; E0_pj, E0_ji 4x4xN; I_i 6xN;
 *   qRest, tau, stiffness, damping, qLimL, qLimU, qLimK, qLimD 1xN (optional: the Joint.m:77-83 defaults apply); grav 3x1;
 *   plane 6xN ([b1;b2] of JointPlanar, optional); qRestR nr x 1 (rest position of every DOF, optional);
 *   ground contact (optional, ForceGroundCuboid): contact int32 1xN, sides 3xN, groundE 4x4, kn, kt, mu, kd */
static void cmd_create(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    (void)nlhs;
    if (nrhs < 3) die("usage: h = redmax_hip_mex('create', desc, batch [, devices])");
    const mxArray* s = prhs[1];
    if (!mxIsStruct(s)) die("desc must be a struct (redmax.flattenScene)");
    const int batch = (int)mxGetScalar(prhs[2]);
    int devices[MAX_SHARDS] = {0};
    int ndev = 1;
    if (nrhs > 3 && !mxIsEmpty(prhs[3])) {     /* a device index or a vector of them: one shard per entry */
        if (!mxIsDouble(prhs[3]) || mxIsComplex(prhs[3])) die("devices must be a real double scalar or vector");
        const size_t nd = mxGetNumberOfElements(prhs[3]);
        if (nd > MAX_SHARDS) die("too many devices listed");
        ndev = (int)nd;
        for (int i = 0; i < ndev; ++i) devices[i] = (int)mxGetPr(prhs[3])[i];
    }
    rmx_model_desc d;
    memset(&d, 0, sizeof d);
    d.njoints = (int)scalar_field(s, "njoints", 0);
    if (d.njoints < 1) die("desc.njoints must be >= 1");
    const size_t n = (size_t)d.njoints;
    d.parent = i32(s, "parent", n, 1);
    d.type = i32(s, "type", n, 1);
    d.axis = f64(s, "axis", 3 * n, 1);
    d.E0_pj = f64(s, "E0_pj", 16 * n, 1);
    d.E0_ji = f64(s, "E0_ji", 16 * n, 1);
    d.I_i = f64(s, "I_i", 6 * n, 1);
    d.qRest = f64(s, "qRest", n, 0);
    d.tau = f64(s, "tau", n, 0);
    d.stiffness = f64(s, "stiffness", n, 0);
    d.damping = f64(s, "damping", n, 0);
    d.qLimL = f64(s, "qLimL", n, 0);
    d.qLimU = f64(s, "qLimU", n, 0);
    d.qLimK = f64(s, "qLimK", n, 0);
    d.qLimD = f64(s, "qLimD", n, 0);
    d.plane = f64(s, "plane", 6 * n, 0);
    memcpy(d.grav, f64(s, "grav", 3, 1), 3 * sizeof(double));
    {   /* qRestR has nr entries; nr is only known after lowering, so its length is checked against the DOF counts here */
        const mxArray* f = field(s, "qRestR", 0);
        if (f) {
            static const int ndof_of[] = {0, 1, 1, 2, 3, 2, 3, 3, 6};
            size_t nr = 0;
            for (size_t i = 0; i < n; ++i) {
                if (d.type[i] < 0 || d.type[i] > RMX_JOINT_FREE3D) die("desc.type holds an unknown joint type");
                nr += (size_t)ndof_of[d.type[i]];
            }
            d.qRestR = f64(s, "qRestR", nr, 1);
        }
    }
    /* every field of desc is read and validated BEFORE anything is created: a validation failure leaves through
     * mexErrMsgIdAndTxt (a longjmp out of the MEX function), which must not strand a device model or a persistent handle */
    const int has_contact = field(s, "contact", 0) != NULL;
    rmx_ground_contact gc;
    memset(&gc, 0, sizeof gc);
    if (has_contact) {   /* scene.forces holds ForceGroundCuboid objects (scenesRedMax.m:303-309) */
        gc.flags = i32(s, "contact", n, 1);
        gc.sides = f64(s, "sides", 3 * n, 1);
        memcpy(gc.E, f64(s, "groundE", 16, 1), 16 * sizeof(double));
        gc.kn = scalar_field(s, "kn", 1.0);   /* ForceGroundCuboid.m:22-26 defaults */
        gc.kt = scalar_field(s, "kt", 0.0);
        gc.mu = scalar_field(s, "mu", 0.0);
        gc.kd = scalar_field(s, "kd", 0.0);
        /* one frame / parameter set per force object (ForceGroundCuboid.m:6-13); absent: the shared values above */
        if (field(s, "groundE_body", 0)) gc.E_body = f64(s, "groundE_body", 16 * n, 1);
        if (field(s, "kn_body", 0)) gc.kn_body = f64(s, "kn_body", n, 1);
        if (field(s, "kt_body", 0)) gc.kt_body = f64(s, "kt_body", n, 1);
        if (field(s, "mu_body", 0)) gc.mu_body = f64(s, "mu_body", n, 1);
        if (field(s, "kd_body", 0)) gc.kd_body = f64(s, "kd_body", n, 1);
    }
    const int slot = live_slot(NULL);
    if (slot < 0) die("too many live handles (destroy some first)");
    handle_t* h = (handle_t*)mxCalloc(1, sizeof *h);
    mexMakeMemoryPersistent(h);
    if (rmx_group_create(&d, has_contact ? &gc : NULL, batch, devices, ndev, &h->g)) { mxFree(h); die_rmx("rmx_group_create"); }
    h->nshards = rmx_group_nshards(h->g);
    h->nr = rmx_model_nr(rmx_group_shard_model(h->g, 0));
    h->nm = rmx_model_nm(rmx_group_shard_model(h->g, 0));
    h->nsph = rmx_model_nsph(rmx_group_shard_model(h->g, 0));
    h->B = batch;
    h->njoints = d.njoints;
    h->magic = HANDLE_MAGIC;
    g_live[slot] = h;
    plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    *(uint64_t*)mxGetData(plhs[0]) = (uint64_t)(uintptr_t)h;
}

static void cmd_destroy(int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    g_live[live_slot(h)] = NULL;
    rmx_group_destroy(h->g);
    h->magic = 0;
    mxFree(h);
}

static void cmd_info(mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    static const char* names[] = {"nr", "nm", "nsph", "batch", "idxR", "nshards", "devices", "shard_first", "shard_count"};
    plhs[0] = mxCreateStructMatrix(1, 1, 9, names);
    mxSetField(plhs[0], 0, "nr", mxCreateDoubleScalar(h->nr));
    mxSetField(plhs[0], 0, "nm", mxCreateDoubleScalar(h->nm));
    mxSetField(plhs[0], 0, "nsph", mxCreateDoubleScalar(h->nsph));
    mxSetField(plhs[0], 0, "batch", mxCreateDoubleScalar(h->B));
    mxArray* idx = new_i32(1, (size_t)h->njoints);
    if (rmx_model_idxR(rmx_group_shard_model(h->g, 0), (int*)mxGetData(idx))) die_rmx("rmx_model_idxR");
    mxSetField(plhs[0], 0, "idxR", idx);
    mxSetField(plhs[0], 0, "nshards", mxCreateDoubleScalar(h->nshards));
    mxArray* dv = mxCreateDoubleMatrix(1, (size_t)h->nshards, mxREAL);
    mxArray* sf = mxCreateDoubleMatrix(1, (size_t)h->nshards, mxREAL);
    mxArray* sc = mxCreateDoubleMatrix(1, (size_t)h->nshards, mxREAL);
    for (int i = 0; i < h->nshards; ++i) {
        int dev = 0, first = 0, count = 0;
        if (rmx_group_shard(h->g, i, &dev, &first, &count)) die_rmx("rmx_group_shard");
        mxGetPr(dv)[i] = dev; mxGetPr(sf)[i] = first; mxGetPr(sc)[i] = count;
    }
    mxSetField(plhs[0], 0, "devices", dv);
    mxSetField(plhs[0], 0, "shard_first", sf);
    mxSetField(plhs[0], 0, "shard_count", sc);
}

static void read_opts(const mxArray* s, rmx_opts* o) {
    if (!s || mxIsEmpty(s)) return;
    if (!mxIsStruct(s)) die("opts must be a struct");
    o->tol = scalar_field(s, "tol", o->tol);
    o->dxMax = scalar_field(s, "dxMax", o->dxMax);
    o->iterMaxPerDof = (int)scalar_field(s, "iterMaxPerDof", o->iterMaxPerDof);
    o->iterLsMax = (int)scalar_field(s, "iterLsMax", o->iterLsMax);
    o->ls_fail_limit = (int)scalar_field(s, "ls_fail_limit", o->ls_fail_limit);
    o->lu_mode = (int)scalar_field(s, "lu_mode", o->lu_mode);
    o->compensated = (int)scalar_field(s, "compensated", o->compensated);
}

/* the outputs of 'step' / 'sync' for nsteps steps: T, V (B x K), st (B x 3 int32), and, when asked for, Q, Qd (nr x B x K) and
 * C (nsph x B x K int32); fills the rmx_stats / rmx_history that point into them */
typedef struct { mxArray *T, *V, *st, *Q, *Qd, *C; rmx_stats stats; rmx_history hist; } step_out_t;
static void step_outputs(const handle_t* h, int nsteps, int want_energy, int want_state, int want_charts, step_out_t* o) {
    const size_t B = (size_t)h->B, K = (size_t)nsteps;
    memset(o, 0, sizeof *o);
    o->T = mxCreateDoubleMatrix(B, want_energy ? K : 0, mxREAL);
    o->V = mxCreateDoubleMatrix(B, want_energy ? K : 0, mxREAL);
    o->st = new_i32(B, 3);
    int* sp = (int*)mxGetData(o->st);
    o->stats.newton_iters = sp;
    o->stats.ls_halvings = sp + B;
    o->stats.status = sp + 2 * B;
    o->hist.T = (K && want_energy) ? mxGetPr(o->T) : NULL;
    o->hist.V = (K && want_energy) ? mxGetPr(o->V) : NULL;
    if (want_state) {   /* the full Scene.saveHistory record */
        const mwSize dims[3] = {(mwSize)h->nr, (mwSize)B, (mwSize)K};
        o->Q = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
        o->Qd = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
        if (K && h->nr) { o->hist.q = mxGetPr(o->Q); o->hist.qdot = mxGetPr(o->Qd); }
    }
    if (want_charts) {   /* JointSpherical.chart after every step: nsph x B x nsteps int32 */
        const mwSize dims[3] = {(mwSize)h->nsph, (mwSize)B, (mwSize)K};
        o->C = mxCreateNumericArray(3, dims, mxINT32_CLASS, mxREAL);
        if (K && h->nsph) o->hist.charts = (int*)mxGetData(o->C);
    }
}
static void step_return(int nlhs, mxArray* plhs[], const step_out_t* o) {
    plhs[0] = o->T;
    if (nlhs > 1) plhs[1] = o->V;
    if (nlhs > 2) plhs[2] = o->st;
    if (nlhs > 3) plhs[3] = o->Q;
    if (nlhs > 4) plhs[4] = o->Qd;
    if (nlhs > 5) plhs[5] = o->C;
}
static int step_args(int nrhs, const mxArray* prhs[], const char* usage, int* itype, rmx_opts* o) {
    if (nrhs < 5) die(usage);
    *itype = (int)mxGetScalar(prhs[2]);
    const int nsteps = (int)mxGetScalar(prhs[4]);
    if (*itype != 1 && *itype != 2) die("itype must be 1 (BDF1) or 2 (BDF2)");
    if (nsteps < 0) die("nsteps < 0");
    rmx_opts_default(o);
    o->h = mxGetScalar(prhs[3]);
    if (nrhs > 5) read_opts(prhs[5], o);
    return nsteps;
}

static void cmd_step(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    int itype;
    rmx_opts o;
    const int nsteps = step_args(nrhs, prhs, "usage: [T,V,stats,Q,Qdot,C] = redmax_hip_mex('step', h, itype, hstep, nsteps [, opts])", &itype, &o);
    if (h->pending) die("a 'step_async' of this handle is in flight: 'sync' first");
    step_out_t out;
    step_outputs(h, nsteps, 1, nlhs > 3, nlhs > 5, &out);
    /* simLoop of the whole batch: every shard's launch goes out before the first is waited for (rmx_group_step) */
    if (rmx_group_step(h->g, &o, nsteps, itype, &out.stats, &out.hist)) die_rmx("rmx_group_step");
    step_return(nlhs, plhs, &out);
}

/* redmax_hip_mex('step_async', h, itype, hstep, nsteps [, opts [, record]]): launch and return */
static void cmd_step_async(int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    int itype;
    rmx_opts o;
    const int nsteps = step_args(nrhs, prhs, "usage: redmax_hip_mex('step_async', h, itype, hstep, nsteps [, opts [, record]])", &itype, &o);
    if (h->pending) die("a 'step_async' of this handle is already in flight: 'sync' first");
    const int record = nrhs > 6 ? (int)mxGetScalar(prhs[6]) : RMX_REC_ENERGY;
    if (rmx_group_step_async(h->g, &o, nsteps, itype, record)) {
        char msg[512];
        strncpy(msg, rmx_last_error(), sizeof msg - 1);
        msg[sizeof msg - 1] = 0;
        rmx_group_sync(h->g, NULL, NULL);      /* drain the shards that did start */
        mexErrMsgIdAndTxt("redmax:hip", "rmx_group_step_async: %s", msg);
    }
    h->pending = 1;
    h->pending_nsteps = nsteps;
    h->pending_record = record;
}

/* [T,V,st,Q,Qd,C] = redmax_hip_mex('sync', h): wait for the launches of 'step_async' and gather */
static void cmd_sync(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (!h->pending) die("'sync' without a 'step_async' in flight");
    const int rec = h->pending_record;
    if (nlhs > 3 && !(rec & RMX_REC_STATE)) die("'sync': Q, Qdot were not recorded (record bit 2 of 'step_async')");
    if (nlhs > 5 && !(rec & RMX_REC_CHARTS)) die("'sync': the charts were not recorded (record bit 4 of 'step_async')");
    step_out_t out;
    step_outputs(h, h->pending_nsteps, rec & RMX_REC_ENERGY, nlhs > 3, nlhs > 5, &out);
    h->pending = 0;
    if (rmx_group_sync(h->g, &out.stats, &out.hist)) die_rmx("rmx_group_sync");
    step_return(nlhs, plhs, &out);
}

static void cmd_euler(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 4) die("usage: [T,V] = redmax_hip_mex('euler', h, hstep, nsteps)");
    const int nsteps = (int)mxGetScalar(prhs[3]);
    if (nsteps < 0) die("nsteps < 0");
    mxArray* T = mxCreateDoubleMatrix((size_t)h->B, (size_t)nsteps, mxREAL);
    mxArray* V = mxCreateDoubleMatrix((size_t)h->B, (size_t)nsteps, mxREAL);
    if (h->nshards == 1) {
        size_t f;
        if (rmx_step_euler(shard(h, 0, &f), mxGetScalar(prhs[2]), nsteps, nsteps ? mxGetPr(T) : NULL, nsteps ? mxGetPr(V) : NULL)) die_rmx("rmx_step_euler");
    } else {      /* rmx_step_euler writes dense [nsteps][shard] arrays: per shard into a scratch matrix, then into the columns */
        for (int s = 0; s < h->nshards; ++s) {
            size_t f;
            int cnt = 0;
            rmx_batch* b = shard(h, s, &f);
            rmx_group_shard(h->g, s, NULL, NULL, &cnt);
            double* tmp = (double*)mxCalloc(2 * (size_t)cnt * (size_t)nsteps + 1, sizeof(double));
            double* tv = tmp + (size_t)cnt * (size_t)nsteps;
            if (rmx_step_euler(b, mxGetScalar(prhs[2]), nsteps, nsteps ? tmp : NULL, nsteps ? tv : NULL)) { mxFree(tmp); die_rmx("rmx_step_euler"); }
            for (int k = 0; k < nsteps; ++k) {
                memcpy(mxGetPr(T) + (size_t)k * (size_t)h->B + f, tmp + (size_t)k * (size_t)cnt, sizeof(double) * (size_t)cnt);
                memcpy(mxGetPr(V) + (size_t)k * (size_t)h->B + f, tv + (size_t)k * (size_t)cnt, sizeof(double) * (size_t)cnt);
            }
            mxFree(tmp);
        }
    }
    mxArray* const out[2] = {T, V};
    give(nlhs, plhs, out, 2);
}

static void cmd_eval(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 6) die("usage: [g,H] = redmax_hip_mex('eval', h, q, qA, qB, eta)");
    const double* q = state_arg(prhs[2], h, "q");
    const double* qA = state_arg(prhs[3], h, "qA");
    const double* qB = state_arg(prhs[4], h, "qB");
    mxArray* g = mxCreateDoubleMatrix((size_t)h->nr, (size_t)h->B, mxREAL);
    mxArray* H = NULL;
    if (nlhs > 1) {   /* nargout == 1 selects the residual-only path, as in evalBDF1 (driverRedMaxBDF1.m:165) */
        const mwSize dims[3] = {(mwSize)h->nr, (mwSize)h->nr, (mwSize)h->B};
        H = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    }
    for (int s = 0; s < h->nshards; ++s) {
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        const size_t o = f * (size_t)h->nr;
        if (rmx_eval(b, q + o, qA + o, qB + o, mxGetScalar(prhs[5]), mxGetPr(g) + o, H ? mxGetPr(H) + o * (size_t)h->nr : NULL)) die_rmx("rmx_eval");
    }
    mxArray* const out[2] = {g, H};
    give(nlhs, plhs, out, 2);
}

/* [M,f,K,D,dMv] = redmax_hip_mex('values', h, q, qdot [, v]) - computeValues' full output (driverRedMaxBDF1.m:188-243: [M,f,dMdq,K,D])
 * at (q, qdot): M, K, D nr x nr x B, f nr x B; with v (nr x B) also dMv, whose column i is dMdq(:,:,i) v (evalBDF1 :181-184 uses the
 * tensor in exactly this form, v = dqtmp).  rmx_compute_values, per shard. */
static void cmd_values(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 4) die("usage: [M,f,K,D,dMv] = redmax_hip_mex('values', h, q, qdot [, v])");
    const double* q = state_arg(prhs[2], h, "q");
    const double* qd = state_arg(prhs[3], h, "qdot");
    const double* v = nrhs > 4 ? state_arg(prhs[4], h, "v") : NULL;
    if (nlhs > 4 && !v) die("values: the fifth output dMv needs v");
    const mwSize dims[3] = {(mwSize)h->nr, (mwSize)h->nr, (mwSize)h->B};
    mxArray* out[5] = {NULL, NULL, NULL, NULL, NULL};
    out[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    out[1] = mxCreateDoubleMatrix((size_t)h->nr, (size_t)h->B, mxREAL);
    if (nlhs > 2) out[2] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    if (nlhs > 3) out[3] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    if (nlhs > 4) out[4] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    for (int s = 0; s < h->nshards; ++s) {
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        const size_t o = f * (size_t)h->nr, oo = o * (size_t)h->nr;
        if (rmx_compute_values(b, q + o, qd + o, v ? v + o : NULL, mxGetPr(out[0]) + oo, mxGetPr(out[1]) + o,
                               out[3] ? mxGetPr(out[3]) + oo : NULL, out[2] ? mxGetPr(out[2]) + oo : NULL,
                               out[4] ? mxGetPr(out[4]) + oo : NULL, NULL))
            die_rmx("rmx_compute_values");
    }
    for (int i = 0; i < 5 && (i == 0 || i < nlhs); ++i) plhs[i] = out[i];
}

/* the options of an 'adjoint*' or tape-recording command: the defaults under the step size of the call */
static rmx_opts tape_opts(double hstep) {
    rmx_opts o;
    rmx_opts_default(&o);
    o.h = hstep;
    o.iterMaxPerDof = 5;                               /* driverRedMaxAdjointBDF1.m:108 */
    return o;
}

/* the task struct of 'adjoint' / 'adjoint_controls' (TaskBDF1PointPos) */
static void read_task(const mxArray* t, rmx_task_pointpos* task) {
    if (!mxIsStruct(t)) die("task must be a struct");
    memset(task, 0, sizeof *task);
    task->body = (int)scalar_field(t, "body", 1) - 1;   /* MATLAB listing index -> 0-based */
    const mxArray* xl = field(t, "xlocal", 1);
    const mxArray* xt = field(t, "xtarget", 1);
    if (mxGetNumberOfElements(xl) != 3 || mxGetNumberOfElements(xt) != 3) die("task.xlocal / task.xtarget must have 3 elements");
    memcpy(task->xlocal, mxGetPr(xl), 3 * sizeof(double));
    memcpy(task->xtarget, mxGetPr(xt), 3 * sizeof(double));
    task->step = (int)scalar_field(t, "step", 0);
    task->pscale = scalar_field(t, "pscale", 1.0);
    task->wreg = scalar_field(t, "wreg", 0.0);
    task->wpos = scalar_field(t, "wpos", 1.0);
}

static void cmd_adjoint(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 6) die("usage: [P,dPdp,stats] = redmax_hip_mex('adjoint', h, hstep, nsteps, task, p [, integrator])");
    rmx_task_pointpos task;
    read_task(prhs[4], &task);
    const rmx_opts o = tape_opts(mxGetScalar(prhs[2]));
    const int nsteps = (int)mxGetScalar(prhs[3]);
    const double* p = state_arg(prhs[5], h, "p");
    mxArray* P = mxCreateDoubleMatrix(1, (size_t)h->B, mxREAL);
    mxArray* dPdp = mxCreateDoubleMatrix((size_t)h->nr, (size_t)h->B, mxREAL);
    mxArray* st = new_i32((size_t)h->B, 2);
    /* optional 7th argument: the integrator, 1 = BDF1 (driverRedMaxAdjointBDF1.m, default), 2 = BDF2 (driverRedMaxAdjointBDF2.m) */
    const int integ = nrhs > 6 ? (int)mxGetScalar(prhs[6]) : 1;
    if (integ != 1 && integ != 2) die("adjoint: the integrator must be 1 (BDF1) or 2 (BDF2)");
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard (the adjoint has no asynchronous entry: its outputs are per-call host buffers) */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_stats st_s = shard_stats(st, h, f);
        if ((integ == 1 ? rmx_adjoint_bdf1 : rmx_adjoint_bdf2)(b, &o, nsteps, &task, p + f * (size_t)h->nr, mxGetPr(P) + f,
                                                                mxGetPr(dPdp) + f * (size_t)h->nr, &st_s))
            die_rmx(integ == 1 ? "rmx_adjoint_bdf1" : "rmx_adjoint_bdf2");
    }
    mxArray* const out[3] = {P, dPdp, st};
    give(nlhs, plhs, out, 3);
}

static void cmd_adjoint_controls(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 6) die("usage: [P,dPdu,stats] = redmax_hip_mex('adjoint_controls', h, hstep, nsteps, task, u [, integrator])");
    rmx_task_pointpos task;
    read_task(prhs[4], &task);
    const rmx_opts o = tape_opts(mxGetScalar(prhs[2]));
    const int nsteps = (int)mxGetScalar(prhs[3]);
    if (nsteps < 1) die("adjoint_controls: nsteps must be at least 1");
    const int integ = nrhs > 6 ? (int)mxGetScalar(prhs[6]) : 1;
    if (integ != 1 && integ != 2) die("adjoint_controls: the integrator must be 1 (BDF1) or 2 (BDF2)");
    const mxArray* ua = prhs[5];
    const size_t per = (size_t)h->nr * (size_t)nsteps;      /* one rollout's controls: nr x nsteps x B is the ABI's [B][nsteps][nr] */
    if (!mxIsDouble(ua) || mxIsComplex(ua) || mxGetNumberOfElements(ua) != per * (size_t)h->B)
        mexErrMsgIdAndTxt("redmax:hip", "u must be a real double nr x nsteps x batch (%d x %d x %d) array", h->nr, nsteps, h->B);
    const double* u = mxGetPr(ua);
    mxArray* P = mxCreateDoubleMatrix(1, (size_t)h->B, mxREAL);
    mxArray* dPdu = NULL;                              /* one output: the forward sweep alone */
    if (nlhs > 1) {
        const size_t dims[3] = {(size_t)h->nr, (size_t)nsteps, (size_t)h->B};
        dPdu = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    }
    mxArray* st = new_i32((size_t)h->B, 2);
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard, as 'adjoint' */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_stats st_s = shard_stats(st, h, f);
        if (rmx_adjoint_controls(b, &o, nsteps, integ, &task, u + f * per, mxGetPr(P) + f, dPdu ? mxGetPr(dPdu) + f * per : NULL, &st_s))
            die_rmx("rmx_adjoint_controls");
    }
    mxArray* const out[3] = {P, dPdu, st};
    give(nlhs, plhs, out, 3);
}

/* an nr x nsteps x B argument of 'rollout_tape' / 'rollout_vjp' (the ABI's [B][nsteps][nr]) */
static const double* traj_arg(const mxArray* a, const handle_t* h, int nsteps, const char* what) {
    if (!mxIsDouble(a) || mxIsComplex(a) || mxGetNumberOfElements(a) != (size_t)h->nr * (size_t)nsteps * (size_t)h->B)
        mexErrMsgIdAndTxt("redmax:hip", "%s must be a real double nr x nsteps x batch (%d x %d x %d) array", what, h->nr, nsteps, h->B);
    return mxGetPr(a);
}

/* the head of a tape-recording command `cmd` ('rollout_tape', 'rollout_feedback', 'rollout_feedback_box'): hstep, nsteps, pscale in
 * prhs[2..4], the required arguments up to prhs[nreq - 1] and the optional integrator behind them */
typedef struct { rmx_opts o; int nsteps, integ; double pscale; } tape_head_t;
static tape_head_t tape_head(int nrhs, const mxArray* prhs[], int nreq, const char* cmd, const char* usage) {
    tape_head_t t;
    if (nrhs < nreq) die(usage);
    const double integ_arg = nrhs > nreq ? mxGetScalar(prhs[nreq]) : 1.0;
    if (integ_arg != 1.0 && integ_arg != 2.0) mexErrMsgIdAndTxt("redmax:hip", "%s: integrator must be 1 (BDF1) or 2 (BDF2)", cmd);
    t.integ = integ_arg == 2.0 ? 2 : 1;
    t.o = tape_opts(mxGetScalar(prhs[2]));
    t.nsteps = (int)mxGetScalar(prhs[3]);
    if (t.nsteps < 1) mexErrMsgIdAndTxt("redmax:hip", "%s: nsteps must be at least 1", cmd);
    t.pscale = mxGetScalar(prhs[4]);
    return t;
}

static void cmd_rollout_tape(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    const tape_head_t t = tape_head(nrhs, prhs, 6, "rollout_tape",
                                    "usage: [qtraj,qdtraj,stats] = redmax_hip_mex('rollout_tape', h, hstep, nsteps, pscale, u [, integrator])");
    const int nsteps = t.nsteps;
    const double* u = traj_arg(prhs[5], h, nsteps, "u");
    const size_t per = (size_t)h->nr * (size_t)nsteps;
    const size_t dims[3] = {(size_t)h->nr, (size_t)nsteps, (size_t)h->B};
    mxArray* const out[3] = {mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL), mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL),
                             new_i32((size_t)h->B, 2)};
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard, as 'adjoint_controls' */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_stats st_s = shard_stats(out[2], h, f);
        if ((t.integ == 2 ? rmx_rollout_tape_bdf2 : rmx_rollout_tape)(b, &t.o, nsteps, t.pscale, u + f * per, mxGetPr(out[0]) + f * per,
                                                                      mxGetPr(out[1]) + f * per, &st_s))
            die_rmx(t.integ == 2 ? "rmx_rollout_tape_bdf2" : "rmx_rollout_tape");
    }
    h->tape_integ = t.integ;
    give(nlhs, plhs, out, 3);
}

/* a table argument of 'rollout_feedback': [] (NULL), `per` elements per step shared by the batch, or as many for every rollout;
 * *per_rollout is set by the first table given and the other must agree */
static const double* feedback_arg(const mxArray* a, const handle_t* h, size_t per, int nsteps, int* per_rollout, const char* what) {
    if (mxIsEmpty(a)) return NULL;
    const size_t n = mxGetNumberOfElements(a), shared = per * (size_t)nsteps;
    const int pr = n == shared * (size_t)h->B && h->B > 1;
    if (!mxIsDouble(a) || mxIsComplex(a) || (n != shared && !pr) || (*per_rollout >= 0 && pr != *per_rollout))
        mexErrMsgIdAndTxt("redmax:hip", "rollout_feedback: %s must be a real double array of %d x nsteps or %d x nsteps x batch elements, K and xref alike",
                          what, (int)per, (int)per);
    *per_rollout = pr;
    return mxGetPr(a);
}

/* a limit argument of 'rollout_feedback_box' / 'rollout_lqr_box': [] (NULL: that side is unbounded) or nr doubles */
static const double* bound_arg(const mxArray* a, const handle_t* h, const char* cmd, const char* what) {
    if (mxIsEmpty(a)) return NULL;
    if (!mxIsDouble(a) || mxIsComplex(a) || mxGetNumberOfElements(a) != (size_t)h->nr)
        mexErrMsgIdAndTxt("redmax:hip", "%s: %s must be [] or a real double array of nr = %d elements", cmd, what, h->nr);
    return mxGetPr(a);
}

/* 'rollout_feedback' and, with box, 'rollout_feedback_box': the same with the applied torque clamped into ulo <= u <= uhi
 * (rmx_rollout_tape_feedback_box); the limits push the optional integrator two arguments back */
static void cmd_rollout_feedback(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[], int box) {
    handle_t* h = get_handle(nrhs, prhs);
    const char* cmd = box ? "rollout_feedback_box" : "rollout_feedback";
    const tape_head_t t = tape_head(nrhs, prhs, box ? 10 : 8, cmd, box
        ? "usage: [qtraj,qdtraj,uapp,stats] = redmax_hip_mex('rollout_feedback_box', h, hstep, nsteps, pscale, uff, K, xref, ulo, uhi [, integrator])"
        : "usage: [qtraj,qdtraj,uapp,stats] = redmax_hip_mex('rollout_feedback', h, hstep, nsteps, pscale, uff, K, xref [, integrator])");
    const int nsteps = t.nsteps;
    const double* uff = traj_arg(prhs[5], h, nsteps, "uff");
    const size_t nr = (size_t)h->nr, per = nr * (size_t)nsteps;
    int per_rollout = -1;
    const double* K = feedback_arg(prhs[6], h, 2 * nr * nr, nsteps, &per_rollout, "K");            /* nr x 2nr x nsteps [x B] */
    const double* xref = feedback_arg(prhs[7], h, 2 * nr, nsteps, &per_rollout, "xref");           /* 2nr x nsteps [x B] */
    if (per_rollout < 0) per_rollout = 0;
    rmx_box lim = {NULL, NULL};
    if (box) {
        lim.ulo = bound_arg(prhs[8], h, cmd, "ulo");
        lim.uhi = bound_arg(prhs[9], h, cmd, "uhi");
    }
    const size_t dims[3] = {nr, (size_t)nsteps, (size_t)h->B};
    mxArray* out[4];
    for (int i = 0; i < 3; ++i) out[i] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    out[3] = new_i32((size_t)h->B, 2);
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard, as 'rollout_tape' */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_stats st_s = shard_stats(out[3], h, f);
        rmx_feedback fb;
        fb.uff = uff + f * per;
        fb.K = table_at(K, per_rollout, f, per * 2 * nr);
        fb.xref = table_at(xref, per_rollout, f, per * 2);
        fb.per_rollout = per_rollout;
        double *qt = mxGetPr(out[0]) + f * per, *qdt = mxGetPr(out[1]) + f * per, *uapp = mxGetPr(out[2]) + f * per;
        if (box ? rmx_rollout_tape_feedback_box(b, &t.o, nsteps, t.integ, t.pscale, &fb, &lim, qt, qdt, uapp, &st_s)
                : rmx_rollout_tape_feedback(b, &t.o, nsteps, t.integ, t.pscale, &fb, qt, qdt, uapp, &st_s))
            die_rmx(box ? "rmx_rollout_tape_feedback_box" : "rmx_rollout_tape_feedback");
    }
    h->tape_integ = t.integ;
    give(nlhs, plhs, out, 4);
}

static void cmd_rollout_vjp(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 5) die("usage: [du,dq0,dqd0] = redmax_hip_mex('rollout_vjp', h, nsteps, gq, gqd)");
    const int nsteps = (int)mxGetScalar(prhs[2]);
    if (nsteps < 1) die("rollout_vjp: nsteps must be at least 1");
    const double* gq = traj_arg(prhs[3], h, nsteps, "gq");
    const double* gqd = traj_arg(prhs[4], h, nsteps, "gqd");
    const size_t per = (size_t)h->nr * (size_t)nsteps;
    const size_t dims[3] = {(size_t)h->nr, (size_t)nsteps, (size_t)h->B};
    mxArray* const out[3] = {mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL), mxCreateDoubleMatrix((size_t)h->nr, (size_t)h->B, mxREAL),
                             mxCreateDoubleMatrix((size_t)h->nr, (size_t)h->B, mxREAL)};      /* du, dq0, dqd0 */
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard: every shard's batch holds its own tape */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        if (rmx_rollout_vjp(b, nsteps, gq + f * per, gqd + f * per, mxGetPr(out[0]) + f * per, mxGetPr(out[1]) + f * (size_t)h->nr,
                            mxGetPr(out[2]) + f * (size_t)h->nr))
            die_rmx("rmx_rollout_vjp");
    }
    give(nlhs, plhs, out, 3);
}

/* 'rollout_vjp_feedback': the closed-loop adjoint on the tape 'rollout_feedback' left.  K, xref as there ([]: none); gu [] or as gq.
 * The gradient rows are per rollout whatever the tables are: dK nr x 2nr x nsteps x B, dxref 2nr x nsteps x B. */
static void cmd_rollout_vjp_feedback(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 7) die("usage: [duff,dK,dxref,dq0,dqd0] = redmax_hip_mex('rollout_vjp_feedback', h, nsteps, gq, gqd, K, xref [, gu])");
    const int nsteps = (int)mxGetScalar(prhs[2]);
    if (nsteps < 1) die("rollout_vjp_feedback: nsteps must be at least 1");
    const double* gq = traj_arg(prhs[3], h, nsteps, "gq");
    const double* gqd = traj_arg(prhs[4], h, nsteps, "gqd");
    const size_t nr = (size_t)h->nr, per = nr * (size_t)nsteps;
    int per_rollout = -1;
    const double* K = feedback_arg(prhs[5], h, 2 * nr * nr, nsteps, &per_rollout, "K");
    const double* xref = feedback_arg(prhs[6], h, 2 * nr, nsteps, &per_rollout, "xref");
    if (per_rollout < 0) per_rollout = 0;
    const double* gu = (nrhs > 7 && !mxIsEmpty(prhs[7])) ? traj_arg(prhs[7], h, nsteps, "gu") : NULL;
    const size_t dims[3] = {nr, (size_t)nsteps, (size_t)h->B}, dimsK[4] = {nr, 2 * nr, (size_t)nsteps, (size_t)h->B};
    const size_t dimsx[3] = {2 * nr, (size_t)nsteps, (size_t)h->B};
    mxArray* out[5];
    out[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    out[1] = (K && nlhs > 1) ? mxCreateNumericArray(4, dimsK, mxDOUBLE_CLASS, mxREAL) : mxCreateDoubleMatrix(0, 0, mxREAL);
    out[2] = (K && nlhs > 2) ? mxCreateNumericArray(3, dimsx, mxDOUBLE_CLASS, mxREAL) : mxCreateDoubleMatrix(0, 0, mxREAL);
    out[3] = mxCreateDoubleMatrix(nr, (size_t)h->B, mxREAL);
    out[4] = mxCreateDoubleMatrix(nr, (size_t)h->B, mxREAL);
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard: every shard's batch holds its own tape */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_feedback fb;
        fb.uff = NULL;
        fb.K = table_at(K, per_rollout, f, per * 2 * nr);
        fb.xref = table_at(xref, per_rollout, f, per * 2);
        fb.per_rollout = per_rollout;
        rmx_feedback_grads g;
        g.duff = mxGetPr(out[0]) + f * per;
        g.dK = (K && nlhs > 1) ? mxGetPr(out[1]) + f * (size_t)nsteps * 2 * nr * nr : NULL;
        g.dxref = (K && nlhs > 2) ? mxGetPr(out[2]) + f * (size_t)nsteps * 2 * nr : NULL;
        g.dq0 = mxGetPr(out[3]) + f * nr;
        g.dqd0 = mxGetPr(out[4]) + f * nr;
        if (rmx_rollout_vjp_feedback(b, nsteps, &fb, gq + f * per, gqd + f * per, gu ? gu + f * per : NULL, &g)) die_rmx("rmx_rollout_vjp_feedback");
    }
    give(nlhs, plhs, out, 5);
}

static void cmd_rollout_vjp_params(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 5) die("usage: [du,dq0,dqd0,dk,dd,dqrest,dI,dgrav] = redmax_hip_mex('rollout_vjp_params', h, nsteps, gq, gqd)");
    const int nsteps = (int)mxGetScalar(prhs[2]);
    if (nsteps < 1) die("rollout_vjp_params: nsteps must be at least 1");
    const double* gq = traj_arg(prhs[3], h, nsteps, "gq");
    const double* gqd = traj_arg(prhs[4], h, nsteps, "gqd");
    const size_t nr = (size_t)h->nr, per = nr * (size_t)nsteps, perI = 6 * (size_t)h->njoints;
    const size_t dims[3] = {nr, (size_t)nsteps, (size_t)h->B}, dimsI[3] = {6, (size_t)h->njoints, (size_t)h->B};
    mxArray* out[8];
    out[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    for (int i = 1; i < 6; ++i) out[i] = mxCreateDoubleMatrix(nr, (size_t)h->B, mxREAL);      /* dq0, dqd0, dk, dd, dqrest */
    out[6] = mxCreateNumericArray(3, dimsI, mxDOUBLE_CLASS, mxREAL);
    out[7] = mxCreateDoubleMatrix(3, (size_t)h->B, mxREAL);
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard: every shard's batch holds its own tape */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_param_grads pg;
        pg.stiffness = mxGetPr(out[3]) + f * nr;
        pg.damping = mxGetPr(out[4]) + f * nr;
        pg.qrest = mxGetPr(out[5]) + f * nr;
        pg.inertia = mxGetPr(out[6]) + f * perI;
        pg.grav = mxGetPr(out[7]) + f * 3;
        if (rmx_rollout_vjp_params(b, nsteps, gq + f * per, gqd + f * per, mxGetPr(out[0]) + f * per, mxGetPr(out[1]) + f * nr,
                                   mxGetPr(out[2]) + f * nr, &pg))
            die_rmx("rmx_rollout_vjp_params");
    }
    give(nlhs, plhs, out, 8);
}

/* 'rollout_vjp_forces': rmx_rollout_vjp_forces shard by shard.  nforces: the rows of the force table the shards' models carry (the
 * gateway cannot ask the library for it); the five model arrays are formed only where they are asked for (nlhs > 6). */
static void cmd_rollout_vjp_forces(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 6)
        die("usage: [du,dq0,dqd0,dks,dkd,dL,dk,dd,dqrest,dI,dgrav] = redmax_hip_mex('rollout_vjp_forces', h, nsteps, gq, gqd, nforces)");
    const int nsteps = (int)mxGetScalar(prhs[2]);
    if (nsteps < 1) die("rollout_vjp_forces: nsteps must be at least 1");
    const double* gq = traj_arg(prhs[3], h, nsteps, "gq");
    const double* gqd = traj_arg(prhs[4], h, nsteps, "gqd");
    if (mxGetNumberOfElements(prhs[5]) != 1) die("rollout_vjp_forces: nforces must be a scalar");
    const double nfd = mxGetScalar(prhs[5]);
    if (!(nfd >= 0.0 && nfd <= (double)RMX_PF_MAX_FORCES) || nfd != (double)(int)nfd) die("rollout_vjp_forces: nforces must be an integer in 0 .. RMX_PF_MAX_FORCES");
    const size_t nf = (size_t)nfd, nr = (size_t)h->nr, per = nr * (size_t)nsteps, perI = 6 * (size_t)h->njoints;
    const size_t dims[3] = {nr, (size_t)nsteps, (size_t)h->B}, dimsI[3] = {6, (size_t)h->njoints, (size_t)h->B};
    const int model = nlhs > 6;
    mxArray* out[11];
    out[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    for (int i = 1; i < 3; ++i) out[i] = mxCreateDoubleMatrix(nr, (size_t)h->B, mxREAL);       /* dq0, dqd0 */
    for (int i = 3; i < 6; ++i) out[i] = mxCreateDoubleMatrix(nf, (size_t)h->B, mxREAL);       /* dks, dkd, dL */
    for (int i = 6; i < 9; ++i) out[i] = mxCreateDoubleMatrix(model ? nr : 0, model ? (size_t)h->B : 0, mxREAL);      /* dk, dd, dqrest */
    out[9] = model ? mxCreateNumericArray(3, dimsI, mxDOUBLE_CLASS, mxREAL) : mxCreateDoubleMatrix(0, 0, mxREAL);
    out[10] = mxCreateDoubleMatrix(model ? 3 : 0, model ? (size_t)h->B : 0, mxREAL);
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard: every shard's batch holds its own tape */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_force_grads fg;
        fg.stiffness = nf ? mxGetPr(out[3]) + f * nf : NULL;
        fg.damping = nf ? mxGetPr(out[4]) + f * nf : NULL;
        fg.L = nf ? mxGetPr(out[5]) + f * nf : NULL;
        rmx_param_grads pg;
        pg.stiffness = model ? mxGetPr(out[6]) + f * nr : NULL;
        pg.damping = model ? mxGetPr(out[7]) + f * nr : NULL;
        pg.qrest = model ? mxGetPr(out[8]) + f * nr : NULL;
        pg.inertia = model ? mxGetPr(out[9]) + f * perI : NULL;
        pg.grav = model ? mxGetPr(out[10]) + f * 3 : NULL;
        if (rmx_rollout_vjp_forces(b, nsteps, gq + f * per, gqd + f * per, mxGetPr(out[0]) + f * per, mxGetPr(out[1]) + f * nr,
                                   mxGetPr(out[2]) + f * nr, &pg, &fg))
            die_rmx("rmx_rollout_vjp_forces");
    }
    give(nlhs, plhs, out, 11);
}

static void cmd_rollout_linearize(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 3) die("usage: [XA,XB,XU] = redmax_hip_mex('rollout_linearize', h, nsteps)");
    const int nsteps = (int)mxGetScalar(prhs[2]);
    if (nsteps < 1) die("rollout_linearize: nsteps must be at least 1");
    const size_t nslots = (size_t)nsteps + (h->tape_integ == 2 ? 1 : 0);
    const size_t per = (size_t)h->nr * (size_t)h->nr * nslots;
    const size_t dims[4] = {(size_t)h->nr, (size_t)h->nr, nslots, (size_t)h->B};
    const int nout = nlhs < 1 ? 1 : (nlhs > 3 ? 3 : nlhs);      /* outputs nobody asked for are not computed */
    mxArray* X[3] = {NULL, NULL, NULL};
    for (int i = 0; i < nout; ++i) X[i] = mxCreateNumericArray(4, dims, mxDOUBLE_CLASS, mxREAL);
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard: every shard's batch holds its own tape */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        if (rmx_rollout_linearize(b, nsteps, mxGetPr(X[0]) + f * per, X[1] ? mxGetPr(X[1]) + f * per : NULL,
                                  X[2] ? mxGetPr(X[2]) + f * per : NULL))
            die_rmx("rmx_rollout_linearize");
    }
    for (int i = 0; i < nout; ++i) plhs[i] = X[i];
}

/* a real double argument of 'rollout_lqr' with `want` elements (or, where alt != 0, `alt`) */
static const double* lqr_arg(const mxArray* a, size_t want, size_t alt, const char* what, const char* shape) {
    const size_t n = mxGetNumberOfElements(a);
    if (!mxIsDouble(a) || mxIsComplex(a) || (n != want && !(alt && n == alt)))
        mexErrMsgIdAndTxt("redmax:hip", "rollout_lqr: %s must be a real double %s array", what, shape);
    return mxGetPr(a);
}

/* 'rollout_lqr' (fourth output notpd, 1 x B: 0 or 1) and, with box, 'rollout_lqr_box': the same under the torque limits ulo <= u <= uhi
 * (rmx_rollout_lqr_box) - the fourth output is status 1 x B (0, 1: a pivot not > 0, 2: a QP did not terminate), the fifth clamped
 * nsteps x B (the bit masks as doubles: nr <= 32, exact); ubar and the limits push the optional mu three arguments back */
static void cmd_rollout_lqr(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[], int box) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < (box ? 10 : 7))
        die(box ? "usage: [kff,K,expected,status,clamped] = redmax_hip_mex('rollout_lqr_box', h, nsteps, lx, lu, Q, R, ubar, ulo, uhi [, mu [, max_iter]])"
                : "usage: [kff,K,expected,notpd] = redmax_hip_mex('rollout_lqr', h, nsteps, lx, lu, Q, R [, mu])");
    const int nsteps = (int)mxGetScalar(prhs[2]);
    if (nsteps < 1) die(box ? "rollout_lqr_box: nsteps must be at least 1" : "rollout_lqr: nsteps must be at least 1");
    const size_t nr = (size_t)h->nr, N = (size_t)nsteps, B = (size_t)h->B;
    const size_t perq = 4 * nr * nr * N;
    const double* lx = lqr_arg(prhs[3], 2 * nr * N * B, 0, "lx", "2nr x nsteps x batch");
    const double* lu = lqr_arg(prhs[4], nr * N * B, 0, "lu", "nr x nsteps x batch");
    const double* Q = lqr_arg(prhs[5], perq, perq * B, "Q", "2nr x 2nr x nsteps or 2nr x 2nr x nsteps x batch");
    const double* R = lqr_arg(prhs[6], nr * nr, 0, "R", "nr x nr");
    const double* ubar = box ? lqr_arg(prhs[7], nr * N * B, 0, "ubar", "nr x nsteps x batch") : NULL;
    rmx_box lim = {NULL, NULL};
    if (box) {
        lim.ulo = bound_arg(prhs[8], h, "rollout_lqr_box", "ulo");
        lim.uhi = bound_arg(prhs[9], h, "rollout_lqr_box", "uhi");
    }
    const int imu = box ? 10 : 7;      /* where the optional mu stands */
    const int max_iter = (box && nrhs > 11) ? (int)mxGetScalar(prhs[11]) : 0;
    const size_t dk[3] = {nr, N, B}, dK[4] = {nr, 2 * nr, N, B};
    mxArray* const out[5] = {mxCreateNumericArray(3, dk, mxDOUBLE_CLASS, mxREAL), mxCreateNumericArray(4, dK, mxDOUBLE_CLASS, mxREAL),
                             mxCreateDoubleMatrix(1, B, mxREAL), mxCreateDoubleMatrix(1, B, mxREAL),
                             box ? mxCreateDoubleMatrix(N, B, mxREAL) : NULL};      /* kff, K, expected, notpd | status, clamped */
    int* status = (int*)mxCalloc(B, sizeof *status);
    unsigned* mask = box ? (unsigned*)mxCalloc(N * B, sizeof *mask) : NULL;
    rmx_lqr_cost cost;
    memset(&cost, 0, sizeof cost);
    cost.R = R;
    /* (a batch of one: Q is one table either way) */
    cost.per_rollout = mxGetNumberOfElements(prhs[5]) == perq * B && B > 1;
    cost.mu = nrhs > imu ? mxGetScalar(prhs[imu]) : 0.0;
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard: every shard's batch holds its own tape */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_lqr_gains g;
        cost.lx = lx + f * 2 * nr * N;
        cost.lu = lu + f * nr * N;
        cost.Q = table_at(Q, cost.per_rollout, f, perq);
        g.kff = mxGetPr(out[0]) + f * nr * N;
        g.K = mxGetPr(out[1]) + f * 2 * nr * nr * N;
        g.expected = mxGetPr(out[2]) + f;
        g.status = status + f;
        if (box ? rmx_rollout_lqr_box(b, nsteps, &cost, &lim, ubar + f * nr * N, max_iter, &g, mask + f * N) : rmx_rollout_lqr(b, nsteps, &cost, &g))
            die_rmx(box ? "rmx_rollout_lqr_box" : "rmx_rollout_lqr");
    }
    for (size_t i = 0; i < B; ++i) mxGetPr(out[3])[i] = box ? (double)status[i] : (status[i] ? 1.0 : 0.0);
    for (size_t i = 0; box && i < N * B; ++i) mxGetPr(out[4])[i] = (double)mask[i];
    mxFree(status);
    if (mask) mxFree(mask);
    give(nlhs, plhs, out, box ? 5 : 4);
}

/* one tangent argument of 'rollout_jvp': [] (NULL: zero) or a double array of `per` * ntan * B elements; *ntan is set by the first
 * array given and the others must agree */
static const double* tangent_arg_of(const char* cmd, const mxArray* a, const handle_t* h, size_t per, size_t* ntan, const char* what) {
    if (mxIsEmpty(a)) return NULL;
    const size_t n = mxGetNumberOfElements(a), unit = per * (size_t)h->B;
    if (!mxIsDouble(a) || mxIsComplex(a) || !unit || n % unit != 0 || (*ntan && n != unit * *ntan))
        mexErrMsgIdAndTxt("redmax:hip", "%s: %s must be a real double array of %d x ntan x %d elements, the same ntan in every array",
                          cmd, what, (int)per, h->B);
    *ntan = n / unit;
    return mxGetPr(a);
}
static const double* tangent_arg(const mxArray* a, const handle_t* h, size_t per, size_t* ntan, const char* what) {
    return tangent_arg_of("rollout_jvp", a, h, per, ntan, what);
}

static void cmd_rollout_jvp(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 6) die("usage: [tq,tqd] = redmax_hip_mex('rollout_jvp', h, nsteps, tu, tq0, tqd0)");
    const int nsteps = (int)mxGetScalar(prhs[2]);
    if (nsteps < 1) die("rollout_jvp: nsteps must be at least 1");
    const size_t nr = (size_t)h->nr, per = nr * (size_t)nsteps;
    size_t ntan = 0;
    const double* tu = tangent_arg(prhs[3], h, per, &ntan, "tu");          /* nr x nsteps x ntan x B */
    const double* tq0 = tangent_arg(prhs[4], h, nr, &ntan, "tq0");         /* nr x ntan x B */
    const double* tqd0 = tangent_arg(prhs[5], h, nr, &ntan, "tqd0");
    if (!ntan) ntan = 1;      /* (every tangent empty: the library refuses it in its own words) */
    const size_t dims[4] = {nr, (size_t)nsteps, ntan, (size_t)h->B};
    mxArray* const out[2] = {mxCreateNumericArray(4, dims, mxDOUBLE_CLASS, mxREAL), mxCreateNumericArray(4, dims, mxDOUBLE_CLASS, mxREAL)};
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard: every shard's batch holds its own tape */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        if (rmx_rollout_jvp(b, nsteps, (int)ntan, table_at(tu, 1, f, ntan * per), table_at(tq0, 1, f, ntan * nr), table_at(tqd0, 1, f, ntan * nr),
                            mxGetPr(out[0]) + f * ntan * per, mxGetPr(out[1]) + f * ntan * per))
            die_rmx("rmx_rollout_jvp");
    }
    give(nlhs, plhs, out, 2);
}

/* 'rollout_jvp_params': rmx_rollout_jvp_params shard by shard.  Eight tangent arguments, [] is NULL; ntan comes from the first
 * non-empty one, as 'rollout_jvp' reads it. */
static void cmd_rollout_jvp_params(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 11)
        die("usage: [tq,tqd] = redmax_hip_mex('rollout_jvp_params', h, nsteps, tk, td, tqrest, tI, tgrav, tu, tq0, tqd0)");
    const int nsteps = (int)mxGetScalar(prhs[2]);
    if (nsteps < 1) die("rollout_jvp_params: nsteps must be at least 1");
    const char* const cmd = "rollout_jvp_params";
    const size_t nr = (size_t)h->nr, per = nr * (size_t)nsteps, perI = 6 * (size_t)h->njoints;
    size_t ntan = 0;
    const double* tk = tangent_arg_of(cmd, prhs[3], h, nr, &ntan, "tk");             /* nr x ntan x B */
    const double* td = tangent_arg_of(cmd, prhs[4], h, nr, &ntan, "td");
    const double* tr = tangent_arg_of(cmd, prhs[5], h, nr, &ntan, "tqrest");
    const double* tI = tangent_arg_of(cmd, prhs[6], h, perI, &ntan, "tI");           /* 6 x njoints x ntan x B */
    const double* tg = tangent_arg_of(cmd, prhs[7], h, 3, &ntan, "tgrav");           /* 3 x ntan x B */
    const double* tu = tangent_arg_of(cmd, prhs[8], h, per, &ntan, "tu");            /* nr x nsteps x ntan x B */
    const double* tq0 = tangent_arg_of(cmd, prhs[9], h, nr, &ntan, "tq0");
    const double* tqd0 = tangent_arg_of(cmd, prhs[10], h, nr, &ntan, "tqd0");
    if (!ntan) ntan = 1;      /* (every tangent empty: the library refuses it in its own words) */
    const size_t dims[4] = {nr, (size_t)nsteps, ntan, (size_t)h->B};
    mxArray* const out[2] = {mxCreateNumericArray(4, dims, mxDOUBLE_CLASS, mxREAL), mxCreateNumericArray(4, dims, mxDOUBLE_CLASS, mxREAL)};
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard: every shard's batch holds its own tape */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_param_tangents tp;
        tp.stiffness = table_at(tk, 1, f, ntan * nr);
        tp.damping = table_at(td, 1, f, ntan * nr);
        tp.qrest = table_at(tr, 1, f, ntan * nr);
        tp.inertia = table_at(tI, 1, f, ntan * perI);
        tp.grav = table_at(tg, 1, f, ntan * 3);
        if (rmx_rollout_jvp_params(b, nsteps, (int)ntan, &tp, table_at(tu, 1, f, ntan * per), table_at(tq0, 1, f, ntan * nr),
                                   table_at(tqd0, 1, f, ntan * nr), mxGetPr(out[0]) + f * ntan * per, mxGetPr(out[1]) + f * ntan * per))
            die_rmx("rmx_rollout_jvp_params");
    }
    give(nlhs, plhs, out, 2);
}

/* field k of element i of the struct array task.terms */
static const mxArray* term_field(const mxArray* terms, size_t i, const char* k) {
    const mxArray* f = mxGetField(terms, i, k);
    if (!f || mxIsEmpty(f)) mexErrMsgIdAndTxt("redmax:hip", "task.terms(%d).%s is required", (int)i + 1, k);
    return f;
}

static void cmd_adjoint_track(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 6) die("usage: [P,dPdu,stats] = redmax_hip_mex('adjoint_track', h, hstep, nsteps, task, u [, integrator])");
    const mxArray* t = prhs[4];
    if (!mxIsStruct(t)) die("task must be a struct");
    const mxArray* ta = field(t, "terms", 1);
    if (!mxIsStruct(ta)) die("task.terms must be a struct array with the fields body, xlocal, step, wpos");
    const size_t nterms = mxGetNumberOfElements(ta);
    const rmx_opts o = tape_opts(mxGetScalar(prhs[2]));
    const int nsteps = (int)mxGetScalar(prhs[3]);
    if (nsteps < 1) die("adjoint_track: nsteps must be at least 1");
    const int integ = nrhs > 6 ? (int)mxGetScalar(prhs[6]) : 1;
    if (integ != 1 && integ != 2) die("adjoint_track: the integrator must be 1 (BDF1) or 2 (BDF2)");
    const mxArray* ua = prhs[5];
    const size_t per = (size_t)h->nr * (size_t)nsteps;      /* one rollout's controls: nr x nsteps x B is the ABI's [B][nsteps][nr] */
    if (!mxIsDouble(ua) || mxIsComplex(ua) || mxGetNumberOfElements(ua) != per * (size_t)h->B)
        mexErrMsgIdAndTxt("redmax:hip", "u must be a real double nr x nsteps x batch (%d x %d x %d) array", h->nr, nsteps, h->B);
    const mxArray* xa = field(t, "xtarget", 1);
    const size_t nxt = mxGetNumberOfElements(xa);           /* 3 x nterms, or 3 x nterms x B: the ABI's [B][nterms][3] */
    if (!mxIsDouble(xa) || mxIsComplex(xa) || (nxt != 3 * nterms && nxt != 3 * nterms * (size_t)h->B))
        mexErrMsgIdAndTxt("redmax:hip", "task.xtarget must be a real double 3 x nterms (3 x %d) or 3 x nterms x batch (3 x %d x %d) array",
                          (int)nterms, (int)nterms, h->B);
    rmx_track_term* terms = (rmx_track_term*)mxCalloc(nterms, sizeof *terms);
    /* (if a field check below raises, MATLAB frees it on the way out; mex/stub, where mxCalloc is calloc, lets it go with P, dPdu, st) */
    for (size_t i = 0; i < nterms; ++i) {
        terms[i].body = (int)mxGetScalar(term_field(ta, i, "body")) - 1;   /* MATLAB listing index -> 0-based */
        const mxArray* xl = term_field(ta, i, "xlocal");
        if (!mxIsDouble(xl) || mxGetNumberOfElements(xl) != 3) mexErrMsgIdAndTxt("redmax:hip", "task.terms(%d).xlocal must have 3 elements", (int)i + 1);
        memcpy(terms[i].xlocal, mxGetPr(xl), 3 * sizeof(double));
        terms[i].step = (int)mxGetScalar(term_field(ta, i, "step"));
        terms[i].wpos = mxGetScalar(term_field(ta, i, "wpos"));
    }
    rmx_task_track task;
    memset(&task, 0, sizeof task);
    task.nterms = (int)nterms;
    task.terms = terms;
    task.per_rollout = nxt != 3 * nterms;             /* (a batch of one: the two shapes are the same table) */
    task.pscale = scalar_field(t, "pscale", 1.0);
    task.wreg = scalar_field(t, "wreg", 0.0);
    mxArray* P = mxCreateDoubleMatrix(1, (size_t)h->B, mxREAL);
    mxArray* dPdu = NULL;                              /* one output: the forward sweep alone */
    if (nlhs > 1) {
        const size_t dims[3] = {(size_t)h->nr, (size_t)nsteps, (size_t)h->B};
        dPdu = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    }
    mxArray* st = new_i32((size_t)h->B, 2);
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard, as 'adjoint_controls': u, the per-rollout targets and the outputs advance */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_stats st_s = shard_stats(st, h, f);
        task.xtarget = table_at(mxGetPr(xa), task.per_rollout, f, 3 * nterms);
        if (rmx_adjoint_track(b, &o, nsteps, integ, &task, mxGetPr(ua) + f * per, mxGetPr(P) + f, dPdu ? mxGetPr(dPdu) + f * per : NULL, &st_s)) {
            mxFree(terms);
            die_rmx("rmx_adjoint_track");
        }
    }
    mxFree(terms);
    mxArray* const out[3] = {P, dPdu, st};
    give(nlhs, plhs, out, 3);
}

/* body (MATLAB listing index -> 0-based), xlocal and step of terms(i): the fields point and frame terms share */
static void term_place(const mxArray* ta, size_t i, const char* who, int* body, double xlocal[3], int* step) {
    *body = (int)mxGetScalar(term_field(ta, i, "body")) - 1;
    const mxArray* xl = term_field(ta, i, "xlocal");
    if (!mxIsDouble(xl) || mxGetNumberOfElements(xl) != 3) mexErrMsgIdAndTxt("redmax:hip", "%s: terms(%d).xlocal must have 3 elements", who, (int)i + 1);
    memcpy(xlocal, mxGetPr(xl), 3 * sizeof(double));
    *step = (int)mxGetScalar(term_field(ta, i, "step"));
}
/* the struct array `ta` (body 1-based, xlocal, step[, wpos]) as rmx_track_term's; the caller frees the result */
static rmx_track_term* point_terms(const mxArray* ta, const char* who, int need_wpos, size_t* nterms) {
    if (!mxIsStruct(ta)) mexErrMsgIdAndTxt("redmax:hip", "%s: terms must be a struct array with the fields body, xlocal, step%s", who, need_wpos ? ", wpos" : "");
    *nterms = mxGetNumberOfElements(ta);
    rmx_track_term* terms = (rmx_track_term*)mxCalloc(*nterms ? *nterms : 1, sizeof *terms);
    for (size_t i = 0; i < *nterms; ++i) {
        term_place(ta, i, who, &terms[i].body, terms[i].xlocal, &terms[i].step);
        terms[i].wpos = need_wpos ? mxGetScalar(term_field(ta, i, "wpos")) : 0.0;
    }
    return terms;
}
/* ... (body 1-based, xlocal, step[, wpos, wvel, wrot]: a missing weight is 0) as rmx_frame_term's; the caller frees */
static rmx_frame_term* frame_terms(const mxArray* ta, const char* who, size_t* nterms) {
    if (!mxIsStruct(ta)) mexErrMsgIdAndTxt("redmax:hip", "%s: terms must be a struct array with the fields body, xlocal, step[, wpos, wvel, wrot]", who);
    *nterms = mxGetNumberOfElements(ta);
    rmx_frame_term* terms = (rmx_frame_term*)mxCalloc(*nterms ? *nterms : 1, sizeof *terms);
    for (size_t i = 0; i < *nterms; ++i) {
        term_place(ta, i, who, &terms[i].body, terms[i].xlocal, &terms[i].step);
        const char* const names[3] = {"wpos", "wvel", "wrot"};
        double* const w[3] = {&terms[i].wpos, &terms[i].wvel, &terms[i].wrot};
        for (int k = 0; k < 3; ++k) {
            const mxArray* f = mxGetField(ta, i, names[k]);
            *w[k] = (f && !mxIsEmpty(f)) ? mxGetScalar(f) : 0.0;
        }
    }
    return terms;
}
/* a real double argument with `want` elements (or `alt`, where alt != 0), or - where empty_ok - []: NULL */
static const double* cost_arg(const mxArray* a, size_t want, size_t alt, int empty_ok, const char* who, const char* what, const char* shape) {
    if (empty_ok && mxIsEmpty(a)) return NULL;
    const size_t n = mxGetNumberOfElements(a);
    if (!mxIsDouble(a) || mxIsComplex(a) || (n != want && !(alt && n == alt)))
        mexErrMsgIdAndTxt("redmax:hip", "%s: %s must be a real double %s array", who, what, shape);
    return mxGetPr(a);
}

static void cmd_rollout_points(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 5) die("usage: [x,gq] = redmax_hip_mex('rollout_points', h, nsteps, q, terms [, gx])");
    const int nsteps = (int)mxGetScalar(prhs[2]);
    if (nsteps < 1) die("rollout_points: nsteps must be at least 1");
    const size_t nr = (size_t)h->nr, N = (size_t)nsteps, B = (size_t)h->B;
    const double* q = cost_arg(prhs[3], nr * N * B, 0, 0, "rollout_points", "q", "nr x nsteps x batch");
    size_t nterms;
    rmx_track_term* terms = point_terms(prhs[4], "rollout_points", 0, &nterms);
    const double* gx = nrhs > 5 ? cost_arg(prhs[5], 3 * nterms * B, 0, 1, "rollout_points", "gx", "3 x nterms x batch") : NULL;
    if (nlhs > 1 && !gx) die("rollout_points: gq needs gx");
    const size_t dx[3] = {3, nterms, B}, dg[3] = {nr, N, B};
    mxArray* x = mxCreateNumericArray(3, dx, mxDOUBLE_CLASS, mxREAL);
    mxArray* gq = nlhs > 1 ? mxCreateNumericArray(3, dg, mxDOUBLE_CLASS, mxREAL) : NULL;
    rmx_point_terms pts;
    memset(&pts, 0, sizeof pts);
    pts.nterms = (int)nterms;
    pts.terms = terms;
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard: the record, the points and the cotangents advance */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        if (rmx_rollout_points(b, nsteps, q + f * nr * N, &pts, mxGetPr(x) + f * 3 * nterms, gq ? gx + f * 3 * nterms : NULL,
                               gq ? mxGetPr(gq) + f * nr * N : NULL)) {
            mxFree(terms);
            die_rmx("rmx_rollout_points");
        }
    }
    mxFree(terms);
    mxArray* const out[2] = {x, gq};
    give(nlhs, plhs, out, 2);
}

/* 'rollout_cost' and, with frames, 'rollout_cost_frames': the same arguments with vtarget and Rtarget behind xtarget */
static void cmd_rollout_cost(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[], int frames) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < (frames ? 11 : 9))
        die(frames ? "usage: [Jk,lx,Q] = redmax_hip_mex('rollout_cost_frames', h, nsteps, q, qdot, Qin, xgoal, terms, xtarget, vtarget, Rtarget)"
                   : "usage: [Jk,lx,Q] = redmax_hip_mex('rollout_cost', h, nsteps, q, qdot, Qin, xgoal, terms, xtarget)");
    const int nsteps = (int)mxGetScalar(prhs[2]);
    if (nsteps < 1) die(frames ? "rollout_cost_frames: nsteps must be at least 1" : "rollout_cost: nsteps must be at least 1");
    const size_t nr = (size_t)h->nr, N = (size_t)nsteps, B = (size_t)h->B;
    const size_t perq = 4 * nr * nr * N, perg = 2 * nr * N;
    const char* who = frames ? "rollout_cost_frames" : "rollout_cost";
    const double* q = cost_arg(prhs[3], nr * N * B, 0, 0, who, "q", "nr x nsteps x batch");
    const double* qd = cost_arg(prhs[4], nr * N * B, 0, 0, who, "qdot", "nr x nsteps x batch");
    const double* Qin = cost_arg(prhs[5], perq, perq * B, 1, who, "Qin", "2nr x 2nr x nsteps or 2nr x 2nr x nsteps x batch");
    const double* xg = cost_arg(prhs[6], perg, perg * B, 1, who, "xgoal", "2nr x nsteps or 2nr x nsteps x batch");
    /* (a batch of one: a table is one table either way) */
    const int Q_per = Qin && mxGetNumberOfElements(prhs[5]) == perq * B && B > 1;
    const int g_per = xg && mxGetNumberOfElements(prhs[6]) == perg * B && B > 1;
    size_t nterms = 0;
    void* terms = mxIsEmpty(prhs[7]) ? NULL : frames ? (void*)frame_terms(prhs[7], who, &nterms) : (void*)point_terms(prhs[7], who, 1, &nterms);
    /* the target tables - one for point terms, which must be given; three for frame terms, each [] where no term weighs it (the library
       refuses otherwise) - share one per-rollout flag */
    const size_t width[3] = {3 * nterms, 3 * nterms, 9 * nterms};
    const char* const tname[3] = {"xtarget", "vtarget", "Rtarget"};
    const char* const tshape[3] = {"3 x nterms or 3 x nterms x batch", "3 x nterms or 3 x nterms x batch", "3 x 3 x nterms or 3 x 3 x nterms x batch"};
    const double* tab[3] = {NULL, NULL, NULL};
    int t_per = -1;
    for (int k = 0; k < (frames ? 3 : 1) && terms; ++k) {
        tab[k] = cost_arg(prhs[8 + k], width[k], width[k] * B, frames, who, tname[k], tshape[k]);
        if (!tab[k] || B == 1) continue;
        const int per = mxGetNumberOfElements(prhs[8 + k]) == width[k] * B;
        if (t_per >= 0 && per != t_per) {
            mxFree(terms);
            die("rollout_cost_frames: xtarget, vtarget and Rtarget must all be shared by the batch or all hold one table per rollout");
        }
        t_per = per;
    }
    if (t_per < 0) t_per = 0;
    const size_t dJ[2] = {N, B}, dl[3] = {2 * nr, N, B}, dQ[4] = {2 * nr, 2 * nr, N, B};
    mxArray* Jk = mxCreateNumericArray(2, dJ, mxDOUBLE_CLASS, mxREAL);
    mxArray* lx = nlhs > 1 ? mxCreateNumericArray(3, dl, mxDOUBLE_CLASS, mxREAL) : NULL;
    mxArray* Qo = nlhs > 2 ? mxCreateNumericArray(4, dQ, mxDOUBLE_CLASS, mxREAL) : NULL;
    rmx_state_cost sc;
    rmx_point_terms pts;
    rmx_frame_terms ft;
    memset(&sc, 0, sizeof sc);
    memset(&pts, 0, sizeof pts);
    memset(&ft, 0, sizeof ft);
    sc.Q_per_rollout = Q_per;
    sc.goal_per_rollout = g_per;
    pts.nterms = ft.nterms = (int)nterms;
    pts.terms = frames ? NULL : (const rmx_track_term*)terms;
    ft.terms = frames ? (const rmx_frame_term*)terms : NULL;
    pts.per_rollout = ft.per_rollout = t_per;
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard: the record, the per-rollout tables and the outputs advance */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_cost_model out;
        sc.Q = table_at(Qin, Q_per, f, perq);
        sc.xgoal = table_at(xg, g_per, f, perg);
        pts.xtarget = ft.xtarget = table_at(tab[0], t_per, f, width[0]);
        ft.vtarget = table_at(tab[1], t_per, f, width[1]);
        ft.Rtarget = table_at(tab[2], t_per, f, width[2]);
        out.Jk = mxGetPr(Jk) + f * N;
        out.lx = lx ? mxGetPr(lx) + f * perg : NULL;
        out.Q = Qo ? mxGetPr(Qo) + f * perq : NULL;
        const rmx_state_cost* scp = (Qin || xg) ? &sc : NULL;
        if (frames ? rmx_rollout_cost_frames(b, nsteps, q + f * nr * N, qd + f * nr * N, scp, terms ? &ft : NULL, &out)
                   : rmx_rollout_cost(b, nsteps, q + f * nr * N, qd + f * nr * N, scp, terms ? &pts : NULL, &out)) {
            if (terms) mxFree(terms);
            die_rmx(frames ? "rmx_rollout_cost_frames" : "rmx_rollout_cost");
        }
    }
    if (terms) mxFree(terms);
    mxArray* const res[3] = {Jk, lx, Qo};
    give(nlhs, plhs, res, 3);
}

/* a member of the `cost` struct of 'rollout_search': absent or [] (NULL), or a real double array of `want` (or `alt`) elements */
static const double* search_cost_field(const mxArray* c, const char* k, size_t want, size_t alt, int* per, const char* shape) {
    const mxArray* f = mxGetField(c, 0, k);
    if (!f || mxIsEmpty(f)) return NULL;
    const double* p = cost_arg(f, want, alt, 0, "rollout_search", k, shape);
    if (per) *per = alt && alt != want && mxGetNumberOfElements(f) == alt;
    return p;
}

/* 'rollout_search': rmx_rollout_search - the line search of iLQR in one launch.  cost: a struct with the fields Q, xgoal, R, terms,
 * xtarget, vtarget, Rtarget, each optional ([] or absent: that part is not there), shaped as 'rollout_cost_frames' takes them */
static void cmd_rollout_search(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    if (nrhs < 12 || nrhs == 13)
        die("usage: [qtraj,qdtraj,uapp,J,alpha,stats] = redmax_hip_mex('rollout_search', h, hstep, nsteps, pscale, ubar, kff, K, xref, alphas, "
            "Jbar, cost [, ulo, uhi])");
    rmx_opts o = tape_opts(mxGetScalar(prhs[2]));
    const int nsteps = (int)mxGetScalar(prhs[3]);
    if (nsteps < 1) die("rollout_search: nsteps must be at least 1");
    const double pscale = mxGetScalar(prhs[4]);
    const size_t nr = (size_t)h->nr, N = (size_t)nsteps, B = (size_t)h->B, per = nr * N;
    const double* ubar = traj_arg(prhs[5], h, nsteps, "ubar");
    const size_t nalpha = mxGetNumberOfElements(prhs[9]);
    if (nalpha && (!mxIsDouble(prhs[9]) || mxIsComplex(prhs[9]))) die("rollout_search: alphas must be a real double vector");
    if (nalpha > RMX_SEARCH_MAX_ALPHAS) die("rollout_search: at most 16 alphas");
    const double* kff = nalpha ? traj_arg(prhs[6], h, nsteps, "kff") : NULL;
    const double* Jbar = nalpha ? cost_arg(prhs[10], B, 0, 0, "rollout_search", "Jbar", "1 x batch") : NULL;
    int per_rollout = -1;
    const double* K = feedback_arg(prhs[7], h, 2 * nr * nr, nsteps, &per_rollout, "K");
    const double* xref = feedback_arg(prhs[8], h, 2 * nr, nsteps, &per_rollout, "xref");
    if (per_rollout < 0) per_rollout = 0;
    const mxArray* c = prhs[11];
    if (!mxIsStruct(c) || mxGetNumberOfElements(c) != 1) die("rollout_search: cost must be a struct with the fields Q, xgoal, R, terms, xtarget, vtarget, Rtarget");
    const size_t perq = 4 * nr * nr * N, perg = 2 * nr * N;
    int Q_per = 0, g_per = 0;
    const double* Qin = search_cost_field(c, "Q", perq, perq * B, &Q_per, "2nr x 2nr x nsteps or 2nr x 2nr x nsteps x batch");
    const double* xg = search_cost_field(c, "xgoal", perg, perg * B, &g_per, "2nr x nsteps or 2nr x nsteps x batch");
    const double* R = search_cost_field(c, "R", nr * nr, 0, NULL, "nr x nr");
    const mxArray* ta = mxGetField(c, 0, "terms");
    size_t nterms = 0;
    rmx_frame_term* terms = (ta && !mxIsEmpty(ta)) ? frame_terms(ta, "rollout_search", &nterms) : NULL;
    const size_t width[3] = {3 * nterms, 3 * nterms, 9 * nterms};
    const char* const tname[3] = {"xtarget", "vtarget", "Rtarget"};
    const double* tab[3] = {NULL, NULL, NULL};
    int t_per = -1;
    for (int k = 0; k < 3 && terms; ++k) {
        int p = 0;
        tab[k] = search_cost_field(c, tname[k], width[k], width[k] * B, &p, "3 (x 3) x nterms or 3 (x 3) x nterms x batch");
        if (!tab[k] || B == 1) continue;
        if (t_per >= 0 && p != t_per) {
            mxFree(terms);
            die("rollout_search: xtarget, vtarget and Rtarget must all be shared by the batch or all hold one table per rollout");
        }
        t_per = p;
    }
    if (t_per < 0) t_per = 0;
    rmx_box lim = {NULL, NULL};
    const int box = nrhs >= 14;
    if (box) {
        lim.ulo = bound_arg(prhs[12], h, "rollout_search", "ulo");
        lim.uhi = bound_arg(prhs[13], h, "rollout_search", "uhi");
    }
    const size_t dims[3] = {nr, N, B};
    mxArray* out[6];
    for (int i = 0; i < 3; ++i) out[i] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    out[3] = mxCreateDoubleMatrix(1, B, mxREAL);
    out[4] = mxCreateDoubleMatrix(1, B, mxREAL);
    out[5] = new_i32(B, 2);
    rmx_state_cost sc;
    rmx_frame_terms ft;
    memset(&sc, 0, sizeof sc);
    memset(&ft, 0, sizeof ft);
    sc.Q_per_rollout = Q_per;
    sc.goal_per_rollout = g_per;
    ft.nterms = (int)nterms;
    ft.terms = terms;
    ft.per_rollout = t_per;
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard, as 'rollout_feedback' */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        rmx_stats st_s = shard_stats(out[5], h, f);
        rmx_feedback fb;
        fb.uff = ubar + f * per;
        fb.K = table_at(K, per_rollout, f, per * 2 * nr);
        fb.xref = table_at(xref, per_rollout, f, per * 2);
        fb.per_rollout = per_rollout;
        sc.Q = table_at(Qin, Q_per, f, perq);
        sc.xgoal = table_at(xg, g_per, f, perg);
        ft.xtarget = table_at(tab[0], t_per, f, width[0]);
        ft.vtarget = table_at(tab[1], t_per, f, width[1]);
        ft.Rtarget = table_at(tab[2], t_per, f, width[2]);
        rmx_search_cost sco;
        sco.sc = (Qin || xg) ? &sc : NULL;
        sco.ft = terms ? &ft : NULL;
        sco.R = R;
        rmx_search sr;
        sr.kff = kff ? kff + f * per : NULL;
        sr.alphas = nalpha ? mxGetPr(prhs[9]) : NULL;
        sr.nalpha = (int)nalpha;
        sr.Jbar = Jbar ? Jbar + f : NULL;
        rmx_search_out so;
        so.J = mxGetPr(out[3]) + f;
        so.alpha = mxGetPr(out[4]) + f;
        so.trials = NULL;
        so.status = NULL;
        if (rmx_rollout_search(b, &o, nsteps, pscale, &fb, box ? &lim : NULL, &sr, &sco, mxGetPr(out[0]) + f * per, mxGetPr(out[1]) + f * per,
                               mxGetPr(out[2]) + f * per, &so, &st_s)) {
            if (terms) mxFree(terms);
            die_rmx("rmx_rollout_search");
        }
    }
    if (terms) mxFree(terms);
    h->tape_integ = 1;
    give(nlhs, plhs, out, 6);
}

static void cmd_rollout_frames(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    handle_t* h = get_handle(nrhs, prhs);
    const char* who = "rollout_frames";
    if (nrhs < 6) die("usage: [x,v,R,gq,gqd] = redmax_hip_mex('rollout_frames', h, nsteps, q, qdot, terms [, gx, gv, gR])");
    const int nsteps = (int)mxGetScalar(prhs[2]);
    if (nsteps < 1) die("rollout_frames: nsteps must be at least 1");
    const size_t nr = (size_t)h->nr, N = (size_t)nsteps, B = (size_t)h->B;
    const double* q = cost_arg(prhs[3], nr * N * B, 0, 0, who, "q", "nr x nsteps x batch");
    const double* qd = cost_arg(prhs[4], nr * N * B, 0, 0, who, "qdot", "nr x nsteps x batch");
    size_t nterms;
    rmx_frame_term* terms = frame_terms(prhs[5], who, &nterms);
    const double* gx = nrhs > 6 ? cost_arg(prhs[6], 3 * nterms * B, 0, 1, who, "gx", "3 x nterms x batch") : NULL;
    const double* gv = nrhs > 7 ? cost_arg(prhs[7], 3 * nterms * B, 0, 1, who, "gv", "3 x nterms x batch") : NULL;
    const double* gR = nrhs > 8 ? cost_arg(prhs[8], 9 * nterms * B, 0, 1, who, "gR", "3 x 3 x nterms x batch") : NULL;
    if (nlhs > 3 && !gx && !gv && !gR) die("rollout_frames: gq needs gx, gv or gR");
    const size_t dx[3] = {3, nterms, B}, dR[4] = {3, 3, nterms, B}, dg[3] = {nr, N, B};
    mxArray* x = mxCreateNumericArray(3, dx, mxDOUBLE_CLASS, mxREAL);
    mxArray* v = nlhs > 1 ? mxCreateNumericArray(3, dx, mxDOUBLE_CLASS, mxREAL) : NULL;
    mxArray* R = nlhs > 2 ? mxCreateNumericArray(4, dR, mxDOUBLE_CLASS, mxREAL) : NULL;
    mxArray* gq = nlhs > 3 ? mxCreateNumericArray(3, dg, mxDOUBLE_CLASS, mxREAL) : NULL;
    mxArray* gqd = nlhs > 4 ? mxCreateNumericArray(3, dg, mxDOUBLE_CLASS, mxREAL) : NULL;      /* (zeros without gv) */
    rmx_frame_terms ft;
    memset(&ft, 0, sizeof ft);
    ft.nterms = (int)nterms;
    ft.terms = terms;
    for (int s = 0; s < h->nshards; ++s) {     /* shard by shard: the record, the frames and the cotangents advance */
        size_t f;
        rmx_batch* b = shard(h, s, &f);
        if (rmx_rollout_frames(b, nsteps, q + f * nr * N, qd + f * nr * N, &ft, mxGetPr(x) + f * 3 * nterms, v ? mxGetPr(v) + f * 3 * nterms : NULL,
                               R ? mxGetPr(R) + f * 9 * nterms : NULL, (gq && gx) ? gx + f * 3 * nterms : NULL,
                               (gq && gv) ? gv + f * 3 * nterms : NULL, (gq && gR) ? gR + f * 9 * nterms : NULL,
                               gq ? mxGetPr(gq) + f * nr * N : NULL, (gqd && gv) ? mxGetPr(gqd) + f * nr * N : NULL)) {
            mxFree(terms);
            die_rmx("rmx_rollout_frames");
        }
    }
    mxFree(terms);
    mxArray* const out[5] = {x, v, R, gq, gqd};
    give(nlhs, plhs, out, 5);
}

/* `clear mex` / MATLAB exit: free what is still alive on the device */
static void at_exit(void) {
    for (int i = 0; i < MAX_LIVE; ++i)
        if (g_live[i]) {
            rmx_group_destroy(g_live[i]->g);
            mxFree(g_live[i]);
            g_live[i] = NULL;
        }
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    static int registered = 0;
    if (!registered) {
        mexAtExit(at_exit);
        registered = 1;
    }
    char cmd[24];      /* the command table: tests/test_mex_gateway.py checks that matlab/+redmax/HipSim.m uses these and only these */
    if (nrhs < 1 || mxGetString(prhs[0], cmd, sizeof cmd)) die("first argument must be a command string");
    /* include/redmax_hip.h "Asynchronous stepping": between a 'step_async' and its 'sync' only 'sync', 'timing', 'info' and 'destroy'
     * may name the handle ('step' / 'step_async' refuse with their own text).  Everything below reads or writes the state, the
     * scratch buffers or the counters of a launch in flight, and would clear its pending mark without taking the event time. */
    static const char* const needs_idle[] = {"set", "get", "gather", "euler", "eval", "values", "energy", "getcharts", "setcharts", "ticks",
                                             "adjoint", "adjoint_controls", "adjoint_track", "rollout_tape", "rollout_vjp", "rollout_linearize",
                                             "rollout_vjp_params", "rollout_vjp_forces", "rollout_jvp", "rollout_jvp_params", "rollout_feedback", "rollout_vjp_feedback", "rollout_lqr", "rollout_feedback_box", "rollout_lqr_box",
                                             "rollout_points", "rollout_cost", "rollout_frames", "rollout_cost_frames", "rollout_search", NULL};
    for (int i = 0; needs_idle[i]; ++i)
        if (!strcmp(cmd, needs_idle[i]) && get_handle(nrhs, prhs)->pending)
            mexErrMsgIdAndTxt("redmax:hip", "'%s' while a 'step_async' of this handle is in flight: 'sync' first", cmd);
    if (!strcmp(cmd, "version")) {
        plhs[0] = mxCreateDoubleScalar((double)rmx_version());
    } else if (!strcmp(cmd, "devices")) {
        plhs[0] = mxCreateDoubleScalar((double)rmx_device_count());
    } else if (!strcmp(cmd, "create")) {
        cmd_create(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "destroy")) {
        cmd_destroy(nrhs, prhs);
    } else if (!strcmp(cmd, "info")) {
        cmd_info(plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "set")) {
        handle_t* h = get_handle(nrhs, prhs);
        if (nrhs < 4) die("usage: redmax_hip_mex('set', h, q, qdot)");
        if (rmx_group_set_state(h->g, state_arg(prhs[2], h, "q"), state_arg(prhs[3], h, "qdot"))) die_rmx("rmx_group_set_state");
    } else if (!strcmp(cmd, "get")) {
        handle_t* h = get_handle(nrhs, prhs);
        mxArray* q = mxCreateDoubleMatrix((size_t)h->nr, (size_t)h->B, mxREAL);
        mxArray* qd = mxCreateDoubleMatrix((size_t)h->nr, (size_t)h->B, mxREAL);
        if (rmx_group_get_state(h->g, mxGetPr(q), mxGetPr(qd))) die_rmx("rmx_group_get_state");
        plhs[0] = q;
        if (nlhs > 1) plhs[1] = qd;
    } else if (!strcmp(cmd, "step")) {
        cmd_step(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "step_async")) {
        cmd_step_async(nrhs, prhs);
    } else if (!strcmp(cmd, "sync")) {
        cmd_sync(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "timing")) {
        handle_t* h = get_handle(nrhs, prhs);
        mxArray* k = mxCreateDoubleMatrix(1, (size_t)h->nshards, mxREAL);
        mxArray* t0 = mxCreateDoubleMatrix(1, (size_t)h->nshards, mxREAL);
        mxArray* t1 = mxCreateDoubleMatrix(1, (size_t)h->nshards, mxREAL);
        double wall = 0.0;
        if (rmx_group_timing(h->g, &wall, mxGetPr(k), mxGetPr(t0), mxGetPr(t1))) die_rmx("rmx_group_timing");
        plhs[0] = mxCreateDoubleScalar(wall);
        if (nlhs > 1) plhs[1] = k;
        if (nlhs > 2) plhs[2] = t0;
        if (nlhs > 3) plhs[3] = t1;
    } else if (!strcmp(cmd, "euler")) {
        cmd_euler(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "eval")) {
        cmd_eval(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "values")) {
        cmd_values(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "energy")) {
        handle_t* h = get_handle(nrhs, prhs);
        mxArray* T = mxCreateDoubleMatrix(1, (size_t)h->B, mxREAL);
        mxArray* V = mxCreateDoubleMatrix(1, (size_t)h->B, mxREAL);
        if (rmx_group_energy(h->g, mxGetPr(T), mxGetPr(V))) die_rmx("rmx_group_energy");
        plhs[0] = T;
        if (nlhs > 1) plhs[1] = V;
    } else if (!strcmp(cmd, "gather")) {
        /* [q, qdot, path] = redmax_hip_mex('gather', h [, root]): the final gather of the sharded batch with DEVICE-resident destinations
         * (rmx_group_gather: RCCL over the group's devices, copies when a device is listed twice) - every shard's device (root omitted or
         * < 0) or shard `root`'s device alone ends up with the whole batch; q, qdot: that device copy read back (nr x batch), what a host
         * with gpuArray support would wrap in place (rmx_group_gathered); path: how the gather travelled (rmx_group_gather_path) */
        handle_t* h = get_handle(nrhs, prhs);
        const int root = (nrhs > 2 && mxGetScalar(prhs[2]) >= 0.0) ? (int)mxGetScalar(prhs[2]) : RMX_GATHER_ALL;
        if (rmx_group_gather(h->g, root)) die_rmx("rmx_group_gather");
        mxArray* q = mxCreateDoubleMatrix((size_t)h->nr, (size_t)h->B, mxREAL);
        mxArray* qd = mxCreateDoubleMatrix((size_t)h->nr, (size_t)h->B, mxREAL);
        if (rmx_group_gathered_read(h->g, root >= 0 ? root : 0, mxGetPr(q), mxGetPr(qd))) die_rmx("rmx_group_gathered_read");
        plhs[0] = q;
        if (nlhs > 1) plhs[1] = qd;
        if (nlhs > 2) plhs[2] = mxCreateString(rmx_group_gather_path(h->g));
    } else if (!strcmp(cmd, "getcharts")) {
        handle_t* h = get_handle(nrhs, prhs);
        mxArray* c = new_i32((size_t)h->nsph, (size_t)h->B);
        for (int s = 0; s < h->nshards && h->nsph; ++s) {
            size_t f;
            rmx_batch* b = shard(h, s, &f);
            if (rmx_get_charts(b, (int*)mxGetData(c) + f * (size_t)h->nsph)) die_rmx("rmx_get_charts");
        }
        plhs[0] = c;
    } else if (!strcmp(cmd, "setcharts")) {
        handle_t* h = get_handle(nrhs, prhs);
        if (nrhs < 3 || !mxIsInt32(prhs[2]) || mxGetNumberOfElements(prhs[2]) != (size_t)h->nsph * (size_t)h->B)
            die("charts must be an int32 nsph x batch array");
        for (int s = 0; s < h->nshards && h->nsph; ++s) {
            size_t f;
            rmx_batch* b = shard(h, s, &f);
            if (rmx_set_charts(b, (const int*)mxGetData(prhs[2]) + f * (size_t)h->nsph)) die_rmx("rmx_set_charts");
        }
    } else if (!strcmp(cmd, "ticks")) {      /* t = redmax_hip_mex('ticks', h): per-rollout share of the last step launch (rmx_step_ticks) */
        handle_t* h = get_handle(nrhs, prhs);
        unsigned long long* t = (unsigned long long*)mxCalloc((size_t)h->B, sizeof *t);
        for (int s = 0; s < h->nshards; ++s) {
            size_t f;
            rmx_batch* b = shard(h, s, &f);
            if (rmx_step_ticks(b, t + f)) { mxFree(t); die_rmx("rmx_step_ticks"); }
        }
        mxArray* out = mxCreateDoubleMatrix(1, (size_t)h->B, mxREAL);
        for (int i = 0; i < h->B; ++i) mxGetPr(out)[i] = (double)t[i];
        mxFree(t);
        plhs[0] = out;
    } else if (!strcmp(cmd, "tape_point_forces")) {      /* on = redmax_hip_mex('tape_point_forces', h, enable) */
        handle_t* h = get_handle(nrhs, prhs);
        if (nrhs < 3 || mxGetNumberOfElements(prhs[2]) != 1) die("tape_point_forces: enable must be a scalar, 0 or 1");
        const double en = mxGetScalar(prhs[2]);
        if (en != 0.0 && en != 1.0) die("tape_point_forces: enable must be 0 or 1");
        for (int s = 0; s < h->nshards; ++s)
            if (rmx_model_tape_point_forces(rmx_group_shard_model(h->g, s), (int)en)) die_rmx("rmx_model_tape_point_forces");
        if (nlhs > 0) plhs[0] = mxCreateDoubleScalar((double)rmx_model_get_tape_point_forces(rmx_group_shard_model(h->g, 0)));
    } else if (!strcmp(cmd, "adjoint")) {
        cmd_adjoint(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "adjoint_controls")) {
        cmd_adjoint_controls(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "adjoint_track")) {
        cmd_adjoint_track(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_tape")) {
        cmd_rollout_tape(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_feedback")) {
        cmd_rollout_feedback(nlhs, plhs, nrhs, prhs, 0);
    } else if (!strcmp(cmd, "rollout_vjp")) {
        cmd_rollout_vjp(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_vjp_feedback")) {
        cmd_rollout_vjp_feedback(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_linearize")) {
        cmd_rollout_linearize(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_vjp_params")) {
        cmd_rollout_vjp_params(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_vjp_forces")) {
        cmd_rollout_vjp_forces(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_jvp")) {
        cmd_rollout_jvp(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_jvp_params")) {
        cmd_rollout_jvp_params(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_lqr")) {
        cmd_rollout_lqr(nlhs, plhs, nrhs, prhs, 0);
    } else if (!strcmp(cmd, "rollout_feedback_box")) {
        cmd_rollout_feedback(nlhs, plhs, nrhs, prhs, 1);
    } else if (!strcmp(cmd, "rollout_lqr_box")) {
        cmd_rollout_lqr(nlhs, plhs, nrhs, prhs, 1);
    } else if (!strcmp(cmd, "rollout_points")) {
        cmd_rollout_points(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_cost")) {
        cmd_rollout_cost(nlhs, plhs, nrhs, prhs, 0);
    } else if (!strcmp(cmd, "rollout_frames")) {
        cmd_rollout_frames(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_search")) {
        cmd_rollout_search(nlhs, plhs, nrhs, prhs);
    } else if (!strcmp(cmd, "rollout_cost_frames")) {
        cmd_rollout_cost(nlhs, plhs, nrhs, prhs, 1);
    } else {
        mexErrMsgIdAndTxt("redmax:hip", "unknown command '%s'", cmd);
    }
}
