/*
 * redmax_hip.h -- C ABI of the MI355X-native batched RedMax BDF1/BDF2 forward-dynamics step.
 *
 * The reference (sueda/redmax) has no plugin / FFI / MEX boundary for this path: everything runs
 * inside one MATLAB interpreter.  The seam this library replaces is the body of
 *     simLoop(scene)                     matlab-diff/driverRedMaxBDF1.m:57-91
 *       newton(@(q1)evalBDF1(q1,scene))  driverRedMaxBDF1.m:94-157, 160-187
 *         computeValues(scene)           driverRedMaxBDF1.m:190-243
 *           Joint.update / computeJacobian / computeForce   +redmax/Joint.m:382-613
 *           Body.update / computeMassGrav                   +redmax/Body.m:70-135
 *           se3.Ad / ad / inv / aaToMat                     se3.m:11-176
 * re-expressed as a batch over independent trajectories of ONE scene.  Each entry point cites the
 * reference code it stands in for.  A MATLAB MEX gateway or any other host binds
 * these symbols; the in-repo host is the ctypes mirror in redmax_amd/.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  No exceptions cross the boundary.
 *   - every function returns 0 on success, a negative RMX_E_* code otherwise; rmx_last_error()
 *     gives the text.  Numerical failure (Newton diverged / not converged) is NOT an error: like
 *     the reference (driverRedMaxBDF1.m:118-121,150-153: print and continue) it is reported per
 *     trajectory in the stats arrays and stepping continues.
 *   - all 4x4 transforms are COLUMN-MAJOR (what MATLAB's mxGetPr returns for a 4x4 double).
 *   - reduced vectors use the reference's leaf-to-root DOF numbering (Scene.m:65-71): the LAST
 *     listed joint owns index 0.  Batched arrays are [batch][nr], trajectory-major, fp64.
 *   - matrices returned by rmx_eval are nr x nr COLUMN-MAJOR per trajectory ([batch][nr*nr]).
 *   - host pointers are copied in/out and never retained; the library owns device memory.
 *   - there is NO CPU fallback: without a usable HIP device every create call fails loudly.
 */
#ifndef REDMAX_HIP_H
#define REDMAX_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define RMX_VERSION 111

enum {
    RMX_OK = 0,
    RMX_E_INVALID = -1,     /* bad argument / unsupported scene                        */
    RMX_E_NODEVICE = -2,    /* no HIP device (there is no CPU fallback)                */
    RMX_E_HIP = -3,         /* HIP runtime error, see rmx_last_error()                 */
    RMX_E_NOMEM = -4
};

enum {
    RMX_JOINT_FIXED = 0,          /* JointFixed.m                                                              */
    RMX_JOINT_REVOLUTE = 1,       /* JointRevolute.m    (axis)                                                 */
    RMX_JOINT_PRISMATIC = 2,      /* JointPrismatic.m   (axis)                                                 */
    RMX_JOINT_PLANAR = 3,         /* JointPlanar.m        2 DOF, p = B q            (plane, default x-y)       */
    RMX_JOINT_TRANSLATIONAL = 4,  /* JointTranslational.m 3 DOF, p = q                                         */
    RMX_JOINT_UNIVERSAL = 5,      /* JointUniversal.m     2 DOF, R = X(q1) Y(q2)                               */
    RMX_JOINT_FREE2D = 6,         /* JointFree2D.m        3 DOF, Q = [Rz(q3) [q1;q2;0]]                        */
    RMX_JOINT_SPHERICAL = 7,      /* JointSpherical.m     3 DOF, Euler angles in 12 switching charts           */
    RMX_JOINT_FREE3D = 8          /* JointFree3D.m        6 DOF, JointTranslational then JointSpherical        */
};

/* rmx_stats.status bits */
/* RMX_ST_STALLED accompanies RMX_ST_MAXITER when the Newton iteration reached a floating-point fixed point
 * (alpha*dx below one ulp of x): the reference repeats that identical iteration until iterMax and keeps x;
 * the library returns the same x without spinning. */
/* RMX_ST_PIVOTED is informational: at least one linear solve tripped the diagonal-pivot growth guard and was redone
 * with full partial pivoting (see rmx_device.h lu_solve_neg_diag). */
enum { RMX_ST_DIVERGED = 1, RMX_ST_MAXITER = 2, RMX_ST_NAN = 4, RMX_ST_STALLED = 8, RMX_ST_PIVOTED = 16,
       RMX_ST_CHART = 32 /* informational: a JointSpherical changed its Euler chart (the reference prints 'XYZ->YXZ') */,
       RMX_ST_LS_CUT = 128 /* with RMX_ST_MAXITER: rmx_opts.ls_fail_limit ended the Newton loop of a step (off by default) */,
       RMX_ST_COOP_FAULT = 512 /* with RMX_ST_NAN, chains with ForceGroundCuboid only: the wavefronts that share a creeping line search
                                  (DESIGN.md "Chains with ground contact") waited in vain for each other, or a rollout handed to them was
                                  never picked up; the rollout's state is NaN.  Never observed: a guard, not a code path of the method.
                                  (Bits 64 and 256 are internal to the kernels and never reach rmx_stats.status.) */ };

/* Scene listing, one entry per joint/body pair in the order the scene file lists them
 * (parent before child; scenesRedMax.m).  Replaces the handle-object graph that Scene.init()
 * links up (Scene.m:59-119).  Arrays are [njoints] unless noted. */
typedef struct rmx_model_desc {
    int njoints;
    const int* parent;       /* parent joint index, -1 for the root          Joint.m:56-92       */
    const int* type;         /* RMX_JOINT_*                                   JointRevolute/Prismatic/Fixed.m */
    const double* axis;      /* [n][3] unit joint axis                        JointRevolute.m:14   */
    const double* E0_pj;     /* [n][16] joint wrt parent joint at q=0         Joint.setJointTransform :95-99 */
    const double* E0_ji;     /* [n][16] body wrt joint                        Body.setBodyTransform :46-51   */
    const double* I_i;       /* [n][6] diagonal body inertia                  se3.inertiaCuboid :366-379     */
    const double* qRest;     /* rest position of the joint spring (= initial q, Joint.m:157)     */
    const double* tau;       /* joint torque                                  Joint.m:446          */
    const double* stiffness; /* Joint.setStiffness                                                 */
    const double* damping;   /* Joint.setDamping                                                   */
    const double* qLimL;     /* joint limits                                  Joint.m:449-454      */
    const double* qLimU;
    const double* qLimK;
    const double* qLimD;
    double grav[3];          /* Scene.grav                                    Scene.m:48           */
    /* multi-DOF joints (may be NULL when the scene has none) */
    const double* plane;     /* [n][6] JointPlanar: the two in-plane directions b1, b2 (normalised by the caller,
                                JointPlanar.m:16-17); NULL = x-y plane                              */
    const double* qRestR;    /* [nr] rest position of EVERY DOF in reduced order (Joint.m:157 qRest = q); overrides qRest.
                                qRest[n] alone only reaches the first DOF of a multi-DOF joint      */
} rmx_model_desc;

/* Newton constants of driverRedMaxBDF1.m:95-98; rmx_opts_default() fills the reference values. */
typedef struct rmx_opts {
    double h;              /* time step (Scene.h)                                  */
    double tol;            /* 1e-9   ||g||_2 convergence threshold                 */
    double dxMax;          /* 1e3    "Newton diverged" threshold on ||dx||_2       */
    int iterMaxPerDof;     /* 10     iterMax = iterMaxPerDof * nr                  */
    int iterLsMax;         /* 20     line-search halvings                          */
    int lu_mode;           /* dx = -H\g (driverRedMaxBDF1.m:117, LU with partial pivoting in MATLAB):
                              0 (default) eliminate on the diagonal under a growth guard (|multiplier| <= 8 on the symmetrically
                                equilibrated matrix, i.e. threshold pivoting with tau = 1/8; trees of up to 64 nodes also require
                                positive pivots, larger trees - blocked LU, rmx_big.hip big_solve_diag - take pivots of either sign)
                                and redo the solve with full partial pivoting when the guard trips (RMX_ST_PIVOTED);
                              1 always full partial pivoting (the reference behaviour, ~2x slower solve).  The pivot search compares
                                |H(a,k)| as full doubles, lowest row first among equals: LAPACK's first maximum (idamax in dgetf2),
                                in every kernel of the library (ABI 108; up to ABI 107 the one-wavefront kernels compared the top 26
                                bits only); the elimination scales by the reciprocal of the pivot, as dgetf2 does  */
    int compensated;       /* the Newton iterate of newton() (driverRedMaxBDF1.m:94-157):
                              1 (default) carried as an unevaluated sum x + xlo, |xlo| <= ulp(x)/2; xlo enters the residual where x
                                enters linearly with large coefficients (dqtmp = q1 - q0 - h qdot0 and qdot1 = (q1 - q0)/h,
                                :167-169) and nowhere else, and is dropped when the step stores q1.  On long chains in cgs units
                                |M| ulp(q) reaches the reference's tol = 1e-9: on the lattice of doubles ||g|| < tol is then met only
                                at lucky points, which MATLAB's Newton finds because its own evaluation noise dithers the update
                                and a smoother evaluation does not.  With xlo no Newton correction is lost to
                                the rounding of x and the iteration converges to the evaluation noise, at the reference's constants;
                              0 plain doubles: the reference's arithmetic, decision for decision  */
    int ls_fail_limit;     /* straggler policy for batches, 0 (default) = off = the reference: newton() keeps iterating after a line
                              search that ran out its iterLsMax trials without a decrease of ||g|| (:126-138), up to iterMax = 10 nr
                              times - at a non-smooth point of the residual (stick/slip or touch-down of a ground contact) every one of
                              them fails or creeps the same way, ~4600 evaluations for one step of one rollout, and the launch of a whole
                              batch ends with its slowest wavefront.  N > 0: the Newton loop of a step ends ("did not converge", status
                              RMX_ST_MAXITER | RMX_ST_LS_CUT) at the N-th failed line search of that step (failed and barely
                              successful ones alternate at such a point, so they are not required to be consecutive); the iterate
                              is the one that line search left (x0 + 2^-19 dx, as in the reference).  The state after such a step
                              differs from the reference's by the drift of the iterations not run; a step in which no line search
                              fails N times runs exactly as without the option  */
} rmx_opts;

typedef struct rmx_model rmx_model;
typedef struct rmx_batch rmx_batch;

const char* rmx_last_error(void);
int rmx_version(void);
int rmx_device_count(void);
void rmx_opts_default(rmx_opts* o);

/* Scene.init(): validates the listing, orders it depth-first, counts DOFs leaf-to-root and uploads
 * the constant per-joint data.  (Scene.m:59-119, Joint.countDofs :149-158, Body.countDofs :54-60) */
int rmx_model_create(const rmx_model_desc* desc, int device, rmx_model** out);
void rmx_model_destroy(rmx_model* m);
int rmx_model_nr(const rmx_model* m);      /* redmax.Scene.countR()  Scene.m:410-421 */
int rmx_model_nm(const rmx_model* m);      /* redmax.Scene.countM()  Scene.m:398-409 */
/* idx[n]: reduced index of each listed joint, -1 for a fixed joint (Joint.idxR) */
int rmx_model_idxR(const rmx_model* m, int* idx);

/* ForceGroundCuboid (matlab-diff/+redmax/ForceGroundCuboid.m:18-48, 54-183): penalty ground contact with Coulomb friction
 * on the 8 corners of the flagged cuboid bodies -- normal spring kn and damper kd, tangential stick spring kt, friction mu
 * (static/dynamic branch per corner, :112-150), energy 0.5 kn d^2 (:176).  Replaces, for one ground frame per scene,
 *     f = redmax.ForceGroundCuboid(body); f.setTransform(E); f.setStiffness(kn,kt); f.setDamping(kd); f.setFriction(mu);
 * (scenesRedMax.m:303-309).  Arrays follow the scene listing like rmx_model_desc.  Call before stepping; BDF1/BDF2/eval/energy
 * honour it, rmx_step_euler and rmx_adjoint_bdf1 refuse such a model.  All flags zero removes the contact.
 * The reference keeps its force objects in a list (Force.m:26-56) and a body may carry several (a floor and a wall).  This struct
 * holds ONE object per listing entry: a host lists every further force of a body as an extra entry of rmx_model_desc - a
 * RMX_JOINT_FIXED child of the body's joint, E0_pj = identity, E0_ji and sides those of the body, I_i = 0 - flagged here with its own
 * frame and constants.  Same corners, same twist: the same wrench, K and D through the same Jacobian rows; no DOF is added
 * (redmax_amd.Scene.desc() and matlab/+redmax/flattenScene.m do this; tests/test_oracle_fd.py, tests/test_gpu_contact.py). */
typedef struct rmx_ground_contact {
    const int* flags;        /* [n] 1: this body carries a ForceGroundCuboid                       */
    const double* sides;     /* [n][3] cuboid side lengths (BodyCuboid.sides)  ForceGroundCuboid.m:71-75 */
    double E[16];            /* ground frame, column-major 4x4; its Z axis is the plane normal    :30-32, 56-57 */
    double kn, kt;           /* setStiffness(kn, kt)   :35-38 */
    double mu;               /* setFriction(mu)        :46-48 */
    double kd;               /* setDamping(kd)         :41-43 */
    /* Every ForceGroundCuboid object holds its own E, kn, kt, mu, kd (:6-13): scenes whose force objects differ (a floor and a wall,
     * a slippery patch) pass them per body, in listing order; NULL = the shared value above for every flagged body (ABI 106). */
    const double* E_body;    /* [n][16] column-major 4x4 per body, or NULL */
    const double* kn_body;   /* [n] or NULL */
    const double* kt_body;   /* [n] or NULL */
    const double* mu_body;   /* [n] or NULL */
    const double* kd_body;   /* [n] or NULL */
} rmx_ground_contact;
int rmx_model_set_ground_contact(rmx_model* m, const rmx_ground_contact* gc);

/* Body-to-body forces of the reference, acting between points of two (or, for a cable, several) bodies:
 *   RMX_PF_POINTPOINT    ForcePointPoint(body1, x1, body2, x2)    f = ks dx + kd dv, V = ks |dx|^2 / 2      (ForcePointPoint.m:50-133)
 *   RMX_PF_SPRINGDAMPER  ForceSpringDamper(body1, x1, body2, x2)  fs = k (l - L)/L + d ldot/L, V = k/2 ((l - L)/L)^2 L
 *                                                                  (ForceSpringGeneric.m:37-176, ForceSpringDamper.m:37-71)
 *   RMX_PF_CABLE         ForceCable() + addBodyPoint(body, x)     the same law on the TOTAL length of a polyline through npts points,
 *                                                                  zero while slack (ForceSpringMultiPointGeneric.m:28-190, ForceCable.m:37-82)
 * body[k] is the index of the point's body in the caller's joint listing (a multi-DOF joint's body: its last node), -1 the world;
 * x[k] the point in the body's frame.  L is the rest length of kinds 1, 2 and must be > 0 (the host computes it from the initial
 * configuration as Force.init does unless setRetLength gave one); kind 0 ignores it.  setStiffness / setDamping: stiffness, damping.
 * The forces enter rmx_eval (g and H), rmx_step_bdf1 / rmx_step_bdf2 / rmx_step_history (and their _async forms) and the potential
 * energy of rmx_energy and of the per-step record.  A spring between bodies on different branches makes H dense: such a model always
 * takes the dense elimination order under the growth guard (RMX_ST_PIVOTED may be set).
 * Limits: at most RMX_PF_MAX_FORCES forces, 2 .. RMX_PF_MAX_POINTS points per force, RMX_PF_MAX_TOTAL points in all; models of at
 * most 64 nodes after lowering.  Refused with RMX_E_INVALID: beyond those limits; together with ForceGroundCuboid or JointSpherical /
 * JointFree3D in one model; and, for a model that has point forces, rmx_step_euler, rmx_adjoint_*, rmx_eval_mfd and
 * rmx_compute_values.  rmx_group_create has no slot for them.  nforces = 0 removes the forces.  Call before stepping. */
enum { RMX_PF_POINTPOINT = 0, RMX_PF_SPRINGDAMPER = 1, RMX_PF_CABLE = 2 };
enum { RMX_PF_MAX_FORCES = 32, RMX_PF_MAX_POINTS = 8, RMX_PF_MAX_TOTAL = 128 };
typedef struct rmx_point_force {
    int kind;                /* RMX_PF_*                                              */
    int npts;                /* 2 (kinds 0, 1) or 2 .. RMX_PF_MAX_POINTS (cable)     */
    const int* body;         /* [npts] listing index of each point's body, -1 = world */
    const double* x;         /* [npts][3] the points in their bodies' frames          */
    double stiffness, damping, L;
} rmx_point_force;
int rmx_model_set_point_forces(rmx_model* m, const rmx_point_force* f, int nforces);

/* JointSpherical / JointFree3D (JointSpherical.m:4-17, 28-34, 63-102): every such joint is in one of 12 Euler charts, numbered as
 * the reference's CHART_* constants (1 XYX, 2 XZX, 3 YZY, 4 YXY, 5 ZXZ, 6 ZYZ, 7 XYZ, 8 XZY, 9 YZX, 10 YXZ, 11 ZXY, 12 ZYX) and
 * constructed in CHART_XYZ.  rmx_step_bdf1/bdf2 run reparam_ after every step per trajectory (status bit RMX_ST_CHART when a
 * chart changed), so q/qdot returned by rmx_get_state are coordinates in the charts rmx_get_charts reports.  rmx_set_state
 * puts every joint back to CHART_XYZ; rmx_set_charts (after it) declares other charts for the given coordinates.
 * charts: host [batch][nsph], spherical joints in listing order.  rmx_step_euler / rmx_adjoint_bdf1 refuse such models.  A scene may
 * hold as many JointSpherical / JointFree3D joints as its node limit allows (256 nodes: 85; ABI 109 - 21 up to ABI 108). */
int rmx_model_nsph(const rmx_model* m);
int rmx_get_charts(rmx_batch* b, int* charts);
int rmx_set_charts(rmx_batch* b, const int* charts);

/* `batch` independent trajectories of the model, state resident in HBM on the model's device. */
int rmx_batch_create(rmx_model* m, int batch, rmx_batch** out);
void rmx_batch_destroy(rmx_batch* b);
int rmx_batch_size(const rmx_batch* b);

/* Joint.setQ / Joint.getQ (Joint.m:173-292) for the whole batch: host arrays [batch][nr]. */
int rmx_set_state(rmx_batch* b, const double* q, const double* qdot);
int rmx_get_state(rmx_batch* b, double* q, double* qdot);
/* Same, with DEVICE pointers (no host round trip; used to feed the final RCCL gather). */
int rmx_set_state_device(rmx_batch* b, const double* d_q, const double* d_qdot);
int rmx_get_state_device(rmx_batch* b, double* d_q, double* d_qdot);

/* Parity hook = evalBDF1 / evalSDIRK2a / evalSDIRK2b / evalBDF2 (driverRedMaxBDF1.m:160-187,
 * driverRedMaxBDF2.m:194-293) in their common form
 *     qdot = (q - qA)/eta ;  dqtmp = q - qB ;  g = M dqtmp - eta^2 f ;  H = M - eta D - eta^2 K + dMdq dqtmp
 * evaluated for every trajectory.  BDF1: eta = h, qA = q0, qB = q0 + h qdot0.
 * q,qA,qB: host [batch][nr].  g: host [batch][nr].  H: host [batch][nr*nr] column-major or NULL
 * (NULL selects the cheap residual-only path, nargout==1 in the reference).  Does not change state. */
int rmx_eval(rmx_batch* b, const double* q, const double* qA, const double* qB, double eta,
             double* g, double* H);

/* Parity hook = computeValues (driverRedMaxBDF1.m:190-243) at (q, qdot) for every trajectory: the reduced mass matrix
 * M = J'MmJ (:212), the force vector f = fr + J'(fm - Mm Jdot qdot) (:215-216) and D = df/dqdot (:227-237).  q, qdot, f: host
 * [batch][nr]; M, D: host [batch][nr*nr] column-major.  K = df/dq is not returned on its own: it only exists folded into H
 * (rmx_eval gives H = M - eta D - eta^2 K + dMdq dqtmp).  Spherical joints: in the coordinates of the batch's current Euler charts
 * (rmx_get_charts).  ForceGroundCuboid: its wrench is part of f, its damping block J' Dm J part of D (ForceGroundCuboid.m:104-106).
 * Does not change state. */
int rmx_eval_mfd(rmx_batch* b, const double* q, const double* qdot, double* M, double* f, double* D);

/* computeValues' FULL output, [M, f, dMdq, K, D] (driverRedMaxBDF1.m:188-243), at (q, qdot) for every trajectory, for trees of ANY
 * size the library takes (ABI 108).  Every output may be NULL.
 *   M, D, K : [batch][nr*nr] column-major;  K = df/dq (:239-243: Kr + J'KmJ + Kqvv + the dJdq terms), D = df/dqdot, M = J'MmJ
 *   f       : [batch][nr]
 *   dMv     : [batch][nr*nr] column-major, column i = dMdq(:,:,i) v for the caller's v [batch][nr] - the form in which evalBDF1
 *             consumes the tensor (:181-184, v = dqtmp); needs v
 *   dMdq    : the tensor itself, [batch][nr*nr*nr], entry (r, c, i) at r + nr (c + nr i)  (nr evaluations: a test hook)
 * The world-frame kernels never form K, D or the tensor on their own: H(eta; v) = M + dMdq v - eta D - eta^2 K is what
 * they evaluate, exactly, for any eta and v.  This hook takes the pieces apart on the host from a few such evaluations at the SAME
 * (q, qdot) (qA = q - eta qdot): v = 0 at eta = 1 (and 2, 1/2 for trees of more than 64 nodes, where M and D have no kernel of their
 * own) gives M, D, K; one more with the caller's v gives dMv = H(1; v) - H(1; 0).
 * Accuracy: up to 64 nodes M and D come from their own kernel and K = (M - D) - H(1; 0) carries an absolute error of order eps |M|.  Larger
 * trees: an evaluation of H(eta) carries roundoff of order eps (|M| + eta |D| + eta^2 |K|), so each piece is taken from a triple H(e),
 * H(2 e), H(e / 2) at its own power-of-two e - K at e_K ~ sqrt(|M| / |K|), D at min(|M| / |D|, e_K), M at the smallest of these and 1 - which
 * leaves every piece with an error of order eps times ITS OWN norm (plus the cross terms eps |D| sqrt(|K| / |M|) in K and
 * eps sqrt(|M| |K|) in D); 3 to 9 evaluations (ABI 109; ABI 108 took all three at e = 1: eps |M| absolute in D and K).  Same conventions as rmx_eval_mfd for Euler
 * charts and ForceGroundCuboid.  Does not change state. */
int rmx_compute_values(rmx_batch* b, const double* q, const double* qdot, const double* v,
                       double* M, double* f, double* D, double* K, double* dMv, double* dMdq);

/* Per-trajectory counters of one rmx_step_* call (host arrays [batch], any may be NULL). */
typedef struct rmx_stats {
    int* newton_iters;   /* Newton iterations summed over the steps                    */
    int* ls_halvings;    /* line-search halvings summed over the steps                 */
    int* status;         /* OR of RMX_ST_* over the steps                              */
} rmx_stats;

/* simLoop of driverRedMaxBDF1.m:57-91: nsteps fully-implicit BDF1 steps for every trajectory in ONE
 * kernel launch (trajectories are independent, so the step loop runs on the device).
 * hist_T/hist_V: optional host [nsteps][batch] kinetic / potential energy after each step
 * (Scene.saveHistory, Scene.m:134-161; Joint/Body.computeEnergies).  May be NULL. */
int rmx_step_bdf1(rmx_batch* b, const rmx_opts* opts, int nsteps, rmx_stats* stats,
                  double* hist_T, double* hist_V);

/* The same two loops with the full per-step record of Scene.saveHistory (Scene.m:134-161: q, qdot, T, V after every step;
 * t = k*h).  integrator: 1 = BDF1 (driverRedMaxBDF1.m), 2 = BDF2 (driverRedMaxBDF2.m), the reference's itype numbering
 * (scenesRedMax.m:5-6).  Host arrays, any pair may be NULL. */
typedef struct rmx_history {
    double* T;       /* [nsteps][batch]      kinetic energy   (with V)      */
    double* V;       /* [nsteps][batch]      potential energy                */
    double* q;       /* [nsteps][batch][nr]  reduced positions (with qdot)   */
    double* qdot;    /* [nsteps][batch][nr]  reduced velocities              */
    int* charts;     /* [nsteps][batch][nsph] Euler chart (1..12) of every JointSpherical / JointFree3D after each step, i.e. the
                        chart the step's q / qdot are expressed in (the reference keeps chart and q together on the joint,
                        JointSpherical.m:28-34; its own history has a TODO for it, Scene.m:138).  May be NULL; ignored when the
                        model has no spherical joint */
} rmx_history;
int rmx_step_history(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, rmx_stats* stats,
                     const rmx_history* hist);

/* simLoop of driverRedMaxBDF2.m:57-125: the first call after set_state takes the SDIRK2 start step
 * (two Newton solves, :64-88), later steps are BDF2 (:89-106).  The batch keeps (q,qdot) of step k-1. */
int rmx_step_bdf2(rmx_batch* b, const rmx_opts* opts, int nsteps, rmx_stats* stats,
                  double* hist_T, double* hist_V);

/* TaskBDF1PointPos (matlab-diff/+redmax/TaskBDF1PointPos.m): bring a point of a body to a world target at one step;
 * the parameters are constant joint torques tau = pscale * p. */
typedef struct rmx_task_pointpos {
    int body;              /* listing index of the body             setBody                       */
    double xlocal[3];      /* point in body coordinates             setPoint                      */
    double xtarget[3];     /* world target                          setTarget                     */
    int step;              /* 1-based step at which the point is measured (setTime: step = round(t/h)) */
    double pscale;         /* torque scale                          setScale                      */
    double wreg, wpos;     /* regulariser / position weights        setWeights                    */
} rmx_task_pointpos;

/* taskObjective of driverRedMaxAdjointBDF1.m:39-62, batched (BASELINE.json configs[3]): starting from the batch's current
 * state, forward simLoop (:65-102) with the line-search-free newton (:105-146; opts->iterMaxPerDof should be 5 as at :108)
 * under the torques tau = pscale*p, storing H, M, D of the last evaluated iterate of every step in HBM, then the backward
 * sweep TaskBDF1.calcFinal (TaskBDF1.m:45-81).  p: host [batch][nr]; P: host [batch]; dPdp: host [batch][nr].
 * The batch state is left at the end of the forward rollout.  The forward solves take diagonal pivots under the growth guard
 * first, as the step kernels do (RMX_ST_PIVOTED in stats->status when one was redone with partial pivoting; the reference's
 * lu(H,'vector') always pivots, :127). */
int rmx_adjoint_bdf1(rmx_batch* b, const rmx_opts* opts, int nsteps, const rmx_task_pointpos* task, const double* p,
                     double* P, double* dPdp, rmx_stats* stats);

/* The same for driverRedMaxAdjointBDF2.m:38-62 with TaskBDF2 / TaskBDF2PointPos (matlab-diff/+redmax/TaskBDF2.m, TaskBDF2PointPos.m;
 * scene 101, scenesRedMax.m:437-471): the forward simLoop (:65-136) takes the SDIRK2a / SDIRK2b start step and BDF2 steps with the
 * line-search-free newton (:139-181), the backward sweep is TaskBDF2.calcFinal (TaskBDF2.m:45-107: four off-diagonal blocks per
 * step, the k == 1 variants with the SDIRK2 coefficients).  As in the reference dg/dp = -(4/9) h^2 pscale I is used for every step
 * and dg/dqa of the start step is dropped (TaskBDF2PointPos.m:97-106, TaskBDF2.m:52-55), so dPdp carries the reference's own
 * O(1/nsteps) start-step error.  Arguments as rmx_adjoint_bdf1.  The batch is left at the end of the forward rollout with the
 * BDF2 history in place (rmx_step_bdf2 may continue it). */
int rmx_adjoint_bdf2(rmx_batch* b, const rmx_opts* opts, int nsteps, const rmx_task_pointpos* task, const double* p,
                     double* P, double* dPdp, rmx_stats* stats);

/* The same two calls with DEVICE pointers for p, P and dPdp (ABI 110): an optimiser that lives on the device - or a caller that
 * evaluates many parameter batches - pays no host round trip for them (three small copies and their synchronisation were a sixth
 * of the 20-step configs[3] call).  d_p: [batch][nr], d_P: [batch], d_dPdp: [batch][nr], none of them retained; stats (host
 * arrays, may be NULL) as above.  The call returns when the kernels have finished. */
int rmx_adjoint_bdf1_device(rmx_batch* b, const rmx_opts* opts, int nsteps, const rmx_task_pointpos* task, const double* d_p,
                            double* d_P, double* d_dPdp, rmx_stats* stats);
int rmx_adjoint_bdf2_device(rmx_batch* b, const rmx_opts* opts, int nsteps, const rmx_task_pointpos* task, const double* d_p,
                            double* d_P, double* d_dPdp, rmx_stats* stats);

/* One torque per joint and STEP, and the gradient for each of them: what trajectory optimisation and policy training need, where
 * rmx_adjoint_bdf1 / bdf2 take one constant torque vector per rollout.  The reference's own structure is per step - task.applyStep
 * runs at every step (driverRedMaxAdjointBDF1.m:74) and TaskBDF1.calcFinal forms one z_k per step (TaskBDF1.m:52-79); its one
 * shipped task sums them because its parameters are constant.
 * integrator: 1 = BDF1, 2 = BDF2 (as rmx_step_history).  u: host [batch][nsteps][nr], trajectory-major, reduced DOF order; at step
 * k = 1 .. nsteps the joint torque is tau + pscale * u[b][k-1][:] (under BDF2 step 1's torque holds for both SDIRK2 solves).
 *     P[b]            = wpos/2 |x(task->step) - xtarget|^2 + wreg/2 * sum over k, j of u[b][k-1][j]^2
 *     dPdu[b][k-1][j] = wreg * u[b][k-1][j] + e2 * pscale * z_k[j] ,   e2 = h^2 (BDF1) or (4/9) h^2 (BDF2, every step)
 * which is the constant-parameter formula before its sum over the steps; rows behind task->step hold wreg * u exactly.  Under
 * BDF2 the k = 1 row therefore carries the reference's own start-step approximation (dg/dp = -(4/9) h^2 pscale I for the SDIRK2
 * start step too and dg/dqa dropped, TaskBDF2PointPos.m:97-106, TaskBDF2.m:52-55); the rows of k >= 2 are exact.
 * P: host [batch]; dPdu: host, shape of u, or NULL: the forward sweep alone (the backward kernel is not launched, P is still
 * written) - a controlled rollout with the reference's line-search-free newton.  u is neither retained nor modified.  Refusals,
 * opts, stats and the state the batch is left in (with the BDF2 history in place) as rmx_adjoint_bdf1 / bdf2.
 * rmx_adjoint_controls_device: the same with DEVICE pointers d_u, d_P, d_dPdu (d_dPdu may be NULL), as rmx_adjoint_bdf1_device. */
int rmx_adjoint_controls(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, const rmx_task_pointpos* task,
                         const double* u, double* P, double* dPdu, rmx_stats* stats);
int rmx_adjoint_controls_device(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, const rmx_task_pointpos* task,
                                const double* d_u, double* d_P, double* d_dPdu, rmx_stats* stats);

/* rmx_adjoint_controls with a tracking objective: point targets on several bodies at several steps, and optionally a target
 * table of its own for every rollout - the running costs and goal-conditioned objectives of trajectory optimisation and policy
 * training, in ONE forward and ONE backward sweep (TaskBDF1.calcFinal reads a dPdq of every step, TaskBDF1.m:52-57; the
 * reference's one shipped task leaves all but one of them zero).  These two entries and their two structs were added WITHOUT a
 * change of RMX_VERSION (it stays 111): a host that wants them probes for the symbol.
 *     P[b]            = sum_i wpos_i/2 |x_i(step_i) - xtarget[b][i]|^2  +  wreg/2 * sum over k, j of u[b][k-1][j]^2
 *     dPdu[b][k-1][j] = wreg * u[b][k-1][j] + e2 * pscale * z_k[j] ,   e2 = h^2 (BDF1) or (4/9) h^2 (BDF2)
 * z comes from the same backward recursion with the source y_k = sum over the terms with step_i == k of dPdq_i (zero at steps
 * without a term); each dPdq_i is formed as rmx_task_pointpos's is: the body frame from the final state of the step, J from the
 * last evaluated Newton iterate (TaskBDF1PointPos.m:77-93).  Terms of one step add up, in P and in y_k, in the order they have
 * in `terms`; several terms may share a step, a body, or both.  Rows behind the last measured step hold wreg * u exactly.
 * u, P, dPdu (NULL: the forward sweep alone, P is still written), integrator, opts, stats, the refusals and the state the batch
 * is left in: as rmx_adjoint_controls.  Further refusals (RMX_E_INVALID): a null task, terms or target table, nterms < 1, a term
 * whose body is outside the listing or whose step is outside [1, nsteps] (the message names the term's index).  Neither u nor
 * the targets are retained or modified.
 * rmx_adjoint_track_device: DEVICE pointers d_u, d_P, d_dPdu (may be NULL) and d_xtarget, a device array of the shape
 * task->per_rollout names; task->xtarget is ignored, task->terms stays a host array. */
typedef struct rmx_track_term {
    int body;            /* listing index of the body, as rmx_task_pointpos.body          */
    double xlocal[3];    /* point in body coordinates                                      */
    int step;            /* 1-based step at which this term is measured, 1 .. nsteps      */
    double wpos;         /* weight of this term                                            */
} rmx_track_term;
typedef struct rmx_task_track {
    int nterms;                    /* >= 1; several terms may share a step, a body, or both */
    const rmx_track_term* terms;   /* host, any order */
    const double* xtarget;         /* host: [nterms][3] (per_rollout 0) or [batch][nterms][3] (per_rollout 1),
                                      indexed by the term's position in `terms` */
    int per_rollout;
    double pscale, wreg;
} rmx_task_track;
int rmx_adjoint_track(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, const rmx_task_track* task,
                      const double* u, double* P, double* dPdu, rmx_stats* stats);
int rmx_adjoint_track_device(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, const rmx_task_track* task,
                             const double* d_xtarget, const double* d_u, double* d_P, double* d_dPdu, rmx_stats* stats);

/* A differentiable controlled rollout (BDF1, BDF2): the forward sweep records the trajectory and keeps H, M, D of every step (the
 * "tape"), the backward sweep takes ANY cotangents dL/dq_k, dL/dqdot_k and returns dL/du, dL/dq0 and dL/dqdot0 - an objective of
 * the caller's own (joint-space and velocity costs, a learned critic, a policy's loss), and the gradient with respect to the
 * initial state that multiple shooting, receding-horizon control and chained rollouts need.  rmx_adjoint_controls / _track compute
 * one objective inside the library; here there is none.  Added WITHOUT a change of RMX_VERSION (it stays 111): probe for the symbols.
 *
 * rmx_rollout_tape: from the batch's current state, the forward sweep of rmx_adjoint_controls with integrator 1 - the
 * line-search-free newton, the same guarded solve, the same compensated iterate - under the torques tau + pscale * u[b][k-1][:].
 * u: host [batch][nsteps][nr] as in rmx_adjoint_controls.  qtraj, qdtraj: host [batch][nsteps][nr], trajectory-major, reduced DOF
 * order (the layout of u); row k-1 is the state after step k; NULL together: no record.  H, M, D of every step's last evaluated
 * iterate stay in the batch's adjoint workspace.  The batch is left at the end of the rollout; opts and stats as in
 * rmx_adjoint_controls.  Refusals as rmx_adjoint_controls, with the same words (ground contact, spherical joints, more than 64
 * nodes, point forces).
 *
 * rmx_rollout_vjp: reads the tape of the preceding rmx_rollout_tape on the same batch.  gq, gqd: host, shape of qtraj: dL/dq_k and
 * dL/dqdot_k.  du: host, shape of u; dq0, dqd0: host [batch][nr], NULL together: not formed.  With z_{N+1} = z_{N+2} = 0,
 * gqd_{N+1} = 0, N = nsteps, for k = N .. 1:
 *     y_k  = gq_k + (gqd_k - gqd_{k+1})/h - (-2 M_{k+1} + h D_{k+1})' z_{k+1} - M_{k+2}' z_{k+2}
 *     H_k' z_k = y_k
 *     du_k = h^2 pscale z_k
 *     dq0  = -gqd_1/h - (-M_1 + h D_1)' z_1 - M_2' z_2
 *     dqd0 = h M_1' z_1
 * The off-diagonal blocks are those of TaskBDF1.calcFinal (TaskBDF1.m:58-70); the gqd terms come from qdot_k = (q_k - q_{k-1})/h.
 * The last two lines are the k = 0 row: -M_1 where the recursion has -2 M_1, because nothing precedes q0.  h and pscale are the
 * tape's.  The call changes neither the batch's state nor the tape: it may be called again with other cotangents.
 *
 * The tape is valid until the next rmx_rollout_tape / rmx_rollout_tape_bdf2 or rmx_adjoint_* call on that batch (both reuse the workspace); step calls and
 * rmx_set_state leave it alone.  rmx_rollout_vjp refuses (RMX_E_INVALID) without a valid tape (the message says "no tape"), with
 * an nsteps that differs from the tape's, and null arguments.
 *
 * rmx_rollout_tape_bdf2: the same under BDF2 - arguments, layouts, refusals and words are rmx_rollout_tape's.  The call starts from
 * the batch's current (q, qdot) and ALWAYS takes the SDIRK2 start step (as rmx_adjoint_bdf2 does), so (q0, qdot0) is the complete
 * state and dq0, dqd0 are well defined; row k-1 of qtraj is the state after step k, step 1 being the start step.  The batch is
 * left at the end of the rollout with the BDF2 history in place: rmx_step_bdf2 may continue it.  The tape holds H, M, D of every
 * step's final solve AND of the SDIRK2a stage (nsteps + 1 slots per rollout), and rmx_rollout_vjp - which follows the integrator
 * of the tape it finds - differentiates every solve exactly.  Every solve is the same implicit function: given qA, qB, eta and
 * the step's torque, x solves g = M(x)(x - qB) - eta^2 (f(x, (x - qA)/eta) + pscale u) = 0, and v = (x - qA)/eta.  With H = dg/dx,
 * M, D = df/dqdot at the solution, cotangents xbar, vbar of x, v go back as
 *     solve_bwd:  H' z = xbar + vbar/eta ;  A = -vbar/eta - eta D' z (of qA) ;  Bq = M' z (of qB) ;  ubar = eta^2 pscale z
 * With al = (2 - sqrt 2)/2 the solves are (driverRedMaxBDF2.m:64-117)
 *     SDIRK2a: eta = al h, qA = q0, qB = q0 + al h qd0                                         -> qa, qda = (qa - q0)/(al h)
 *     SDIRK2b: eta = al h, qA = q0 + (1-al) h qda, qB = q0 + (2al-1) h qd0 + 2(1-al) h qda     -> q1, qd1
 *     BDF2   : eta = 2h/3, qA = 4/3 q_k - 1/3 q_{k-1}, qB = qA + 8/9 h qd_k - 2/9 h qd_{k-1}   -> q_{k+1}, qd_{k+1}
 * and the sweep carries qbar[k], vbar[k], which start as gq_k, gqd_k (zero for k = 0).  For k = N-1 .. 1:
 *     (A, Bq, z) = solve_bwd(step k+1; qbar[k+1], vbar[k+1]) ;  du_{k+1} = (2h/3)^2 pscale z ;  s = A + Bq
 *     qbar[k]   += 4/3 s ;  vbar[k]   += 8/9 h Bq ;  qbar[k-1] -= 1/3 s ;  vbar[k-1] -= 2/9 h Bq
 * then the start step:
 *     (A, Bq, zb) = solve_bwd(SDIRK2b; qbar[1], vbar[1])
 *     qbar[0] += A + Bq ;  vbar[0] += (2al-1) h Bq ;  qdabar = (1-al) h A + 2(1-al) h Bq
 *     (A2, B2, za) = solve_bwd(SDIRK2a; 0, qdabar)               (qa is read only through qda)
 *     qbar[0] += A2 + B2 ;  vbar[0] += al h B2
 *     du_1 = (al h)^2 pscale (za + zb)                           (step 1's torque holds for both solves)
 *     dq0 = qbar[0] ;  dqd0 = vbar[0]
 * rmx_adjoint_bdf2 and rmx_adjoint_controls / _track with integrator 2 keep the reference's APPROXIMATE k = 1 row (dg/dp =
 * -(4/9) h^2 for the start step, dg/dqa dropped: TaskBDF2.calcFinal); only the taped rollout is exact there.
 * The _device forms: the same with DEVICE pointers, nothing staged, nothing copied back; they return when the kernels have finished. */
int rmx_rollout_tape(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const double* u,
                     double* qtraj, double* qdtraj, rmx_stats* stats);
int rmx_rollout_tape_bdf2(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const double* u,
                          double* qtraj, double* qdtraj, rmx_stats* stats);
int rmx_rollout_tape_bdf2_device(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const double* d_u,
                                 double* d_qtraj, double* d_qdtraj, rmx_stats* stats);
int rmx_rollout_vjp(rmx_batch* b, int nsteps, const double* gq, const double* gqd,
                    double* du, double* dq0, double* dqd0);
int rmx_rollout_tape_device(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const double* d_u,
                            double* d_qtraj, double* d_qdtraj, rmx_stats* stats);
int rmx_rollout_vjp_device(rmx_batch* b, int nsteps, const double* d_gq, const double* d_gqd,
                           double* d_du, double* d_dq0, double* d_dqd0);

/* The taped rollout in CLOSED LOOP: time-varying affine state feedback evaluated on the device, inside the one launch - the forward
 * pass of iLQR / DDP and time-varying-LQR tracking, u_k = uff_k + K_k (x_{k-1} - xref_{k-1}), where the torque of step k depends on
 * the state the rollout itself has reached.  Added WITHOUT a change of RMX_VERSION (it stays 111): probe for the symbols.
 *
 * rmx_rollout_tape_feedback is rmx_rollout_tape (integrator 1) / rmx_rollout_tape_bdf2 (integrator 2) with the torque of step k
 *     uapp[b][k-1][i] = uff[b][k-1][i] + sum_j K_k[i][j] (x_j - xref_{k-1,j}),     x = (q, qdot) at the START of step k
 * - for k = 1 the batch's state at the call, for k > 1 the bits of row k-2 of qtraj / qdtraj.  Under BDF2 the torque of step 1 holds
 * for both SDIRK2 solves.  Reduced DOF order throughout; x has 2 nr entries, q first.
 * K: one table of 2 nr nr doubles per step, column-major as everywhere in this header: entry j*nr + i of step k's table (row k-1) is
 * du_i/dx_j, j in 0 .. 2nr-1.  xref: one row of 2 nr doubles per step.  per_rollout 0: [nsteps][..], shared by the batch; 1:
 * [batch][nsteps][..].  The sum runs in one fixed order (the nodes of the tree ascending - depth first -, the q block before the
 * qdot block), so a rollout's result does not depend on its position in the batch.  K NULL: no feedback, uapp == uff bit for bit
 * (xref is not read).  uapp: host [batch][nsteps][nr], the applied torques (out), or NULL.  Everything else - opts, stats, qtraj,
 * qdtraj, the state the batch is left in - as rmx_rollout_tape / _bdf2.
 *
 * The tape the call leaves has rmx_rollout_tape's layout and IS the open-loop tape under the torques uapp: rmx_rollout_vjp,
 * rmx_rollout_linearize, rmx_rollout_jvp and rmx_rollout_vjp_params read it unchanged and differentiate the open-loop rollout at
 * uapp - what iLQR re-linearises around.  Gradients through the feedback law itself (dL/dK, dL/dxref, the closed-loop dL/duff) are
 * formed by rmx_rollout_vjp_feedback below, from the same tape.
 *
 * Refusals (RMX_E_INVALID): everything rmx_rollout_tape refuses, in its words; a null struct or uff ("null argument"); an integrator
 * other than 1 or 2; per_rollout other than 0 or 1.  A refused call leaves an existing tape alone.  The host form stages K, xref
 * and uapp through a device allocation of its own, freed before it returns.  The _device form: every array a DEVICE pointer (the
 * struct itself is a host object), nothing staged; it returns when the kernel has finished. */
typedef struct rmx_feedback {
    const double* uff;   /* [batch][nsteps][nr]                 required                                  */
    const double* K;     /* [nsteps][2*nr*nr] or [batch][..]    NULL: no feedback, uapp == uff bit for bit */
    const double* xref;  /* [nsteps][2*nr] or [batch][..]       row k-1: (q, qdot) reference for the state
                            at the START of step k; NULL: zero                                            */
    int per_rollout;     /* 0: K and xref shared by the batch, 1: one table per rollout                   */
} rmx_feedback;
int rmx_rollout_tape_feedback(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, double pscale,
                              const rmx_feedback* fb, double* qtraj, double* qdtraj, double* uapp, rmx_stats* stats);
int rmx_rollout_tape_feedback_device(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, double pscale,
                                     const rmx_feedback* fb, double* d_qtraj, double* d_qdtraj, double* d_uapp, rmx_stats* stats);

/* The closed-loop adjoint of the taped rollout: dL/duff, dL/dK, dL/dxref, dL/dq0, dL/dqdot0 of a rollout that ran under
 * rmx_rollout_tape_feedback, for any cotangents of its states and of its applied torques - tuning a controller on the device: gain
 * and reference learning, policy gradients, differentiating an iLQR / MPC result through its own feedback policy.  Added WITHOUT a
 * change of RMX_VERSION (it stays 111): probe for the symbols.
 *
 * With uapp_k = uff_k + K_k (x_{k-1} - xref_{k-1}) the tape is the open-loop tape under uapp; the closed loop adds one term per step:
 * the cotangent ubar_k of the applied torque goes back into the cotangent of the state the step started from.  K_k = (Kq_k, Kv_k), the
 * q block and the qdot block of row k-1's table (entry j*nr + i is du_i/dx_j), and (K' ubar)_j = sum_i K[j*nr + i] ubar_i.  gu: the
 * caller's cotangent of uapp (costs on the applied control), shape of uff, or NULL: zero.  solve_bwd and the notation are those of
 * rmx_rollout_tape_bdf2 above; the sweep carries qbar[k], vbar[k], which start as gq_k, gqd_k (zero for k = 0).
 *   BDF1 (eta = h, slot k-1 is step k, qA = q_{k-1}, qB = q_{k-1} + h qd_{k-1}), for k = N .. 1:
 *     (A, Bq, z) = solve_bwd(slot k-1, h; qbar[k], vbar[k]) ;  ubar_k = h^2 pscale z + gu_k
 *     qbar[k-1] += A + Bq + Kq_k' ubar_k ;  vbar[k-1] += h Bq + Kv_k' ubar_k
 *   (without the K terms this is rmx_rollout_vjp's recursion in another arrangement.)
 *   BDF2: the recursion at rmx_rollout_tape_bdf2 with two additions.  Behind the solve of step k+1:
 *     ubar_{k+1} = (2h/3)^2 pscale z + gu_{k+1} ;  qbar[k] += Kq_{k+1}' ubar_{k+1} ;  vbar[k] += Kv_{k+1}' ubar_{k+1}
 *   - before qbar[k] enters the solve of step k -, and in the start step
 *     ubar_1 = (al h)^2 pscale (za + zb) + gu_1 ;  qbar[0] += Kq_1' ubar_1 ;  vbar[0] += Kv_1' ubar_1
 *   (step 1's torque holds for both SDIRK2 solves and reads x_0 only.)
 *   Outputs, both integrators:
 *     duff_k = ubar_k ;  dxref_{k-1} = -(Kq_k' ubar_k, Kv_k' ubar_k)          (row k-1, 2 nr entries)
 *     dK_k[j*nr + i] = (x_{k-1} - xref_{k-1})_j ubar_{k,i}     (x_0 = (q0, qdot0) of the tape; for k > 1 row k-2 of its trajectory)
 *     dq0 = qbar[0] ;  dqd0 = vbar[0]
 *
 * The call reads the tape on the batch and follows its integrator, as rmx_rollout_vjp does; h and pscale are the tape's.  fb->K,
 * fb->xref and fb->per_rollout are as in the forward call (xref NULL: a zero reference); fb->uff is not read.  gq, gqd: as
 * rmx_rollout_vjp.  The call does NOT check that the tape was recorded under these gains - a replay under uapp leaves the identical
 * tape, so it cannot: passing the K, xref of the forward call is the caller's contract.
 * Gradient rows are ALWAYS per rollout, whether the tables are shared or not: for tables the batch shares the caller sums over the
 * batch (the rule of rmx_rollout_vjp_params, for the same reason: a loss may weight rollouts).  dK is batch * nsteps * 2 nr^2 doubles;
 * for a shared table it is cheaper formed as the caller's own contraction of duff with the states (sum_b dx_{b,k-1,j} duff_{b,k,i}),
 * with dK NULL here.  Every output has the same bits whichever others are NULL, and a rollout's rows do not depend on its place in
 * the batch or on the batch size (K' ubar runs in one fixed order: the nodes of the tree ascending, one fused multiply-add per term).
 * fb->K NULL: no gains.  With gu NULL too the call IS rmx_rollout_vjp on that tape - the same kernel, the same bits in duff, dq0,
 * dqd0 -; with gu, duff = du + gu and dq0, dqd0 are the open-loop ones up to rounding.  dK or dxref asked for without gains is refused.
 *
 * The call changes neither the batch's state nor the tape: it may be repeated with the same bits, and rmx_rollout_vjp,
 * rmx_rollout_linearize, rmx_rollout_jvp and rmx_rollout_vjp_params return the same bits before and after it.  Refusals
 * (RMX_E_INVALID), in rmx_rollout_vjp's words where they coincide: "no tape", an nsteps that differs from the tape's, a null batch,
 * fb, gq, gqd or out ("null argument"), "all outputs are null", dq0 and dqd0 not given together, per_rollout other than 0 or 1, dK or
 * dxref without K ("no gains").  The host form stages the cotangents, K, xref and the outputs through a device allocation of its own,
 * made ahead of anything else and freed before it returns; the tape's workspace does not grow.  The _device form: every array a
 * DEVICE pointer (both structs are host objects), nothing staged; it returns when the kernel has finished. */
typedef struct rmx_feedback_grads {   /* every pointer may be NULL (not formed), but not all of duff, dK, dxref, dq0 */
    double* duff;    /* [batch][nsteps][nr]                                                     */
    double* dK;      /* [batch][nsteps][2*nr*nr]  one row per rollout, layout of a per-rollout K */
    double* dxref;   /* [batch][nsteps][2*nr]     one row per rollout                            */
    double* dq0;     /* [batch][nr]  \ NULL together                                             */
    double* dqd0;    /* [batch][nr]  /                                                           */
} rmx_feedback_grads;
int rmx_rollout_vjp_feedback(rmx_batch* b, int nsteps, const rmx_feedback* fb, const double* gq, const double* gqd,
                             const double* gu, const rmx_feedback_grads* out);
int rmx_rollout_vjp_feedback_device(rmx_batch* b, int nsteps, const rmx_feedback* fb, const double* d_gq, const double* d_gqd,
                                    const double* d_gu, const rmx_feedback_grads* out);

/* The linearisation of the taped rollout: the forward sensitivities of every taped solve, from which a host assembles the per-step
 * A_k = d(q_k, qdot_k)/d(q_{k-1}, qdot_{k-1}) and B_k = d(q_k, qdot_k)/du_k that iLQR / DDP, time-varying LQR, Gauss-Newton shooting
 * and SQP-style MPC work with.  Added WITHOUT a change of RMX_VERSION (it stays 111): probe for the symbols.
 *
 * Every taped solve is x(qA, qB, u): g = M(x)(x - qB) - eta^2 (f(x, (x - qA)/eta) + pscale u) = 0 with H = dg/dx, dg/dqA = eta D,
 * dg/dqB = -M, dg/du = -eta^2 pscale I (the implicit function of rmx_rollout_tape_bdf2 above).  Its forward sensitivities are
 *     XA = dx/dqA = -eta H^-1 D        XB = dx/dqB = H^-1 M        XU = dx/du = eta^2 pscale H^-1
 * the forward-mode counterparts of solve_bwd: with w = xbar + vbar/eta,  A = -vbar/eta + XA' w,  Bq = XB' w,  ubar = XU' w.
 * With v = (x - qA)/eta:  dv/dqA = (XA - I)/eta,  dv/dqB = XB/eta,  dv/du = XU/eta.
 *
 * rmx_rollout_linearize reads the tape of the preceding rmx_rollout_tape / rmx_rollout_tape_bdf2 on the same batch and follows the
 * integrator of the tape it finds, as rmx_rollout_vjp does.  XA, XB, XU: host [batch][nslots][nr*nr], column-major in the last
 * index (the convention of rmx_eval and rmx_eval_mfd): entry j*nr + i is dx_i/d(.)_j, reduced DOF order.  Any of them may be NULL -
 * that output is neither computed nor stored - but not all three.  nslots = nsteps for a BDF1 tape, nsteps + 1 for a BDF2 tape: slot
 * s-1 is step s (step 1 of a BDF2 tape is the SDIRK2b solve), slot nsteps the SDIRK2a solve.  eta per slot: h under BDF1; under BDF2
 * al h for slot 0 and slot nsteps, al = (2 - sqrt 2)/2, and 2h/3 for the others.  h and pscale are the tape's.
 *
 * BDF1 (qA = q_{k-1}, qB = q_{k-1} + h qdot_{k-1}, eta = h, qdot_k = (q_k - q_{k-1})/h), state order (q, qdot), slot k-1:
 *     A_k = [ XA + XB          h XB ]        B_k = [ XU   ]
 *           [ (XA + XB - I)/h    XB ]              [ XU/h ]
 * BDF2: with dqA, dqB the variations of a solve's qA, qB, its results vary as dx = XA dqA + XB dqB + XU du, dv = (dx - dqA)/eta, and
 *     SDIRK2a (slot nsteps): dqA = dq0 ;  dqB = dq0 + al h dqd0                                              -> dqa, dqda
 *     SDIRK2b (slot 0)     : dqA = dq0 + (1-al) h dqda ;  dqB = dq0 + (2al-1) h dqd0 + 2(1-al) h dqda        -> dq1, dqd1
 *     BDF2    (slot k)     : dqA = 4/3 dq_k - 1/3 dq_{k-1} ;  dqB = dqA + 8/9 h dqd_k - 2/9 h dqd_{k-1}      -> dq_{k+1}, dqd_{k+1}
 * (du = du_1 in both SDIRK2 solves), which gives the blocks of the augmented state (q_k, qdot_k, q_{k-1}, qdot_{k-1}).
 *
 * The call changes neither the batch's state nor the tape: it may be repeated, and rmx_rollout_vjp before and after it returns the
 * same bits.  Refusals (RMX_E_INVALID), in rmx_rollout_vjp's words where they coincide: "no tape", an nsteps that differs from the
 * tape's, a null batch, all outputs null.  The slots of a rollout whose tape call reported a failed Newton solve (stats->status) are
 * unspecified.  The host form stages through a device allocation of its own, freed before it returns; the tape's workspace does not
 * grow.  The _device form: DEVICE pointers, nothing staged; it returns when the kernel has finished. */
int rmx_rollout_linearize(rmx_batch* b, int nsteps, double* XA, double* XB, double* XU);
int rmx_rollout_linearize_device(rmx_batch* b, int nsteps, double* d_XA, double* d_XB, double* d_XU);

/* Forward-mode tangents of the taped rollout: J t, the perturbation of the whole trajectory for a perturbation of the controls and of
 * the initial state - what Gauss-Newton / Levenberg-Marquardt / CG shooting (J'(J t)), sensitivity analysis and forward-mode automatic
 * differentiation ask for.  One sweep over the tape, one elimination of H per slot shared by all directions of the call; nothing but
 * the tangent trajectory is written.  Added WITHOUT a change of RMX_VERSION (it stays 111): probe for the symbols.
 *
 * Every taped solve is x(qA, qB, u) with dg/dx = H, dg/dqA = eta D, dg/dqB = -M, dg/du = -eta^2 pscale I (rmx_rollout_tape_bdf2 and
 * rmx_rollout_linearize above), so
 *     solve_fwd(slot; dqA, dqB, du):   H dx = -eta D dqA + M dqB + eta^2 pscale du ;   dv = (dx - dqA)/eta
 * BDF1 (eta = h, slot k-1 is step k), for k = 1 .. N from (dq_0, dqd_0) = (tq0, tqd0):
 *     (dq_k, dqd_k) = solve_fwd(slot k-1; dq_{k-1}, dq_{k-1} + h dqd_{k-1}, tu_k)
 * BDF2 (al = (2 - sqrt 2)/2; eta = al h in slots 0 and N, 2h/3 in the others; step 1's tangent tu_1 holds for both start solves):
 *     SDIRK2a (slot N): (dqa, dqda)   = solve_fwd(dq0, dq0 + al h dqd0, tu_1)
 *     SDIRK2b (slot 0): (dq_1, dqd_1) = solve_fwd(dq0 + (1-al) h dqda, dq0 + (2al-1) h dqd0 + 2(1-al) h dqda, tu_1)
 *     BDF2    (slot k, k = 1 .. N-1): dqA = 4/3 dq_k - 1/3 dq_{k-1} ;  dqB = dqA + 8/9 h dqd_k - 2/9 h dqd_{k-1}
 *                                     (dq_{k+1}, dqd_{k+1}) = solve_fwd(dqA, dqB, tu_{k+1})
 * It is the transpose of rmx_rollout_vjp on the same tape: for cotangents (gq, gqd) with (du, dq0, dqd0) = rmx_rollout_vjp(gq, gqd),
 *     <gq, tq> + <gqd, tqd> = <du, tu> + <dq0, tq0> + <dqd0, tqd0>.
 *
 * rmx_rollout_jvp reads the tape of the preceding rmx_rollout_tape / rmx_rollout_tape_bdf2 on the batch and follows the integrator of
 * the tape it finds, as rmx_rollout_vjp and rmx_rollout_linearize do; h and pscale are the tape's.  ntan >= 1 tangent directions per
 * rollout.  tu: host [batch][ntan][nsteps][nr] (one direction has the layout of u); tq0, tqd0: [batch][ntan][nr].  Each of the three
 * may be NULL - zero - but not all three.  tq, tqd: [batch][ntan][nsteps][nr], row k-1 the tangent of the state after step k; both
 * required.  Reduced DOF order throughout.
 *
 * The call changes neither the batch's state nor the tape: it may be repeated, and rmx_rollout_vjp, rmx_rollout_linearize and
 * rmx_rollout_vjp_params return the same bits before and after it.  The pivots of a slot's elimination depend on H alone and the
 * directions never mix: one direction's result has the same bits whatever ntan is, wherever the direction stands in the call, and
 * whether a zero input is NULL or an array of zeros.  Refusals (RMX_E_INVALID), in rmx_rollout_vjp's words where they coincide: "no
 * tape", an nsteps that differs from the tape's, a null batch, tq or tqd ("null argument"), "ntan < 1", "all tangents are null".  The
 * rows of a rollout whose tape call reported a failed Newton solve (stats->status) are unspecified.  The host form stages through a
 * device allocation of its own, freed before it returns; the tape's workspace does not grow.  The _device form: DEVICE pointers,
 * nothing staged; it returns when the kernel has finished. */
int rmx_rollout_jvp(rmx_batch* b, int nsteps, int ntan, const double* tu, const double* tq0, const double* tqd0,
                    double* tq, double* tqd);
int rmx_rollout_jvp_device(rmx_batch* b, int nsteps, int ntan, const double* d_tu, const double* d_tq0, const double* d_tqd0,
                           double* d_tq, double* d_tqd);

/* The Riccati sweep of iLQR / DDP over the taped rollout: the backward pass of one iteration for a quadratic model of the cost, the
 * whole recursion in one launch, with the per-step sensitivities formed inside it.  Added WITHOUT a change of RMX_VERSION (it stays
 * 111): probe for the symbols.
 *
 * rmx_rollout_lqr reads the BDF1 tape on the batch, left by rmx_rollout_tape or by rmx_rollout_tape_feedback with integrator 1 (the
 * open-loop tape under the applied torques: what iLQR re-linearises around).  h and pscale are the tape's.  Per step k, with
 * S = XA + XB, XB, XU of slot k-1 (rmx_rollout_linearize's definitions and bits) and x = (q, qdot),
 *     A_k = [ S          h XB ]      B_k = [ XU   ]
 *           [ (S - I)/h    XB ]            [ XU/h ]
 * and with Vx_N = lx_N, Vxx_N = Q_N, for k = N .. 1:
 *     Qx = A'Vx      Qu = lu_k + B'Vx      Qxx = A'Vxx A      Qux = B'Vxx A      Quu0 = R + B'Vxx B   (symmetric)
 *     [k_k, K_k] = -(Quu0 + mu I)^-1 [Qu, Qux]
 *     Vx  <- lx_{k-1} + Qx  + K'Quu0 k + K'Qu  + Qux'k            (lx_0 = 0, Q_0 = 0: x_0 is fixed)
 *     Vxx <- Q_{k-1}  + Qxx + K'Quu0 K + K'Qux + Qux'K            (kept symmetric)
 *     expected = -sum_k (Qu'k_k + 1/2 k_k'Quu0 k_k)
 * expected is the decrease of the quadratic model under the full step.  Arrays over the steps hold step k in row k-1.
 *
 * K is written in the layout rmx_rollout_tape_feedback reads per rollout (rmx_feedback.K with per_rollout = 1), kff in the layout of
 * uff: one iLQR trial is this call, uff = ubar + alpha kff, and the feedback call with xref the nominal states.
 *
 * Quu0 + mu I is factorised without pivoting (LDL').  A pivot that is not > 0 flags the rollout: status 1, every kff and K row of that
 * rollout zero, expected 0 - with K = 0 around its own nominal the feedback call reproduces that nominal, so a flagged rollout takes
 * no step.  The other rollouts of the batch are not affected, and the call still returns RMX_OK.
 *
 * The call changes neither the batch's state nor the tape: it may be repeated with the same bits, and rmx_rollout_vjp, _linearize,
 * _jvp and _vjp_params return the same bits before and after it.  A rollout's rows do not depend on its place in the batch, on the
 * batch size, on whether Q is shared or passed as per-rollout copies, on mu against a constant mu_b, or on expected / status being
 * NULL.  The rows of a rollout whose tape call reported a failed Newton solve (stats->status) are unspecified.
 * Refusals (RMX_E_INVALID), in rmx_rollout_vjp's words where they coincide: "no tape", an nsteps that differs from the tape's, a BDF2
 * tape ("BDF1 tape"), a null batch, cost, out, lx, lu, Q, R, kff or K ("null argument"), per_rollout other than 0 or 1, mu negative or
 * not finite (checked whether or not mu_b is given; the entries of mu_b are the caller's to keep >= 0), and nr > 32 (the message names
 * the model's nr; a tree of more than 32 nodes is refused too): the kernel keeps Vxx and a step's temporaries in LDS and exists for
 * the padded sizes up to 32.
 * The host form stages through a device allocation of its own, made ahead of anything else and freed before it returns; the tape's
 * workspace does not grow, and no scratch proportional to batch * nsteps * nr^2 is allocated by either form.  The _device form:
 * every array a DEVICE pointer (both structs are host objects), nothing staged; it returns when the kernel has finished. */
typedef struct rmx_lqr_cost {
    const double* lx;    /* [batch][nsteps][2*nr]   dJ/dx_k at the nominal, row k-1: state after step k, (q, qdot)   required */
    const double* lu;    /* [batch][nsteps][nr]     dJ/du_k at the nominal                                          required */
    const double* Q;     /* [nsteps][2nr*2nr] or [batch][nsteps][2nr*2nr]  symmetric, column-major                   required */
    const double* R;     /* [nr*nr] symmetric, shared by steps and rollouts                                          required */
    int per_rollout;     /* 0: Q shared by the batch, 1: one table per rollout                                       */
    double mu;           /* >= 0: regulariser of Quu                                                                 */
    const double* mu_b;  /* [batch] or NULL; when given it replaces mu, rollout by rollout                           */
} rmx_lqr_cost;
typedef struct rmx_lqr_gains {          /* kff and K required */
    double* kff;        /* [batch][nsteps][nr]                                                                         */
    double* K;          /* [batch][nsteps][2*nr*nr]  entry j*nr + i of row k-1 is du_i/dx_j: rmx_feedback.K, per rollout */
    double* expected;   /* [batch] or NULL                                                                             */
    int* status;        /* [batch] or NULL: 0, or 1 = some Quu + mu I was not positive definite                        */
} rmx_lqr_gains;
int rmx_rollout_lqr(rmx_batch* b, int nsteps, const rmx_lqr_cost* cost, const rmx_lqr_gains* out);
int rmx_rollout_lqr_device(rmx_batch* b, int nsteps, const rmx_lqr_cost* cost, const rmx_lqr_gains* out);

/* Torque limits ulo <= u <= uhi in the device iLQR: control-limited DDP (Tassa, Mansard, Todorov 2014) - a box-constrained QP for
 * the feed-forward term at every step of the Riccati sweep, zero feedback rows for the torques on a bound, and the applied torque
 * clamped in the forward pass.  Added WITHOUT a change of RMX_VERSION (it stays 111): probe for the symbols.  No existing struct
 * grows.  One box for all steps and rollouts.
 *
 * rmx_rollout_tape_feedback_box is rmx_rollout_tape_feedback with one change to the torque of step k:
 *     uapp = min(max(uff + K (x - xref), ulo), uhi)      per DOF
 * - the clamp comes behind the feedback sum, and applies with fb->K NULL too (actuator saturation of an open-loop torque); both
 * integrators; under BDF2 the clamped torque of step 1 holds for both SDIRK2 solves.  Everything else is that entry's, in its words:
 * the record and uapp, the tape (the open-loop tape under uapp: rmx_rollout_vjp, _linearize, _jvp, _vjp_params and _lqr read it
 * unchanged), the state the batch is left in, the refusals.  New refusals (RMX_E_INVALID), which leave an existing tape alone: a null
 * box ("null argument"); an entry with ulo > uhi, or a NaN bound (the message names the DOF).  With both pointers NULL, or every bound
 * infinite, the call returns rmx_rollout_tape_feedback's bits.  The _device form: ulo and uhi are DEVICE pointers too (the struct is
 * a host object); it reads them back once for the check.
 *
 * rmx_rollout_lqr_box is rmx_rollout_lqr with one change: the solve [k, K] = -(Quu0 + mu I)^-1 [Qu, Qux] of every step becomes the
 * box QP   min Qu'x + 1/2 x'Hq x,  lo_k <= x <= hi_k,   Hq = Quu0 + mu I,  lo_k = ulo - ubar_k,  hi_k = uhi - ubar_k
 * with ubar [batch][nsteps][nr] the nominal applied torques (the uapp of the launch that left the tape; required).  Per step, with
 * val(x) = Qu'x + 1/2 x'Hq x (a bound at +-inf never counts as reached):
 *     x = clamp(0, lo, hi); full = false; prev = none
 *     for it = 1 .. max_iter:
 *         grad = Qu + Hq x
 *         c_i  = (x_i == lo_i and grad_i > 0) or (x_i == hi_i and grad_i < 0);   f = not c
 *         if prev is set and c == prev and full: converged
 *         if every DOF is in c: converged
 *         factorise Hq_ff (LDL' without pivoting); a pivot not > 0: status 1
 *         xn_f = -Hq_ff^-1 (Qu_f + Hq_fc x_c);  xn_c = x_c;  s = xn - x;  sg = s'grad
 *         if not (sg < 0): converged
 *         step = 1;  while (val(clamp(x + step s)) - val(x)) / (step sg) < 0.1:  step *= 0.6;  if step < 1e-20: status 2
 *         full = (step == 1 and the clamp moved nothing);  x = clamp(x + step s);  prev = c
 *     cap reached: status 2
 * The outputs depend on the final set c alone: k_c = x_c (exactly lo_i or hi_i), K_c = 0, [k_f, K_f] = -Hq_ff^-1 [Qu_f + Hq_fc k_c,
 * Qux_f] by one final solve, k_f then clamped into the box.  The value recursion and expected keep rmx_rollout_lqr's formulas, with
 * the constrained k, K.  max_iter: the cap on the QP iterations of a step; 0 selects the default of 64, a negative value is refused.
 * clamped [batch][nsteps] or NULL: bit i of row k-1 is set where DOF i of step k ended on a bound (the final set; nr <= 32 holds here).
 * out->status: 0, 1 = some factorised free block of Quu0 + mu I had a pivot that is not > 0, 2 = the QP of some step did not terminate
 * within max_iter or its line search ran out.  A rollout with status 1 or 2 gets what rmx_rollout_lqr gives a flagged rollout - every
 * kff, K and clamped row zero, expected 0 -, the other rollouts are untouched and the call returns RMX_OK.
 * Every refusal of rmx_rollout_lqr holds in its words, and: a null box or ubar ("null argument"), ulo > uhi or a NaN bound (as above),
 * max_iter < 0.  The tape and state are not touched, the call can be repeated with the same bits, and a rollout's rows do not depend
 * on its place in the batch, the batch size, shared against per-rollout Q, mu against mu_b, or which optional outputs are NULL.  With
 * every bound infinite or NULL, kff, K, expected and status are THE BITS of rmx_rollout_lqr, and clamped is zero.
 *
 * Out of scope: rmx_rollout_vjp_feedback does not know about the clamp (gradients through a saturated feedback law); BDF2 tapes in
 * the Riccati sweep; per-step or per-rollout limits. */
typedef struct rmx_box {
    const double* ulo;   /* [nr] reduced DOF order, or NULL: no lower bound; entries may be -inf */
    const double* uhi;   /* [nr], or NULL: no upper bound; entries may be +inf                    */
} rmx_box;
int rmx_rollout_tape_feedback_box(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, double pscale,
                                  const rmx_feedback* fb, const rmx_box* box, double* qtraj, double* qdtraj, double* uapp,
                                  rmx_stats* stats);
int rmx_rollout_tape_feedback_box_device(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, double pscale,
                                         const rmx_feedback* fb, const rmx_box* box, double* d_qtraj, double* d_qdtraj, double* d_uapp,
                                         rmx_stats* stats);
int rmx_rollout_lqr_box(rmx_batch* b, int nsteps, const rmx_lqr_cost* cost, const rmx_box* box, const double* ubar, int max_iter,
                        const rmx_lqr_gains* out, unsigned* clamped);
int rmx_rollout_lqr_box_device(rmx_batch* b, int nsteps, const rmx_lqr_cost* cost, const rmx_box* box, const double* d_ubar,
                               int max_iter, const rmx_lqr_gains* out, unsigned* d_clamped);

/* Task-space costs for the device iLQR: world positions of body points along a state record, the pull-back of cotangents through
 * them, and the second-order model of "a joint-space quadratic plus point targets" in the tables rmx_rollout_lqr takes.  Added
 * WITHOUT a change of RMX_VERSION (it stays 111): probe for the symbols.  No existing struct grows.
 *
 * A term is rmx_adjoint_track's: a point xlocal of a body, the step k (1 .. nsteps) at which it is read, a weight.  Arrays over the
 * steps hold step k in row k-1; q [batch][nsteps][nr] is ANY state record in reduced DOF order, typically the qtraj of the last
 * rollout.  For a term t with step_t == k, p_t(q_k) is the world position of its point at the posture q_k and Jp_t = dp_t/dq_k its
 * 3 x nr Jacobian AT THAT STATE (columns of joints off the path from the root to the body are exact zeros) - not at a Newton
 * iterate of the step that produced q_k, which is what rmx_adjoint_track reproduces from the reference.
 *
 * rmx_rollout_points:   x[b][t] = p_t          gq[b][k-1] = sum over the terms of step k of Jp_t' gx[b][t]   (zero rows elsewhere)
 * x and gx are indexed by the term's position in `terms`.  It reads neither xtarget nor wpos.  x or gq may be NULL, not both; gq
 * needs gx.
 *
 * rmx_rollout_cost, with x_k = (q_k, qdot_k), dx = x_k - xgoal_k and r_t = p_t(q_k) - xtarget_t:
 *     Jk[b][k-1] = 1/2 dx' Q_k dx + sum_t 1/2 w_t |r_t|^2                 (the caller sums over k: one fixed order)
 *     lx[b][k-1] = Q_k dx + ( sum_t w_t Jp_t' r_t ; 0 )                   the exact gradient of Jk: rmx_lqr_cost.lx
 *     Q [b][k-1] = Q_k + [ sum_t w_t Jp_t' Jp_t, 0 ; 0, 0 ]               rmx_lqr_cost.Q with per_rollout = 1
 * The last is the GAUSS-NEWTON model: the term sum_t w_t r_t . d2p_t/dq2 of the Hessian is dropped, so the block stays positive
 * semi-definite whatever the residuals.  Every sum runs in one order - the joint-space part, then the terms of the step in the
 * caller's order - and entry (i, j) is formed by the products of entry (j, i) in the same order: the Q written is symmetric bit for
 * bit whenever Q_k is.  The rows and columns of the qdot block, and the rows of steps without a term, are Q_k's bits.
 * sc may be NULL (no joint-space part), and so may sc->Q and sc->xgoal (zero: the bits a table of zeros gives); pts may be NULL (no
 * terms); not sc and pts both.  Any of out's members may be NULL, not all.
 *
 * Both calls read the model and their arguments only: they need no tape, change neither the batch's state nor its tape
 * (rmx_rollout_vjp and the others return the same bits before and after), and can be repeated with the same bits.  A rollout's
 * rows do not depend on its place in the batch, on the batch size, on shared against per-rollout tables, or on which optional
 * outputs are NULL.
 * Refusals (RMX_E_INVALID): the kinematic ones of rmx_rollout_tape, in its words - spherical joints, more than 64 nodes (ground
 * contact and point forces do not enter kinematics: such models are taken); a null batch, q, qdot, out or both of sc and pts, a
 * null pts in rmx_rollout_points, a null xtarget in rmx_rollout_cost ("null argument"); "all outputs are null"; gq without gx;
 * rmx_adjoint_track's messages about the terms; a per-rollout flag other than 0 or 1; nsteps < 1; in rmx_rollout_cost a wpos that is
 * negative or not finite (the message names the term).
 * The host forms stage through one device allocation of their own, made first and freed before they return.  The _device forms:
 * every array a DEVICE pointer (the structs are host objects, `terms` stays a host array), nothing staged but the term table, which
 * goes to a small area of the batch's own; they return when the kernel has finished.
 * Out of scope: a table of the q block alone for rmx_rollout_lqr (the full 2nr x 2nr table per rollout and step is written here and
 * read there).  Orientation and velocity targets: rmx_rollout_frames / rmx_rollout_cost_frames below. */
typedef struct rmx_point_terms {
    int nterms;                    /* >= 1 */
    const rmx_track_term* terms;   /* host; body, xlocal, step (1..nsteps), wpos - rmx_adjoint_track's term */
    const double* xtarget;         /* [nterms][3] or [batch][nterms][3], row = the term's position in `terms` */
    int per_rollout;
} rmx_point_terms;
int rmx_rollout_points(rmx_batch* b, int nsteps, const double* q /*[batch][nsteps][nr]*/, const rmx_point_terms* pts,
                       double* x /*[batch][nterms][3] or NULL*/, const double* gx /*[batch][nterms][3] or NULL*/,
                       double* gq /*[batch][nsteps][nr] or NULL; needs gx*/);
int rmx_rollout_points_device(rmx_batch* b, int nsteps, const double* d_q, const rmx_point_terms* pts, double* d_x, const double* d_gx,
                              double* d_gq);
typedef struct rmx_state_cost {    /* the joint-space quadratic of ilqr.QuadraticCost; may be passed as NULL */
    const double* Q;       /* [nsteps][2nr*2nr] or [batch][..], symmetric, column-major; NULL: zero */
    const double* xgoal;   /* [nsteps][2nr] or [batch][..]; NULL: zero */
    int Q_per_rollout, goal_per_rollout;
} rmx_state_cost;
typedef struct rmx_cost_model {    /* any may be NULL, not all */
    double* Jk;   /* [batch][nsteps]            state cost of step k (the caller sums over k: one fixed order) */
    double* lx;   /* [batch][nsteps][2nr]       rmx_lqr_cost.lx */
    double* Q;    /* [batch][nsteps][2nr*2nr]   rmx_lqr_cost.Q with per_rollout = 1 */
} rmx_cost_model;
int rmx_rollout_cost(rmx_batch* b, int nsteps, const double* q, const double* qdot /*[batch][nsteps][nr] each*/,
                     const rmx_state_cost* sc, const rmx_point_terms* pts /* either may be NULL, not both */,
                     const rmx_cost_model* out);
int rmx_rollout_cost_device(rmx_batch* b, int nsteps, const double* d_q, const double* d_qdot, const rmx_state_cost* sc,
                            const rmx_point_terms* pts, const rmx_cost_model* out);

/* Frame targets in the task-space cost: position, point velocity and orientation of a body frame along a state record, the pull-back
 * of cotangents through them, and the second-order model of "a joint-space quadratic plus frame targets" in the tables
 * rmx_rollout_lqr takes.  Added WITHOUT a change of RMX_VERSION (it stays 111): probe for the symbols.  No existing struct grows and
 * no existing entry changes.
 *
 * A frame term is a point xlocal of body n, read at step k (1-based), with three weights wpos, wvel, wrot >= 0.  At the state
 * (q_k, qdot_k) of row k-1 of the record, with Rw[i], pw[i] the world frame of node i, (sw_j, sv_j) the world screw of joint j and
 * path = n and its strict ancestors (every Jacobian column of a DOF off the path is an exact zero):
 *     position       p = Rw[n] xlocal + pw[n]                          Jp_j = sv_j + sw_j x p
 *     orientation    R = Rw[n]                                          Jw_j = sw_j
 *     node twists    om_i = sum_{j in anc*(i)} sw_j qdot_j             V_i = sum_{j in anc*(i)} sv_j qdot_j     (i itself included)
 *     point velocity v = V_n + om_n x p  ( = Jp qdot )                 dv/dqdot_j = Jp_j
 *                    dv/dq_i = G_i = sw_i x (v - (V_i + om_i x p)) + om_i x Jp_i       for i on the path
 *     residuals      r = p - xtarget,  rv = v - vtarget,  e_w = 1/2 a(R Rtarget'),  a(M) = (M32 - M23, M13 - M31, M21 - M12)
 *     cost           wpos/2 |r|^2 + wvel/2 |rv|^2 + wrot/4 |R - Rtarget|_F^2
 * The last piece is wrot (1 - cos theta), theta the angle between the two frames: the chordal cost.  Its gradient VANISHES at
 * theta = pi (a target exactly opposite gives no direction); keep targets away from it or pass through an intermediate one.
 *     gradient       q rows: wpos Jp'r + wvel G'rv + wrot Jw'e_w        qdot rows: wvel Jp'rv                      (exact)
 *     Gauss-Newton   qq: wpos Jp'Jp + wvel G'G + wrot Jw'Jw    q,qdot: wvel G'Jp    qdot,q: wvel Jp'G    qdot,qdot: wvel Jp'Jp
 * The curvature of p, v and R is dropped, so the addition is positive semi-definite whatever the residuals; wrot Jw'Jw does not
 * depend on R or Rtarget.  A 3x3 is column-major, as everywhere in this header.  A constant frame offset Rl on the body is not an
 * argument: it folds into the target, R Rl against Rt being R against Rt Rl'.
 *
 * rmx_rollout_frames: x[b][t] = p_t, v[b][t] = v_t, R[b][t] = R_t (any may be NULL), and for cotangents gx, gv, gR (any may be NULL:
 * zero)   gq[b][k-1] = sum_t Jp'gx + G'gv + Jw'a(gR R'),   gqd[b][k-1] = sum_t Jp'gv   over the terms of step k, zero rows at steps
 * without a term.  gq needs one of the cotangents, gqd needs gv.  It reads neither the weights nor the targets.  With v, R, gv, gR and
 * gqd all NULL, x and gq are the bits of rmx_rollout_points.
 *
 * rmx_rollout_cost_frames is rmx_rollout_cost with frame terms: Jk, lx and Q keep the layouts rmx_rollout_lqr reads.  Order of every
 * sum: the joint-space part, then the terms in the caller's order, inside a term position, velocity, rotation.  Entries (i, j) and
 * (j, i) of Q are formed from the same products in the same order: Q is symmetric bit for bit whenever the input is, the two cross
 * blocks included.  A structural zero adds nothing: a step whose terms all have wvel = wrot = 0, and a step without terms, has the
 * bits rmx_rollout_cost writes for the same position terms (Jk, lx and Q), whatever the other steps of the call carry.  A target
 * table may be NULL only if every term's matching weight is zero; otherwise the call is refused and the message names the table.
 *
 * Everything else is rmx_rollout_cost's: no tape is needed, state and tape are left untouched, calls repeat with the same bits, a
 * rollout's rows do not depend on its place in the batch, the batch size, shared against per-rollout tables or which outputs are
 * NULL; models with ground contact and point forces are taken; the refusals in its words (spherical joints, more than 64 nodes,
 * the terms, the per-rollout flags, nsteps; "null argument" for a null batch, q, qdot, out - ft in rmx_rollout_frames - or both of
 * sc and ft; "all outputs are null"); a weight that is negative or not finite is refused by the term and the weight's name.  The host
 * forms stage through one allocation of their own; the _device forms take DEVICE pointers for every array (`terms` stays host).
 * Out of scope: angular-velocity targets; the logarithmic-map residual; a q-block-only table. */
typedef struct rmx_frame_term { int body; double xlocal[3]; int step; double wpos, wvel, wrot; } rmx_frame_term;
typedef struct rmx_frame_terms {
    int nterms; const rmx_frame_term* terms;          /* host */
    const double *xtarget, *vtarget, *Rtarget;        /* [nterms][3], [nterms][3], [nterms][9], or [batch][..] */
    int per_rollout;
} rmx_frame_terms;
int rmx_rollout_frames(rmx_batch* b, int nsteps, const double* q, const double* qdot /*[batch][nsteps][nr] each*/, const rmx_frame_terms* ft,
                       double* x /*[batch][nterms][3]*/, double* v /*[batch][nterms][3]*/, double* R /*[batch][nterms][9]*/,
                       const double* gx, const double* gv, const double* gR /* the shapes of x, v, R */,
                       double* gq, double* gqd /*[batch][nsteps][nr] each*/);
int rmx_rollout_frames_device(rmx_batch* b, int nsteps, const double* d_q, const double* d_qdot, const rmx_frame_terms* ft, double* d_x,
                              double* d_v, double* d_R, const double* d_gx, const double* d_gv, const double* d_gR, double* d_gq,
                              double* d_gqd);
int rmx_rollout_cost_frames(rmx_batch* b, int nsteps, const double* q, const double* qdot, const rmx_state_cost* sc,
                            const rmx_frame_terms* ft /* either may be NULL, not both */, const rmx_cost_model* out);
int rmx_rollout_cost_frames_device(rmx_batch* b, int nsteps, const double* d_q, const double* d_qdot, const rmx_state_cost* sc,
                                   const rmx_frame_terms* ft, const rmx_cost_model* out);

/* The backtracking line search of the device iLQR in ONE launch: every rollout tries its step lengths in turn, inside the wavefront
 * that integrates it, and stops at the first that lowers its own cost; the record, uapp and the tape it leaves belong to the
 * trajectory it kept.  An iLQR iteration is then three calls: rmx_rollout_cost[_frames] (the model), rmx_rollout_lqr[_box] (the
 * gains), rmx_rollout_search.  Added WITHOUT a change of RMX_VERSION (it stays 111): probe for the symbols.  No existing struct grows
 * and no existing entry changes.  BDF1 only: that is the tape rmx_rollout_lqr reads.
 *
 * fb->uff is the NOMINAL torque ubar; fb->K, fb->xref and fb->per_rollout keep the meaning they have in rmx_rollout_tape_feedback.
 * Per rollout, from the state the batch holds at the call (q0, qdot0):
 *     for a in alphas, in order:
 *         uff_k = ubar_k + a * kff_k        the product rounded, then the sum - two roundings, NOT a fused multiply-add: the bits of
 *                                           the float64 expression a caller forms
 *         run the closed loop of rmx_rollout_tape_feedback_box (integrator 1) under uff, K, xref, box from (q0, qdot0)
 *         J = the cost of that pass (below)
 *         if no solve of the pass failed (status bits 1, 2, 4 clear) and J < Jbar (false for a NaN):   alpha = a; stop
 *     if nothing was accepted, or nalpha == 0:
 *         one pass with uff = ubar (kff is not read: a non-finite kff cannot reach it); alpha = 0; J = its cost
 * The record (qtraj, qdtraj), uapp, the state the batch is left in, `out` and the tape all belong to the LAST pass the rollout ran.
 * The tape is the open-loop BDF1 tape under uapp: rmx_rollout_vjp, _linearize, _jvp, _vjp_params, _lqr and _lqr_box read it
 * unchanged.  Trial passes and the nominal pass run the same instructions - alpha is a value, not a code path -, hence, exactly:
 * a call with nalpha = 0 and uff = ubar + a*kff formed by the caller in float64 returns the bits of a call that accepts a; and the
 * nominal pass of a call reproduces the trajectory a previous call of this entry left, with its J, bit for bit, when xref is that
 * trajectory (row 0: the initial state) and uff its uapp.  A rollout's results do not depend on its place in the batch, the batch
 * size, shared against per-rollout tables, or which optional outputs are NULL.
 *
 * The cost, evaluated inside the launch on the states the pass has just produced - x_k = (q_k, qdot_k) the state after step k, u_k
 * the APPLIED torque (behind the clamp), dx_k = x_k - xgoal_k:
 *     J = sum_{k=1..N} [ 1/2 dx_k' Q_k dx_k  +  1/2 u_k' R u_k  +  sum_{t: step_t = k} wpos/2 |r|^2 + wvel/2 |rv|^2 + wrot/4 |R - Rtarget|_F^2 ]
 * with the definitions of rmx_rollout_cost_frames (a point term is a frame term with wvel = wrot = 0).  One fixed order: steps
 * ascending; within a step the state part, then the control part, then the terms in the caller's order.  Neither the gradient nor
 * the Gauss-Newton table is formed here: rmx_rollout_cost* stays the call that makes them once per iteration.
 * out->trials: passes run (trial passes + the nominal pass if it ran).  out->status and stats->status: the Newton status of the
 * pass the rollout ended on; stats->newton_iters: its iterations.
 *
 * Refusals (RMX_E_INVALID), which leave an existing tape and the batch alone: everything rmx_rollout_tape_feedback_box refuses, in
 * its words (box itself may be NULL here: no limits); everything rmx_rollout_cost_frames refuses about terms, weights, target tables
 * and per-rollout flags, in its words; a null b, fb, fb->uff, s, cost, out or out->J ("null argument"); all of sc, ft, R null;
 * nalpha outside 0 .. RMX_SEARCH_MAX_ALPHAS; an alpha that is not finite or not > 0 (the message names its index); a null kff or
 * Jbar with nalpha > 0; nr > 32 or a tree of more than 32 nodes, in rmx_rollout_lqr's words - the search exists where the sweep that
 * feeds it exists.  The host form stages through one allocation of its own, made first and freed before it returns.  The _device
 * form: every array a DEVICE pointer (the structs, `alphas` and `terms` are host objects); it returns when the kernel has finished.
 * Against rmx_rollout_tape_feedback_box on the same inputs a nalpha = 0 pass agrees to rounding, not bit for bit (the kernel is a
 * text of its own).  Measured on an MI355X over 5 steps of 4 rollouts under LQR gains, the largest |difference| over q, qdot and
 * uapp: 3.6e-15 (3-link chain), 0 - the same bits - (5), 4.2e-14 (11), 6.8e-14 (32); with limits that bind 2.6e-15, 2.7e-15,
 * 6.8e-15, 2.9e-13 (tests/test_gpu_rollout_search.py).
 * Out of scope: BDF2 tapes; nr > 32; gradients through the search; a regulariser schedule; per-step or per-rollout limits; several
 * alphas of one rollout in parallel wavefronts. */
#define RMX_SEARCH_MAX_ALPHAS 16
typedef struct rmx_search_cost {       /* not all three NULL */
    const rmx_state_cost*  sc;         /* joint-space quadratic on x_k = (q_k, qdot_k); may be NULL        */
    const rmx_frame_terms* ft;         /* frame terms (a point term has wvel = wrot = 0); may be NULL      */
    const double*          R;          /* [nr*nr] column-major, symmetric; NULL: no control cost           */
} rmx_search_cost;
typedef struct rmx_search {
    const double* kff;      /* [batch][nsteps][nr]; may be NULL when nalpha == 0                            */
    const double* alphas;   /* HOST [nalpha], each finite and > 0, tried in this order                      */
    int           nalpha;   /* 0 .. RMX_SEARCH_MAX_ALPHAS; 0: the nominal pass alone                        */
    const double* Jbar;     /* [batch] the cost a trial has to beat; may be NULL when nalpha == 0           */
} rmx_search;
typedef struct rmx_search_out {         /* J required, the others may be NULL */
    double* J;        /* [batch] cost of the trajectory the rollout ended on                                */
    double* alpha;    /* [batch] the accepted step length, 0: none                                          */
    int*    trials;   /* [batch] passes run (trial passes + the nominal pass if it ran)                     */
    int*    status;   /* [batch] Newton status of the pass the rollout ended on (rmx_stats' bits)           */
} rmx_search_out;
int rmx_rollout_search(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const rmx_feedback* fb,
                       const rmx_box* box /* may be NULL */, const rmx_search* s, const rmx_search_cost* cost,
                       double* qtraj, double* qdtraj, double* uapp, const rmx_search_out* out, rmx_stats* stats);
int rmx_rollout_search_device(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const rmx_feedback* fb,
                              const rmx_box* box, const rmx_search* s, const rmx_search_cost* cost, double* d_qtraj,
                              double* d_qdtraj, double* d_uapp, const rmx_search_out* out, rmx_stats* stats);

/* Model-parameter gradients from the taped rollout (system identification, calibration): dL/dtheta for joint stiffness, damping and
 * rest position, body inertia and mass, and gravity, for the same cotangents rmx_rollout_vjp takes.  Added WITHOUT a change of
 * RMX_VERSION (it stays 111): probe for the symbols.
 *
 * Every taped solve is the implicit function g(x; qA, qB, u, theta) = 0 of rmx_rollout_tape_bdf2 above, and the backward sweep forms
 * the adjoint vector z of every solve (the z of solve_bwd; under BDF2 the SDIRK2a and SDIRK2b solves of step 1 each have their own).
 * g is linear in each of these parameters, so
 *     dL/dtheta = - sum over all slots s of the tape   z_s' dg_s/dtheta
 * with dg_s/dtheta taken at the slot's solution x_s with its qA, qB and eta - the rule that gives du = eta^2 pscale z.  With
 * v = (x - qA)/eta, and per body i, in the BODY frame (where the inertia is diag(I_i[0..5])), w = (J z)_i, phi = (J v)_i,
 * beta = (J (x - qB) + eta^2 Jdot v)_i:
 *     d(z'g)/dstiffness_j = eta^2 z_j (x_j - qRest_j)      d(z'g)/ddamping_j = eta^2 z_j v_j      d(z'g)/dqRest_j = -eta^2 k_j z_j
 *     d(z'g)/dI_i[c]      = w_c beta_c - eta^2 (ad(phi) w)_c phi_c   ( - eta^2 w_lin . R_i' grav  for c = 3 )      c = 0 .. 5
 *     d(z'g)/dgrav_k      = -eta^2 sum_i m_i (R_i w_i,lin)_k
 * The weight of a body is I_i[3] R_i' grav (the reference reads the mass from that entry alone, Body.m:104-109), so the gravity term
 * belongs to c = 3; the entries 3 .. 5 must be equal (rmx_model_create), and the gradient of the mass is the sum of the three.
 * A body on a fixed joint has no DOF of its own and still gets its inertia row, through its ancestors' columns of J.  Joint-limit
 * constants, axes, frames and the constant tau are not parameters here (dL/dtau is the sum over the steps of du / pscale).
 *
 * rmx_rollout_vjp_params reads the tape of the preceding rmx_rollout_tape / rmx_rollout_tape_bdf2 on the batch and follows its
 * integrator.  gq, gqd, du, dq0, dqd0: as rmx_rollout_vjp, and du, dq0, dqd0 are the bits rmx_rollout_vjp returns for the same tape and
 * cotangents (dq0, dqd0 NULL together: not formed).  out: one row per rollout - the gradient of a parameter the rollouts share is the
 * caller's sum over the batch (the rows stay apart because a loss may weight rollouts).  stiffness, damping and qrest are per reduced
 * DOF: a value set per joint reaches every DOF of a multi-DOF joint, and its gradient is the sum of those DOFs' entries.  Any of the
 * five pointers may be NULL - that output is neither computed nor stored - but not all of them; an output has the same bits
 * whichever others are asked for.  The sum over the slots runs in a fixed order: repeated calls return the same bits.
 *
 * The tape keeps the states it differentiates at - q0, qdot0 and the trajectory, copied on the batch's stream by the tape call
 * (recorded in place where the caller asked for no record) - exactly as long as it keeps H, M, D; the SDIRK2a result qa of a BDF2
 * tape is rebuilt from them: qda = (q1 - al h qd1 - q0)/((1 - al) h), qa = q0 + al h qda.
 *
 * The call changes neither the batch's state nor the tape: it may be repeated, and rmx_rollout_vjp and rmx_rollout_linearize return
 * the same bits before and after it.  Refusals (RMX_E_INVALID), in rmx_rollout_vjp's words where they coincide: "no tape", an nsteps
 * that differs from the tape's, a null batch, gq, gqd, du or out ("null argument"), "all outputs are null".  The rows of a rollout whose
 * tape call reported a failed Newton solve (stats->status) are unspecified.
 * The _device form: every array a DEVICE pointer (the struct itself is a host object), nothing staged; it returns when the kernels
 * have finished. */
typedef struct rmx_param_grads {   /* every pointer may be NULL (not formed), but not all five */
    double* stiffness;   /* [batch][nr]          reduced DOF order                         */
    double* damping;     /* [batch][nr]                                                    */
    double* qrest;       /* [batch][nr]                                                    */
    double* inertia;     /* [batch][njoints][6]  listing order, the layout of desc.I_i     */
    double* grav;        /* [batch][3]                                                     */
} rmx_param_grads;
int rmx_rollout_vjp_params(rmx_batch* b, int nsteps, const double* gq, const double* gqd, double* du, double* dq0, double* dqd0,
                           const rmx_param_grads* out);
int rmx_rollout_vjp_params_device(rmx_batch* b, int nsteps, const double* d_gq, const double* d_gqd, double* d_du, double* d_dq0,
                                  double* d_dqd0, const rmx_param_grads* out);

/* Taped rollouts of a model with point forces (ForcePointPoint, ForceSpringDamper, ForceCable: rmx_model_set_point_forces), so that
 * spring-coupled and cable-driven mechanisms can be differentiated, linearised and controlled.  Added WITHOUT a change of RMX_VERSION
 * (it stays 111): probe for the symbols.  No existing struct grows and no existing entry changes: the feature is a switch per model,
 * off by default.
 *
 * enable = 1: rmx_rollout_tape, rmx_rollout_tape_bdf2, rmx_rollout_tape_feedback and rmx_rollout_tape_feedback_box (and their
 * _device forms) take a model that has a force table; 0 (the default) restores the refusal, word for word.  A model without a force
 * table is not affected either way: the same kernels, the same bits.  May be called before or after rmx_model_set_point_forces, any
 * number of times; it takes effect at the next tape call and leaves an existing tape alone.
 *
 * The tape has the layout of every other tape.  Its H carries the forces' blocks (the H of rmx_eval on such a model), and its
 * D = df/dqdot their damping.  With x_k the points of a force on their bodies, A_k(a) the column of the point Jacobian for joint a,
 * and per segment j = (point j, point j+1) of the force's polyline dA_j = A_{j+1} - A_j, u_j the segment's unit vector:
 *     point-point            D(a,i) -= kd  dA(a) . dA(i)
 *     spring / taut cable    D(a,i) -= (kd/L) lam(a) lam(i),   lam(a) = sum_j u_j . dA_j(a)
 *     slack cable            nothing
 * which is the reference's J' Dm J (computeValues adds it to D).  The readers of a tape read the n x n blocks densely, so they run
 * on such a tape unchanged: rmx_rollout_vjp, rmx_rollout_linearize, rmx_rollout_jvp, rmx_rollout_vjp_feedback, rmx_rollout_lqr,
 * rmx_rollout_lqr_box.  rmx_last_step_kernel reports "k_adjoint_fwd<bdf1,tape,pf>", "<bdf2,tape,pf>", "<bdf1,tape,feedback,pf>" or
 * "<bdf2,tape,feedback,pf>" after the tape call.
 *
 * A cable is not differentiable where a solve ends exactly at l = L.  The tape holds the blocks of the branch the last evaluated
 * iterate of each solve was on (taut: l > L), and the gradients are those of that branch.
 * The sweep is rmx_rollout_tape's: Newton WITHOUT a line search.  A solve whose iterates keep crossing l = L of a stiff cable can
 * end at the iteration limit (stats->status bit 2) where rmx_step_bdf1's line search converges; the rows of such a rollout are
 * unspecified, as for every tape call.  Measured on a 32-node tree with a stiff four-point cable from 512 random states: no
 * rollout within 20 steps, 152 (BDF1) and 176 (BDF2) within 100 (profiles/tape_pf.txt; the numpy restatement of the sweep, without
 * a line search either, fails from such states too).
 *
 * rmx_rollout_vjp_params refuses a tape that carries point forces (RMX_E_INVALID, "point forces"): its contraction covers the joint
 * and body parameters of a model without them; rmx_rollout_vjp_forces (below) is the call for such a tape, and forms the gradients in
 * the force constants too.  These refuse a model with a force table in the words they always had, whatever the
 * switch says: rmx_rollout_search, rmx_adjoint_bdf1, rmx_adjoint_bdf2, rmx_adjoint_controls, rmx_adjoint_track, rmx_step_euler,
 * rmx_eval_mfd, rmx_compute_values.
 * Out of scope: gradients in the attachment points of the forces; forward-mode tangents in the force constants; the device line search; the
 * in-library objectives; forces together with ground contact or spherical joints (rmx_model_set_point_forces refuses those). */
int rmx_model_tape_point_forces(rmx_model* m, int enable);   /* enable: 0 or 1 */
int rmx_model_get_tape_point_forces(const rmx_model* m);     /* 0 / 1; a null model: RMX_E_INVALID */

/* Parameter gradients from a tape that carries point forces (calibration of a spring stiffness, a damper, a cable's rest length):
 * rmx_rollout_vjp_params for such a tape, plus dL/dtheta for the constants of every row of the force table.  Added WITHOUT a change
 * of RMX_VERSION (it stays 111): probe for the symbols.
 *
 * The rule is rmx_rollout_vjp_params': dL/dtheta = - sum over all slots s of the tape  z_s' dg_s/dtheta.  The forces' share of g is
 * eta^2 sum_j dA_j(a) . F_j over the segments j of the force's polyline (dA_j = A_{j+1} - A_j: the columns of the point Jacobian,
 * u_j the segment's unit vector, lam(a) = sum_j u_j . dA_j(a), l and ldot the total length and its rate).  Per slot:
 *     point-point            with zA = sum_a z_a dA(a):   d(z'g)/dks = eta^2 zA . dx      d(z'g)/dkd = eta^2 zA . dv      (no L: +0.0)
 *     spring / taut cable    with zl = sum_a z_a lam(a):  d(z'g)/dks = eta^2 zl (l - L)/L   d(z'g)/dkd = eta^2 zl ldot/L
 *                                                         d(z'g)/dL  = -eta^2 zl (ks l + kd ldot)/L^2
 *     cable with !(strain > 0) at the slot's solution: nothing in any of the three (the branch the tape holds)
 * The joint, inertia and gravity parameters' dg/dtheta does not involve the forces: `model` fills rmx_rollout_vjp_params' five arrays
 * by that entry's own contraction, from the z of this tape.
 *
 * rmx_rollout_vjp_forces reads the tape of the preceding rmx_rollout_tape / _tape_bdf2 / _tape_feedback / _tape_feedback_box call on a
 * model whose tape carries point forces, and follows its integrator (a closed-loop tape is the open-loop tape under uapp).  gq, gqd,
 * du, dq0, dqd0: as rmx_rollout_vjp, and the same bits.  model (may be NULL): as `out` of rmx_rollout_vjp_params.  forces (may be
 * NULL): one row per rollout and force, in the order of the table given to rmx_model_set_point_forces.  Any pointer of either struct may be NULL -
 * that output is neither computed nor stored - but not all eight; an output has the same bits whichever others are asked for, and
 * repeated calls return the same bits.  The call changes neither the batch's state nor the tape.
 * Refusals (RMX_E_INVALID): a null batch, gq, gqd or du ("null argument"); dq0 and dqd0 not given together; both structs NULL or all
 * eight pointers NULL ("all outputs are null"); "no tape"; an nsteps that differs from the tape's; a tape without point forces (the
 * message names rmx_rollout_vjp_params, the call for it).
 * The _device form: every array a DEVICE pointer (the structs themselves are host objects), nothing staged. */
typedef struct rmx_force_grads {   /* every pointer may be NULL (not formed) */
    double* stiffness;   /* [batch][nforces]  the order of the force table               */
    double* damping;     /* [batch][nforces]                                             */
    double* L;           /* [batch][nforces]  a point-point force has no L: +0.0 there   */
} rmx_force_grads;
int rmx_rollout_vjp_forces(rmx_batch* b, int nsteps, const double* gq, const double* gqd, double* du, double* dq0, double* dqd0,
                           const rmx_param_grads* model, const rmx_force_grads* forces);
int rmx_rollout_vjp_forces_device(rmx_batch* b, int nsteps, const double* d_gq, const double* d_gqd, double* d_du, double* d_dq0,
                                  double* d_dqd0, const rmx_param_grads* model, const rmx_force_grads* forces);

/* Forward-mode tangents of the taped rollout with respect to the model's parameters: J t for directions in joint stiffness, damping
 * and rest position, body inertia and mass, and gravity - whole columns of the Jacobian of the trajectory, what Gauss-Newton and
 * Levenberg-Marquardt system identification (few parameters, many residuals) ask for.  With it the taped rollout is differentiable in
 * both modes with respect to everything rmx_rollout_vjp and rmx_rollout_vjp_params differentiate.  Added WITHOUT a change of
 * RMX_VERSION (it stays 111): probe for the symbols.
 *
 * Every taped solve is g(x; qA, qB, u, theta) = 0, so the recursion is rmx_rollout_jvp's with one more term on the right,
 *     H dx = M dqB - eta D dqA + eta^2 pscale du - (dg/dtheta) ttheta ,     dv = (dx - dqA)/eta
 * with dg/dtheta taken at the slot's recorded x, qA, qB and eta (under BDF2 the SDIRK2a solve, slot nsteps, has its own term; its
 * state is rebuilt as rmx_rollout_vjp_params rebuilds it).  With v = (x - qA)/eta, and per body i in the BODY frame phi = (J v)_i,
 * beta = (J (x - qB) + eta^2 Jdot v)_i, the entry of (dg/dtheta) ttheta at DOF j is
 *     eta^2 (tstiffness_j (x_j - qRest_j) + tdamping_j v_j - k_j tqrest_j)  +  s_j . (sum over the bodies i of j's subtree of W_i)
 *     W_i = the wrench  tI_i o beta - eta^2 ad(phi)'(tI_i o phi) - eta^2 (0 ; tI_i[3] R_i' grav)  carried to the world frame
 *           - eta^2 m_i (p_i x tgrav ; tgrav)
 * (o: entry by entry; s_j the world-frame screw of joint j).  It is the transpose of rmx_rollout_vjp_params on the same tape: with
 * that call's per-rollout rows for cotangents (gq, gqd),
 *     <gq, tq> + <gqd, tqd> = <du, tu> + <dq0, tq0> + <dqd0, tqd0> + sum over the five groups of <grad_group[b], ttheta_group[b, t]>.
 * The inertia entries 3 .. 5 are each "the mass", and gravity belongs to entry 3, exactly as for the gradient: a physical mass
 * tangent is the same number in all three.  Only the `inertia` rows whose listing index maps to a node are read.
 *
 * rmx_rollout_jvp_params reads the tape of the preceding rmx_rollout_tape / _tape_bdf2 / _tape_feedback / _tape_feedback_box call on
 * the batch and follows its integrator; h and pscale are the tape's (a closed-loop tape is the open-loop tape under uapp).  A tape
 * that carries point forces is accepted: the five groups' dg/dtheta does not involve the forces, and H and D on the tape already
 * carry them.  ntan >= 1 directions per rollout; direction t of rollout b moves the parameters by tp's rows (b, t) and u, q0, qdot0
 * by tu, tq0, tqd0 (rmx_rollout_jvp's layouts; NULL: zero).  tq, tqd: [batch][ntan][nsteps][nr], both required.
 *
 * The call changes neither the batch's state nor the tape: it may be repeated with the same bits, and the other readers of the tape
 * return the same bits before and after it.  One direction has the same bits whatever ntan is and wherever it stands in the call; a
 * rollout's rows do not depend on its place in the batch.  With all five parameter tangents given as arrays of zeros, tq and tqd
 * equal rmx_rollout_jvp's for the same tu, tq0, tqd0 as numbers.  Refusals (RMX_E_INVALID), in rmx_rollout_jvp's words where they
 * coincide: "no tape", an nsteps that differs from the tape's, a null batch, tp, tq or tqd ("null argument"), "ntan < 1", all five
 * pointers of tp NULL (the message names rmx_rollout_jvp, the call for it).  The rows of a rollout whose tape call reported a failed
 * Newton solve are unspecified.  Both forms allocate [batch][ntan][nslots][n] doubles for the parameter term, and the host form its
 * staging, in an allocation of the call's own, freed before it returns; the tape's workspace does not grow.
 * The _device form: every array a DEVICE pointer (the struct itself is a host object); it returns when the kernels have finished.
 * Out of scope: tangents in the force constants and attachment points; joint-limit constants, axes and frames, as for the
 * gradients; models the tape calls refuse. */
typedef struct rmx_param_tangents {   /* every pointer may be NULL (zero), but not all five */
    const double* stiffness;   /* [batch][ntan][nr]          reduced DOF order                 */
    const double* damping;     /* [batch][ntan][nr]                                            */
    const double* qrest;       /* [batch][ntan][nr]                                            */
    const double* inertia;     /* [batch][ntan][njoints][6]  listing order, layout of desc.I_i */
    const double* grav;        /* [batch][ntan][3]                                             */
} rmx_param_tangents;
int rmx_rollout_jvp_params(rmx_batch* b, int nsteps, int ntan, const rmx_param_tangents* tp, const double* tu, const double* tq0,
                           const double* tqd0, double* tq, double* tqd);
int rmx_rollout_jvp_params_device(rmx_batch* b, int nsteps, int ntan, const rmx_param_tangents* tp, const double* d_tu,
                                  const double* d_tq0, const double* d_tqd0, double* d_tq, double* d_tqd);

/* euler() of matlab-simple/testRedMax.m:67-109 (BASELINE.json configs[0]): nsteps linearly-implicit Euler steps,
 *   Mr = J'MmJ ; (Mr + h Dr - h^2 Kr) qdot1 = Mr qdot0 + h (J'(fm - Mm Jdot qdot0) + fr) ; q1 = q0 + h qdot1.
 * hist_T/hist_V as in rmx_step_bdf1. */
int rmx_step_euler(rmx_batch* b, double h, int nsteps, double* hist_T, double* hist_V);

/* Joint.computeEnergies + Body.computeEnergies at the current state (Joint.m:616-637, Body.m:167-173):
 * host arrays [batch]. */
int rmx_energy(rmx_batch* b, double* T, double* V);

/* The HIP stream the batch's kernels are enqueued on (as void*), for callers that order other work
 * (e.g. a torch.distributed gather) after it. */
void* rmx_batch_stream(const rmx_batch* b);
/* ---- Asynchronous stepping: one host thread (MATLAB has one) driving several batches / devices at once (ABI 107).
 * simLoop (driverRedMaxBDF1.m:57-91, driverRedMaxBDF2.m:57-125) of a batch is ONE kernel launch on the batch's own stream; the
 * *_async entries enqueue it and return without waiting, so a host loop over batches that live on different devices (or on one
 * device) has all of them running before it blocks on the first rmx_sync().  Rules: between an *_async call and rmx_sync() on the
 * same batch only *_async / rmx_sync / rmx_stats_reset may be called on it; other batches are free.  The per-trajectory counters
 * accumulate on the device (rmx_stats_reset before, rmx_stats_read after the sync).
 *   rmx_step_bdf1_async / rmx_step_bdf2_async   nsteps steps, no per-step record
 *   rmx_step_history_async                      integrator 1 | 2 as rmx_step_history; `record` chooses what Scene.saveHistory
 *                                               (Scene.m:134-161) keeps ON THE DEVICE for every step: RMX_REC_ENERGY (T, V),
 *                                               RMX_REC_STATE (q, qdot), RMX_REC_CHARTS (Euler charts), OR-ed together
 *   rmx_sync                                    waits for the batch's stream; reports a failed launch
 *   rmx_history_read                            after rmx_sync: copies the record of the last rmx_step_history_async into host arrays
 *                                               shaped as in rmx_history (any pointer whose part was not recorded must be NULL);
 *                                               the record stays readable until the next step call on the batch */
enum { RMX_REC_ENERGY = 1, RMX_REC_STATE = 2, RMX_REC_CHARTS = 4 };
int rmx_step_bdf1_async(rmx_batch* b, const rmx_opts* opts, int nsteps);
int rmx_step_bdf2_async(rmx_batch* b, const rmx_opts* opts, int nsteps);
int rmx_step_history_async(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, int record);
int rmx_sync(rmx_batch* b);
int rmx_history_read(rmx_batch* b, const rmx_history* hist);

/* ---- Multi-device groups (ABI 107): BASELINE.json's north_star shards the batch axis across GPUs and names MATLAB as the host.
 * A group owns one model + one batch per listed device (a device may be listed more than once: its shards then share it, each on
 * its own stream) and splits `batch` trajectories into contiguous shards whose sizes differ by at most one, in device-list order
 * (the "strong" plan of redmax_amd/sharding.py).  Every array argument is the WHOLE batch, shaped exactly as for a single rmx_batch;
 * the group scatters / gathers the shards' slices.  rmx_group_step is simLoop for the whole batch: it launches every shard's
 * kernel asynchronously, then waits for all of them and gathers the counters and the per-step record into the caller's arrays -
 * the one "collective" of the path, here a set of device-to-host copies (no RCCL: the host array is the destination).
 * gc may be NULL (no ForceGroundCuboid).  devices == NULL: devices 0 .. ndevices-1. */
typedef struct rmx_group rmx_group;
int rmx_group_create(const rmx_model_desc* desc, const rmx_ground_contact* gc, int batch, const int* devices, int ndevices,
                     rmx_group** out);
void rmx_group_destroy(rmx_group* g);
int rmx_group_batch_size(const rmx_group* g);
int rmx_group_nshards(const rmx_group* g);
/* shard s: its device, the index of its first trajectory in the whole batch and its trajectory count (any pointer may be NULL) */
int rmx_group_shard(const rmx_group* g, int s, int* device, int* first, int* count);
/* the shard's own batch / model, for the hooks that have no group form (rmx_eval, rmx_eval_mfd, rmx_adjoint_*, rmx_step_euler,
 * rmx_get_charts ...): call them per shard with the array pointers advanced to the shard's first trajectory */
rmx_batch* rmx_group_shard_batch(rmx_group* g, int s);
rmx_model* rmx_group_shard_model(rmx_group* g, int s);
int rmx_group_set_state(rmx_group* g, const double* q, const double* qdot);     /* [batch][nr], as rmx_set_state */
int rmx_group_get_state(rmx_group* g, double* q, double* qdot);
/* stats, hist: as rmx_step_history, arrays for the whole batch; hist (and any of its members) may be NULL */
int rmx_group_step(rmx_group* g, const rmx_opts* opts, int nsteps, int integrator, rmx_stats* stats, const rmx_history* hist);
/* the two halves of rmx_group_step for hosts that overlap their own work with the devices: launch all shards (record: RMX_REC_*),
 * then wait and gather (stats / hist as above; hist members outside `record` must be NULL) */
int rmx_group_step_async(rmx_group* g, const rmx_opts* opts, int nsteps, int integrator, int record);
int rmx_group_sync(rmx_group* g, rmx_stats* stats, const rmx_history* hist);
int rmx_group_energy(rmx_group* g, double* T, double* V);                      /* [batch], as rmx_energy */
/* The final gather with DEVICE-resident destinations (ABI 111) - BASELINE.json north_star: "the batch axis shards naturally across GPUs
 * with RCCL over xGMI only for the final gather"; SURVEY.md 8(e): one collective at the end of the rollout, [B/N][nr] x 2 per shard.
 * d_q[s], d_qdot[s] (s < nshards): device pointers to [batch][nr] arrays ON SHARD s's DEVICE (a shard that receives nothing may pass
 * NULL).  root_or_all = RMX_GATHER_ALL: every shard's device receives the whole batch; a shard index: that shard's device alone.
 * Groups whose devices are pairwise distinct form a single-process RCCL clique at the first call (ncclCommInitAll on the device list;
 * librccl is bound at run time, the library itself links the HIP runtime only) and run ncclAllGather (equal shards), one
 * ncclBroadcast per shard inside a group call (shards that differ by one rollout) or ncclSend / ncclRecv (one root), enqueued on
 * the shards' own streams behind their step kernels.  A group that lists a device more than once - RCCL refuses such a clique -
 * exchanges by device-to-device / peer copies on the same streams (RMX_GROUP_GATHER=copy in the environment forces that path).
 * Returns when the destinations are complete.  rmx_group_gather_path: how the last gather travelled ("rccl:allgather",
 * "rccl:broadcast", "rccl:sendrecv", "copy"; "" before the first). */
enum { RMX_GATHER_ALL = -1 };
int rmx_group_gather_device(rmx_group* g, double* const* d_q, double* const* d_qdot, int root_or_all);
const char* rmx_group_gather_path(const rmx_group* g);
/* The same gather into [batch][nr] destinations the GROUP owns on every receiving shard's device (allocated at the first call; for
 * hosts that cannot allocate device memory themselves - the MEX gateway's 'gather').  rmx_group_gathered: the device pointers of shard
 * s's copy (valid until the group is destroyed; what a MATLAB host would wrap as gpuArray); rmx_group_gathered_read: that copy into host
 * arrays ([batch][nr]; either pointer may be NULL). */
int rmx_group_gather(rmx_group* g, int root_or_all);
int rmx_group_gathered(rmx_group* g, int s, const double** d_q, const double** d_qdot);
int rmx_group_gathered_read(rmx_group* g, int s, double* q, double* qdot);
/* Timing of the last rmx_group_step / rmx_group_step_async + rmx_group_sync: wall_ms = host wall clock from the first launch to
 * the last shard's completion; per shard (arrays [nshards], any may be NULL) kernel_ms = HIP-event time of its launch, start_ms /
 * end_ms = when its launch began / ended relative to the start of the FIRST shard on the same device (HIP events of one device
 * share a clock; 0 / kernel_ms for that first shard).  Shards run concurrently when start_ms of one lies before end_ms of another. */
int rmx_group_timing(rmx_group* g, double* wall_ms, double* kernel_ms, double* start_ms, double* end_ms);
/* Per-trajectory counters kept on the device across *_async calls (see "Asynchronous stepping" above). */
int rmx_stats_reset(rmx_batch* b);
int rmx_stats_read(rmx_batch* b, rmx_stats* stats);

#ifdef __cplusplus
}
#endif
#endif
