"""What the differentiable rollout costs beside the adjoint it grew out of: BASELINE.json configs[3] (16-link chain, 512 rollouts,
20 steps, BDF1) through
  (a) rmx_adjoint_controls_device (forward + backward kernel in one call, the objective inside the library),
  (b) rmx_rollout_tape_device + rmx_rollout_vjp_device (the same two sweeps as two calls: no task code, the state of every step
      recorded, cotangents of every step read, dL/dq0 and dL/dqdot0 formed),
in one process, device pointers throughout, the two alternating; one rehearsal round, then the median of --reps rounds.  Per call
the host wall clock (the calls return when their kernels have finished) and the kernel time by the library's HIP events
(rmx_last_step_ms).  (a) is untouched by the work that added (b), so it stands for the parent commit.
Writes profiles/rollout_vjp_bench.json.
--integrator 2: the same under BDF2 (rmx_rollout_tape_bdf2_device: the SDIRK2a stage on the tape, one wavefront per rollout).
--integrator 1 2: BDF1 with its helper wave, BDF1 without (RMX_ADJ_HELP=0, what the BDF2 tape always runs) and BDF2 alternate in
one process, and the ratios BDF2 / BDF1 are formed; writes profiles/rollout_vjp_bench_bdf2.json.

--linearize: rmx_rollout_linearize_device (XA, XB, XU of every slot) beside the tape and vjp calls of the same run, BDF1, at
512 x 20 of the 16-link chain (the configs[3] shape), 512 x 20 of the 32-link chain and 256 x 20 of a 40-link chain; writes
profiles/rollout_linearize_bench.json.

--params: rmx_rollout_vjp_params_device (du, dq0, dqd0 and all five parameter gradients: the z-storing backward sweep and the
contraction over the slots, one kernel each) beside the tape and vjp calls of the same run, BDF1, at 512 x 20 of the 16-, 32- and
40-link chains; writes profiles/rollout_params_bench.json.

--jvp: rmx_rollout_jvp_device with 1 and with 8 tangent directions (tu, tq0 and tqd0 all given) beside the tape, vjp (the same number
of eliminations per direction-sweep) and linearize (the route the call replaces) calls of the same run, BDF1 and BDF2, at 1024 x 20 of
the 32-link chain; writes profiles/rollout_jvp_bench.json.

    python tools/rollout_vjp_bench.py [--reps 20] [--integrator 1 2] [--linearize] [--params] [--jvp]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B, K = 16, 512, 20


class Dev:
    """A device array through the HIP runtime the library is linked against."""
    hip = None

    def __init__(self, host):
        if Dev.hip is None:
            Dev.hip = C.CDLL("libamdhip64.so")
        self.host = np.ascontiguousarray(host, dtype=np.float64)
        self.p = C.c_void_p()
        assert Dev.hip.hipMalloc(C.byref(self.p), C.c_size_t(self.host.nbytes)) == 0
        assert Dev.hip.hipMemcpy(self.p, self.host.ctypes.data_as(C.c_void_p), C.c_size_t(self.host.nbytes), 1) == 0
        self.ptr = self.p.value

    def get(self):
        out = np.empty_like(self.host)
        assert Dev.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(out.nbytes), 2) == 0
        return out


LIN_SHAPES = ((16, 512, 20), (32, 512, 20), (40, 256, 20))      # (links, rollouts, steps)


def main_linearize(args):
    """tape, vjp and linearize alternate per shape; one rehearsal round, then the median of --reps rounds of the kernel time by the
    library's events (rmx_last_step_ms) and of the host wall clock."""
    sys.path.insert(0, ROOT)
    from redmax_amd import BatchSim
    from redmax_amd.scenes import sceneAdjointChain
    out = {"workload": "BDF1 tape of a serial chain; device pointers; XA, XB, XU all asked for; median of %d rounds after one rehearsal" % args.reps,
           "shapes": {}}
    rng = np.random.default_rng(20240)
    for n, b, k in LIN_SHAPES:
        sc = sceneAdjointChain(n)
        sc.init()
        nr = sc.nr
        q0, qd0 = sc.getQ()
        sim = BatchSim(sc, batch=b)
        u = 0.1 * rng.standard_normal((b, k, nr))
        ud, qt, qdt, dud = Dev(u), Dev(np.zeros_like(u)), Dev(np.zeros_like(u)), Dev(np.zeros_like(u))
        gq, gqd = Dev(rng.standard_normal(u.shape)), Dev(rng.standard_normal(u.shape))
        dq0, dqd0 = Dev(np.zeros((b, nr))), Dev(np.zeros((b, nr)))
        q0d, qd0d = Dev(np.repeat(q0[None], b, axis=0)), Dev(np.repeat(qd0[None], b, axis=0))
        X = [Dev(np.zeros((b, k, nr * nr))) for _ in range(3)]
        rows = {"rollout_tape": [], "rollout_vjp": [], "rollout_linearize": [], "rollout_linearize_XU_only": []}

        def timed(call, fn):
            t0 = time.perf_counter()
            fn()
            rows[call].append(((time.perf_counter() - t0) * 1e3, sim._L.rmx_last_step_ms(sim._batch)))

        for _ in range(1 + args.reps):
            sim.set_state_device(q0d.ptr, qd0d.ptr)
            timed("rollout_tape", lambda: sim.rollout_tape_device(k, sc.h, ud.ptr, qt.ptr, qdt.ptr, pscale=sc.task["pscale"]))
            timed("rollout_vjp", lambda: sim.rollout_vjp_device(k, gq.ptr, gqd.ptr, dud.ptr, dq0.ptr, dqd0.ptr))
            timed("rollout_linearize", lambda: sim.rollout_linearize_device(k, X[0].ptr, X[1].ptr, X[2].ptr))
            timed("rollout_linearize_XU_only", lambda: sim.rollout_linearize_device(k, None, None, X[2].ptr))
        finite = bool(all(np.isfinite(x.get()).all() for x in X))
        sim.close()
        for d in [ud, qt, qdt, dud, gq, gqd, dq0, dqd0, q0d, qd0d] + X:
            Dev.hip.hipFree(d.p)
        med = {c + "_device": {"wall_ms": float(np.median([r[0] for r in v[1:]])), "kernel_ms": float(np.median([r[1] for r in v[1:]]))}
               for c, v in rows.items()}
        med["linearize_over_tape_kernel"] = med["rollout_linearize_device"]["kernel_ms"] / med["rollout_tape_device"]["kernel_ms"]
        med["outputs_finite"] = finite
        out["shapes"]["%d-link chain, %d rollouts x %d steps" % (n, b, k)] = med
    path = args.out or os.path.join(ROOT, "profiles", "rollout_linearize_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


PARAM_SHAPES = ((16, 512, 20), (32, 512, 20), (40, 512, 20))      # (links, rollouts, steps)


def main_params(args):
    """tape, vjp and vjp_params alternate per shape; one rehearsal round, then the median of --reps rounds of the kernel time by the
    library's events (rmx_last_step_ms) and of the host wall clock."""
    sys.path.insert(0, ROOT)
    from redmax_amd import BatchSim
    from redmax_amd.scenes import sceneAdjointChain
    out = {"workload": "BDF1 tape of a serial chain; device pointers; vjp_params with all five outputs (and with the three joint "
                       "outputs alone); median of %d rounds after one rehearsal" % args.reps, "shapes": {}}
    rng = np.random.default_rng(20240)
    for n, b, k in PARAM_SHAPES:
        sc = sceneAdjointChain(n)
        sc.init()
        nr = sc.nr
        q0, qd0 = sc.getQ()
        sim = BatchSim(sc, batch=b)
        u = 0.1 * rng.standard_normal((b, k, nr))
        ud, qt, qdt, dud = Dev(u), Dev(np.zeros_like(u)), Dev(np.zeros_like(u)), Dev(np.zeros_like(u))
        gq, gqd = Dev(rng.standard_normal(u.shape)), Dev(rng.standard_normal(u.shape))
        dq0, dqd0 = Dev(np.zeros((b, nr))), Dev(np.zeros((b, nr)))
        q0d, qd0d = Dev(np.repeat(q0[None], b, axis=0)), Dev(np.repeat(qd0[None], b, axis=0))
        shapes = sim._param_shapes()
        G = {name: Dev(np.zeros((b,) + sh)) for name, sh in shapes.items()}
        rows = {"rollout_tape": [], "rollout_vjp": [], "rollout_vjp_params": [], "rollout_vjp_params_joints_only": []}

        def timed(call, fn):
            t0 = time.perf_counter()
            fn()
            rows[call].append(((time.perf_counter() - t0) * 1e3, sim._L.rmx_last_step_ms(sim._batch)))

        for _ in range(1 + args.reps):
            sim.set_state_device(q0d.ptr, qd0d.ptr)
            timed("rollout_tape", lambda: sim.rollout_tape_device(k, sc.h, ud.ptr, qt.ptr, qdt.ptr, pscale=sc.task["pscale"]))
            timed("rollout_vjp", lambda: sim.rollout_vjp_device(k, gq.ptr, gqd.ptr, dud.ptr, dq0.ptr, dqd0.ptr))
            timed("rollout_vjp_params", lambda: sim.rollout_vjp_params_device(k, gq.ptr, gqd.ptr, dud.ptr, dq0.ptr, dqd0.ptr,
                                                                              **{name + "_ptr": G[name].ptr for name in G}))
            timed("rollout_vjp_params_joints_only", lambda: sim.rollout_vjp_params_device(
                k, gq.ptr, gqd.ptr, dud.ptr, dq0.ptr, dqd0.ptr, stiffness_ptr=G["stiffness"].ptr, damping_ptr=G["damping"].ptr, qrest_ptr=G["qrest"].ptr))
        finite = bool(all(np.isfinite(g.get()).all() and np.abs(g.get()).max() > 0 for g in G.values()))
        sim.close()
        for d in [ud, qt, qdt, dud, gq, gqd, dq0, dqd0, q0d, qd0d] + list(G.values()):
            Dev.hip.hipFree(d.p)
        med = {c + "_device": {"wall_ms": float(np.median([r[0] for r in v[1:]])), "kernel_ms": float(np.median([r[1] for r in v[1:]]))}
               for c, v in rows.items()}
        kp = med["rollout_vjp_params_device"]["kernel_ms"]
        med["vjp_params_over_tape_kernel"] = kp / med["rollout_tape_device"]["kernel_ms"]
        med["vjp_params_over_vjp_kernel"] = kp / med["rollout_vjp_device"]["kernel_ms"]
        med["outputs_finite_and_nonzero"] = finite
        out["shapes"]["%d-link chain, %d rollouts x %d steps" % (n, b, k)] = med
    path = args.out or os.path.join(ROOT, "profiles", "rollout_params_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


JVP_SHAPE = (32, 1024, 20)      # (links, rollouts, steps)
JVP_NTAN = (1, 8)


def main_jvp(args):
    """tape, vjp, linearize and jvp (1 and 8 directions) alternate, under BDF1 and under BDF2; one rehearsal round, then the median of
    --reps rounds of the kernel time by the library's events (rmx_last_step_ms) and of the host wall clock."""
    sys.path.insert(0, ROOT)
    from redmax_amd import BatchSim
    from redmax_amd.scenes import sceneAdjointChain
    n, b, k = JVP_SHAPE
    out = {"workload": "%d-link chain, %d rollouts x %d steps; device pointers; jvp with tu, tq0 and tqd0 given, linearize with XA, XB, XU "
                       "asked for; median of %d rounds after one rehearsal" % (n, b, k, args.reps), "integrators": {}}
    rng = np.random.default_rng(20240)
    for integ in (1, 2):
        sc = sceneAdjointChain(n, bdf2=integ == 2)
        sc.init()
        nr = sc.nr
        q0, qd0 = sc.getQ()
        sim = BatchSim(sc, batch=b)
        u = 0.1 * rng.standard_normal((b, k, nr))
        ud, qt, qdt, dud = Dev(u), Dev(np.zeros_like(u)), Dev(np.zeros_like(u)), Dev(np.zeros_like(u))
        gq, gqd = Dev(rng.standard_normal(u.shape)), Dev(rng.standard_normal(u.shape))
        dq0, dqd0 = Dev(np.zeros((b, nr))), Dev(np.zeros((b, nr)))
        q0d, qd0d = Dev(np.repeat(q0[None], b, axis=0)), Dev(np.repeat(qd0[None], b, axis=0))
        nslots = k + (integ == 2)
        X = [Dev(np.zeros((b, nslots, nr * nr))) for _ in range(3)]
        T = {t: (Dev(rng.standard_normal((b, t, k, nr))), Dev(rng.standard_normal((b, t, nr))), Dev(rng.standard_normal((b, t, nr))),
                 Dev(np.zeros((b, t, k, nr))), Dev(np.zeros((b, t, k, nr)))) for t in JVP_NTAN}
        rows = dict({"rollout_tape": [], "rollout_vjp": [], "rollout_linearize": []}, **{"rollout_jvp_ntan%d" % t: [] for t in JVP_NTAN})

        def timed(call, fn):
            t0 = time.perf_counter()
            fn()
            rows[call].append(((time.perf_counter() - t0) * 1e3, sim._L.rmx_last_step_ms(sim._batch)))

        for _ in range(1 + args.reps):
            sim.set_state_device(q0d.ptr, qd0d.ptr)
            timed("rollout_tape", lambda: sim.rollout_tape_device(k, sc.h, ud.ptr, qt.ptr, qdt.ptr, pscale=sc.task["pscale"], integrator=integ))
            timed("rollout_vjp", lambda: sim.rollout_vjp_device(k, gq.ptr, gqd.ptr, dud.ptr, dq0.ptr, dqd0.ptr))
            timed("rollout_linearize", lambda: sim.rollout_linearize_device(k, X[0].ptr, X[1].ptr, X[2].ptr))
            for t in JVP_NTAN:
                tu, tq0, tqd0, tq, tqd = T[t]
                timed("rollout_jvp_ntan%d" % t, lambda: sim.rollout_jvp_device(k, t, tu.ptr, tq0.ptr, tqd0.ptr, tq.ptr, tqd.ptr))
        finite = bool(all(np.isfinite(T[t][i].get()).all() and np.abs(T[t][i].get()).max() > 0 for t in JVP_NTAN for i in (3, 4)))
        sim.close()
        for d in [ud, qt, qdt, dud, gq, gqd, dq0, dqd0, q0d, qd0d] + X + [x for t in JVP_NTAN for x in T[t]]:
            Dev.hip.hipFree(d.p)
        med = {c + "_device": {"wall_ms": float(np.median([r[0] for r in v[1:]])), "kernel_ms": float(np.median([r[1] for r in v[1:]]))}
               for c, v in rows.items()}
        for t in JVP_NTAN:
            kj = med["rollout_jvp_ntan%d_device" % t]["kernel_ms"]
            med["jvp_ntan%d_over_vjp_kernel" % t] = kj / med["rollout_vjp_device"]["kernel_ms"]
            med["jvp_ntan%d_over_linearize_kernel" % t] = kj / med["rollout_linearize_device"]["kernel_ms"]
        med["outputs_finite_and_nonzero"] = finite
        out["integrators"]["BDF%d" % integ] = med
    path = args.out or os.path.join(ROOT, "profiles", "rollout_jvp_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--integrator", type=int, nargs="+", choices=(1, 2), default=[1],
                    help="1 BDF1, 2 BDF2; both: they alternate in one process and the ratios BDF2 / BDF1 are formed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--linearize", action="store_true", help="time rmx_rollout_linearize_device beside tape and vjp at three shapes")
    ap.add_argument("--params", action="store_true", help="time rmx_rollout_vjp_params_device beside tape and vjp at three shapes")
    ap.add_argument("--jvp", action="store_true", help="time rmx_rollout_jvp_device (1 and 8 directions) beside tape, vjp and linearize")
    args = ap.parse_args()
    if args.jvp:
        return main_jvp(args)
    if args.linearize:
        return main_linearize(args)
    if args.params:
        return main_params(args)
    integs = sorted(set(args.integrator))
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "rollout_vjp_bench.json" if integs == [1] else "rollout_vjp_bench_bdf2.json")
    sys.path.insert(0, ROOT)
    from redmax_amd import BatchSim
    from redmax_amd.scenes import sceneAdjointChain
    # the variants that alternate: (name, integrator, RMX_ADJ_HELP).  With both integrators BDF1 also runs without its helper wave
    # (the knob is read at every call): the BDF2 tape never has one, so that is the like-for-like pair
    # (helper None: RMX_ADJ_HELP is left as the caller set it - the single-integrator runs, and BDF2, which the knob does not reach)
    variants = [("bdf%d" % i, i, None) for i in integs]
    if integs == [1, 2]:
        variants = [("bdf1", 1, "1"), ("bdf1_one_wave", 1, "0"), ("bdf2", 2, None)]
    caller_help = os.environ.get("RMX_ADJ_HELP")
    rng = np.random.default_rng(20240)
    scenes = {}
    for i in integs:
        scenes[i] = sceneAdjointChain(N, bdf2=i == 2)
        scenes[i].init()
    nr = scenes[integs[0]].nr
    u = 0.1 * rng.standard_normal((B, K, nr))
    ud, Pd, dPdud = Dev(u), Dev(np.zeros(B)), Dev(np.zeros_like(u))
    qt, qdt, dud = Dev(np.zeros_like(u)), Dev(np.zeros_like(u)), Dev(np.zeros_like(u))
    gq, gqd = Dev(rng.standard_normal(u.shape)), Dev(rng.standard_normal(u.shape))
    dq0, dqd0 = Dev(np.zeros((B, nr))), Dev(np.zeros((B, nr)))
    sims, starts, rows, checks = {}, {}, {}, {}
    for name, i, _ in variants:
        sc = scenes[i]
        if i not in sims:
            q0, qd0 = sc.getQ()
            sims[i] = BatchSim(sc, batch=B)
            starts[i] = (Dev(np.repeat(q0[None], B, axis=0)), Dev(np.repeat(qd0[None], B, axis=0)))
        rows[name] = {"adjoint_controls": [], "rollout_tape": [], "rollout_vjp": []}

    def timed(name, call, sim, fn):
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        rows[name][call].append((wall, sim._L.rmx_last_step_ms(sim._batch)))

    for rep in range(1 + args.reps):                   # (round 0: the rehearsal)
        for name, i, helper in variants:
            if helper is not None:
                os.environ["RMX_ADJ_HELP"] = helper
            elif caller_help is None:
                os.environ.pop("RMX_ADJ_HELP", None)
            else:
                os.environ["RMX_ADJ_HELP"] = caller_help
            sim, sc, (q0d, qd0d) = sims[i], scenes[i], starts[i]
            task = dict(sc.task, step=K)
            sim.set_state_device(q0d.ptr, qd0d.ptr)
            timed(name, "adjoint_controls", sim, lambda: sim.adjoint_controls_device(K, sc.h, task, ud.ptr, Pd.ptr, dPdud.ptr, integrator=i))
            qa = sim.get_state()[0]
            sim.set_state_device(q0d.ptr, qd0d.ptr)
            timed(name, "rollout_tape", sim,
                  lambda: sim.rollout_tape_device(K, sc.h, ud.ptr, qt.ptr, qdt.ptr, pscale=task["pscale"], integrator=i))
            timed(name, "rollout_vjp", sim, lambda: sim.rollout_vjp_device(K, gq.ptr, gqd.ptr, dud.ptr, dq0.ptr, dqd0.ptr))
            qb = sim.get_state()[0]
            checks[name] = {"same_final_state": bool(np.array_equal(qa, qb) and np.array_equal(qt.get()[:, -1], qb)),
                            "final_state_rel_diff": float(np.linalg.norm(qa - qb) / np.linalg.norm(qa)),
                            "gradients_finite": bool(np.isfinite(dud.get()).all() and np.isfinite(dq0.get()).all()
                                                     and np.isfinite(dqd0.get()).all())}
    if caller_help is None:
        os.environ.pop("RMX_ADJ_HELP", None)
    else:
        os.environ["RMX_ADJ_HELP"] = caller_help
    for sim in sims.values():
        sim.close()

    def summary(name, i, helper):
        med = {k: {"wall_ms": float(np.median([r[0] for r in v[1:]])), "kernel_ms": float(np.median([r[1] for r in v[1:]])),
                   "wall_min_ms": float(min(r[0] for r in v[1:])), "wall_max_ms": float(max(r[0] for r in v[1:]))}
               for k, v in rows[name].items()}
        pair = {k: med["rollout_tape"][k] + med["rollout_vjp"][k] for k in ("wall_ms", "kernel_ms")}
        return dict({"integrator": i, "RMX_ADJ_HELP": None if helper is None else int(helper),
                     "adjoint_controls_device": med["adjoint_controls"], "rollout_tape_device": med["rollout_tape"],
                     "rollout_vjp_device": med["rollout_vjp"], "tape_plus_vjp": pair,
                     "tape_plus_vjp_over_adjoint_controls": {k: pair[k] / med["adjoint_controls"][k] for k in pair}}, **checks[name])

    res = {name: summary(name, i, helper) for name, i, helper in variants}
    workload = ("configs[3]: %d-link chain, %d rollouts, %d steps, %s; device pointers; median of %d rounds after one rehearsal"
                % (N, B, K, " / ".join("BDF%d" % i for i in integs), args.reps))
    if len(variants) == 1:
        out = dict({"workload": workload}, **{k: v for k, v in res[variants[0][0]].items() if k not in ("integrator", "RMX_ADJ_HELP", "final_state_rel_diff")})
    else:
        out = dict({"workload": workload + "; the variants alternate within every round"}, **res)
        if integs == [1, 2]:
            for base in ("bdf1", "bdf1_one_wave"):
                out["bdf2_over_" + base] = {call: {k: res["bdf2"][call][k] / res[base][call][k] for k in ("wall_ms", "kernel_ms")}
                                            for call in ("rollout_tape_device", "rollout_vjp_device", "tape_plus_vjp")}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
