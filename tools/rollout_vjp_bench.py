"""What the differentiable rollout costs beside the adjoint it grew out of: BASELINE.json configs[3] (16-link chain, 512 rollouts,
20 steps, BDF1) through
  (a) rmx_adjoint_controls_device (forward + backward kernel in one call, the objective inside the library),
  (b) rmx_rollout_tape_device + rmx_rollout_vjp_device (the same two sweeps as two calls: no task code, the state of every step
      recorded, cotangents of every step read, dL/dq0 and dL/dqdot0 formed),
in one process, device pointers throughout, the two alternating; one rehearsal round, then the median of --reps rounds.  Per call
the host wall clock (the calls return when their kernels have finished) and the kernel time by the library's HIP events
(rmx_last_step_ms).  (a) is untouched by the work that added (b), so it stands for the parent commit.
Writes profiles/rollout_vjp_bench.json.

    python tools/rollout_vjp_bench.py [--reps 20]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_vjp_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from redmax_amd import BatchSim
    from redmax_amd.scenes import sceneAdjointChain
    sc = sceneAdjointChain(N)
    sc.init()
    rng = np.random.default_rng(20240)
    u = 0.1 * rng.standard_normal((B, K, sc.nr))
    task = dict(sc.task, step=K)
    q0, qd0 = sc.getQ()
    q0d, qd0d = Dev(np.repeat(q0[None], B, axis=0)), Dev(np.repeat(qd0[None], B, axis=0))
    ud, Pd, dPdud = Dev(u), Dev(np.zeros(B)), Dev(np.zeros_like(u))
    qt, qdt, dud = Dev(np.zeros_like(u)), Dev(np.zeros_like(u)), Dev(np.zeros_like(u))
    gq, gqd = Dev(rng.standard_normal(u.shape)), Dev(rng.standard_normal(u.shape))
    dq0, dqd0 = Dev(np.zeros((B, sc.nr))), Dev(np.zeros((B, sc.nr)))
    sim = BatchSim(sc, batch=B)
    rows = {"adjoint_controls": [], "rollout_tape": [], "rollout_vjp": []}

    def timed(name, fn):
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        rows[name].append((wall, sim._L.rmx_last_step_ms(sim._batch)))

    for rep in range(1 + args.reps):                   # (round 0: the rehearsal)
        sim.set_state_device(q0d.ptr, qd0d.ptr)
        timed("adjoint_controls", lambda: sim.adjoint_controls_device(K, sc.h, task, ud.ptr, Pd.ptr, dPdud.ptr))
        qa = sim.get_state()[0]
        sim.set_state_device(q0d.ptr, qd0d.ptr)
        timed("rollout_tape", lambda: sim.rollout_tape_device(K, sc.h, ud.ptr, qt.ptr, qdt.ptr, pscale=task["pscale"]))
        timed("rollout_vjp", lambda: sim.rollout_vjp_device(K, gq.ptr, gqd.ptr, dud.ptr, dq0.ptr, dqd0.ptr))
        qb = sim.get_state()[0]
    same = bool(np.array_equal(qa, qb) and np.array_equal(qt.get()[:, -1], qb))
    finite = bool(np.isfinite(dud.get()).all() and np.isfinite(dq0.get()).all() and np.isfinite(dqd0.get()).all())
    sim.close()
    med = {k: {"wall_ms": float(np.median([r[0] for r in v[1:]])), "kernel_ms": float(np.median([r[1] for r in v[1:]])),
               "wall_min_ms": float(min(r[0] for r in v[1:])), "wall_max_ms": float(max(r[0] for r in v[1:]))} for k, v in rows.items()}
    pair = {k: med["rollout_tape"][k] + med["rollout_vjp"][k] for k in ("wall_ms", "kernel_ms")}
    out = {"workload": "configs[3]: %d-link chain, %d rollouts, %d steps, BDF1; device pointers; median of %d rounds after one rehearsal"
                       % (N, B, K, args.reps),
           "adjoint_controls_device": med["adjoint_controls"], "rollout_tape_device": med["rollout_tape"],
           "rollout_vjp_device": med["rollout_vjp"], "tape_plus_vjp": pair,
           "tape_plus_vjp_over_adjoint_controls": {k: pair[k] / med["adjoint_controls"][k] for k in pair},
           "same_final_state": same, "gradients_finite": finite}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
