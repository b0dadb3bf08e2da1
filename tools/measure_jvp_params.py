"""Time of rmx_rollout_jvp_params beside rmx_rollout_jvp on the same tape, and beside what central differences of the same
directions cost without it: the figures of profiles/jvp_params.txt.  A record, not a gate.

    python tools/measure_jvp_params.py [--n 32] [--batch 512] [--steps 100] [--ntan 8] [--repeats 7] [--out FILE]

The scene is the n-link chain of the taped-rollout tests (tests/test_gpu_adjoint_controls.py _scene) from its own initial state under
the random torques of tests/test_rollout_vjp_proto.py case(), BDF1.  After one tape call the two readers alternate on that tape with the same number of directions: rmx_rollout_jvp
(tu, tq0, tqd0: the sweep alone, the yardstick) and rmx_rollout_jvp_params (all five parameter groups: k_rollout_param_rhs and the
sweep that subtracts its term).  Kernel time: rmx_last_step_ms, device events around the launches of the
call; call time: the host clock around the host form, staging copies included.  Two untimed rounds, then the median, minimum and
maximum of --repeats rounds.  Central differences of ntan parameter directions need 2 ntan rollouts on perturbed MODELS: a BatchSim
rebuilt from the perturbed scene and one rollout_tape each - their wall time is measured once, sims built and closed inside it.
The number of rollouts whose tape call failed a Newton solve is printed.  The readers' work does not depend on it; the rollout_tape
runs of the central differences do: where the solves fail (the tape's Newton has no line search, and over 100 steps of this chain
under these torques they do) those runs go to the iteration limit, and their time is an upper figure.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--ntan", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import proto_rollout_jvp as pj
    import proto_rollout_jvp_params as pjp
    import proto_rollout_params as pp
    from redmax_amd import BatchSim
    from test_gpu_adjoint_controls import _scene
    from test_rollout_vjp_proto import case
    B, N, T, REP = args.batch, args.steps, args.ntan, args.repeats
    sc = _scene(args.n, 1)
    cs = case(sc, 17, nsteps=N, B=B)
    # every rollout from the scene's own state, under case()'s torques
    q0, qd0 = sc.getQ()
    cs["q0"], cs["qd0"] = np.repeat(q0[None], B, axis=0), np.repeat(qd0[None], B, axis=0)
    pscale = sc.task["pscale"]
    sim = BatchSim(sc, batch=B)
    idx = sim.idxR()
    d = sc.desc()
    vals = {g: np.zeros(sc.nr) for g in pp.GROUPS[:3]}
    for j, r in enumerate(idx):
        if r >= 0:
            for g in pp.GROUPS[:3]:
                vals[g][r] = np.asarray(d[pp.DESC_KEY[g]], dtype=np.float64)[j]
    vals["inertia"] = np.array(d["I_i"], dtype=np.float64).reshape(-1, 6)
    vals["grav"] = np.array(d["grav"], dtype=np.float64).reshape(3)
    t = pj.tangents(53, B, T, N, sc.nr)
    tp = pjp.directions(vals, 71, (B, T))
    tp["inertia"][..., 4:] = tp["inertia"][..., 3:4]      # (a physical mass direction: the model takes one mass per body)
    sim.set_state(cs["q0"], cs["qd0"])
    _, _, info = sim.rollout_tape(N, sc.h, cs["u"], pscale=pscale, stats=True)
    failed = int(((info["status"] & 7) != 0).sum())
    calls = (("rmx_rollout_jvp", lambda: sim.rollout_jvp(N, t["tu"], t["tq0"], t["tqd0"])),
             ("rmx_rollout_jvp_params", lambda: sim.rollout_jvp_params(N, tp)),
             ("rmx_rollout_jvp_params + tu, tq0, tqd0", lambda: sim.rollout_jvp_params(N, tp, t["tu"], t["tq0"], t["tqd0"])))
    ms = {k: [] for k, _ in calls}
    wall = {k: [] for k, _ in calls}
    for rep in range(REP + 2):
        for name, call in calls:
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            if rep >= 2:
                ms[name].append(sim._L.rmx_last_step_ms(sim._batch))
                wall[name].append(1e3 * (t1 - t0))
    sim.close()
    lines = ["readers of the BDF1 tape of the %d-link chain, %d rollouts, %d steps of h = %g, %d directions; median [min .. max] of %d calls" % (
        args.n, B, N, sc.h, T, REP)]
    for name, _ in calls:
        lines.append("%-42s kernel %8.3f ms [%8.3f .. %8.3f]   call %8.3f ms [%8.3f .. %8.3f]" % (
            name, np.median(ms[name]), min(ms[name]), max(ms[name]), np.median(wall[name]), min(wall[name]), max(wall[name])))
    base = np.median(ms["rmx_rollout_jvp"])
    lines.append("tape call: %.3f ms, %d rollouts failed a solve; kernel time over rmx_rollout_jvp's: parameters alone %.2f, with tu, tq0, tqd0 %.2f" % (
        info["ms"], failed, np.median(ms["rmx_rollout_jvp_params"]) / base, np.median(ms["rmx_rollout_jvp_params + tu, tq0, tqd0"]) / base))
    # what central differences of T parameter directions cost today: 2 T rollouts, each on a sim rebuilt from a perturbed scene
    group = {0: "stiffness", 1: "damping", 2: "qrest", 3: "inertia", 4: "grav"}
    kernel = []
    t0 = time.perf_counter()
    for k in range(T):
        g = group[k % 5]
        for sgn in (1.0, -1.0):
            fd = BatchSim(pp.perturbed(None, sc, g, sgn * 1e-5 * tp[g][0, k], idx), batch=B)
            fd.set_state(cs["q0"], cs["qd0"])
            kernel.append(fd.rollout_tape(N, sc.h, cs["u"], pscale=pscale, stats=True)[2]["ms"])
            fd.close()
    t1 = time.perf_counter()
    lines.append("central differences of %d parameter directions: %d rollout_tape runs on rebuilt sims, wall %.1f ms in all (their kernels %.1f ms)" % (
        T, 2 * T, 1e3 * (t1 - t0), sum(kernel)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
