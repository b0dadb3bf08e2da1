"""Time of rmx_rollout_vjp_forces beside rmx_rollout_vjp on the same tape of a tree with body-to-body forces: the figures of
profiles/force_params.txt.  A record, not a gate.

    python tools/measure_force_params.py [--n 32] [--batch 512] [--steps 100 20] [--repeats 7] [--out FILE]

The scene and the states are those of tools/measure_tape_pf.py (tests/proto_point_forces.sizedSceneWithForces(n) from
nearInitialStates, zero control torques, BDF1 and BDF2).  After one tape call the readers alternate on that tape: rmx_rollout_vjp (the
backward sweep alone: the yardstick), rmx_rollout_vjp_forces with the three force arrays (the z-storing backward sweep and
k_rollout_force_grad) and with the five model arrays too (plus k_rollout_param_grad).  Kernel time: rmx_last_step_ms, device events
around the launches of the call; call time: the host clock around the host form, staging copies included.  Two untimed rounds, then
the median, minimum and maximum of --repeats rounds.  The work of the readers does not depend on how the forward Newton fared: a
rollout that failed a solve in the tape call (their number is printed) costs what every other costs.
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
    ap.add_argument("--steps", type=int, nargs="+", default=[100, 20])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import proto_point_forces as ppf
    from redmax_amd import BatchSim, _abi
    B, REP = args.batch, args.repeats
    sc = ppf.sizedSceneWithForces(args.n)
    q0, qd0 = ppf.nearInitialStates(sc, args.n + 100, B)[:2]
    sim = BatchSim(sc, batch=B, tape_forces=True)
    rng = np.random.default_rng(7)
    lines = []
    for N, integ in [(N, integ) for N in args.steps for integ in (1, 2)]:
        u = np.zeros((B, N, sc.nr))
        gq, gqd = rng.standard_normal(u.shape), rng.standard_normal(u.shape)
        sim.set_state(q0, qd0)
        _, _, info = sim.rollout_tape(N, sc.h, u, stats=True, integrator=integ)
        failed = int(((info["status"] & 7) != 0).sum())
        if integ == 1:
            lines.append("readers of the tape of sizedSceneWithForces(%d), %d rollouts, %d steps of h = %g; median [min .. max] of %d calls" % (
                args.n, B, N, sc.h, REP))
        calls = (("rmx_rollout_vjp", lambda: sim.rollout_vjp(N, gq, gqd)),
                 ("rmx_rollout_vjp_forces, forces", lambda: sim.rollout_vjp_forces(N, gq, gqd)),
                 ("rmx_rollout_vjp_forces, forces + model", lambda: sim.rollout_vjp_forces(N, gq, gqd, model=_abi.PARAM_NAMES)))
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
        for name, _ in calls:
            lines.append("BDF%d %-40s kernel %8.3f ms [%8.3f .. %8.3f]   call %8.3f ms [%8.3f .. %8.3f]" % (
                integ, name, np.median(ms[name]), min(ms[name]), max(ms[name]), np.median(wall[name]), min(wall[name]), max(wall[name])))
        base = np.median(ms["rmx_rollout_vjp"])
        lines.append("BDF%d tape call: %.3f ms, %d rollouts failed a solve; kernel time over rmx_rollout_vjp's: forces %.2f, forces + model %.2f" % (
            integ, info["ms"], failed, np.median(ms["rmx_rollout_vjp_forces, forces"]) / base,
            np.median(ms["rmx_rollout_vjp_forces, forces + model"]) / base))
    sim.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
