"""Time of rmx_rollout_tape on a tree with body-to-body forces (the switch of rmx_model_tape_point_forces on) beside the same
tree without its force table: the figures of profiles/tape_pf.txt.  A record, not a gate.

    python tools/measure_tape_pf.py [--n 32] [--batch 512] [--steps 100 50 20] [--repeats 7] [--out FILE]

The scene is tests/proto_point_forces.sizedSceneWithForces(n) - a point-point force, two spring-dampers and a four-point cable on
sceneTree(n) - from nearInitialStates, under zero control torques; the second model is the same scene with `forces` emptied.  Both
integrators.  A call is timed twice: the library's kernel time (rmx_last_step_ms: device events around the launch) and the host
clock around the call, which ends in a device synchronise and includes the staging copies; after two untimed calls of each model,
the two models alternate, and the median, the minimum and the maximum of --repeats calls are printed.  Newton iterations per step
and the status words go with them: a rollout whose status has one of the bits 1, 2, 4 set failed a solve, and the exit status is 2.
The taped sweeps run the Newton iteration WITHOUT a line search (as every rmx_rollout_tape does): on this scene, whose cable goes
slack and taut along the way, a share of the random states ends a solve at the iteration limit somewhere in 100 steps - the
proto of tests/proto_rollout_pf.py does the same from the same states -, and one wavefront integrates one rollout, so the kernel time of a
long horizon is that of the rollouts that ran into the limit (10 nr iterations in one solve); shorter horizons are listed beside it.
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
    ap.add_argument("--steps", type=int, nargs="+", default=[100, 50, 20])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import proto_point_forces as ppf
    from redmax_amd import BatchSim
    B, REP = args.batch, args.repeats
    sc = ppf.sizedSceneWithForces(args.n)
    q0, qd0 = ppf.nearInitialStates(sc, args.n + 100, B)[:2]
    plain = ppf.sizedSceneWithForces(args.n)
    plain.forces = []
    plain.init()
    sims = {"forces": BatchSim(sc, batch=B, tape_forces=True), "plain": BatchSim(plain, batch=B)}
    lines, bad = [], 0
    for N, integ in [(N, integ) for N in args.steps for integ in (1, 2)]:
        u = np.zeros((B, N, sc.nr))
        if integ == 1:
            lines.append("rmx_rollout_tape: sizedSceneWithForces(%d), %d rollouts, %d steps of h = %g; median [min .. max] of %d calls" % (
                args.n, B, N, sc.h, REP))
        ms = {k: [] for k in sims}
        wall = {k: [] for k in sims}
        info = {}
        for rep in range(REP + 2):
            for name, sim in sims.items():
                sim.set_state(q0, qd0)
                t0 = time.perf_counter()
                _, _, info[name] = sim.rollout_tape(N, sc.h, u, stats=True, integrator=integ)
                t1 = time.perf_counter()
                if rep >= 2:
                    ms[name].append(info[name]["ms"])
                    wall[name].append(1e3 * (t1 - t0))
        for name, sim in sims.items():
            st, it = info[name]["status"], info[name]["newton_iters"]
            failed = int(((st & 7) != 0).sum())
            bad += failed
            # (rmx_last_step_kernel: the BDF1 tape of a model without forces reports no label of its own)
            label = sim.last_step_kernel() if (name == "forces" or integ == 2) else "k_adjoint_fwd, BDF1 tape"
            lines.append("BDF%d %-6s %-40s kernel %8.3f ms [%8.3f .. %8.3f]   call %8.3f ms [%8.3f .. %8.3f]   %.2f iterations/step, "
                         "%d rollouts pivoted, %d failed (diverged %d, iteration limit %d, NaN %d)" % (
                             integ, name, label, np.median(ms[name]), min(ms[name]), max(ms[name]), np.median(wall[name]), min(wall[name]),
                             max(wall[name]), it.mean() / N, int(((st & 16) != 0).sum()), failed, int(((st & 1) != 0).sum()),
                             int(((st & 2) != 0).sum()), int(((st & 4) != 0).sum())))
        lines.append("BDF%d kernel time with forces / without: %.2f" % (integ, np.median(ms["forces"]) / np.median(ms["plain"])))
    for sim in sims.values():
        sim.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 2 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
