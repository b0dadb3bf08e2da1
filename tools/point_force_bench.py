"""What the body-to-body forces cost: rollout-steps per second and per-rollout shader-clock ticks (rmx_step_ticks) of
  chainsprings32  sceneChainSprings(32): the 32-link chain with a world-anchored spring-damper, a point-point force and a cable
  scene13         the reference's scene 13 'Cables'
  chain32_1pt     the same chain WITHOUT forces on the generic one-point step kernel (RMX_PAIRC=0): the kernel this change leaves
                  untouched, so the ratio to chainsprings32 is the price of the point stage plus the dense-order solve
at B rollouts x K BDF1 steps from synthetic states around each scene's own configuration.  Recorded, not gated: nothing pins these numbers.
Every case runs in a child process of its own under a time limit, one after the other; the first failure ends the run.
Usage: point_force_bench.py [B] [K] [--out FILE]      (child: point_force_bench.py --case NAME B K)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ("chainsprings32", "scene13", "chain32_1pt")


def run_case(name, B, K):
    if name == "chain32_1pt":
        os.environ["RMX_PAIRC"] = "0"
        os.environ["RMX_W2_MAX"] = "0"
    from redmax_amd import BatchSim, sceneChain, sceneChainSprings, scenesRedMax, syntheticStates
    sc = {"chainsprings32": lambda: sceneChainSprings(32), "scene13": lambda: scenesRedMax(13), "chain32_1pt": lambda: sceneChain(32)}[name]()
    sc.init()
    # states: the benchmark's synthetic ones at half their amplitude AROUND the scene's own configuration (where its springs and
    # cables are defined), rollout 0 the scene's own state - at the full amplitude the reference's own Newton (the numpy port of
    # tests/proto_point_forces.py) diverges on 3 of the 1024 states of the chain with springs, and so does the kernel, on the same three
    q, qd = syntheticStates(sc.nr, B, sq=0.05, sv=0.05)
    q0, qd0 = sc.getQ()
    q, qd = q0[None, :] + q, qd0[None, :] + qd
    q[0], qd[0] = q0, qd0
    sim = BatchSim(sc, batch=B)
    sim.set_state(q, qd)
    sim.step_bdf1(5, h=sc.h)                                 # warm-up: code objects loaded, every shape launched once
    qw, qdw = sim.get_state()
    best = None
    for _ in range(5):
        sim.set_state(qw, qdw)
        out = sim.step_bdf1(K, h=sc.h, stats=True)
        t = sim.step_ticks().astype(np.float64)
        if best is None or out["ms"] < best["kernel_ms"]:
            best = {"case": name, "kernel": sim.last_step_kernel(), "B": B, "K": K, "kernel_ms": out["ms"],
                    "rollout_steps_per_s": B * K / (out["ms"] * 1e-3),
                    "ticks_per_rollout": {"p50": float(np.percentile(t, 50)), "p99": float(np.percentile(t, 99)), "max": float(t.max())},
                    "newton_iters_per_step": float(out["newton_iters"].mean() / K),
                    "ls_halvings_per_step": float(out["ls_halvings"].mean() / K),
                    "status_counts": {str(int(s)): int((out["status"] == s).sum()) for s in np.unique(out["status"])},
                    "rollouts_not_converged": [int(i) for i in np.nonzero(out["status"] & 15)[0][:16]]}
    sim.close()
    print(json.dumps(best))


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--case":
        return run_case(argv[1], int(argv[2]), int(argv[3]))
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    B = int(argv[0]) if len(argv) > 0 else 1024
    K = int(argv[1]) if len(argv) > 1 else 20
    res = []
    for name in CASES:
        p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--case", name, str(B), str(K)],
                           capture_output=True, text=True)
        if p.returncode != 0:
            print("case %s failed (exit status %d); stopping\n%s" % (name, p.returncode, p.stderr[-2000:]), file=sys.stderr)
            return 1
        res.append(json.loads(p.stdout.strip().split("\n")[-1]))
        print(json.dumps(res[-1]), flush=True)
    by = {r["case"]: r for r in res}
    # the launch ends with its slowest rollout (a rollout whose Newton runs out its iterations holds it up); the median rollout is
    # what the point stage and the dense-order solve cost where the solver converges
    summary = {"chainsprings32_over_chain32_1pt_kernel_time": by["chainsprings32"]["kernel_ms"] / by["chain32_1pt"]["kernel_ms"],
               "chainsprings32_over_chain32_1pt_median_rollout_ticks": by["chainsprings32"]["ticks_per_rollout"]["p50"] / by["chain32_1pt"]["ticks_per_rollout"]["p50"]}
    print(json.dumps(summary))
    if out:
        with open(out, "w") as f:
            json.dump({"cases": res, "summary": summary}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
