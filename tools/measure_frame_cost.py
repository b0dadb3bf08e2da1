"""Kernel time of the cost model with frame targets (label k_rollout_frames) next to the point-target instantiation (k_rollout_cost) on
the same record: the figures of profiles/frame_cost.txt.

    python tools/measure_frame_cost.py [--links 32] [--batch 1024] [--steps 100] [--repeats 9] [--out FILE]

The record is sceneAdjointChain(links)'s initial state plus noise per step (the kernels read any record; no rollout is run), the
joint-space cost that of tools/measure_point_cost.py, and every step owns one term on the tip:
  (a) diff.cost_model with wpos, wvel and wrot on the term (rmx_rollout_cost_frames_device), every output;
  (b) the same with wpos and wrot (no velocity front, no cross blocks);
  (c) diff.cost_model with the same terms position-only (rmx_rollout_cost_device: k_rollout_cost), every output;
  (d) (a) and (c) with the value alone.
Kernel times as the library reports them (rmx_last_step_ms: events around the launch on the batch's stream): the median, minimum
and maximum of --repeats launches after two untimed ones, (a) and (c) in alternation so that both see the same clocks.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from redmax_amd import BatchSim, diff
    from redmax_amd.scenes import sceneAdjointChain
    B, N, REP = args.batch, args.steps, args.repeats
    dev = torch.device("cuda", 0)
    sc = sceneAdjointChain(args.links)
    sc.init()
    nr = sc.nr
    q0s, qd0s = sc.getQ()
    rng = np.random.default_rng(3)
    qt = torch.tensor(q0s[None, None] + 0.05 * rng.standard_normal((B, N, nr)), dtype=torch.float64, device=dev)
    qdt = torch.tensor(qd0s[None, None] + 0.2 * rng.standard_normal((B, N, nr)), dtype=torch.float64, device=dev)
    Q = torch.diag(torch.tensor([1.0] * nr + [0.01] * nr, dtype=torch.float64, device=dev)).repeat(N, 1, 1)
    xg = torch.tensor(np.concatenate([q0s - 0.1, np.zeros(nr)]), dtype=torch.float64, device=dev).repeat(N, 1)
    full = [dict(body=nr - 1, xlocal=[5.0, 0.0, 0.0], step=k, wpos=0.05, wvel=0.01, wrot=0.5) for k in range(1, N + 1)]
    norot = [dict(t, wvel=0.0) for t in full]
    pos = [dict(body=t["body"], xlocal=t["xlocal"], step=t["step"], wpos=t["wpos"]) for t in full]
    xt = torch.tensor(sc.task["xtarget"], dtype=torch.float64, device=dev).repeat(N, 1)
    vt = torch.zeros((N, 3), dtype=torch.float64, device=dev)
    Rt = torch.eye(3, dtype=torch.float64, device=dev).repeat(N, 1, 1)
    sim = BatchSim(sc, batch=B)
    ms = lambda: sim._L.rmx_last_step_ms(sim._batch)      # noqa: E731
    calls = {
        "a": lambda: diff.cost_model(sim, qt, qdt, Q=Q, xgoal=xg, terms=full, xtarget=xt, vtarget=vt, Rtarget=Rt),
        "b": lambda: diff.cost_model(sim, qt, qdt, Q=Q, xgoal=xg, terms=norot, xtarget=xt, Rtarget=Rt),
        "c": lambda: diff.cost_model(sim, qt, qdt, Q=Q, xgoal=xg, terms=pos, xtarget=xt),
        "da": lambda: diff.cost_model(sim, qt, qdt, Q=Q, xgoal=xg, terms=full, xtarget=xt, vtarget=vt, Rtarget=Rt, want=("J",)),
        "dc": lambda: diff.cost_model(sim, qt, qdt, Q=Q, xgoal=xg, terms=pos, xtarget=xt, want=("J",)),
    }
    labels = {}
    v = {k: [] for k in calls}
    for _ in range(REP + 2):      # two untimed rounds first; the calls in alternation
        for k, fn in calls.items():
            torch.cuda.synchronize()
            fn()
            v[k].append(ms())
            labels[k] = sim.last_step_kernel()
    sim.close()
    t = {k: (float(np.median(a[2:])), float(np.min(a[2:])), float(np.max(a[2:]))) for k, a in v.items()}
    d2 = 2 * nr
    moved = B * N * 8 * (d2 * d2 + 2 * nr + d2 + 1)      # Q out, q and qdot in, lx and Jk out (the shared Q and goal come from cache)
    lines = ["%d-link chain, %d rollouts, %d steps, one term on the tip per step; kernel times (rmx_last_step_ms), median (min, max) of %d "
             "launches, the calls in alternation:" % (args.links, B, N, REP),
             "  (a) %-16s wpos + wvel + wrot, Jk + lx + Q   %9.3f ms  (%.3f, %.3f)   %.0f MB to move: %.0f GB/s"
             % ((labels["a"],) + t["a"] + (moved / 1e6, moved / t["a"][0] / 1e6)),
             "  (b) %-16s wpos + wrot, Jk + lx + Q          %9.3f ms  (%.3f, %.3f)" % ((labels["b"],) + t["b"]),
             "  (c) %-16s wpos alone, Jk + lx + Q           %9.3f ms  (%.3f, %.3f)   (a) / (c) = %.3f   %.0f GB/s"
             % ((labels["c"],) + t["c"] + (t["a"][0] / t["c"][0], moved / t["c"][0] / 1e6)),
             "  (d) the value alone: %s %.3f ms (%.3f, %.3f), %s %.3f ms (%.3f, %.3f)" % ((labels["da"],) + t["da"] + (labels["dc"],) + t["dc"])]
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
