"""Time of the forward part of one iLQR iteration - the line search -, the two ways ilqr.solve can run it, on the same nominal and
gains: the figures of profiles/ilqr_search.txt and of DESIGN.md.

    python tools/measure_ilqr_search.py [--links 32] [--batch 512] [--steps 20 100] [--h-div 5] [--repeats 9] [--scale S] [--out FILE]

  (a) search="host":   the loop of solve as it stands - per alpha one diff.rollout_feedback launch on the whole batch, cost.value in
      torch, bool(accepted.all()) on the host, and one more launch where the last one still held a rejected candidate;
  (b) search="device": one diff.rollout_search (rmx_rollout_search_device).

Both are timed with torch.cuda events around the call(s) on a synchronised device - wall time on the device's clock, launch gaps and
the host work of the Python loop included, which is what an iteration pays -, after two untimed calls each, in ALTERNATING repeats
(a, b, a, b, ..), and reported as the median with the spread (min, max) of --repeats; for (b) the library's own kernel time
(rmx_last_step_ms) is printed next to it.  The scene is sceneAdjointChain(links) at the scene's step size divided by --h-div (see
tools/measure_vjp_feedback.py), the cost that of tests/test_gpu_ilqr.py, the gains those of diff.lqr_backward on the nominal's tape.
Printed with the times: the share of rollouts per accepted alpha, of either path, and how many rollouts the two paths decide
differently.  --scale S searches along S * kff in the place of kff (both paths alike): with S > 2 the full step overshoots and the
first alphas are refused - the case in which the host loop pays one full-batch launch per alpha.  The exit status is 2 when a
rollout of the nominal reports a failed Newton solve: then the figures are not ones to quote.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ALPHAS = (1.0, 0.5, 0.25, 0.125, 0.0625)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=32)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--h-div", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--mu", type=float, default=1e-6)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from redmax_amd import BatchSim, diff, ilqr
    from redmax_amd.scenes import sceneAdjointChain
    B, REP = args.batch, args.repeats
    dev = torch.device("cuda", 0)
    lines, bad_total = [], 0
    sc = sceneAdjointChain(args.links)
    sc.init()
    nr, h, ps = sc.nr, sc.h / args.h_div, sc.task["pscale"]
    q0s, qd0s = sc.getQ()

    def once(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for N in args.steps:
        rng = np.random.default_rng(3)
        q0 = torch.tensor(q0s[None] + 0.05 * rng.standard_normal((B, nr)), dtype=torch.float64, device=dev)
        qd0 = torch.tensor(qd0s[None] + 0.2 * rng.standard_normal((B, nr)), dtype=torch.float64, device=dev)
        u = torch.tensor(0.1 * rng.standard_normal((B, N, nr)), dtype=torch.float64, device=dev)
        Q = torch.diag(torch.tensor([1.0] * nr + [0.01] * nr, dtype=torch.float64, device=dev)).repeat(N, 1, 1)
        R = 0.1 * torch.eye(nr, dtype=torch.float64, device=dev)
        xg = torch.tensor(np.concatenate([q0s - 0.1, np.zeros(nr)]), dtype=torch.float64, device=dev).repeat(1, N, 1)
        cost = ilqr.QuadraticCost(Q, R, xg)
        sim = BatchSim(sc, batch=B)
        # the nominal and its gains, as solve(search="device") forms them
        qt, qdt, ubar, Jbar, _, st = diff.rollout_search(sim, q0, qd0, u, None, None, None, (), None, cost=cost, h=h, pscale=ps)
        nom_ms = sim._L.rmx_last_step_ms(sim._batch)
        bad = int(((st & 7) != 0).sum())
        xbar = torch.cat([qt, qdt], dim=-1)
        lx, lu = cost.gradients(xbar, ubar)
        kff, K, _, notpd = diff.lqr_backward(sim, lx, lu, cost.Q, cost.R, args.mu)
        kff = (args.scale * kff).contiguous()
        x0 = torch.cat([q0, qd0], dim=-1).unsqueeze(1)
        xref = torch.cat([x0, xbar[:, :-1]], dim=1).contiguous()
        out = {}

        def launch(uff):
            a, b, ua, failed = diff.rollout_feedback(sim, q0, qd0, uff, K, xref, check=False, status=True, h=h, pscale=ps, integrator=1)
            J = cost.value(torch.cat([a, b], dim=-1), ua)
            return a, b, ua, torch.where(torch.isfinite(J) & ~failed, J, torch.full_like(J, float("inf")))

        def host_path():      # the loop of ilqr.solve(search="host")
            alpha = torch.zeros(B, dtype=torch.float64, device=dev)
            accepted = torch.zeros(B, dtype=torch.bool, device=dev)
            clean, launches = False, 0
            for al in ALPHAS:
                trial = torch.where(accepted, alpha, torch.full_like(alpha, float(al)))
                res = launch(ubar + trial[:, None, None] * kff)
                launches += 1
                better = ~accepted & (res[3] < Jbar) & ~notpd
                alpha = torch.where(better, trial, alpha)
                accepted = accepted | better
                clean = bool(accepted.all())
                if clean:
                    break
            if not clean:
                res = launch(ubar + alpha[:, None, None] * kff)
                launches += 1
            out["a"] = (alpha, res[3], launches)

        def device_path():
            bar = torch.where(notpd, torch.full_like(Jbar, float("-inf")), Jbar)
            r = diff.rollout_search(sim, q0, qd0, ubar, kff, K, xref, ALPHAS, bar, cost=cost, h=h, pscale=ps)
            out["b"] = (r[4], r[3])
            out["b_ms"] = sim._L.rmx_last_step_ms(sim._batch)

        for _ in range(2):      # two untimed calls of each first
            host_path()
            device_path()
        ta, tb, kb = [], [], []
        for _ in range(REP):      # alternating repeats
            ta.append(once(host_path))
            tb.append(once(device_path))
            kb.append(out["b_ms"])
        ta, tb = np.array(ta), np.array(tb)
        aa, ab = out["a"][0].cpu().numpy(), out["b"][0].cpu().numpy()
        share = lambda a: "  ".join("%g: %.1f %%" % (x, 100.0 * float((a == x).mean())) for x in ALPHAS + (0.0,))      # noqa: E731
        lines.append("%d-link chain, %d rollouts, %d steps of h = %g (the scene's %g / %g), alphas %s, direction %g * kff; nominal (a nalpha = 0 launch) "
                     "%.3f ms, %d rollouts with a failed Newton solve, %d flagged by the sweep"
                     % (args.links, B, N, h, sc.h, args.h_div, ALPHAS, args.scale, nom_ms, bad, int(notpd.sum())))
        lines.append("  (a) search=\"host\"   %d launches of rollout_feedback + cost.value   median %9.3f ms  (min %.3f, max %.3f over %d repeats)"
                     % (out["a"][2], float(np.median(ta)), ta.min(), ta.max(), REP))
        lines.append("  (b) search=\"device\" one rollout_search                              median %9.3f ms  (min %.3f, max %.3f over %d repeats); "
                     "kernel alone %.3f ms" % (float(np.median(tb)), tb.min(), tb.max(), REP, float(np.median(kb))))
        lines.append("  (a) / (b) = %.2f;  (b) %s (a)'s median" % (np.median(ta) / np.median(tb), "is not above" if np.median(tb) <= np.median(ta) else "IS ABOVE"))
        lines.append("  accepted alpha, share of the rollouts (0: none):  (a) %s" % share(aa))
        lines.append("                                                   (b) %s" % share(ab))
        lines.append("  rollouts the two paths decide differently: %d; max |J_b - J_a| / |J_a| where they agree: %.2e"
                     % (int((aa != ab).sum()), float(((out["b"][1] - out["a"][1]).abs() / out["a"][1].abs())[torch.as_tensor(aa == ab, device=dev)].max())))
        bad_total += bad
        sim.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")
    return 2 if bad_total else 0


if __name__ == "__main__":
    sys.exit(main())
