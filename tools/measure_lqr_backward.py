"""Time of the backward pass of one iLQR iteration, the two ways ilqr.solve can run it, on the same nominal: the figures of
profiles/lqr_backward.txt and of DESIGN.md.

    python tools/measure_lqr_backward.py [--links 32] [--batch 512] [--steps 20 100] [--h-div 5] [--box [--box-quantile Q]] [--out FILE]

  (a) backward="torch":  diff.linearize (rmx_rollout_tape_device + rmx_rollout_linearize_device + the torch assembly of A_k, B_k) and
      ilqr.backward_pass (a Python loop over the steps), as solve runs the pair;
  (b) backward="device": diff.lqr_backward (rmx_rollout_lqr_device) on the tape that stands.

Both are timed with torch.cuda events around the call(s) on a synchronised device - wall time on the device's clock, launch gaps
and host work of the Python loop included, which is what an iteration pays -, after two untimed calls, as the median of --repeats
calls; for (b) the library's own kernel time (rmx_last_step_ms) is printed next to it.  The scene is sceneAdjointChain(links) at the
scene's step size divided by --h-div (see tools/measure_vjp_feedback.py), the cost that of tests/test_gpu_ilqr.py.  The exit status
is 2 when a rollout of the nominal reports a failed Newton solve, when a rollout is flagged not positive definite, or when the two
paths' gains differ by more than 1e-9 relative: then the figures are not ones to quote.

--box adds, on the same tape: (c) diff.lqr_backward_box (rmx_rollout_lqr_box_device) under torque limits - r_i = half the median of
|kff_i| of (b), ulo_i = min ubar_i - r_i, uhi_i = max ubar_i + r_i, DOF 0 unbounded above and DOF 1 unbounded (the recipe of
tests/test_gpu_rollout_lqr_box.py), or with --box-quantile Q the Q and 1 - Q quantiles of ubar + kff per DOF -, its kernel time next
to (b)'s, the share of DOF-steps on a bound, and the mean number of QP iterations per step, counted by the float64 run of
tests/proto_lqr_box.py on the first --proto-rollouts rollouts (whose clamped sets must be the device's); and the clamped feedback
launch (rmx_rollout_tape_feedback_box_device, uff = ubar + kff, the gains of (c)) against rmx_rollout_tape_feedback_device on the
same inputs, kernel times as the library reports them, the median of --repeats launches each.
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
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--h-div", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--mu", type=float, default=1e-6)
    ap.add_argument("--box", action="store_true")
    ap.add_argument("--box-quantile", type=float, default=0.0)
    ap.add_argument("--proto-rollouts", type=int, default=4)
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

    def timed(fn, also=None):
        v, w = [], []
        for _ in range(REP + 2):      # two untimed calls first
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            v.append(e0.elapsed_time(e1))
            if also:
                w.append(also())
        v = np.array(v[2:])
        return float(np.median(v)), float(v.min()), float(v.max()), (float(np.median(w[2:])) if also else None)

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
        qt, qdt, ubar, failed = diff.rollout_feedback(sim, q0, qd0, u, h=h, pscale=ps, check=False, status=True)
        fwd_ms = sim._L.rmx_last_step_ms(sim._batch)
        bad = int(failed.sum())
        xbar = torch.cat([qt, qdt], dim=-1)
        lx, lu = cost.gradients(xbar, ubar)
        out = {}

        def torch_path():
            _, _, A, Bm = diff.linearize(sim, q0, qd0, ubar, h=h, pscale=ps, check=False)
            out["a"] = ilqr.backward_pass(A, Bm, lx, lu, cost.Q, cost.R, args.mu)

        def device_path():
            out["b"] = diff.lqr_backward(sim, lx, lu, cost.Q, cost.R, args.mu)

        ta = timed(torch_path)
        tb = timed(device_path, also=lambda: sim._L.rmx_last_step_ms(sim._batch))
        ka, Ka, ea = out["a"]
        kb, Kb, eb, notpd = out["b"]
        dk = float((kb - ka).abs().max() / ka.abs().max())
        dK = float((Kb - Ka.transpose(-1, -2)).abs().max() / Ka.abs().max())
        flagged = int(notpd.sum())
        lines.append("%d-link chain, %d rollouts, %d steps of h = %g (the scene's %g / %g); nominal: rmx_rollout_tape_feedback %.3f ms, %d rollouts "
                     "with a failed Newton solve" % (args.links, B, N, h, sc.h, args.h_div, fwd_ms, bad))
        lines.append("  (a) diff.linearize + ilqr.backward_pass   median %9.3f ms  (min %.3f, max %.3f over %d calls)" % (ta[:3] + (REP,)))
        lines.append("  (b) diff.lqr_backward                     median %9.3f ms  (min %.3f, max %.3f over %d calls); kernel alone %.3f ms"
                     % (tb[:3] + (REP, tb[3])))
        lines.append("  (a) / (b) = %.1f;  (b) against (a): max |kff diff| / max |kff| = %.2e, K %.2e; rollouts flagged not positive definite: %d"
                     % (ta[0] / tb[0], dk, dK, flagged))
        lines.append("  memory (a) writes for XA, XB, XU, A, B: %.0f MB; (b): none" % (B * N * (3 * nr * nr + 4 * nr * nr + 2 * nr * nr) * 8 / 1e6))
        bad_total += bad + flagged + (0 if max(dk, dK) < 1e-9 else 1)
        if args.box:
            bad_total += box_section(args, sim, cost, q0, qd0, ubar, xbar, lx, lu, kb, tb, timed, lines, h, ps)
        sim.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")
    return 2 if bad_total else 0


def box_section(args, sim, cost, q0, qd0, ubar, xbar, lx, lu, kfree, tb, timed, lines, h, ps):
    """(c) and the clamped feedback launch on the tape that stands; returns the number of reasons not to quote the figures."""
    import torch
    from redmax_amd import diff
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import proto_lqr_box as PB
    B, N, nr = ubar.shape
    if args.box_quantile > 0:
        tgt = (ubar + kfree).reshape(-1, nr)
        ulo, uhi = torch.quantile(tgt, args.box_quantile, dim=0), torch.quantile(tgt, 1 - args.box_quantile, dim=0)
        what = "the %g / %g quantiles of ubar + kff" % (args.box_quantile, 1 - args.box_quantile)
    else:
        r = 0.5 * kfree.abs().reshape(-1, nr).median(dim=0).values
        ulo, uhi = ubar.reshape(-1, nr).min(dim=0).values - r, ubar.reshape(-1, nr).max(dim=0).values + r
        what = "min ubar - r, max ubar + r, r = half the median of |kff|"
    uhi[0] = float("inf")
    ulo[1], uhi[1] = -float("inf"), float("inf")
    out = {}

    def box_path():
        out["c"] = diff.lqr_backward_box(sim, lx, lu, cost.Q, cost.R, ubar, (ulo, uhi), args.mu)

    tc = timed(box_path, also=lambda: sim._L.rmx_last_step_ms(sim._batch))
    kff, K, expected, status, clamped = out["c"]
    share = float(sum(((clamped >> i) & 1).sum() for i in range(nr))) / (B * N * nr)
    # the QP iterations: the float64 proto on the first rollouts, on A, B of the same nominal
    _, _, A, Bm = diff.linearize(sim, q0, qd0, ubar, h=h, pscale=ps, check=False)
    sim_tape_again = diff.rollout_feedback(sim, q0, qd0, ubar, h=h, pscale=ps, check=False)      # (linearize replaced the tape: the same one again)
    assert torch.equal(sim_tape_again[2], ubar)
    n = lambda t: t.cpu().numpy()      # noqa: E731
    iters, agree = [], True
    for b in range(min(args.proto_rollouts, B)):
        res = PB.backward_pass_box(n(A[b]), n(Bm[b]), n(lx[b]), n(lu[b]), n(cost.Q), n(cost.R), n(ubar[b]), n(ulo), n(uhi), args.mu,
                                   dtype=np.float64)
        iters.append(res["iters"].mean())
        agree = agree and res["status"] == 0 and np.array_equal(res["clamped"], n(clamped[b]).astype(np.uint32))
    for b in [int(i) for i in torch.nonzero(status).flatten()[:4]]:      # what the float64 proto makes of the rollouts the device flagged
        res = PB.backward_pass_box(n(A[b]), n(Bm[b]), n(lx[b]), n(lu[b]), n(cost.Q), n(cost.R), n(ubar[b]), n(ulo), n(uhi), args.mu,
                                   dtype=np.float64)
        lines.append("      rollout %d: device status %d, float64 proto status %d (QP iterations per step %s)"
                     % (b, int(status[b]), res["status"], res["iters"].tolist()))
    xref = torch.cat([torch.cat([q0, qd0], dim=-1).unsqueeze(1), xbar[:, :-1]], dim=1).contiguous()
    uff = ubar + kff
    tf = timed(lambda: diff.rollout_feedback(sim, q0, qd0, uff, K, xref, h=h, pscale=ps, check=False),
               also=lambda: sim._L.rmx_last_step_ms(sim._batch))
    tg = timed(lambda: diff.rollout_feedback(sim, q0, qd0, uff, K, xref, h=h, pscale=ps, check=False, ulim=(ulo, uhi)),
               also=lambda: sim._L.rmx_last_step_ms(sim._batch))
    nbad = int((status != 0).sum())
    lines.append("  limits: %s; DOF 0 unbounded above, DOF 1 unbounded" % what)
    lines.append("  (c) diff.lqr_backward_box                 median %9.3f ms  (min %.3f, max %.3f over %d calls); kernel alone %.3f ms = %.2f x (b)'s %.3f ms"
                 % (tc[:3] + (args.repeats, tc[3], tc[3] / tb[3], tb[3])))
    lines.append("      %.1f %% of the DOF-steps on a bound; %.2f QP iterations per step (float64 proto, rollouts 0..%d, clamped sets %s the device's); "
                 "rollouts with status != 0: %d" % (100 * share, float(np.mean(iters)), len(iters) - 1, "equal" if agree else "DIFFER FROM", nbad))
    lines.append("  feedback launch, uff = ubar + kff, K of (c): rmx_rollout_tape_feedback_device kernel %.3f ms; rmx_rollout_tape_feedback_box_device "
                 "%.3f ms (medians of %d)" % (tf[3], tg[3], args.repeats))
    return nbad + (0 if agree else 1)


if __name__ == "__main__":
    sys.exit(main())
