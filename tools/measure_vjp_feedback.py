"""Kernel time of rmx_rollout_vjp_feedback next to rmx_rollout_vjp on the same tape (rmx_last_step_ms: the library's events around the
kernel, device pointers, nothing staged): the figures of profiles/rollout_vjp_feedback.txt and of DESIGN.md.

    python tools/measure_vjp_feedback.py [--links 32] [--batch 512] [--steps 100] [--h-div 5] [--out FILE]

The scene is sceneAdjointChain(links); the step size is the scene's divided by --h-div (the scene's own step size is chosen for
20-step horizons: over 100 steps of it the chain's Newton solves fail).  Gains: PD-like tables shared by the batch, as
tests/test_rollout_feedback_proto.py feedback_case builds them.  The exit status is 2 when a rollout of the forward call reports a
failed Newton solve or a non-finite state: then the tape is not one to time gradients on.
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--h-div", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from redmax_amd import BatchSim
    from redmax_amd.scenes import sceneAdjointChain
    B, N, REP = args.batch, args.steps, args.repeats
    dev = torch.device("cuda", 0)
    lines, bad_total = [], 0

    def t(a):
        return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)

    def p(x):
        return x.data_ptr()

    for integ in (1, 2):
        sc = sceneAdjointChain(args.links, bdf2=integ == 2)
        sc.init()
        nr, h = sc.nr, sc.h / args.h_div
        rng = np.random.default_rng(3)
        q0, qd0 = sc.getQ()
        q, qd = t(q0[None] + 0.05 * rng.standard_normal((B, nr))), t(qd0[None] + 0.2 * rng.standard_normal((B, nr)))
        uff = t(0.1 * rng.standard_normal((B, N, nr)))
        Kn = np.zeros((N, 2 * nr, nr))
        for k in range(N):
            Kn[k, :nr] = -0.25 * np.eye(nr) + 0.05 * rng.standard_normal((nr, nr)) / np.sqrt(nr)
            Kn[k, nr:] = -0.06 * np.eye(nr) + 0.012 * rng.standard_normal((nr, nr)) / np.sqrt(nr)
        K = t(Kn)
        xref = t(np.concatenate([q0[None] + 0.05 * rng.standard_normal((N, nr)), qd0[None] + 0.2 * rng.standard_normal((N, nr))], axis=1))
        qt = torch.empty((B, N, nr), dtype=torch.float64, device=dev)
        qdt, ua = torch.empty_like(qt), torch.empty_like(qt)
        sim = BatchSim(sc, batch=B)
        torch.cuda.synchronize()
        sim.set_state_device(p(q), p(qd))
        info = sim.rollout_feedback_device(N, h, p(uff), p(K), p(xref), p(qt), p(qdt), p(ua), pscale=sc.task["pscale"], stats=True,
                                           integrator=integ)
        bad = int(((info["status"] & 15) != 0).sum())
        finite = bool(torch.isfinite(qt).all() and torch.isfinite(qdt).all() and torch.isfinite(ua).all())
        fb_share = float((ua - uff).norm() / uff.norm())
        gq, gqd, gu = (t(rng.standard_normal((B, N, nr))) for _ in range(3))
        du = torch.empty_like(qt)
        dq0 = torch.empty((B, nr), dtype=torch.float64, device=dev)
        dqd0 = torch.empty_like(dq0)
        dx = torch.empty((B, N, 2 * nr), dtype=torch.float64, device=dev)
        dK = torch.empty((B, N, 2 * nr, nr), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def timed(fn):
            v = []
            for _ in range(REP + 2):      # two untimed calls first
                fn()
                v.append(sim._L.rmx_last_step_ms(sim._batch))
            v = np.array(v[2:])
            return float(np.median(v)), float(v.min()), float(v.max()), sim.last_step_kernel()

        fbk = dict(gu_ptr=p(gu), K_ptr=p(K), xref_ptr=p(xref), duff_ptr=p(du), dq0_ptr=p(dq0), dqd0_ptr=p(dqd0))
        cases = [
            ("rmx_rollout_vjp: du, dq0, dqd0", lambda: sim.rollout_vjp_device(N, p(gq), p(gqd), p(du), p(dq0), p(dqd0))),
            ("K NULL, gu NULL: duff, dq0, dqd0", lambda: sim.rollout_vjp_feedback_device(N, p(gq), p(gqd), duff_ptr=p(du), dq0_ptr=p(dq0), dqd0_ptr=p(dqd0))),
            ("K, gu: duff, dq0, dqd0", lambda: sim.rollout_vjp_feedback_device(N, p(gq), p(gqd), **fbk)),
            ("K, gu: duff, dxref, dq0, dqd0", lambda: sim.rollout_vjp_feedback_device(N, p(gq), p(gqd), dxref_ptr=p(dx), **fbk)),
            ("K, gu: duff, dK, dxref, dq0, dqd0", lambda: sim.rollout_vjp_feedback_device(N, p(gq), p(gqd), dK_ptr=p(dK), dxref_ptr=p(dx), **fbk)),
        ]
        lines.append("BDF%d  %d-link chain, %d rollouts, %d steps of h = %g (the scene's %g / %g); forward rmx_rollout_tape_feedback %.3f ms, %.1f Newton "
                     "iterations per rollout, %d rollouts with a failed Newton solve, states finite: %s, |uapp - uff| / |uff| = %.2f"
                     % (integ, args.links, B, N, h, sc.h, args.h_div, info["ms"], info["newton_iters"].mean(), bad, finite, fb_share))
        for name, fn in cases:
            med, lo, hi, label = timed(fn)
            lines.append("  %-36s median %.3f ms  (min %.3f, max %.3f over %d calls)%s"
                         % (name, med, lo, hi, REP, "" if name.startswith("rmx_rollout_vjp:") else "  [%s]" % label))
        outs_finite = all(bool(torch.isfinite(x).all()) for x in (du, dq0, dqd0, dx, dK))
        lines.append("  gradients finite: %s;  dK store: %d doubles per rollout and step, %.1f MB per call" % (outs_finite, 2 * nr * nr, B * N * 2 * nr * nr * 8 / 1e6))
        bad_total += bad + (0 if finite and outs_finite else 1)
        sim.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")
    return 2 if bad_total else 0


if __name__ == "__main__":
    sys.exit(main())
