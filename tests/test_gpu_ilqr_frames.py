"""redmax_amd.ilqr.solve with a TrackingCost that carries frame targets: bring the tip of the 5-link chain to a POSE (position and
orientation) and arrive there at rest - through diff.cost_model (rmx_rollout_cost_frames_device) and the per-rollout Gauss-Newton
table with its q, qdot cross blocks.

The problem: B = 3 rollouts from test_rollout_vjp_proto.case's initial states, N = 8 steps, 4 iterations.  One term on the tip (point
[5 0 0] of the last body) at step N with wpos = 0.5, wrot = 50, wvel = 0.01 and vtarget = 0; the pose target of a rollout is the
tip's frame at the posture q0 - 0.1 of ITS initial state, taken from diff.frames, so it is reachable; the tip is also tracked at
every step with wpos = 0.005; Q = 0.01 on qdot; R = 0.1 I.  The three weights are sized so that under u0 the three pieces of the
terminal cost are of one order: the tip moves at about 40 length units per time unit there (1/2 wvel |v|^2 ~ 8), is some 5 units
from its target (1/2 wpos |r|^2 ~ 6) and 1 - cos theta is about 0.3 (wrot (1 - cos theta) ~ 15) - a descent of the sum then has to
lower each.
"""
import numpy as np
import pytest

import proto_lqr_backward as PL
from test_gpu_adjoint_controls import _scene
from test_rollout_vjp_proto import case

B, N, ITERS = 3, 8, 4
TIP = [5.0, 0.0, 0.0]
EPS = np.finfo(np.float64).eps


def _problem(sim):
    import torch
    from redmax_amd import diff
    from redmax_amd.ilqr import TrackingCost
    sc = _scene(5, 1)
    cs = case(sc, 53, nsteps=N, B=B)
    dev = torch.device("cuda", 0)
    t = {k: torch.tensor(cs[k], dtype=torch.float64, device=dev) for k in ("q0", "qd0", "u")}
    nr = sc.nr
    tip = nr - 1
    terms = [dict(body=tip, xlocal=TIP, step=k, wpos=0.005) for k in range(1, N + 1)] + [dict(body=tip, xlocal=TIP, step=N, wpos=0.5, wvel=0.01, wrot=50.0)]
    q1 = (t["q0"] - 0.1)[:, None, :].contiguous()
    gx, _, gR = diff.frames(sim, q1, torch.zeros_like(q1), [dict(body=tip, xlocal=TIP, step=1)])      # [B][1][3], [B][1][3][3]
    T = len(terms)
    xtarget, Rtarget = gx.expand(B, T, 3).contiguous(), gR.expand(B, T, 3, 3).contiguous()
    vtarget = torch.zeros((T, 3), dtype=torch.float64, device=dev)
    Q = torch.diag(torch.tensor([0.0] * nr + [0.01] * nr, dtype=torch.float64, device=dev)).repeat(N, 1, 1)
    R = 0.1 * torch.eye(nr, dtype=torch.float64, device=dev)
    return sc, cs, t, TrackingCost(sim, Q, R, None, terms, xtarget, vtarget=vtarget, Rtarget=Rtarget), gR[:, 0]


def _pose_error_and_speed(sim, qtraj, qdtraj, Rgoal):
    """(1 - cos theta between the tip's frame and its target, the tip's speed), both at step N: [B] each."""
    from redmax_amd import diff
    _, v, R = diff.frames(sim, qtraj.contiguous(), qdtraj.contiguous(), [dict(body=sim.nr - 1, xlocal=TIP, step=N)])
    return (((R[:, 0] - Rgoal) ** 2).sum(dim=(1, 2)) / 4).cpu().numpy(), v[:, 0].norm(dim=1).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("ulim", [False, True], ids=["free", "ulim"])
def test_the_pose_is_approached_at_rest_and_the_cost_never_rises(ulim):
    import torch
    from redmax_amd import BatchSim, diff, ilqr
    sim = BatchSim(_scene(5, 1), batch=B)
    sc, cs, t, cost, Rgoal = _problem(sim)
    ps = sc.task["pscale"]
    kw = {}
    u0 = t["u"]
    if ulim:
        lim = 0.2                                                    # (u0 is 0.1 * normal: the start is u0 brought into the box)
        ulo = torch.full((sc.nr,), -lim, dtype=torch.float64, device=u0.device)
        kw = dict(ulim=(ulo, -ulo))
        u0 = u0.clamp(-lim, lim)
    qt0, qdt0 = diff.rollout(sim, t["q0"], t["qd0"], u0, h=sc.h, pscale=ps)
    c0, s0 = _pose_error_and_speed(sim, qt0, qdt0, Rgoal)
    J0 = cost.value(torch.cat([qt0, qdt0], dim=-1), u0).cpu().numpy()
    res, hist = ilqr.solve(sim, t["q0"], t["qd0"], u0, cost, iters=ITERS, h=sc.h, pscale=ps, backward="device", **kw)
    h = hist.cpu().numpy()
    c1, s1 = _pose_error_and_speed(sim, res.qtraj, res.qdtraj, Rgoal)
    print("%s: cost history per rollout (rows: before, after iteration 1 ..):\n%s\n1 - cos theta %s -> %s\ntip speed %s -> %s"
          % ("ulim" if ulim else "free", h, c0, c1, s0, s1))
    assert h.shape == (ITERS + 1, B) and np.allclose(h[0], J0, rtol=1e-12)
    assert (h[1:] <= h[:-1]).all()                                   # exact: a rollout keeps a trial only where it lowers its own cost
    assert (h[-1] < h[0]).all() and (c1 < c0).all() and (s1 < s0).all()
    if ulim:
        u = res.u.cpu().numpy()
        assert (u >= -lim).all() and (u <= lim).all()
    sim.close()


@pytest.mark.gpu
def test_the_two_backward_passes_agree_on_the_first_feed_forward():
    """The first iteration's kff from diff.lqr_backward (backward="device") and from ilqr.backward_pass (backward="torch") on the
    frame cost's model at u0, judged as section 1 of test_gpu_rollout_frames.py judges: ext = proto_lqr_backward's longdouble
    recursion, ref = backward_pass in float64, e_gpu <= 8 max(e_ref, 16 eps) per rollout."""
    import torch
    from redmax_amd import BatchSim, diff, ilqr
    sim = BatchSim(_scene(5, 1), batch=B)
    sc, cs, t, cost, _ = _problem(sim)
    mu = 1e-6
    qt, qdt, A, Bm = diff.linearize(sim, t["q0"], t["qd0"], t["u"], h=sc.h, pscale=sc.task["pscale"])
    lx, lu, Qk = cost.model(torch.cat([qt, qdt], dim=-1), t["u"])
    assert Qk.dim() == 4 and torch.equal(Qk, Qk.transpose(-1, -2)) and bool((Qk[:, N - 1, sc.nr:, :sc.nr] != 0).any())      # the cross block
    rk, _, _ = ilqr.backward_pass(A, Bm, lx, lu, Qk, cost.R, mu)
    gk, _, _, notpd = diff.lqr_backward(sim, lx, lu, Qk, cost.R, mu)
    assert not notpd.any()
    sim.close()
    n = lambda a: a.cpu().numpy()      # noqa: E731
    ok = True
    for b in range(B):
        ek = PL.backward_pass_ext(n(A)[b], n(Bm)[b], n(lx)[b], n(lu)[b], n(Qk)[b], n(cost.R), mu)[0]
        e_ref, e_gpu = PL.rel_err(n(rk)[b], ek), PL.rel_err(n(gk)[b], ek)
        bound = 8 * max(e_ref, 16 * EPS)
        print("rollout %d: kff e_ref %.2e e_gpu %.2e (bound %.2e)" % (b, e_ref, e_gpu, bound))
        ok = ok and e_gpu <= bound
    assert ok
