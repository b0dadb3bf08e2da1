"""redmax_amd.ilqr.solve with a TrackingCost: the device iLQR pointed at a task-space objective - bring the tip of the 5-link chain
to a world target - through diff.cost_model (rmx_rollout_cost_device) and the per-rollout Gauss-Newton table.

The problem: B = 3 rollouts from test_rollout_vjp_proto.case's initial states, N = 8 steps, 4 iterations.  The tip (point [5 0 0] of
the last body) is tracked at every step with weight 0.05 and at step N with weight 5; the target of a rollout is the tip at the
posture q0 - 0.1 of ITS initial state, taken from diff.points, so it is reachable; Q = 0.01 on qdot, nothing on q; R = 0.1 I.
"""
import numpy as np
import pytest

from test_gpu_adjoint_controls import _scene
from test_gpu_ilqr import _problem as _joint_problem
from test_rollout_vjp_proto import case

B, N, ITERS = 3, 8, 4
TIP = [5.0, 0.0, 0.0]


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
    terms = [dict(body=tip, xlocal=TIP, step=k, wpos=0.05) for k in range(1, N + 1)] + [dict(body=tip, xlocal=TIP, step=N, wpos=5.0)]
    goal = diff.points(sim, (t["q0"] - 0.1)[:, None, :].contiguous(), [dict(body=tip, xlocal=TIP, step=1)])      # [B][1][3]
    xtarget = goal.expand(B, len(terms), 3).contiguous()
    Q = torch.diag(torch.tensor([0.0] * nr + [0.01] * nr, dtype=torch.float64, device=dev)).repeat(N, 1, 1)
    R = 0.1 * torch.eye(nr, dtype=torch.float64, device=dev)
    return sc, cs, t, TrackingCost(sim, Q, R, None, terms, xtarget), goal[:, 0]


def _tip_distance(sim, qtraj, goal):
    from redmax_amd import diff
    tipN = diff.points(sim, qtraj.contiguous(), [dict(body=sim.nr - 1, xlocal=TIP, step=N)])[:, 0]
    return (tipN - goal).norm(dim=1).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("backward", ["torch", "device"])
def test_tracking_descends_reaches_for_the_target_and_leaves_the_tape_of_its_result(backward):
    import torch
    from redmax_amd import BatchSim, diff, ilqr
    sim = BatchSim(_scene(5, 1), batch=B)
    sc, cs, t, cost, goal = _problem(sim)
    ps = sc.task["pscale"]
    qt0, qdt0 = diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, pscale=ps)
    d0 = _tip_distance(sim, qt0, goal)
    J0 = cost.value(torch.cat([qt0, qdt0], dim=-1), t["u"]).cpu().numpy()
    res, hist = ilqr.solve(sim, t["q0"], t["qd0"], t["u"], cost, iters=ITERS, h=sc.h, pscale=ps, backward=backward)
    h = hist.cpu().numpy()
    print("%s: cost history per rollout (rows: before, after iteration 1 ..):\n%s\nlast step lengths %s" % (backward, h, res.alpha.cpu().numpy()))
    assert h.shape == (ITERS + 1, B)
    assert np.allclose(h[0], J0, rtol=1e-12)
    assert (h[1:] <= h[:-1]).all()                                   # exact: a rollout keeps a trial only where it lowers its own cost
    assert (h[-1] < h[0]).all()
    # the sim holds the tape of the result (the cost calls in between have not touched it)
    q, qd = sim.get_state()
    assert np.array_equal(q, res.qtraj[:, -1].cpu().numpy()) and np.array_equal(qd, res.qdtraj[:, -1].cpu().numpy())
    rng = np.random.default_rng(3)
    gq, gqd = rng.standard_normal((B, N, sc.nr)), rng.standard_normal((B, N, sc.nr))
    after_solve = sim.rollout_vjp(N, gq, gqd)
    d1 = _tip_distance(sim, res.qtraj, goal)
    assert all(np.array_equal(a, b) for a, b in zip(after_solve, sim.rollout_vjp(N, gq, gqd)))
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, _ = sim.rollout_tape(N, sc.h, res.u.cpu().numpy(), pscale=ps)
    explicit = sim.rollout_vjp(N, gq, gqd)
    assert np.array_equal(qt, res.qtraj.cpu().numpy()) and np.array_equal(qdt, res.qdtraj.cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(after_solve, explicit))
    print("%s: tip distance to the target at step N: %s before, %s after" % (backward, d0, d1))
    assert (d1 < d0).all()
    sim.close()


@pytest.mark.gpu
def test_tracking_under_torque_limits_that_bind():
    import torch
    from redmax_amd import BatchSim, ilqr
    sim = BatchSim(_scene(5, 1), batch=B)
    sc, cs, t, cost, _ = _problem(sim)
    lim = 0.05                                                       # (|u0| is 0.1 per entry: the box binds from the first launch on)
    ulo = torch.full((sc.nr,), -lim, dtype=torch.float64, device=t["u"].device)
    res, hist = ilqr.solve(sim, t["q0"], t["qd0"], t["u"], cost, iters=ITERS, h=sc.h, pscale=sc.task["pscale"], backward="device", ulim=(ulo, -ulo))
    h, u = hist.cpu().numpy(), res.u.cpu().numpy()
    print("boxed: cost history\n%s\ntorques on a bound: %d of %d" % (h, (np.abs(u) == lim).sum(), u.size))
    assert (u >= -lim).all() and (u <= lim).all() and (np.abs(u) == lim).any()
    assert (h[1:] <= h[:-1]).all()
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("backward", ["torch", "device"])
def test_a_quadratic_cost_keeps_its_bits_through_either_branch(backward):
    """solve with a QuadraticCost goes through cost.gradients / cost.Q as before; the same cost behind a `model` of its own - the
    same gradients, the same shared table - goes through the new branch: the same bits."""
    import torch
    from redmax_amd import BatchSim, ilqr
    sc, cs, t, cost = _joint_problem()

    class WithModel(ilqr.QuadraticCost):
        def model(self, x, u):
            return self.gradients(x, u) + (self.Q,)

    outs = []
    for c in (cost, WithModel(cost.Q, cost.R, cost.xgoal)):
        sim = BatchSim(sc, batch=B)
        outs.append(ilqr.solve(sim, t["q0"], t["qd0"], t["u"], c, iters=2, h=sc.h, pscale=sc.task["pscale"], backward=backward))
        sim.close()
    (r0, h0), (r1, h1) = outs
    assert torch.equal(h0, h1) and all(torch.equal(a, b) for a, b in zip(r0, r1))
    assert (h0[-1] < h0[0]).all()
