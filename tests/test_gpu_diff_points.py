"""redmax_amd.diff.points: world positions of body points as a differentiable function of a state record
(rmx_rollout_points_device forward and backward), alone and composed with diff.rollout."""
import numpy as np
import pytest

from test_gpu_adjoint_controls import _scene
from test_rollout_vjp_proto import case

EPS = np.finfo(np.float64).eps


@pytest.mark.gpu
def test_gradcheck_of_points():
    """torch.autograd.gradcheck on the 5-chain, B = 2, N = 2: the tip at both steps, an inner body off its axis, two terms sharing a
    body and a step."""
    import torch
    from redmax_amd import BatchSim, diff
    sc = _scene(5, 1)
    Bs, N = 2, 2
    sim = BatchSim(sc, batch=Bs)
    cs = case(sc, 83, nsteps=N, B=Bs)
    rng = np.random.default_rng(89)
    q = torch.tensor(cs["q0"][:, None] + 0.1 * rng.standard_normal((Bs, N, sc.nr)), dtype=torch.float64, device="cuda:0", requires_grad=True)
    terms = [dict(body=4, xlocal=[5.0, 0.0, 0.0], step=1), dict(body=2, xlocal=[1.0, 0.5, -0.5], step=2),
             dict(body=4, xlocal=[5.0, 0.0, 0.0], step=2), dict(body=4, xlocal=[-1.0, 0.3, 0.2], step=2)]
    x = diff.points(sim, q, terms)
    assert tuple(x.shape) == (Bs, len(terms), 3)
    assert torch.autograd.gradcheck(lambda a: diff.points(sim, a, terms), (q,), eps=1e-6, atol=1e-7, rtol=1e-6)
    with pytest.raises(ValueError, match="points: q must have shape"):
        diff.points(sim, q[:, :, :-1], terms)
    with pytest.raises(ValueError, match="points: q must be float64"):
        diff.points(sim, q.float(), terms)
    sim.close()


@pytest.mark.gpu
def test_a_task_space_loss_on_a_rollout_reaches_the_controls():
    """L = sum_t w_t/2 |points(rollout(u))_t - target_t|^2 backpropagates to u.grad through rmx_rollout_points_device and
    rmx_rollout_vjp_device; the same gradient by hand: rmx_rollout_vjp fed with the q block of cost_model's lx for the same terms.
    Both run the same kernels on the same tape.  The cotangent of q is w_t (Jp'r) in lx and Jp'(w_t r) in the pull-back: with the
    weights powers of two the two differ by exact scalings alone; the comparison is held to the rule's floor, 8 * 16 eps of the
    largest entry."""
    import torch
    from redmax_amd import BatchSim, diff
    sc = _scene(5, 1)
    Bs, N = 3, 6
    sim = BatchSim(sc, batch=Bs)
    cs = case(sc, 97, nsteps=N, B=Bs)
    dev = torch.device("cuda", 0)
    t = {k: torch.tensor(cs[k], dtype=torch.float64, device=dev) for k in ("q0", "qd0", "u")}
    terms = [dict(body=4, xlocal=[5.0, 0.0, 0.0], step=3, wpos=2.0), dict(body=2, xlocal=[1.0, 0.5, -0.5], step=N, wpos=0.5),
             dict(body=4, xlocal=[5.0, 0.0, 0.0], step=N, wpos=4.0)]
    w = torch.tensor([tm["wpos"] for tm in terms], dtype=torch.float64, device=dev)
    target = torch.tensor([[10.0, 0.0, -10.0], [4.0, 1.0, -3.0], [8.0, 1.0, -12.0]], dtype=torch.float64, device=dev)
    u = t["u"].clone().requires_grad_(True)
    qt, qdt = diff.rollout(sim, t["q0"], t["qd0"], u, h=sc.h, pscale=sc.task["pscale"])
    x = diff.points(sim, qt, terms)
    L = (0.5 * w[None, :, None] * (x - target) ** 2).sum()
    L.backward()
    m = diff.cost_model(sim, qt.detach(), qdt.detach(), terms=terms, xtarget=target, want=("J", "lx"))
    assert abs(float(m["J"].sum()) - float(L)) <= 128 * EPS * abs(float(L))
    gq = np.ascontiguousarray(m["lx"][:, :, :sc.nr].cpu().numpy())
    assert not np.any(m["lx"][:, :, sc.nr:].cpu().numpy())
    du, _, _ = sim.rollout_vjp(N, gq, np.zeros_like(gq))
    g = u.grad.cpu().numpy()
    err = np.abs(g - du).max() / np.abs(du).max()
    print("|u.grad - rollout_vjp(lx_q)| / max = %.3e" % err)
    assert np.abs(du).max() > 0 and err <= 8 * 16 * EPS
    sim.close()
