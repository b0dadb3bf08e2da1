"""redmax_amd.diff.frames: position, point velocity and orientation of body frames as a differentiable function of a state record
(rmx_rollout_frames_device forward and backward), alone and composed with diff.rollout."""
import numpy as np
import pytest

from test_gpu_adjoint_controls import _scene
from test_rollout_vjp_proto import case

EPS = np.finfo(np.float64).eps


@pytest.mark.gpu
@pytest.mark.parametrize("size", [2, "tree7"])
def test_gradcheck_of_frames(size):
    """torch.autograd.gradcheck in q and qdot, B = 2, N = 2: the tip at both steps, the root body, two terms sharing a body and a
    step; every output (x, v, R) is differentiated."""
    import torch
    from redmax_amd import BatchSim, diff
    sc = _scene(size, 1)
    Bs, N = 2, 2
    sim = BatchSim(sc, batch=Bs)
    cs = case(sc, 83, nsteps=N, B=Bs)
    rng = np.random.default_rng(101)
    mk = lambda a, s: torch.tensor(a[:, None] + s * rng.standard_normal((Bs, N, sc.nr)), dtype=torch.float64, device="cuda:0",      # noqa: E731
                                   requires_grad=True)
    q, qd = mk(cs["q0"], 0.1), mk(cs["qd0"], 0.3)
    tip = sc.nr - 1
    terms = [dict(body=tip, xlocal=[0.7, 0.2, -0.3], step=1), dict(body=0, xlocal=[0.3, 0.1, 0.2], step=2),
             dict(body=tip, xlocal=[0.5, 0.0, 0.0], step=2), dict(body=tip, xlocal=[-0.2, 0.3, 0.1], step=2)]
    x, v, R = diff.frames(sim, q, qd, terms)
    assert tuple(x.shape) == (Bs, len(terms), 3) and tuple(v.shape) == (Bs, len(terms), 3) and tuple(R.shape) == (Bs, len(terms), 3, 3)
    eye = torch.eye(3, dtype=torch.float64, device="cuda:0")
    assert float((R.transpose(-1, -2) @ R - eye).detach().abs().max()) <= 64 * EPS      # R[..., r, c]: a rotation either way, so also:
    ref = sim.rollout_frames(N, q.detach().cpu().numpy(), qd.detach().cpu().numpy(), terms)[0]
    assert np.array_equal(R.detach().cpu().numpy(), ref["R"]) and np.array_equal(v.detach().cpu().numpy(), ref["v"])
    assert torch.autograd.gradcheck(lambda a, b: diff.frames(sim, a, b, terms), (q, qd), eps=1e-6, atol=1e-7, rtol=1e-6)
    # an output that takes no part in the loss has no cotangent: its pull-back is skipped, the gradient is the others'
    (gq,) = torch.autograd.grad(x.sum(), q, retain_graph=True)
    assert torch.equal(gq, torch.autograd.grad(diff.points(sim, q, terms).sum(), q)[0])
    with pytest.raises(ValueError, match="frames: q must have shape"):
        diff.frames(sim, q[:, :, :-1], qd, terms)
    with pytest.raises(ValueError, match="frames: qdot must be float64"):
        diff.frames(sim, q, qd.float(), terms)
    sim.close()


@pytest.mark.gpu
def test_a_loss_on_orientation_and_velocity_of_a_rollout_reaches_the_controls():
    """L = sum_t wv/2 |v_t - vt_t|^2 + wr/4 |R_t - Rt_t|_F^2 on frames(rollout(u)) backpropagates to u.grad through
    rmx_rollout_frames_device and rmx_rollout_vjp_device; the same gradient by hand: rmx_rollout_vjp fed with cost_model's lx for the
    same terms (its q rows and its qdot rows).  Both run the same kernels on the same tape.  The cotangents differ in where the weight
    multiplies (w (J'r) against J'(w r)): with the weights powers of two by exact scalings alone, but for the rotation, where autograd
    feeds gR = wr/2 (R - Rt) and lx forms e_w from R Rt': two float64 evaluations of one gradient, held to the rule's floor, 8 * 16 eps
    of the largest entry."""
    import torch
    from redmax_amd import BatchSim, diff
    sc = _scene(5, 1)
    Bs, N = 3, 6
    sim = BatchSim(sc, batch=Bs)
    cs = case(sc, 97, nsteps=N, B=Bs)
    dev = torch.device("cuda", 0)
    t = {k: torch.tensor(cs[k], dtype=torch.float64, device=dev) for k in ("q0", "qd0", "u")}
    terms = [dict(body=4, xlocal=[5.0, 0.0, 0.0], step=3, wvel=2.0, wrot=0.5), dict(body=2, xlocal=[1.0, 0.5, -0.5], step=N, wvel=0.5),
             dict(body=4, xlocal=[5.0, 0.0, 0.0], step=N, wrot=4.0)]
    wv = torch.tensor([tm.get("wvel", 0.0) for tm in terms], dtype=torch.float64, device=dev)
    wr = torch.tensor([tm.get("wrot", 0.0) for tm in terms], dtype=torch.float64, device=dev)
    rng = np.random.default_rng(103)
    vt = torch.tensor(rng.standard_normal((len(terms), 3)), dtype=torch.float64, device=dev)
    ax = rng.standard_normal((len(terms), 3))
    Rt = torch.linalg.matrix_exp(torch.tensor([[[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]] for a in ax / np.linalg.norm(ax, axis=1)[:, None]],
                                              dtype=torch.float64, device=dev))
    u = t["u"].clone().requires_grad_(True)
    qt, qdt = diff.rollout(sim, t["q0"], t["qd0"], u, h=sc.h, pscale=sc.task["pscale"])
    x, v, R = diff.frames(sim, qt, qdt, terms)
    L = (0.5 * wv[None, :, None] * (v - vt) ** 2).sum() + (0.25 * wr[None, :, None, None] * (R - Rt) ** 2).sum()
    L.backward()
    m = diff.cost_model(sim, qt.detach(), qdt.detach(), terms=terms, vtarget=vt, Rtarget=Rt, want=("J", "lx"))
    assert abs(float(m["J"].sum()) - float(L)) <= 128 * EPS * abs(float(L))
    lx = m["lx"].cpu().numpy()
    assert np.any(lx[:, :, sc.nr:])
    du, _, _ = sim.rollout_vjp(N, np.ascontiguousarray(lx[:, :, :sc.nr]), np.ascontiguousarray(lx[:, :, sc.nr:]))
    g = u.grad.cpu().numpy()
    err = np.abs(g - du).max() / np.abs(du).max()
    print("|u.grad - rollout_vjp(lx)| / max = %.3e" % err)
    assert np.abs(du).max() > 0 and err <= 8 * 16 * EPS
    sim.close()
