"""redmax_amd.diff on a sim whose tape carries point forces: force_params(sim), rollout(..., force_params=...) and rollout(...,
params=model_params(sim)) there - one rmx_rollout_vjp_forces_device call per backward.

  1. .grad of force_params(sim) and of model_params(sim) is the batch sum of the library's rows (rollout_vjp_forces on a second sim),
     to 1e-14 relative; the trajectory and the input gradients are those of the rollout without the keywords, bit for bit;
  2. a five-iteration gradient descent on one spring's stiffness, the sim rebuilt from the updated table at every iterate, lowers a
     trajectory-matching loss monotonically at n = 4 (step: Polyak's, loss / gradient, the minimum of the loss being 0; on the CPU
     proto the error of the stiffness halves per iterate from 0.7 and from 1.3 times the true value);
  3. a wrong shape, dtype or device, an unknown name and a sim without a force table give ValueError.
Inputs: proto_rollout_pf.case(4)."""
import functools

import numpy as np
import pytest

import proto_rollout_force_params as F
import proto_rollout_pf as P

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(n):
    cs = P.case(n)
    return cs, P.World(cs["sc"])


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


@pytest.mark.parametrize("integ", [1, 2])
def test_torch_gradients_are_the_batch_sum_of_the_call(integ):
    import torch
    from redmax_amd import BatchSim, _abi, diff
    cs, ev = _case(4)
    N, h, ps = cs["nsteps"], cs["h"], cs["pscale"]
    dev = torch.device("cuda", 0)
    t = {k: torch.tensor(cs[k], dtype=torch.float64, device=dev) for k in ("q0", "qd0", "u", "c", "d")}
    sim = BatchSim(cs["sc"], batch=2, tape_forces=True)
    fp, mp = diff.force_params(sim), diff.model_params(sim)
    assert tuple(fp) == _abi.FORCE_PARAM_NAMES == F.NAMES
    assert all(v.is_leaf and v.requires_grad and v.dtype == torch.float64 and v.device == dev for v in fp.values())
    theta = F.constants(ev)
    assert all(np.array_equal(fp[n].detach().cpu().numpy(), theta[:, i]) for i, n in enumerate(F.NAMES))

    def run(**kw):
        q0, qd0, u = (t[k].clone().requires_grad_(True) for k in ("q0", "qd0", "u"))
        qt, qdt = diff.rollout(sim, q0, qd0, u, h=h, pscale=ps, integrator=integ, **kw)
        ((t["c"] * qt).sum() + (t["d"] * qdt).sum() + 0.5 * (qt ** 2).sum()).backward()
        return qt.detach().cpu().numpy(), qdt.detach().cpu().numpy(), [x.grad.cpu().numpy() for x in (q0, qd0, u)]

    qt0, qdt0, g0 = run()
    qt1, qdt1, g1 = run(params=mp, force_params=fp)
    assert np.array_equal(qt0, qt1) and np.array_equal(qdt0, qdt1) and all(np.array_equal(a, b) for a, b in zip(g0, g1))
    ref = BatchSim(cs["sc"], batch=2, tape_forces=True)
    ref.set_state(cs["q0"], cs["qd0"])
    qt, qdt, _ = ref.rollout_tape(N, h, cs["u"], pscale=ps, integrator=integ)
    du, dq0, dqd0, grads = ref.rollout_vjp_forces(N, cs["c"] + qt, cs["d"], model=_abi.PARAM_NAMES)
    ref.close()
    assert np.array_equal(qt, qt1) and np.array_equal(g1[2], du) and np.array_equal(g1[0], dq0) and np.array_equal(g1[1], dqd0)
    both = dict(fp, **mp)
    for n in both:
        got, want = both[n].grad.cpu().numpy(), grads[n].sum(axis=0)
        assert got.shape == want.shape and np.linalg.norm(want) > 0 and _rel(got, want) <= 1e-14, n
    # the force constants alone, and a subset: only the named tensors receive a gradient, and backward accumulates
    before = {n: both[n].grad.clone() for n in both}
    run(force_params={"force_L": fp["force_L"]})
    run(params={"grav": mp["grav"]})
    for n in both:
        want = 2.0 * before[n] if n in ("force_L", "grav") else before[n]
        assert torch.allclose(both[n].grad, want, rtol=1e-14, atol=0.0), n
    # what it cannot take
    a = (sim, t["q0"], t["qd0"], t["u"])
    with pytest.raises(ValueError, match="unknown force parameter 'stiffness'"):
        diff.rollout(*a, h=h, force_params={"stiffness": fp["force_stiffness"]})
    with pytest.raises(ValueError, match=r"force_params\['force_L'\] must have shape \(4,\), got \(3,\)"):
        diff.rollout(*a, h=h, force_params={"force_L": fp["force_L"].detach()[:3]})
    with pytest.raises(ValueError, match="float64"):
        diff.rollout(*a, h=h, force_params={"force_damping": fp["force_damping"].detach().float()})
    with pytest.raises(ValueError, match="device"):
        diff.rollout(*a, h=h, force_params={"force_damping": fp["force_damping"].detach().cpu()})
    with pytest.raises(ValueError, match="torch.Tensor"):
        diff.rollout(*a, h=h, force_params={"force_damping": theta[:, 1]})
    with pytest.raises(ValueError, match="dict"):
        diff.rollout(*a, h=h, force_params=[fp["force_L"]])
    with pytest.raises(ValueError, match="names no parameter"):
        diff.rollout(*a, h=h, force_params={})
    sim.close()
    from redmax_amd.scenes import scenesRedMax
    sc = scenesRedMax(2)
    sc.init()
    plain = BatchSim(sc, batch=1)
    z = torch.zeros((1, sc.nr), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="needs a sim whose tape carries point forces"):
        diff.rollout(plain, z, z, torch.zeros((1, 2, sc.nr), dtype=torch.float64, device=dev), force_params={"force_L": fp["force_L"]})
    assert diff.force_params(plain)["force_L"].shape == (0,)
    plain.close()


def test_gradient_descent_recovers_a_spring_stiffness():
    import torch
    from redmax_amd import BatchSim, diff
    cs, ev = _case(4)
    N, h, ps = cs["nsteps"], cs["h"], cs["pscale"]
    dev = torch.device("cuda", 0)
    q0, qd0, u = (torch.tensor(cs[k], dtype=torch.float64, device=dev) for k in ("q0", "qd0", "u"))
    desc = cs["sc"].desc()
    true = float(desc["point_forces"][1]["stiffness"])

    def sim_with(ks):
        d = dict(desc)
        d["point_forces"] = [dict(f, stiffness=ks) if i == 1 else f for i, f in enumerate(desc["point_forces"])]
        return BatchSim(d, batch=2, tape_forces=True)

    sim = sim_with(true)
    target = diff.rollout(sim, q0, qd0, u, h=h, pscale=ps)[0].detach()
    sim.close()
    ks, losses = 1.3 * true, []
    for _ in range(6):      # five updates: six losses
        sim = sim_with(ks)
        fp = diff.force_params(sim)
        assert fp["force_stiffness"][1].item() == ks
        loss = 0.5 * ((diff.rollout(sim, q0, qd0, u, h=h, pscale=ps, force_params={"force_stiffness": fp["force_stiffness"]})[0] - target) ** 2).sum()
        loss.backward()
        g = fp["force_stiffness"].grad.cpu().numpy()
        sim.close()
        losses.append(loss.item())
        assert g[1] > 0
        ks -= losses[-1] / g[1]
    print("descent on a spring's stiffness: losses " + " ".join("%.3e" % x for x in losses) + "; ks / true = %.4f" % (ks / true))
    assert all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] < 1e-2 * losses[0]
    assert abs(ks / true - 1.0) < 0.02
