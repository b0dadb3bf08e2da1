"""redmax_amd.ilqr.solve(search="device"): every iteration is quadratic_model, the Riccati sweep and ONE rmx_rollout_search launch.

The problems are those of test_gpu_ilqr_tracking.py (the tip of the 5-link chain to a world target; free and under torque limits
that bind) and test_gpu_ilqr_frames.py (the tip to a pose, at rest; free and under limits), B = 3, N = 8, 4 iterations.  Asserted:
the history is non-increasing exactly (a rollout keeps a trial only where it lowers its own cost, and a rollout that keeps none
returns its nominal's J bit for bit), the final cost is below the initial, the sim's tape after solve is the returned trajectory's,
and search="host" on the same problem falls too.  The two histories are printed, not compared: the searches may accept different
alphas where a trial's J sits within rounding of Jbar.
"""
import numpy as np
import pytest
import torch  # (ahead of the library: torch finds its HIP runtime by file name, and a process must hold one runtime only)

import test_gpu_ilqr_frames as frames
import test_gpu_ilqr_tracking as tracking
from test_gpu_adjoint_controls import _scene

B, N, ITERS = tracking.B, tracking.N, tracking.ITERS
CASES = [("tracking", None), ("tracking", 0.05), ("frames", None), ("frames", 0.2)]      # (problem, the torque limit of its own test file)


@pytest.mark.gpu
@pytest.mark.parametrize("name,lim", CASES, ids=["%s-%s" % (n, "free" if l is None else "ulim") for n, l in CASES])
def test_the_device_search_descends_and_leaves_the_tape_of_its_result(name, lim):
    from redmax_amd import BatchSim, diff, ilqr
    sim = BatchSim(_scene(5, 1), batch=B)
    sc, cs, t, cost = (tracking if name == "tracking" else frames)._problem(sim)[:4]
    ps = sc.task["pscale"]
    kw, u0 = {}, t["u"]
    if lim is not None:
        ulo = torch.full((sc.nr,), -lim, dtype=torch.float64, device=u0.device)
        kw = dict(ulim=(ulo, -ulo))
    hists = {}
    for search in ("host", "device"):
        res, hist = ilqr.solve(sim, t["q0"], t["qd0"], u0, cost, iters=ITERS, h=sc.h, pscale=ps, backward="device", search=search, **kw)
        h = hist.cpu().numpy()
        hists[search] = h
        print("%s %s search=%s: cost history per rollout (rows: before, after iteration 1 ..):\n%s\nlast step lengths %s"
              % (name, "free" if lim is None else "ulim", search, h, res.alpha.cpu().numpy()))
        assert h.shape == (ITERS + 1, B) and res.cost.shape == (B,) and res.alpha.shape == (B,)
        assert (h[1:] <= h[:-1]).all()      # exact
        assert (h[-1] < h[0]).all()
        assert np.array_equal(res.cost.cpu().numpy(), h[-1])
        if lim is not None:
            u = res.u.cpu().numpy()
            assert (u >= -lim).all() and (u <= lim).all()
    # both start from the same nominal: the launch's cost and torch's agree to rounding
    assert np.allclose(hists["device"][0], hists["host"][0], rtol=1e-12)
    assert sim.last_step_kernel() == "k_rollout_search<bdf1,tape,feedback>"
    # the sim holds the tape of the (device search's) result: rollout_vjp runs, and a replay of res.u - a nominal pass alone, no gains -
    # leaves the same record and the same tape, bit for bit (the open-loop tape under the applied torques)
    q, qd = sim.get_state()
    assert np.array_equal(q, res.qtraj[:, -1].cpu().numpy()) and np.array_equal(qd, res.qdtraj[:, -1].cpu().numpy())
    rng = np.random.default_rng(3)
    gq, gqd = rng.standard_normal((B, N, sc.nr)), rng.standard_normal((B, N, sc.nr))
    after_solve = sim.rollout_vjp(N, gq, gqd)
    assert all(np.isfinite(a).all() for a in after_solve)
    qt, qdt, ua, J, alpha, _ = diff.rollout_search(sim, t["q0"], t["qd0"], res.u, None, None, None, (), None, cost=cost, h=sc.h, pscale=ps,
                                                   ulim=kw.get("ulim"))
    assert torch.equal(qt, res.qtraj) and torch.equal(qdt, res.qdtraj) and torch.equal(ua, res.u) and (alpha == 0).all()
    assert all(np.array_equal(a, b) for a, b in zip(after_solve, sim.rollout_vjp(N, gq, gqd)))
    sim.close()


@pytest.mark.gpu
def test_a_quadratic_cost_goes_through_the_device_search():
    from redmax_amd import BatchSim, ilqr
    from test_gpu_ilqr import _problem
    sc, _, t, cost = _problem()
    sim = BatchSim(sc, batch=B)
    res, hist = ilqr.solve(sim, t["q0"], t["qd0"], t["u"], cost, iters=3, h=sc.h, pscale=sc.task["pscale"], backward="device", search="device")
    h = hist.cpu().numpy()
    print("quadratic cost, search=device: cost history\n%s" % h)
    assert (h[1:] <= h[:-1]).all() and (h[-1] < h[0]).all()
    sim.close()
