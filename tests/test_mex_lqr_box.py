"""'rollout_feedback_box' and 'rollout_lqr_box' through the MEX gateway (stub), over two shards: the commands return the bits of the
ctypes calls, shaped as tests/test_mex_lqr.py shapes 'rollout_lqr' - ubar nr x nsteps x B, ulo / uhi nr elements or [], status 1 x B,
clamped nsteps x B (the bit masks as doubles)."""
import numpy as np
import pytest

import proto_lqr_backward as P
from test_gpu_rollout_lqr import B, MU, _cost, _setup, _tape
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)


@pytest.mark.gpu
def test_mex_commands_equal_the_ctypes_calls(gw):  # noqa: F811
    from redmax_amd import BatchSim
    sc, cs, N = _setup(5)
    nr, ps = sc.nr, sc.task["pscale"]
    rng = np.random.default_rng(21)
    K = -0.2 * np.tile(np.concatenate([np.eye(nr), 0.2 * np.eye(nr)]), (N, 1, 1)) + 0.02 * rng.standard_normal((N, 2 * nr, nr))
    xref = np.concatenate([np.tile(sc.getQ()[0], (N, 1)), np.zeros((N, nr))], axis=1) + 0.05 * rng.standard_normal((N, 2 * nr))
    sim = BatchSim(sc, batch=B)
    sim.set_state(cs["q0"], cs["qd0"])
    free = sim.rollout_feedback(N, sc.h, cs["u"], K=K, xref=xref, pscale=ps)
    ulo, uhi = np.quantile(free[2].reshape(-1, nr), 1 / 3, axis=0), np.quantile(free[2].reshape(-1, nr), 2 / 3, axis=0)
    fb_refs = []
    for lim in ((ulo, uhi), (ulo, None), (None, None)):
        sim.set_state(cs["q0"], cs["qd0"])
        fb_refs.append((lim, sim.rollout_feedback(N, sc.h, cs["u"], K=K, xref=xref, pscale=ps, ulim=lim, stats=True)))
    assert not np.array_equal(fb_refs[0][1][2], fb_refs[1][1][2]) and np.array_equal(fb_refs[2][1][2], free[2])
    # the sweep: the tape of the two-sided clamped rollout, its applied torques the nominal
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, ubar = sim.rollout_feedback(N, sc.h, cs["u"], K=K, xref=xref, pscale=ps, ulim=(ulo, uhi))
    dQb, dR = P.dense_cost(9300, nr, N, B=B)
    costs = [_cost(sc, dict(cs, u=ubar), qt, qdt), _cost(sc, dict(cs, u=ubar), qt, qdt, QR=(dQb, dR))]
    lqr_refs = [sim.rollout_lqr_box(N, *c, ubar, (ulo, uhi), mu=MU) for c in costs]
    one_sided = sim.rollout_lqr_box(N, *costs[0], ubar, (None, uhi), mu=MU)
    capped = sim.rollout_lqr_box(N, *costs[1], ubar, (ulo, uhi), mu=MU, max_iter=1)
    sim.close()
    assert all(r[4].any() and not r[3].any() for r in lqr_refs) and (capped[3] == 2).all()
    h = gw.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    e = np.zeros((0, 0))
    for (lo, hi), want in fb_refs:
        gw.call(0, "set", h, cs["q0"].T, cs["qd0"].T)
        q, qd, ua, st = gw.call(4, "rollout_feedback_box", h, sc.h, float(N), float(ps), cs["u"].transpose(2, 1, 0), K.transpose(2, 1, 0), xref.T,
                                e if lo is None else lo, e if hi is None else hi)
        assert q.shape == (nr, N, B)
        assert all(np.array_equal(a.transpose(2, 1, 0), w) for a, w in zip((q, qd, ua), want[:3]))
        assert np.array_equal(np.asarray(st)[:, 0], want[3]["newton_iters"]) and np.array_equal(np.asarray(st)[:, 1], want[3]["status"])
    with pytest.raises(MexError, match="ulo must be"):
        gw.call(4, "rollout_feedback_box", h, sc.h, float(N), float(ps), cs["u"].transpose(2, 1, 0), e, e, ulo[:-1], uhi)
    with pytest.raises(MexError, match="ulo > uhi at DOF 0"):
        gw.call(4, "rollout_feedback_box", h, sc.h, float(N), float(ps), cs["u"].transpose(2, 1, 0), e, e, uhi, ulo)
    gw.call(0, "set", h, cs["q0"].T, cs["qd0"].T)
    gw.call(3, "rollout_feedback_box", h, sc.h, float(N), float(ps), cs["u"].transpose(2, 1, 0), K.transpose(2, 1, 0), xref.T, ulo, uhi)
    um = ubar.transpose(2, 1, 0)

    def check(got, want):
        kff, Kg, expected, status, clamped = got
        assert kff.shape == (nr, N, B) and Kg.shape == (nr, 2 * nr, N, B) and np.asarray(clamped).shape == (N, B)
        assert np.array_equal(kff.transpose(2, 1, 0), want[0]) and np.array_equal(Kg.transpose(3, 2, 1, 0), want[1])
        assert np.array_equal(np.asarray(expected).reshape(-1), want[2]) and np.array_equal(np.asarray(status).reshape(-1), want[3])
        assert np.array_equal(np.asarray(clamped).T, want[4])

    for (clx, clu, cQ, cR), want in zip(costs, lqr_refs):
        Qm = cQ.transpose(2, 1, 0) if cQ.ndim == 3 else cQ.transpose(3, 2, 1, 0)
        check(gw.call(5, "rollout_lqr_box", h, float(N), clx.transpose(2, 1, 0), clu.transpose(2, 1, 0), Qm, cR.T, um, ulo, uhi, MU), want)
    clx, clu, cQ, cR = costs[0]
    a0 = (clx.transpose(2, 1, 0), clu.transpose(2, 1, 0), cQ.transpose(2, 1, 0), cR.T)
    check(gw.call(5, "rollout_lqr_box", h, float(N), *a0, um, e, uhi, MU), one_sided)
    clx, clu, cQ, cR = costs[1]
    check(gw.call(5, "rollout_lqr_box", h, float(N), clx.transpose(2, 1, 0), clu.transpose(2, 1, 0), cQ.transpose(3, 2, 1, 0), cR.T, um, ulo, uhi, MU, 1.0),
          capped)
    (kff,) = (gw.call(1, "rollout_lqr_box", h, float(N), *a0, um, ulo, uhi),)      # one output, the default mu = 0
    assert np.asarray(kff).shape == (nr, N, B)
    with pytest.raises(MexError, match="nsteps differs"):
        gw.call(5, "rollout_lqr_box", h, float(N - 1), a0[0][:, :-1], a0[1][:, :-1], a0[2][:, :, :-1], a0[3], um[:, :-1], ulo, uhi, MU)
    with pytest.raises(MexError, match="ubar must be"):
        gw.call(5, "rollout_lqr_box", h, float(N), *a0, um[:, :-1], ulo, uhi, MU)
    with pytest.raises(MexError, match="max_iter"):
        gw.call(5, "rollout_lqr_box", h, float(N), *a0, um, ulo, uhi, MU, -1.0)
    gw.call(0, "destroy", h)
