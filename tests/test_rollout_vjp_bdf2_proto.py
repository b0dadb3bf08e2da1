"""The formulas of the BDF2 rmx_rollout_vjp (rmx_rollout_tape_bdf2), pinned on the CPU before any GPU run: the numpy recursion of
tests/proto_rollout_vjp_bdf2.py against central differences of its own oracle rollout, in u, q0 and qdot0.

As tests/test_rollout_vjp_proto.py pins BDF1: the same case(), loss L = sum_k c_k.q_k + d_k.qdot_k + |q_k|^2/2, eps = 1e-5, 3 random
directions per argument, tolerance rtol 2e-5, atol 1e-6 max|ana| (the project's testGrad bound).  nsteps 4, and 1 (the SDIRK2 start
step alone) and 2 (the first BDF2 step reads q0 as its q_{k-1}).  The recursion is exact - the start step included -, so the errors
printed are central-difference noise: measured 1.0e-10 .. 3.2e-10 (du), 1.2e-9 .. 3.0e-9 (dq0), 1.1e-9 .. 9.1e-9 (dqd0) of max|ana|.
"""
import numpy as np
import pytest

import proto_rollout_vjp_bdf2 as proto
from test_gpu_adjoint_controls import _scene
from test_rollout_vjp_proto import case

EPS, NDIR = 1e-5, 3


@pytest.mark.parametrize("nsteps", [4, 1, 2])
@pytest.mark.parametrize("size", [5, "tree7"])
def test_proto_meets_central_differences(oracle_lib, size, nsteps):
    sc = _scene(size, 2)
    h, pscale = sc.h, sc.task["pscale"]
    cs = {k: v[0] for k, v in case(sc, 7, nsteps=nsteps).items()}
    ref = proto.reference(oracle_lib, sc, cs["q0"], cs["qd0"], cs["u"], h, pscale, cs["c"], cs["d"])
    assert np.isfinite(ref["du"]).all() and np.abs(ref["du"]).max() > 0

    def L(q0, qd0, u):
        qt, qdt = proto.rollout(oracle_lib, sc, q0, qd0, u, h, pscale)
        return proto.loss_and_cotangents(qt, qdt, cs["c"], cs["d"])[0]

    rng = np.random.default_rng(11)
    for name, grad in (("u", ref["du"]), ("q0", ref["dq0"]), ("qd0", ref["dqd0"])):
        dirs = rng.standard_normal((NDIR,) + grad.shape)
        num = np.empty(NDIR)
        for i, dv in enumerate(dirs):
            args = {k: cs[k] for k in ("q0", "qd0", "u")}
            num[i] = (L(**dict(args, **{name: cs[name] + EPS * dv})) - L(**dict(args, **{name: cs[name] - EPS * dv}))) / (2 * EPS)
        ana = (dirs.reshape(NDIR, -1) * grad.reshape(1, -1)).sum(axis=1)
        err = np.abs(num - ana)
        print("bdf2 proto %s nsteps %d, d/d%s: max |num - ana| / max|ana| = %.3e" % (size, nsteps, name, err.max() / np.abs(ana).max()))
        assert (err <= 2e-5 * np.abs(ana) + 1e-6 * np.abs(ana).max()).all(), (name, num, ana)


def test_proto_rollout_is_the_oracles_bdf2_rollout(oracle_lib):
    """With u = 0 the proto's own Newton and stage formulas reproduce the oracle's step_bdf2 (SDIRK2 start, then BDF2) from the scene's
    initial state: both iterate to the same solutions, the oracle to its tol 1e-9 on |g|."""
    sc = _scene(5, 2)
    q0, qd0 = sc.getQ()
    N = 4
    qt, qdt = proto.rollout(oracle_lib, sc, q0, qd0, np.zeros((N, sc.nr)), sc.h, sc.task["pscale"])
    o = oracle_lib.Oracle(sc.desc())
    o.set_state(q0, qd0)
    o.step_bdf2(sc.h, N)
    qo, qdo = o.get_state()
    eq, ed = np.linalg.norm(qt[-1] - qo) / np.linalg.norm(qo), np.linalg.norm(qdt[-1] - qdo) / np.linalg.norm(qdo)
    print("bdf2 proto rollout against step_bdf2: q %.3e qdot %.3e" % (eq, ed))
    assert eq <= 1e-9 and ed <= 1e-7


def test_vjp_is_linear_and_causal():
    """Properties of the recursion alone, on random well-conditioned blocks (N + 1 slots): linear in the cotangents, and cotangents that
    are zero behind step k give du rows behind k that are exactly zero."""
    rng = np.random.default_rng(3)
    N, nr, h, ps = 5, 4, 1e-2, 3.0
    H = rng.standard_normal((N + 1, nr, nr)) + 6 * np.eye(nr)
    M, D = rng.standard_normal((N + 1, nr, nr)), rng.standard_normal((N + 1, nr, nr))
    g1, g2, d1, d2 = (rng.standard_normal((N, nr)) for _ in range(4))
    a = proto.vjp(H, M, D, g1, d1, h, ps)
    b = proto.vjp(H, M, D, g2, d2, h, ps)
    s = proto.vjp(H, M, D, g1 + 2 * g2, d1 + 2 * d2, h, ps)
    for x, y, z in zip(a, b, s):
        assert np.allclose(x + 2 * y, z, rtol=1e-10, atol=1e-10 * np.abs(z).max())
    g1[2:], d1[2:] = 0.0, 0.0
    du, _, _ = proto.vjp(H, M, D, g1, d1, h, ps)
    assert not du[2:].any() and du[:2].any()
    # a one-step rollout is the start step alone: slots 0 (SDIRK2b) and 1 (SDIRK2a)
    du1, dq1, dqd1 = proto.vjp(H[:2], M[:2], D[:2], g2[:1], d2[:1], h, ps)
    assert du1.shape == (1, nr) and du1.any() and dq1.any() and dqd1.any()
