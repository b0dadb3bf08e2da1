"""The formulas of rmx_rollout_vjp, pinned on the CPU before any GPU run: the numpy recursion of tests/proto_rollout_vjp.py against
central differences of the oracle's own rollout, in u, q0 and qdot0.

Loss: L = sum_k c_k.q_k + d_k.qdot_k + |q_k|^2/2 with random c, d; eps = 1e-5, 3 random directions per argument; tolerance
rtol 2e-5, atol 1e-6 max|ana| - the project's testGrad bound (tests/test_gpu_adjoint_controls.py).
"""
import numpy as np
import pytest

import proto_rollout_vjp as proto
from test_gpu_adjoint_controls import _scene

NSTEPS, EPS, NDIR = 4, 1e-5, 3


def case(sc, seed, nsteps=NSTEPS, B=1):
    """Inputs of the loss for B rollouts of a scene: dict(q0, qd0, u, c, d), each with a leading [B]."""
    rng = np.random.default_rng(seed)
    q0, qd0 = sc.getQ()
    return dict(q0=q0[None] + 0.05 * rng.standard_normal((B, sc.nr)), qd0=qd0[None] + 0.2 * rng.standard_normal((B, sc.nr)),
                u=0.1 * rng.standard_normal((B, nsteps, sc.nr)), c=rng.standard_normal((B, nsteps, sc.nr)),
                d=rng.standard_normal((B, nsteps, sc.nr)))


@pytest.mark.parametrize("size", [5, "tree7"])
def test_proto_meets_central_differences(oracle_lib, size):
    sc = _scene(size, 1)
    h, pscale = sc.h, sc.task["pscale"]
    cs = {k: v[0] for k, v in case(sc, 7).items()}
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
        print("proto %s, d/d%s: max |num - ana| / max|ana| = %.3e" % (size, name, err.max() / np.abs(ana).max()))
        assert (err <= 2e-5 * np.abs(ana) + 1e-6 * np.abs(ana).max()).all(), (name, num, ana)


def test_vjp_is_linear_and_causal():
    """Properties of the recursion alone, on random well-conditioned blocks: linear in the cotangents, and cotangents that are zero
    behind step k give du rows behind k that are zero."""
    rng = np.random.default_rng(3)
    N, nr, h, ps = 5, 4, 1e-2, 3.0
    H = rng.standard_normal((N, nr, nr)) + 6 * np.eye(nr)
    M, D = rng.standard_normal((N, nr, nr)), rng.standard_normal((N, nr, nr))
    g1, g2, d1, d2 = (rng.standard_normal((N, nr)) for _ in range(4))
    a = proto.vjp(H, M, D, g1, d1, h, ps)
    b = proto.vjp(H, M, D, g2, d2, h, ps)
    s = proto.vjp(H, M, D, g1 + 2 * g2, d1 + 2 * d2, h, ps)
    for x, y, z in zip(a, b, s):
        assert np.allclose(x + 2 * y, z, rtol=1e-10, atol=1e-10 * np.abs(z).max())
    g1[2:], d1[2:] = 0.0, 0.0
    du, _, _ = proto.vjp(H, M, D, g1, d1, h, ps)
    assert not du[2:].any() and du[:2].any()
