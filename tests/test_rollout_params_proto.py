"""The rule behind rmx_rollout_vjp_params, pinned on the CPU before any GPU run: the numpy proto of tests/proto_rollout_params.py
(dL/dtheta = - sum over the slots of z' dg/dtheta, dg/dtheta by linearity on the oracle) against central differences of the oracle's
own rollout loss on perturbed models, BDF1 and BDF2.

As tests/test_rollout_vjp_proto.py pins the input gradients: the same case(), loss L = sum_k c_k.q_k + d_k.qdot_k + |q_k|^2/2,
eps = 1e-5, tolerance rtol 2e-5, atol 1e-6 max|ana| (the project's testGrad bound).  One random direction per parameter group; the
direction is scaled to the group's own magnitude (max(1, max|theta|)), so that eps = 1e-5 is a relative step for stiffness (1e4) as
it is an absolute one for q0: an absolute 1e-5 on a stiffness of 1e4 moves the loss by less than the oracle's Newton tolerance.
"""
import numpy as np
import pytest

import proto_rollout_params as pp
from test_gpu_adjoint_controls import _scene
from test_rollout_vjp_proto import EPS, NSTEPS, case

_CACHE = {}


def _ref(orc, size, integ):
    key = (size, integ)
    if key not in _CACHE:
        sc = _scene(size, integ)
        cs = {k: v[0] for k, v in case(sc, 7, nsteps=NSTEPS).items()}
        ref = pp.reference(orc, sc, cs["q0"], cs["qd0"], cs["u"], sc.h, sc.task["pscale"], cs["c"], cs["d"], integ)
        _CACHE[key] = (sc, cs, ref)
    return _CACHE[key]


def directions(vals, seed):
    """One random direction per group, scaled to the group's magnitude."""
    rng = np.random.default_rng(seed)
    return {g: max(1.0, float(np.abs(vals[g]).max())) * rng.standard_normal(vals[g].shape) for g in pp.GROUPS}


@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, "tree7"])
def test_proto_meets_central_differences(oracle_lib, size, integ):
    sc, cs, ref = _ref(oracle_lib, size, integ)
    h, pscale = sc.h, sc.task["pscale"]
    dirs = directions(pp.values(oracle_lib, sc), 11)
    for group in pp.GROUPS:
        grad, dv = ref["grads"][group], dirs[group]
        assert np.isfinite(grad).all() and np.abs(grad).max() > 0, group
        Lp, Lm = (pp.loss(oracle_lib, pp.perturbed(oracle_lib, sc, group, s * EPS * dv), cs["q0"], cs["qd0"], cs["u"], h, pscale,
                          cs["c"], cs["d"], integ) for s in (1.0, -1.0))
        num, ana = (Lp - Lm) / (2 * EPS), float((grad * dv).sum())
        print("params proto %s integ %d, d/d%s: |num - ana| / |ana| = %.3e" % (size, integ, group, abs(num - ana) / abs(ana)))
        assert abs(num - ana) <= 2e-5 * abs(ana) + 1e-6 * abs(ana), (group, num, ana)


@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, "tree7"])
def test_residual_is_linear_in_every_group(oracle_lib, size, integ):
    """g(theta + 2 delta) - g(theta) = 2 (g(theta + delta) - g(theta)) to 1e-12 of the larger side: what makes the proto exact."""
    sc, cs, ref = _ref(oracle_lib, size, integ)
    dirs = directions(pp.values(oracle_lib, sc), 13)
    g0 = pp.residuals(oracle_lib, sc, ref["slots"])
    for group in pp.GROUPS:
        d1 = pp.dg(oracle_lib, sc, ref["slots"], group, dirs[group], g0)
        d2 = pp.dg(oracle_lib, sc, ref["slots"], group, 2.0 * dirs[group], g0)
        err = np.abs(d2 - 2.0 * d1).max() / np.abs(d2).max()
        print("params proto %s integ %d: non-linearity of g in %s %.3e" % (size, integ, group, err))
        assert np.abs(d2).max() > 0 and err <= 1e-12, (group, err)


@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, "tree7"])
def test_qrest_gradient_is_stiffness_times_the_summed_control_gradient(oracle_lib, size, integ):
    """qRest enters g only through the joint torque k (qRest - q), beside pscale u: dL/dqRest_j = (k_j / pscale) sum_k du_k[j], for both
    integrators (under BDF2 du_1 already carries za + zb)."""
    sc, cs, ref = _ref(oracle_lib, size, integ)
    k = pp.values(oracle_lib, sc)["stiffness"]
    want = k / sc.task["pscale"] * ref["du"].sum(axis=0)
    err = np.linalg.norm(ref["grads"]["qrest"] - want) / np.linalg.norm(want)
    print("params proto %s integ %d: qrest identity %.3e" % (size, integ, err))
    assert np.linalg.norm(want) > 0 and err <= 1e-10
