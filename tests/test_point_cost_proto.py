"""tests/proto_point_cost.py against itself and the oracle, on the CPU: the Jacobian of a body point formed from the world screws on
its path equals the oracle's body Jacobian pushed to the point; lx and gq meet central differences of the proto's own value and
positions; Qout - Q is sum w Jp'Jp of the explicit Jacobian and positive semi-definite.

Scenes: the 5-chain, the 7-joint tree, "fixed" of test_rollout_feedback_proto (nodes without a DOF inside the tree) and
sceneTree(15) (a branching tree with fixed joints).

Tolerances.  Two float64 evaluations of one Jacobian: 64 eps of its largest entry.  Central differences with step e = 1e-6 of a
smooth function of size one carry e^2 |f'''| + eps |f| / e = 1e-12 + 2e-10: rtol 1e-7 on the largest entry of the gradient.
"""
import numpy as np
import pytest

import proto_point_cost as P
import proto_worldframe as pw
from test_rollout_feedback_proto import scene as _scene_or_fixed

EPS = np.finfo(np.float64).eps
SIZES = [5, "tree7", "fixed", "tree15"]
_CACHE = {}


def _scene(size):
    if size not in _CACHE:
        if size == "tree15":
            from redmax_amd.scenes import sceneTree
            sc = sceneTree(15)
            sc.init()
        else:
            sc = _scene_or_fixed(size, 1)
        _CACHE[size] = (sc, pw.build_model(sc.desc()))
    return _CACHE[size]


def terms_of(m, N):
    """The terms of the tests, for a record of N >= 3 steps: two on one step, two sharing body and step, one on the root body, one on
    an inner body, off-axis local points; step 2 owns no term."""
    n = m["n"]
    tip, inner = n - 1, max(1, n // 2)
    return [dict(body=tip, xlocal=[0.7, 0.2, -0.3], step=1, wpos=2.0), dict(body=inner, xlocal=[0.1, -0.4, 0.25], step=1, wpos=0.5),
            dict(body=tip, xlocal=[0.5, 0.0, 0.0], step=3, wpos=1.5), dict(body=tip, xlocal=[-0.2, 0.3, 0.1], step=3, wpos=0.75),
            dict(body=0, xlocal=[0.3, 0.1, 0.2], step=N, wpos=3.0)]


def _record(sc, seed, N):
    rng = np.random.default_rng(seed)
    q0, qd0 = sc.getQ()
    return q0[None] + 0.1 * rng.standard_normal((N, sc.nr)), qd0[None] + 0.3 * rng.standard_normal((N, sc.nr)), rng


def _dense(rng, N, nr):
    Q = rng.standard_normal((N, 2 * nr, 2 * nr))
    return Q + Q.transpose(0, 2, 1), rng.standard_normal((N, 2 * nr))


@pytest.mark.parametrize("size", SIZES)
def test_the_two_jacobians_agree(oracle_lib, size):
    sc, m = _scene(size)
    q, _, _ = _record(sc, 3, 1)
    orc = oracle_lib.Oracle(sc.desc())
    idxM = [b.idxM[0] for b in sc.bodies]
    kin = P.kinematics(m, q[0])
    for t in terms_of(m, 4):
        pt = P.point(kin, t["body"], t["xlocal"])
        Js, Jb = P.jac_screw(m, kin, t["body"], pt), P.jac_body(orc, idxM, kin, t["body"], t["xlocal"], q[0])
        err = np.max(np.abs(Js - Jb)) / np.max(np.abs(Jb))
        print("%s body %d: |J_screw - J_body| / |J| = %.3e" % (size, t["body"], err))
        assert err <= 64 * EPS
        off = [m["idx"][j] for j in range(m["n"]) if m["idx"][j] >= 0 and not m["anc"][j, t["body"]]]
        assert (Js[:, off] == 0.0).all() and np.max(np.abs(Jb[:, off]), initial=0.0) <= 64 * EPS * np.max(np.abs(Jb))


@pytest.mark.parametrize("size", SIZES)
def test_the_longdouble_frames_are_the_float64_frames(size):
    sc, m = _scene(size)
    q, _, _ = _record(sc, 5, 1)
    for a, b in zip(P.kinematics(m, q[0]), P.kinematics(m, q[0], np.longdouble)):
        assert b.dtype == np.longdouble
        assert np.max(np.abs(a - b)) <= 64 * EPS * max(1.0, float(np.max(np.abs(b))))


@pytest.mark.parametrize("size", SIZES)
def test_lx_and_gq_meet_central_differences(size):
    sc, m = _scene(size)
    N, nr = 4, sc.nr
    q, qd, rng = _record(sc, 7, N)
    terms = terms_of(m, N)
    Q, xg = _dense(rng, N, nr)
    xt = rng.standard_normal((len(terms), 3))
    gx = rng.standard_normal((len(terms), 3))
    out = P.cost(m, q, qd, Q, xg, terms, xt)
    gq = P.pullback(m, q, terms, gx)
    e = 1e-6
    for _ in range(3):
        dq, dqd = rng.standard_normal(q.shape), rng.standard_normal(q.shape)
        fp = P.cost(m, q + e * dq, qd + e * dqd, Q, xg, terms, xt)["Jk"].sum()
        fm = P.cost(m, q - e * dq, qd - e * dqd, Q, xg, terms, xt)["Jk"].sum()
        num, ana = (fp - fm) / (2 * e), np.sum(out["lx"][:, :nr] * dq) + np.sum(out["lx"][:, nr:] * dqd)
        print("%s lx: numeric %.12e analytic %.12e" % (size, num, ana))
        assert abs(num - ana) <= 1e-7 * max(abs(ana), np.max(np.abs(out["lx"])))
        xp, xm = P.points(m, q + e * dq, terms), P.points(m, q - e * dq, terms)
        num, ana = np.sum(gx * (xp - xm)) / (2 * e), np.sum(gq * dq)
        print("%s gq: numeric %.12e analytic %.12e" % (size, num, ana))
        assert abs(num - ana) <= 1e-7 * max(abs(ana), np.max(np.abs(gq)))
    assert (gq[1] == 0.0).all()      # step 2 owns no term


@pytest.mark.parametrize("size", SIZES)
def test_the_gauss_newton_block(size):
    sc, m = _scene(size)
    N, nr = 4, sc.nr
    q, qd, rng = _record(sc, 9, N)
    terms = terms_of(m, N)
    Q, xg = _dense(rng, N, nr)
    xt = rng.standard_normal((len(terms), 3))
    out = P.cost(m, q, qd, Q, xg, terms, xt)
    D = out["Q"] - Q
    assert (D[:, nr:, :] == 0.0).all() and (D[:, :, nr:] == 0.0).all() and (D[1] == 0.0).all()
    for k, own in enumerate(P.by_step(terms, N)):
        G = np.zeros((nr, nr))
        kin = P.kinematics(m, q[k])
        for i in own:
            J = P.jac_screw(m, kin, terms[i]["body"], P.point(kin, terms[i]["body"], terms[i]["xlocal"]))
            G += terms[i]["wpos"] * J.T @ J
        scale = max(np.max(np.abs(out["Q"][k])), 1.0)
        assert np.max(np.abs(D[k, :nr, :nr] - G)) <= 64 * EPS * scale
        assert np.linalg.eigvalsh(0.5 * (G + G.T)).min() >= -64 * EPS * scale
    # without a joint-space part the tables are the terms' alone
    bare = P.cost(m, q, qd, None, None, terms, xt)
    assert np.allclose(bare["Q"], D, rtol=0, atol=64 * EPS * np.max(np.abs(out["Q"])))
