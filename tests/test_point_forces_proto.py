"""Body-to-body forces (ForcePointPoint, ForceSpringDamper, ForceCable), CPU side (tests/proto_point_forces.py):

 1. the literal body-frame blocks Km, Dm are the derivatives of fm (the reference's own ForcePointPoint.test /
    ForceSpringGeneric.test: perturb E exp(eps e_i), perturb phi; 1e-6 relative, Scene.printError's threshold);
 2. a numpy port of the reference's Newton / simLoop on the literal residual reproduces Hexpected of scenes 10, 12, 13 for
    BDF1 and SDIRK2 + BDF2 (the reference's criterion |dH| <= 1e-2, Scene.m:173);
 3. the world-frame form the HIP kernels compute equals the literal one to 1e-12 relative in g and H (the bound of
    tests/test_proto_worldframe.py), with non-zero blocks between unrelated nodes for every kind, and a cable taut and slack.

Deviations of the restatement from the reference's goldens, H_end - Hexpected, as measured (printed by the test; run with -s):
    scene 12  BDF1  4.0e-11 (1.8e-15 relative)   BDF2 -6.5e-10 (7.2e-14)
    scene 13  BDF1  1.3e-10 (4.2e-15)            BDF2 -1.1e-09 (3.9e-14)
    scene 10  BDF1 -2.6e-10 (2.1e-13)            BDF2 -1.4e-10 (3.4e-14)
Every one is below 1e-9 relative, so the GPU test (tests/test_gpu_point_forces.py) holds the kernels to 1e-9 relative on all six.
"""
import numpy as np
import pytest

import proto_point_forces as pf
from redmax_amd import se3
from redmax_amd.scenes import POINT_FORCE_SCENES, scenesRedMax


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _exp6(i, eps):
    """exp(eps e_i) of se(3): a rotation about / a translation along coordinate axis i % 3"""
    E = np.eye(4)
    if i < 3:
        E[:3, :3] = se3.aaToMat(np.eye(3)[i], eps)
    else:
        E[i - 3, 3] = eps
    return E


def _force(kind, rng, P):
    pts = [(k, rng.normal(size=3)) for k in range(P)]
    return (kind, pts, 10 ** rng.uniform(1, 3), 10 ** rng.uniform(0, 2), float(P) * 0.9)


@pytest.mark.parametrize("kind,P", [(pf.PP, 2), (pf.SPRING, 2), (pf.CABLE, 2), (pf.CABLE, 4)])
def test_literal_blocks_are_derivatives_of_fm(kind, P):
    rng = np.random.default_rng(100 * kind + P)
    taut = 0
    for trial in range(4):
        f = _force(kind, rng, P)
        E = [se3.transform(R=se3.aaToMat(rng.normal(size=3), rng.uniform(-2, 2)), p=rng.normal(size=3) * 2) for _ in range(P)]
        phi = [rng.normal(size=6) for _ in range(P)]
        fm, Km, Dm, V = pf.literal_blocks(f, E, phi)
        if kind == pf.CABLE and V == 0.0:
            assert not fm.any() and not Km.any() and not Dm.any()       # slack: no force, no blocks
            continue
        taut += 1
        eps = 1e-6
        Kfd = np.zeros_like(Km)
        Dfd = np.zeros_like(Dm)
        for k in range(P):
            for i in range(6):
                Ep, Em = list(E), list(E)
                Ep[k] = E[k] @ _exp6(i, eps)
                Em[k] = E[k] @ _exp6(i, -eps)
                Kfd[:, 6 * k + i] = (pf.literal_blocks(f, Ep, phi)[0] - pf.literal_blocks(f, Em, phi)[0]) / (2 * eps)
                pp, pm = [x.copy() for x in phi], [x.copy() for x in phi]
                pp[k][i] += eps
                pm[k][i] -= eps
                Dfd[:, 6 * k + i] = (pf.literal_blocks(f, E, pp)[0] - pf.literal_blocks(f, E, pm)[0]) / (2 * eps)
        assert _rel(Km, Kfd) <= 1e-6, (kind, trial, _rel(Km, Kfd))
        assert _rel(Dm, Dfd) <= 1e-6, (kind, trial, _rel(Dm, Dfd))
    assert taut >= 2


@pytest.mark.parametrize("bdf", [1, 2])
@pytest.mark.parametrize("sid", POINT_FORCE_SCENES)
def test_literal_newton_reproduces_the_goldens(oracle_lib, sid, bdf):
    sc = scenesRedMax(sid)
    sc.init()
    lit = pf.Literal(oracle_lib, sc)
    H, status = pf.golden_H(lit.eval, lit.energy, sc, bdf)
    He = sc.Hexpected[bdf - 1]
    print("scene %d BDF%d: H = %.16e, H - Hexpected = %.3e (%.2e relative), Newton status %d" % (sid, bdf, H, H - He, abs(H - He) / abs(He), status))
    assert status == 0
    assert abs(H - He) <= 1e-2                      # the reference's criterion (Scene.m:173)
    assert abs(H - He) <= 1e-9 * abs(He)            # what lets the GPU test hold the kernels to 1e-9 relative (see the module docstring)


def _scene(name):
    return pf.treeWithForces(15) if name == "tree15" else scenesRedMax(int(name))


@pytest.mark.parametrize("name", ["10", "12", "13", "tree15"])
def test_worldframe_equals_literal(oracle_lib, name):
    sc = _scene(name)
    sc.init()
    lit = pf.Literal(oracle_lib, sc)
    m, forces = lit.m, lit.forces
    rng = np.random.default_rng(17)
    nr, h = sc.nr, sc.h
    q0s, _ = sc.getQ()
    cross = {}
    taut = slack = 0
    for trial in range(6):
        q0 = q0s + rng.uniform(-0.7, 0.7, nr) * (0.1 if trial < 2 else 1.0)
        qd0 = rng.uniform(-1, 1, nr)
        q1 = q0 + h * qd0 + rng.uniform(-1e-2, 1e-2, nr)
        for eta, qA, qB in ((h, q0, q0 + h * qd0), (2 * h / 3, q0 + 1e-3 * rng.normal(size=nr), q0 + h * qd0 * 0.9)):
            g, H = lit.eval(q1, qA, qB, eta)
            g2, H2 = pf.eval_world_pf(m, forces, q1, qA, qB, eta)
            assert _rel(g2, g) <= 1e-12, (name, trial, _rel(g2, g))
            assert _rel(H2, H) <= 1e-12, (name, trial, _rel(H2, H))
            assert _rel(pf.eval_world_pf(m, forces, q1, qA, qB, eta, want_H=False), g) <= 1e-12
            for f in forces:                       # per force: entries of H between unrelated nodes; the cable's state
                n_unrel = pf.world_terms(m, [f], q1, (q1 - qA) / eta, eta)[3]
                cross[f[0]] = cross.get(f[0], 0) + n_unrel
                if f[0] == pf.CABLE:
                    V = pf.world_terms(m, [f], q1, (q1 - qA) / eta, eta, False)[2]
                    taut += V > 0
                    slack += V == 0
        T, V = lit.energy(q1, qd0)
        T2, V2 = pf.energy_world_pf(m, forces, q1, qd0)
        assert abs(T - T2) <= 1e-12 * max(abs(T), 1) and abs(V - V2) <= 1e-12 * max(abs(V), 1)
    if name == "10":
        assert cross[pf.PP] > 0                    # the loop-closing spring couples the two branches
    if name == "13":
        assert cross[pf.CABLE] > 0 and taut >= 3 and slack >= 3
    if name == "tree15":
        assert cross[pf.PP] > 0 and cross[pf.SPRING] > 0 and cross[pf.CABLE] > 0 and taut >= 1
