"""Body-to-body forces (ForcePointPoint, ForceSpringDamper, ForceCable), CPU side (tests/proto_point_forces.py):

 1. the literal body-frame blocks Km, Dm are the derivatives of fm (the reference's own ForcePointPoint.test /
    ForceSpringGeneric.test: perturb E exp(eps e_i), perturb phi; 1e-6 relative, Scene.printError's threshold);
 2. a numpy port of the reference's Newton / simLoop on the literal residual reproduces Hexpected of scenes 10, 12, 13 for
    BDF1 and SDIRK2 + BDF2 (the reference's criterion |dH| <= 1e-2, Scene.m:173);
 3. the world-frame form the HIP kernels compute equals the literal one to 1e-12 relative in g and H (the bound of
    tests/test_proto_worldframe.py), with non-zero blocks between unrelated nodes for every kind, and a cable taut and slack.

 4. on multi-DOF joints (scenes 4, 5, 6, 8 with forces added, seeds of pf.randomSceneWithForces) the literal lives on the oracle's
    lowered model; its H is pinned against central differences of its g (1e-6 relative, measured at most 9.3e-10), then the
    world-frame form is held to it (1e-12, measured at most 4.8e-15); the forces carry a tenth or more of |H| and |g|;
 5. the numpy Newton converges on every state tests/test_gpu_point_forces_edges.py uses; the restated guard of the device's diagonal
    solve (pf.lu_guard) on matrices whose elimination is known; the switching scene switches.

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


# ----------------------------------------------------------------------------- multi-DOF joints: the literal on the lowered model
# Scenes 4 (JointPlanar), 5 (JointTranslational), 6 (JointFree2D), 8 (JointUniversal) with forces added and seeds of the generator.
# The literal is pinned by central differences first; then the world-frame form is held to it.  tests/test_gpu_point_forces_edges.py
# uses the names of GPU_SMALL / GPU_BIG and the states of pf.nearInitialStates.
COMPOSITE = ["s4", "s5", "s6", "s8"]
CPU_SEEDS = ["r300", "r304", "r311", "r313"]
GPU_SMALL = pf.GPU_SMALL_SEEDS
GPU_BIG = pf.GPU_BIG_SEEDS


@pytest.mark.parametrize("name", COMPOSITE + CPU_SEEDS)
def test_composite_literal_is_pinned_and_worldframe_equals_it(oracle_lib, name):
    """1. H of the literal = central differences of its g (1e-6 relative: Scene.printError's threshold; measured at most 9.3e-10),
    2. eval_world_pf = the literal, 1e-12 in g and H, energies 1e-12 (measured at most 4.8e-15),
    3. the forces carry a tenth or more of |H| and |g| (from the reference alone),
    4. Scene.bodyTransforms (the rest lengths come from it) = the lowered model's kinematics at the initial state."""
    sc = pf.named_scene(name)
    lit = pf.Literal(oracle_lib, sc)
    m, forces = lit.m, lit.forces
    nr = sc.nr
    q0, qd0, q1, etas = pf.nearInitialStates(sc, pf.seed_of(name), 2)
    has_cable_behind_composite = False
    typ = np.asarray(sc.desc()["type"])
    for kind, pts, _, _, _ in pf.forces_of(sc.desc()):
        if kind == pf.CABLE and len(pts) >= (4 if name.startswith("r") else 3):
            for b, _ in pts:
                k = b
                while k >= 0:
                    has_cable_behind_composite |= bool(typ[k] > 2)
                    k = int(sc.desc()["parent"][k])
    assert has_cable_behind_composite
    for eta, qA, qB in etas:
        for b in range(2):
            g, H = lit.eval(q1[b], qA[b], qB[b], eta)
            sH, sg = pf.force_share(lit, q1[b], qA[b], qB[b], eta)
            assert sH >= 0.1 and sg >= 0.1, (name, b, sH, sg)
            g2, H2 = pf.eval_world_pf(m, forces, q1[b], qA[b], qB[b], eta)
            assert _rel(g2, g) <= 1e-12 and _rel(H2, H) <= 1e-12, (name, b, _rel(g2, g), _rel(H2, H))
            assert _rel(pf.eval_world_pf(m, forces, q1[b], qA[b], qB[b], eta, want_H=False), g) <= 1e-12
            assert _rel(lit.eval(q1[b], qA[b], qB[b], eta, want_H=False), g) <= 1e-14
            if b == 0:
                eps = 1e-6
                Hfd = np.zeros_like(H)
                for i in range(nr):
                    e = np.zeros(nr)
                    e[i] = eps
                    Hfd[:, i] = (lit.eval(q1[b] + e, qA[b], qB[b], eta, False) - lit.eval(q1[b] - e, qA[b], qB[b], eta, False)) / (2 * eps)
                print("%s eta=%.4g: |H - Hfd|/|H| = %.2e, force share of H %.2f, of g %.2f" % (name, eta, _rel(Hfd, H), sH, sg))
                assert _rel(Hfd, H) <= 1e-6, (name, _rel(Hfd, H))
    for b in range(2):
        T, V = lit.energy(q1[b], qd0[b])
        T2, V2 = pf.energy_world_pf(m, forces, q1[b], qd0[b])
        assert abs(T - T2) <= 1e-12 * max(abs(T), 1) and abs(V - V2) <= 1e-12 * max(abs(V), 1)
        assert V != pf.pw.energy_world(m, q1[b], qd0[b])[1]         # the forces' potential entered
    Ew, _, _ = pf.fk(m, *sc.getQ())
    for L, E in enumerate(sc.bodyTransforms()):
        assert np.abs(E - Ew[lit.node_of_body[L]]).max() <= 1e-12 * max(1.0, np.abs(E).max()), (name, L)


def test_literal_on_plain_joints_is_unmoved(oracle_lib):
    """Without a multi-DOF joint the lowered model is the listing: nodes = bodies, rows as Scene.init numbers them."""
    for name in ("10", "12", "13", "tree15"):
        sc = _scene(name)
        sc.init()
        lit = pf.Literal(oracle_lib, sc)
        assert lit.node_of_body == list(range(len(sc.bodies)))
        assert lit.idxM == [b.idxM[0] for b in sc.bodies] and (lit.nm, lit.nr) == (sc.nm, sc.nr)
        d = sc.desc()
        assert [[b for b, _ in f[1]] for f in lit.forces] == [[b for b, _ in f[1]] for f in pf.forces_of(d)]


@pytest.mark.parametrize("name", COMPOSITE + GPU_SMALL + GPU_BIG)
def test_numpy_newton_converges_on_the_gpu_test_states(oracle_lib, name):
    """The rollouts tests/test_gpu_point_forces_edges.py compares the device with: the reference's Newton on the literal converges
    on every step (6 steps, big trees 3; BDF1 and SDIRK2 + BDF2)."""
    sc = pf.named_scene(name)
    lit = pf.Literal(oracle_lib, sc)
    q0, qd0, _, _ = pf.nearInitialStates(sc, pf.seed_of(name), 2)
    for bdf in (1, 2):
        for b in range(2):
            st = pf.sim_loop(lit.eval, lit.energy, q0[b], qd0[b], sc.h, 3 if name in GPU_BIG else 6, bdf)[2]
            assert st == 0, (name, bdf, b, st)


def test_lu_guard_restatement():
    """pf.lu_guard on matrices whose elimination is known: SPD and well scaled passes; a negative pivot, a non-positive diagonal
    and a multiplier above 8 in the equilibrated matrix trip."""
    m = {"idx": [2, -1, 0, 1]}                                  # node order: reduced DOFs 2, 0, 1; one node without a DOF
    A = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.2], [0.5, 0.2, 2.0]])
    P = [2, 0, 1]
    H = np.zeros((3, 3))
    H[np.ix_(P, P)] = A
    assert 0 < pf.lu_guard(m, H) < 1 and not pf.lu_guard_trips(m, H)
    assert abs(pf.lu_guard(m, H) - max(1.0 / 4 / 3, 0.25 / 4 / 2, (0.2 - 0.125) ** 2 / (3 - 0.25) / 2)) <= 1e-15
    B = A.copy()
    B[0, 0] = -4.0
    H[np.ix_(P, P)] = B
    assert pf.lu_guard(m, H) == np.inf
    B = A.copy()
    B[1, 1] = 0.2                                               # second pivot 0.2 - 0.25 < 0
    H[np.ix_(P, P)] = B
    assert pf.lu_guard_trips(m, H)
    B = np.array([[1e-4, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 0.0, 1.0]])      # l^2 u / H_11 = 1e4 / 3
    H[np.ix_(P, P)] = B
    assert pf.lu_guard_trips(m, H)
    B[1, 1] = 2e4                                               # the same multiplier against a large diagonal: 1e4 / 2e4
    H[np.ix_(P, P)] = B
    assert abs(pf.lu_guard(m, H) - 0.5) <= 1e-15


def test_switching_scene_switches(oracle_lib):
    """Both cables of pf.switchingScene are taut, slack and taut again (or the reverse) within 20 steps, under both integrators,
    on the two states the GPU test uses."""
    sc = pf.switchingScene()
    lit = pf.Literal(oracle_lib, sc)
    q, qd = pf.switchingStates(sc)
    for bdf in (1, 2):
        for b in range(2):
            _, _, st, hist = pf.sim_loop(lit.eval, lit.energy, q[b], qd[b], sc.h, 20, bdf, history=True)
            assert st == 0
            states = pf.cable_states(lit, hist)
            assert len(states) == 2 and all(pf.switches(s) for s in states), (bdf, b, states)
