"""Body-to-body forces on the device (ForcePointPoint, ForceSpringDamper, ForceCable; the kernels around csrc/rmx_pf.h) against
the literal restatement of tests/proto_point_forces.py (the oracle's force-free g0, H0, J, dJ/dq plus the reference's body-frame
fm, Km, Dm blocks) and a numpy port of the reference's Newton / simLoop on it.

Tolerances: those of tests/test_gpu_parity.py's header -
  single evaluation  : |dg|/|g| <= 1e-11, |dH|_F/|H|_F <= 1e-11
  single step        : |dq| <= 1e-11 |q| + 1e-10, |dqdot| <= 1e-9 |qdot| + 1e-8
  20-step rollout    : |dq|/|q| <= 1e-8 per trajectory
  energies           : 1e-12 relative (tests/test_proto_worldframe.py)
  goldens            : the reference's criterion |H_end - Hexpected| <= 1e-2 AND 1e-9 relative.  The tight bound is the existing KATs'
                       because the CPU restatement itself meets it on all six cases (tests/test_point_forces_proto.py, measured
                       H_end - Hexpected: scene 12 4.0e-11 / -6.5e-10, scene 13 1.3e-10 / -1.1e-09, scene 10 -2.6e-10 / -1.4e-10 for
                       BDF1 / BDF2, at most 2.1e-13 relative).
"""
import numpy as np
import pytest

import proto_point_forces as pf
from redmax_amd.scenes import POINT_FORCE_SCENES, sceneChain, sceneChainGround, sceneChainSprings, scenesRedMax, syntheticStates

pytestmark = pytest.mark.gpu

# amplitude of the synthetic states per scene: the largest of 0.1 (the benchmark's), 0.02 at which the numpy port of the reference's
# own Newton converges on every step of every trajectory used here (scene 10's loop is closed by a 1e7 spring)
AMP = {"10": 0.02}


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _close(a, b, rtol, atol):
    return np.linalg.norm(a - b) <= rtol * np.linalg.norm(b) + atol


def _scene(name):
    if name == "chainsprings32":
        return sceneChainSprings(32)
    if name.startswith("tree"):
        return pf.treeWithForces(int(name[4:]))
    return scenesRedMax(int(name))


def _states(sc, name, B):
    a = AMP.get(name, 0.1)
    q, qd = syntheticStates(sc.nr, B, sq=a, sv=a)
    q[0], qd[0] = sc.getQ()                                  # trajectory 0 = the scene's own initial state
    return q, qd


@pytest.mark.parametrize("name", ["10", "12", "13", "chainsprings32", "tree48"])
def test_eval_matches_literal(oracle_lib, name):
    """rmx_eval (g, H; with and without want_H) vs the literal assembly at random states, BDF1- and BDF2-style eta."""
    from redmax_amd import BatchSim
    sc = _scene(name)
    sc.init()
    lit = pf.Literal(oracle_lib, sc)
    B = 4
    rng = np.random.default_rng(7)
    nr, h = sc.nr, sc.h
    q0s, _ = sc.getQ()
    q0 = q0s[None, :] + rng.uniform(-0.7, 0.7, (B, nr)) * np.array([0.05, 0.3, 1.0, 1.0])[:, None]
    qd0 = rng.uniform(-1, 1, (B, nr))
    q1 = q0 + h * qd0 + rng.uniform(-1e-2, 1e-2, (B, nr))
    sim = BatchSim(sc, batch=B)
    cross = 0
    for eta, qA, qB in ((h, q0, q0 + h * qd0), (2 * h / 3, q0 + 1e-3 * rng.normal(size=(B, nr)), q0 + 0.9 * h * qd0)):
        g, H = sim.eval_residual(q1, qA, qB, eta)
        g_only = sim.eval_residual(q1, qA, qB, eta, want_H=False)
        for b in range(B):
            go, Ho = lit.eval(q1[b], qA[b], qB[b], eta)
            print("%s eta=%.4g b=%d: |dg|/|g| = %.2e, |dH|/|H| = %.2e" % (name, eta, b, _rel(g[b], go), _rel(H[b], Ho)))
            assert _rel(g[b], go) <= 1e-11, (name, b, _rel(g[b], go))
            assert _rel(H[b], Ho) <= 1e-11, (name, b, _rel(H[b], Ho))
            assert _rel(g_only[b], go) <= 1e-11
            cross += pf.world_terms(lit.m, lit.forces, q1[b], (q1[b] - qA[b]) / eta, eta)[3]
    if name in ("10", "13", "tree48"):
        assert cross > 0                                     # entries of H between unrelated nodes were exercised


@pytest.mark.parametrize("bdf", [1, 2])
@pytest.mark.parametrize("sid", POINT_FORCE_SCENES)
def test_reference_goldens(sid, bdf):
    """driverRedMaxBDF1/2(sid, true): the reference's own known answers (scenesRedMax.m:264-265, 314-315, 340-341)."""
    from redmax_amd import driverRedMaxBDF1, driverRedMaxBDF2
    scene, H, passed = (driverRedMaxBDF1 if bdf == 1 else driverRedMaxBDF2)(sid, True, 0, False)
    He = scene.Hexpected[bdf - 1]
    print("scene %d BDF%d: H = %.16e, H - Hexpected = %.3e (%.2e relative), status %d, %d Newton iterations" % (
        sid, bdf, H, H - He, abs(H - He) / abs(He), scene.solverInfo["status"], scene.solverInfo["newton_iters"]))
    assert passed is True
    assert scene.solverInfo["status"] & 15 == 0
    assert abs(H - He) <= 1e-9 * abs(He)


@pytest.mark.parametrize("bdf", [1, 2])
@pytest.mark.parametrize("name", ["10", "12", "13", "chainsprings32", "tree40"])
def test_steps_match_numpy_newton(oracle_lib, name, bdf):
    """One step and a 20-step rollout (batch of 4) vs the numpy port of the reference's Newton on the literal residual (one
    rollout per trajectory: its first step is the single step); rmx_energy and the per-step record of T, V vs the restatement."""
    from redmax_amd import BatchSim
    sc = _scene(name)
    sc.init()
    lit = pf.Literal(oracle_lib, sc)
    B = 4
    q, qd = _states(sc, name, B)
    ref = []
    for b in range(B):
        qo, qdo, st, hist = pf.sim_loop(lit.eval, lit.energy, q[b], qd[b], sc.h, 20, bdf, history=True)
        assert st == 0                                       # the reference algorithm itself converged on this state
        ref.append({1: hist[0][:2], 20: (qo, qdo)})
    for nsteps in (1, 20):
        sim = BatchSim(sc, batch=B)
        sim.set_state(q, qd)
        out = (sim.step_bdf1 if bdf == 1 else sim.step_bdf2)(nsteps, h=sc.h, stats=True, history=True)
        qg, qdg = sim.get_state()
        assert (out["status"] & 15 == 0).all(), out["status"]
        Tg, Vg = sim.energy()
        for b in range(B):
            qo, qdo = ref[b][nsteps]
            print("%s BDF%d %d steps b=%d: |dq|/|q| = %.2e, |dqdot|/|qdot| = %.2e, status %d" % (
                name, bdf, nsteps, b, _rel(qg[b], qo), _rel(qdg[b], qdo), out["status"][b]))
            if nsteps == 1:
                assert _close(qg[b], qo, 1e-11, 1e-10), (name, b, _rel(qg[b], qo))
                assert _close(qdg[b], qdo, 1e-9, 1e-8), (name, b, _rel(qdg[b], qdo))
            else:
                assert _rel(qg[b], qo) <= 1e-8, (name, b, _rel(qg[b], qo))
            # energies at the device's own end state, and the per-step record at its own states (the last one: the end state)
            T, V = lit.energy(qg[b], qdg[b])
            print("   energy: dT = %.2e, dV = %.2e; history: dT = %.2e, dV = %.2e (T %.6e, V %.6e)" % (
                Tg[b] - T, Vg[b] - V, out["T"][-1, b] - T, out["V"][-1, b] - V, T, V))
            assert abs(Tg[b] - T) <= 1e-12 * max(abs(T), 1) and abs(Vg[b] - V) <= 1e-12 * max(abs(V), 1), (name, b, Tg[b] - T, Vg[b] - V)
            assert abs(out["T"][-1, b] - T) <= 1e-12 * max(abs(T), 1)
            assert abs(out["V"][-1, b] - V) <= 1e-12 * max(abs(V), 1)


@pytest.mark.parametrize("name", ["12", "13", "chainsprings32"])
def test_energy_matches_restatement(oracle_lib, name):
    from redmax_amd import BatchSim
    sc = _scene(name)
    sc.init()
    lit = pf.Literal(oracle_lib, sc)
    B = 6
    rng = np.random.default_rng(3)
    q0s, _ = sc.getQ()
    q = q0s[None, :] + rng.uniform(-0.7, 0.7, (B, sc.nr))
    qd = rng.uniform(-2, 2, (B, sc.nr))
    sim = BatchSim(sc, batch=B)
    sim.set_state(q, qd)
    T, V = sim.energy()
    nforce = 0
    for b in range(B):
        To, Vo = lit.energy(q[b], qd[b])
        assert abs(T[b] - To) <= 1e-12 * max(abs(To), 1) and abs(V[b] - Vo) <= 1e-12 * max(abs(Vo), 1), (name, b, T[b] - To, V[b] - Vo)
        nforce += Vo != pf.pw.energy_world(lit.m, q[b], qd[b])[1]
    assert nforce >= 3                                       # the forces' potential really entered


@pytest.mark.parametrize("name,bdf", [("13", 1), ("chainsprings32", 2), ("tree48", 1)])
def test_batch_independence(name, bdf):
    """Rollout b of a batch of 64 equals the same state run alone, bit for bit."""
    from redmax_amd import BatchSim
    sc = _scene(name)
    sc.init()
    B = 64
    q, qd = _states(sc, name, B)
    sim = BatchSim(sc, batch=B)
    sim.set_state(q, qd)
    (sim.step_bdf1 if bdf == 1 else sim.step_bdf2)(10, h=sc.h)
    qg, qdg = sim.get_state()
    for b in (0, 17, 63):
        one = BatchSim(sc, batch=1)
        one.set_state(q[b:b + 1], qd[b:b + 1])
        (one.step_bdf1 if bdf == 1 else one.step_bdf2)(10, h=sc.h)
        q1, qd1 = one.get_state()
        assert np.array_equal(q1[0], qg[b]) and np.array_equal(qd1[0], qdg[b]), (name, b)


def test_step_kernel_and_plain_models_unmoved():
    """A model with point forces runs the kernels of rmx_pf.h; the same chain without them reaches the kernel it always did."""
    from redmax_amd import BatchSim
    sc = sceneChainSprings(32)
    sc.init()
    sim = BatchSim(sc, batch=2)
    sim.set_state(*_states(sc, "chainsprings32", 2))
    sim.step_bdf1(2, h=sc.h)
    assert sim.last_step_kernel().startswith("k_step_pf<32")
    plain = sceneChain(32)
    plain.init()
    sim = BatchSim(plain, batch=2)
    sim.set_state(*syntheticStates(plain.nr, 2))
    sim.step_bdf1(2, h=plain.h)
    assert not sim.last_step_kernel().startswith("k_step_pf")


def test_refusals():
    """What is refused rather than built: every call names its reason (RMX_E_INVALID)."""
    from redmax_amd import BatchSim, GroupSim, RedMaxHipError
    from redmax_amd.redmax import ForceCable, ForcePointPoint
    sc = scenesRedMax(12)
    sc.init()
    sim = BatchSim(sc, batch=2)
    q, qd = _states(sc, "12", 2)
    sim.set_state(q, qd)
    with pytest.raises(RedMaxHipError, match="point forces"):
        sim.step_euler(1, sc.h)
    with pytest.raises(RedMaxHipError, match="point forces"):
        sim.eval_mfd(q, qd)
    with pytest.raises(RedMaxHipError, match="point forces"):
        sim.compute_values(q, qd)
    task = {"body": 1, "xlocal": [5.0, 0, 0], "xtarget": [10.0, 0, -10.0], "step": 2, "pscale": 1e5, "wreg": 1e-2, "wpos": 1e2}
    with pytest.raises(RedMaxHipError, match="point forces"):
        sim.adjoint_bdf1(2, sc.h, task, np.zeros((2, sc.nr)))
    with pytest.raises(RedMaxHipError, match="point forces"):
        GroupSim(sc, batch=2)
    # more than 64 nodes
    big = sceneChain(70)
    big.forces = [ForcePointPoint(big.bodies[3], [0, 0, 0], big.bodies[40], [0, 0, 0])]
    big.init()
    with pytest.raises(RedMaxHipError, match="at most 64 nodes"):
        BatchSim(big, batch=1)
    # together with ForceGroundCuboid
    mix = sceneChainGround(6, ground_z=-1.0)
    mix.forces.append(ForcePointPoint(mix.bodies[0], [0, 0, 0], mix.bodies[4], [0, 0, 0]))
    mix.init()
    with pytest.raises(RedMaxHipError, match="ForceGroundCuboid"):
        BatchSim(mix, batch=1)
    # the limits
    many = sceneChain(8)
    many.forces = [ForcePointPoint(many.bodies[0], [0, 0, 0], many.bodies[5], [0, 0, 1]) for _ in range(33)]
    many.init()
    with pytest.raises(RedMaxHipError, match="RMX_PF_MAX_FORCES"):
        BatchSim(many, batch=1)
    longc = sceneChain(8)
    c = ForceCable()
    for k in range(9):
        c.addBodyPoint(longc.bodies[k % 8], [0, 0, 1.0 + k])
    longc.forces = [c]
    longc.init()
    with pytest.raises(RedMaxHipError, match="RMX_PF_MAX_POINTS"):
        BatchSim(longc, batch=1)
    # Euler-chart joints
    sph = scenesRedMax(7)
    sph.forces = [ForcePointPoint(None, [0, 0, 0], sph.bodies[-1], [0, 0, 0])]
    with pytest.raises(NotImplementedError, match="JointSpherical"):
        sph.init()
