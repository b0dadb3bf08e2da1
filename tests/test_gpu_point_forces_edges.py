"""Body-to-body forces on the device where tests/test_gpu_point_forces.py does not reach: multi-DOF joints (a body's listing index is
not its node, massless nodes sit in every ancestor mask), every padded size with n = NP and n = NP + 1, the force table at its
limits, cables that switch within a rollout, the solve policy of newton_pf (guard trips, the hold, lu_mode 1) and batch
independence on a tree with multi-DOF joints.  Every comparison is with the literal restatement of tests/proto_point_forces.py
(pinned against central differences in tests/test_point_forces_proto.py) or the numpy port of the reference's Newton on it; the two
stated bit-identity checks (batch independence, a slack cable under a doubled stiffness) compare the device with itself.

The forces are stiff on purpose: in every generated scene they carry a tenth or more of |H|_F and of |g| (asserted here from the
reference alone), so a relative error of the force block shows in the bound on the whole of H.

Tolerances: those of tests/test_gpu_point_forces.py's header -
  single evaluation  : |dg|/|g| <= 1e-11, |dH|_F/|H|_F <= 1e-11
  single step        : |dq| <= 1e-11 |q| + 1e-10, |dqdot| <= 1e-9 |qdot| + 1e-8
  rollouts           : |dq|/|q| <= 1e-8 per trajectory
  energies           : 1e-12 relative

Measured on an MI355X (worst over the two states, BDF1 and BDF2; rollouts: 6 steps, big trees and sizes 3, limits 1):
  case            |dg|/|g|  |dH|/|H|   rollout |dq|/|q|  |dqdot|/|qdot|   energies (T, V relative)
  s4 s5 s6 s8     2.5e-15   2.4e-15    6.6e-15           4.4e-13          6.2e-16  1.5e-15
  r300            3.2e-15   1.0e-15    4.1e-15           8.4e-15          8.9e-16  4.0e-16
  r302            7.7e-15   1.0e-15    2.9e-14           4.5e-14          1.9e-15  1.0e-15
  r304            8.0e-15   2.3e-15    5.6e-15           7.4e-15          6.3e-16  3.5e-16
  r307            4.4e-15   9.3e-16    3.1e-14           1.5e-13          1.7e-15  1.5e-15
  r309            1.1e-14   9.1e-16    1.7e-14           2.1e-14          8.3e-16  6.7e-16
  r311            7.0e-15   1.1e-15    7.5e-15           2.5e-14          1.1e-15  2.2e-16
  r313            1.5e-14   8.2e-16    1.0e-14           1.2e-14          8.5e-16  1.2e-15
  r317            9.4e-15   1.4e-15    4.4e-15           1.3e-14          6.2e-16  2.7e-15
  R401 (45 nodes) 1.9e-14   1.3e-15    4.4e-15           7.6e-15          1.0e-15  < 1e-16
  R403 (52 nodes) 5.5e-15   5.9e-16    7.9e-15           8.9e-15          2.4e-16  1.6e-15
  n = 2 .. 17     1.3e-14   1.2e-15    8.6e-14           8.5e-14          3.2e-15  8.0e-15
  n = 32          4.7e-15   1.8e-15    4.2e-14           7.1e-14          3.8e-16  7.7e-15
  n = 33          3.2e-15   1.2e-15    1.4e-13           2.6e-13          1.3e-16  2.1e-15
  n = 64          4.0e-15   2.0e-15    3.7e-14           1.1e-13          3.7e-16  1.3e-14
  32 forces       5.2e-15   1.7e-15    1.8e-15           4.2e-15          2.0e-15  1.8e-15
  128 points      1.6e-15   2.1e-15    4.3e-15           5.4e-15          2.0e-15  2.8e-15
  one-body spring |g - g0|/|g| 1.0e-15, |H - Hlit|/|H| 1.8e-15 (the literal's own share of H: 9e-17)
  switching       worst per-step |dq|/|q| 7.7e-14 (BDF1), 7.3e-14 (BDF2); slack cable |dg|/|g| 8.2e-16, |dH|/|H| 9.2e-17
Every random tree meets the 1e-11 of the evaluation with three decades to spare: the bound was not raised for any seed.
Guard: RMX_ST_PIVOTED on r307 (all four rollouts), r309 and R403 (BDF1), s6, n = 33 - exactly where the restatement trips.

What these tests found.  Before the fix that came with them, k_step_pf<64, BDF2> did not converge on R403 and on the full 64-node
tree (status 2 after 10 nr iterations per solve, |dq|/|q| 2.9e-6 and 4.3e-4 after 3 steps, where the reference takes 3 to 4
iterations) and needed two extra iterations per step on R401 (2.3e-11); with lu_mode = 1 all three matched to 1e-14.  The cause
was in the guarded 64-row solve as compiled into that kernel: a spill reload (a VALU write) directly in front of a row-broadcast
FMA, whose DPP read then returned the register's old high word - redmax_amd/csrc/rmx_device.h, RMX_DPP_SETTLE.  With the weak
forces of tests/test_gpu_point_forces.py a slightly wrong Newton step only costs an iteration, which no test counted.
"""
import functools

import numpy as np
import pytest

import proto_point_forces as pf

pytestmark = pytest.mark.gpu

COMPOSITE = ["s4", "s5", "s6", "s8"]
SMALL = pf.GPU_SMALL_SEEDS
BIG = pf.GPU_BIG_SEEDS


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _close(a, b, rtol, atol):
    return np.linalg.norm(a - b) <= rtol * np.linalg.norm(b) + atol


def _np_of(nodes):
    return next(p for p in (4, 8, 16, 32, 64) if p >= nodes)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Scene, literal and states of a named case - built once, shared by the tests, never changed."""
    from oracle import oracle as orc
    orc.build()
    if name.startswith("n"):
        sc = pf.sizedSceneWithForces(int(name[1:]))
        states = pf.sizedStates(sc, int(name[1:]))
    elif name.startswith("lim:"):
        sc = pf.limitScene(name[4:])
        states = pf.nearInitialStates(sc, 5, 2)
    else:
        sc = pf.named_scene(name)
        states = pf.nearInitialStates(sc, pf.seed_of(name), 2)
    return sc, pf.Literal(orc, sc), states


@functools.lru_cache(maxsize=None)
def _reference_rollout(name, bdf, nsteps, b):
    """The numpy Newton on the literal from state b of the case, with the restated guard's ratio of every linear solve."""
    sc, lit, (q0, qd0, _, _) = _case(name)
    return pf.guard_trace(lit, q0[b], qd0[b], sc.h, nsteps, bdf)


def _check_eval(name, sim, generated):
    """rmx_eval (with and without want_H) at a BDF1-style and a BDF2-style eta, and rmx_energy, against the literal."""
    sc, lit, (q0, qd0, q1, etas) = _case(name)
    B = len(q0)
    for eta, qA, qB in etas:
        g, H = sim.eval_residual(q1, qA, qB, eta)
        g_only = sim.eval_residual(q1, qA, qB, eta, want_H=False)
        for b in range(B):
            go, Ho = lit.eval(q1[b], qA[b], qB[b], eta)
            sH, sg = pf.force_share(lit, q1[b], qA[b], qB[b], eta)
            print("%s eta=%.4g b=%d: |dg|/|g| = %.2e, |dH|/|H| = %.2e (force share of H %.2f, of g %.2f)" % (
                name, eta, b, _rel(g[b], go), _rel(H[b], Ho), sH, sg))
            if generated:
                assert sH >= 0.1 and sg >= 0.1, (name, b, sH, sg)
            assert _rel(g[b], go) <= 1e-11, (name, b, _rel(g[b], go))
            assert _rel(H[b], Ho) <= 1e-11, (name, b, _rel(H[b], Ho))
            assert _rel(g_only[b], go) <= 1e-11
    sim.set_state(q1, qd0)
    T, V = sim.energy()
    for b in range(B):
        To, Vo = lit.energy(q1[b], qd0[b])
        print("%s b=%d: dT = %.2e, dV = %.2e (T %.6e, V %.6e)" % (name, b, T[b] - To, V[b] - Vo, To, Vo))
        assert abs(T[b] - To) <= 1e-12 * max(abs(To), 1) and abs(V[b] - Vo) <= 1e-12 * max(abs(Vo), 1), (name, b, T[b] - To, V[b] - Vo)
        assert Vo != pf.pw.energy_world(lit.m, q1[b], qd0[b])[1]          # the forces' potential entered


def _check_steps(name, sim, bdf, counts):
    """Rollouts of counts[...] steps from the case's states against the numpy Newton (its first step is the single step); the
    energies at the device's own end state.  Returns the status words of the longest rollout."""
    sc, lit, (q0, qd0, _, _) = _case(name)
    B = len(q0)
    nmax = max(counts)
    ref = [_reference_rollout(name, bdf, nmax, b) for b in range(B)]
    status = None
    for nsteps in counts:
        sim.set_state(q0, qd0)
        out = (sim.step_bdf1 if bdf == 1 else sim.step_bdf2)(nsteps, h=sc.h, stats=True, history=True)
        qg, qdg = sim.get_state()
        Tg, Vg = sim.energy()
        status = out["status"].copy()
        for b in range(B):
            _, _, st, hist, _ = ref[b]
            if st != 0:                                      # the reference algorithm fails on this state: so must the device
                if nsteps == nmax:
                    assert out["status"][b] & 3, (name, bdf, b, out["status"][b])
                continue
            qo, qdo = hist[nsteps - 1][:2]
            print("%s BDF%d %d steps b=%d: |dq|/|q| = %.2e, |dqdot|/|qdot| = %.2e, status %d" % (
                name, bdf, nsteps, b, _rel(qg[b], qo), _rel(qdg[b], qdo), out["status"][b]))
            assert out["status"][b] & 15 == 0, (name, bdf, b, out["status"][b])
            if nsteps == 1:
                assert _close(qg[b], qo, 1e-11, 1e-10), (name, b, _rel(qg[b], qo))
                assert _close(qdg[b], qdo, 1e-9, 1e-8), (name, b, _rel(qdg[b], qdo))
            else:
                assert _rel(qg[b], qo) <= 1e-8, (name, b, _rel(qg[b], qo))
            T, V = lit.energy(qg[b], qdg[b])
            assert abs(Tg[b] - T) <= 1e-12 * max(abs(T), 1) and abs(Vg[b] - V) <= 1e-12 * max(abs(V), 1), (name, b, Tg[b] - T, Vg[b] - V)
            assert abs(out["T"][-1, b] - T) <= 1e-12 * max(abs(T), 1) and abs(out["V"][-1, b] - V) <= 1e-12 * max(abs(V), 1)
    assert sim.last_step_kernel().startswith("k_step_pf<%d," % _np_of(lit.m["n"])), sim.last_step_kernel()
    return status


# ----------------------------------------------------------------------------- a. multi-DOF joints
@pytest.mark.parametrize("name", COMPOSITE + SMALL)
def test_composite_joints_eval_and_energy(oracle_lib, name):
    """Scenes 4, 5, 6, 8 with forces and eight random trees with multi-DOF joints: (g, H), g alone and the energies."""
    from redmax_amd import BatchSim
    sim = BatchSim(_case(name)[0], batch=2)
    _check_eval(name, sim, generated=name in SMALL)
    sim.close()


@pytest.mark.parametrize("bdf", [1, 2])
@pytest.mark.parametrize("name", COMPOSITE + SMALL)
def test_composite_joints_steps(oracle_lib, name, bdf):
    """One step and a 6-step rollout against the numpy Newton on the literal; the kernel is k_step_pf of the padded size."""
    from redmax_amd import BatchSim
    sim = BatchSim(_case(name)[0], batch=2)
    _check_steps(name, sim, bdf, (1, 6))
    sim.close()


@pytest.mark.parametrize("name", BIG)
def test_big_trees(oracle_lib, name):
    """45 and 52 nodes (the 64-lane kernels): evaluation, energies and 3 steps of both integrators."""
    from redmax_amd import BatchSim
    sim = BatchSim(_case(name)[0], batch=2)
    _check_eval(name, sim, generated=True)
    for bdf in (1, 2):
        _check_steps(name, sim, bdf, (3,))
    sim.close()


# ----------------------------------------------------------------------------- b. every padded size
@pytest.mark.parametrize("n", [2, 4, 5, 8, 9, 16, 17, 32, 33, 64])
def test_every_padded_size(oracle_lib, n):
    """n = NP and n = NP + 1 for every padded size, and the full 64-node tree (pf_solve_guarded's 64-row solve with M.n == 64):
    evaluation, energies and 3 steps of BDF1 and of SDIRK2 + BDF2.  At n = 33 the guard trips on three of the four rollouts."""
    from redmax_amd import BatchSim
    name = "n%d" % n
    sc, lit, _ = _case(name)
    assert lit.m["n"] == n
    sim = BatchSim(sc, batch=2)
    _check_eval(name, sim, generated=True)
    for bdf in (1, 2):
        _check_steps(name, sim, bdf, (3,))
    sim.close()


# ----------------------------------------------------------------------------- c. the force table at its limits
@pytest.mark.parametrize("which", ["forces32", "points128"])
def test_at_the_limits(oracle_lib, which):
    """Exactly RMX_PF_MAX_FORCES = 32 forces - among them a cable of exactly RMX_PF_MAX_POINTS = 8 points, a cable with two
    consecutive points on one body, one with two consecutive world anchors and a spring with both ends on one body - and
    RMX_PF_MAX_TOTAL = 128 points in 16 cables of 8: evaluation, energies and one step."""
    from redmax_amd import BatchSim
    name = "lim:" + which
    sc, lit, _ = _case(name)
    npts = [len(f[1]) for f in lit.forces]
    if which == "forces32":
        assert len(npts) == 32 and max(npts) == 8 and sum(npts) <= 128
        same = [f for f in lit.forces if f[0] == pf.CABLE and any(a[0] == b[0] for a, b in zip(f[1], f[1][1:]))]
        assert any(a[0] == b[0] >= 0 for f in same for a, b in zip(f[1], f[1][1:]))
        assert any(a[0] == b[0] == -1 for f in same for a, b in zip(f[1], f[1][1:]))
        assert any(f[0] == pf.SPRING and f[1][0][0] == f[1][1][0] >= 0 for f in lit.forces)
    else:
        assert npts == [8] * 16
    sim = BatchSim(sc, batch=2)
    _check_eval(name, sim, generated=False)
    for bdf in (1, 2):
        _check_steps(name, sim, bdf, (1,))
    sim.close()


def test_spring_on_one_body(oracle_lib):
    """A stretched spring-damper with both ends on ONE body: a tension, but no generalised force - its share of g is zero to
    rounding, and so is the literal's share of H (the tension's and the geometric blocks cancel: the device's two updates must too)."""
    from redmax_amd import BatchSim
    name = "lim:samebody"
    sc, lit, (q0, qd0, q1, etas) = _case(name)
    sim = BatchSim(sc, batch=2)
    for eta, qA, qB in etas:
        g, H = sim.eval_residual(q1, qA, qB, eta)
        for b in range(2):
            go, Ho = lit.eval(q1[b], qA[b], qB[b], eta)
            g0, H0 = lit.o.eval_residual(q1[b], qA[b], qB[b], eta)
            (kind, pts, ks, kd, L), = lit.forces
            assert pf.tension(kind, ks, kd, L, np.linalg.norm(pts[1][1] - pts[0][1]), 0.0)[1] > 1e5      # the tension is there
            print("one body, eta=%.4g b=%d: |g - g0|/|g| = %.2e, |H - Hlit|/|H| = %.2e, literal share of H %.2e" % (
                eta, b, _rel(g[b], g0), _rel(H[b], Ho), _rel(Ho, H0)))
            assert _rel(g[b], g0) <= 1e-11 and _rel(g[b], go) <= 1e-11
            assert _rel(H[b], Ho) <= 1e-11
    sim.set_state(q1, qd0)
    T, V = sim.energy()
    for b in range(2):
        To, Vo = lit.energy(q1[b], qd0[b])
        assert abs(T[b] - To) <= 1e-12 * max(abs(To), 1) and abs(V[b] - Vo) <= 1e-12 * max(abs(Vo), 1)
        assert Vo != pf.pw.energy_world(lit.m, q1[b], qd0[b])[1]
    sim.close()


# ----------------------------------------------------------------------------- d. cables that switch
@pytest.mark.parametrize("bdf", [1, 2])
def test_cables_switch_within_a_rollout(oracle_lib, bdf):
    """20 steps of pf.switchingScene: per cable the reference's trajectory is taut, slack and taut again (or the reverse); the
    device's record of every step against it, T and V of every step against the restatement at the device's own states."""
    from redmax_amd import BatchSim
    sc = pf.switchingScene()
    lit = pf.Literal(oracle_lib, sc)
    q, qd = pf.switchingStates(sc)
    B, nsteps = 2, 20
    ref = [pf.sim_loop(lit.eval, lit.energy, q[b], qd[b], sc.h, nsteps, bdf, history=True) for b in range(B)]
    for b in range(B):
        assert ref[b][2] == 0
        states = pf.cable_states(lit, ref[b][3])
        assert len(states) == 2 and all(pf.switches(s) for s in states), (bdf, b, states)
    sim = BatchSim(sc, batch=B)
    sim.set_state(q, qd)
    out = (sim.step_bdf1 if bdf == 1 else sim.step_bdf2)(nsteps, h=sc.h, stats=True, history="full")
    assert (out["status"] & 15 == 0).all(), out["status"]
    worst = 0.0
    for b in range(B):
        for s in range(nsteps):
            qo, qdo, _, _ = ref[b][3][s]
            worst = max(worst, _rel(out["q"][s, b], qo))
            assert _rel(out["q"][s, b], qo) <= 1e-8, (bdf, b, s, _rel(out["q"][s, b], qo))
            T, V = lit.energy(out["q"][s, b], out["qdot"][s, b])
            assert abs(out["T"][s, b] - T) <= 1e-12 * max(abs(T), 1) and abs(out["V"][s, b] - V) <= 1e-12 * max(abs(V), 1), (bdf, b, s)
    print("switching BDF%d: worst per-step |dq|/|q| = %.2e" % (bdf, worst))
    sim.close()


def test_slack_cable_leaves_no_trace(oracle_lib):
    """At a state of the reference's trajectory where one cable is slack and the other taut, the evaluation equals the literal of
    the scene WITHOUT the slack cable, and doubling the cable's stiffness changes no bit of g, H and the energies."""
    from redmax_amd import BatchSim
    sc = pf.switchingScene()
    lit = pf.Literal(oracle_lib, sc)
    q, qd = pf.switchingStates(sc)
    hist = pf.sim_loop(lit.eval, lit.energy, q[0], qd[0], sc.h, 20, 2, history=True)[3]
    taut = pf.cable_states(lit, hist)
    # a step in the middle of a slack stretch of one cable at which the other one is taut
    found = [(c, s) for c in (0, 1) for s in range(1, 19) if not (taut[c][s - 1] or taut[c][s] or taut[c][s + 1]) and taut[1 - c][s]]
    assert found
    c, s = found[0]
    qs, qds = hist[s][:2]
    bare = pf.switchingScene()
    bare.forces = [bare.forces[1 - c]]
    bare.init()
    lit_bare = pf.Literal(oracle_lib, bare)
    stiff = pf.switchingScene()
    stiff.forces[c].setStiffness(2 * stiff.forces[c].stiffness)
    stiff.init()
    assert stiff.forces[c].L == sc.forces[c].L and bare.forces[0].L == sc.forces[1 - c].L
    eta = 2 * sc.h / 3
    qA, qB = qs - eta * qds, qs - 0.9 * eta * qds
    res = []
    for scene in (sc, stiff):
        sim = BatchSim(scene, batch=1)
        g, H = sim.eval_residual(qs[None], qA[None], qB[None], eta)
        g_only = sim.eval_residual(qs[None], qA[None], qB[None], eta, want_H=False)
        sim.set_state(qs[None], qds[None])
        res.append((g[0], H[0], g_only[0]) + tuple(a[0] for a in sim.energy()))
        sim.close()
    go, Ho = lit_bare.eval(qs, qA, qB, eta)
    To, Vo = lit_bare.energy(qs, qds)
    assert Vo > pf.pw.energy_world(lit.m, qs, qds)[1]                               # the other cable is taut there
    g, H, g_only, T, V = res[0]
    print("slack cable: |dg|/|g| = %.2e, |dH|/|H| = %.2e, dV = %.2e" % (_rel(g, go), _rel(H, Ho), V - Vo))
    assert _rel(g, go) <= 1e-11 and _rel(H, Ho) <= 1e-11 and _rel(g_only, go) <= 1e-11
    assert abs(T - To) <= 1e-12 * max(abs(To), 1) and abs(V - Vo) <= 1e-12 * max(abs(Vo), 1)
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- e. the solve policy
def _trips(trace):
    """Per linear solve of a reference rollout: True (the restated guard trips), False, or None within 1 % of the threshold
    (the device compares high words: 2^-20)."""
    return [None if 64 / 1.01 <= r <= 64 * 1.01 else bool(r > 64) for _, r in trace]


@pytest.mark.parametrize("bdf", [1, 2])
@pytest.mark.parametrize("name", ["r304", "r307"])
def test_lu_mode_1(oracle_lib, name, bdf):
    """rmx_opts.lu_mode = 1 (every solve with partial pivoting): the checks of the multi-DOF tests, and RMX_ST_PIVOTED never set."""
    from redmax_amd import BatchSim
    sim = BatchSim(_case(name)[0], batch=2)
    sim.opts.lu_mode = 1
    status = _check_steps(name, sim, bdf, (1, 6))
    assert (status & 16 == 0).all(), status
    sim.close()


@pytest.mark.parametrize("bdf", [1, 2])
@pytest.mark.parametrize("name", ["r307", "r311"])
def test_guard_trips_where_the_restatement_says(oracle_lib, name, bdf):
    """lu_mode 0.  On r307 the restated guard trips on the first solve of every rollout (H is indefinite at the first iterate)
    and the reference's Newton converges all the same: the device sets RMX_ST_PIVOTED (16) there, redoes the solve with partial
    pivoting and matches the numpy Newton.  On r311 no solve comes near the threshold: the bit stays clear.  lu_mode 1: never set."""
    from redmax_amd import BatchSim
    sc, lit, _ = _case(name)
    expect = []
    for b in range(2):
        _, _, st, _, trace = _reference_rollout(name, bdf, 6, b)
        t = _trips(trace)
        assert st == 0 and None not in t, (name, bdf, b, st, trace)
        expect.append(any(t))
    assert expect == [name == "r307"] * 2
    for mode in (0, 1):
        sim = BatchSim(sc, batch=2)
        sim.opts.lu_mode = mode
        status = _check_steps(name, sim, bdf, (6,))
        print("%s BDF%d lu_mode %d: status %s, restated guard trips %s" % (name, bdf, mode, status, expect))
        assert [bool(s & 16) for s in status] == ([False, False] if mode else expect), (name, bdf, mode, status)
        sim.close()


def test_guard_hold_runs(oracle_lib):
    """12 steps of SDIRK2 + BDF2 on r307, state 1: the restated guard trips on four solves in a row in step 1 (PIV_STREAK = 3 of
    rmx_device.h), so from step 2 on the device runs pivot-only steps under the hold; the rollout matches the numpy Newton as before."""
    from redmax_amd import BatchSim
    name = "r307"
    sc, lit, _ = _case(name)
    _, _, st, _, trace = _reference_rollout(name, 2, 12, 1)
    t = _trips(trace)
    assert st == 0
    run = best = 0
    for x in t:
        run = run + 1 if x else 0
        best = max(best, run)
    assert best >= 3, t
    for mode in (0, 1):
        sim = BatchSim(sc, batch=2)
        sim.opts.lu_mode = mode
        status = _check_steps(name, sim, 2, (12,))
        assert bool(status[1] & 16) == (mode == 0), (mode, status)
        sim.close()


# ----------------------------------------------------------------------------- f. batch independence
def test_batch_independence_on_composite_joints():
    """Rollout b of a batch of 64 equals the same state run alone, bit for bit (r304: 15 nodes, multi-DOF joints; BDF2, 6 steps)."""
    from redmax_amd import BatchSim
    sc = pf.named_scene("r304")
    B = 64
    q, qd, _, _ = pf.nearInitialStates(sc, 304, B)
    sim = BatchSim(sc, batch=B)
    sim.set_state(q, qd)
    sim.step_bdf2(6, h=sc.h)
    qg, qdg = sim.get_state()
    assert np.isfinite(qg).all()
    for b in (0, 17, 63):
        one = BatchSim(sc, batch=1)
        one.set_state(q[b:b + 1], qd[b:b + 1])
        one.step_bdf2(6, h=sc.h)
        q1, qd1 = one.get_state()
        assert np.array_equal(q1[0], qg[b]) and np.array_equal(qd1[0], qdg[b]), b
        one.close()
    sim.close()
