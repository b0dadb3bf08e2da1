"""rmx_adjoint_controls: the adjoint with one torque per joint and STEP (u[B][nsteps][nr]) and the gradient for each of them.

The checks, in the order of the sections below:
  1. with u[b][k] = p[b] for every k the call is the constant-parameter call (rmx_adjoint_bdf1 / bdf2) bit for bit in everything the
     regulariser does not enter, its rows sum to dPdp, and both meet the oracle;
  2. with truly varying controls the forward rollout is the oracle's, driven one step at a time;
  3. the gradient meets the reference's own testGrad identity (driverRedMaxAdjointBDF1.m:46-61) in the full [nsteps][nr] space;
  4. the rows behind the task step are wreg * u exactly;
  5. plumbing: helper wave on / off, device pointers, gradient=False, refusals, the MEX command.
(The step-by-step oracle driver of section 2 is checked against the oracle's single call in tests/test_adjoint_controls_host.py.)

About the regulariser in section 1.  P holds wreg/2 * sum over k, j of u^2 and row k of dPdu holds wreg * u[k]: with u[k] = p for all
nsteps rows that is nsteps times the constant call's wreg/2 |p|^2 and wreg * p.  So the bit-for-bit comparison of P runs with wreg = 0
(where both calls compute the same expression), and the comparisons that carry a regulariser give the controls call wreg / nsteps,
which is the same objective in exact arithmetic.
"""
import ctypes as C

import numpy as np
import pytest

from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)

# chain sizes -> steps: 5 Generic (NP 8), 11 Help16 on a tree that does not fill its 16 slots, 16 Help16 / FullChain16,
# 32 the MFMA M/D store, 40 the 64-lane store-every-iterate path; "tree7" a branching tree on Generic NP 8
STEPS = {5: 12, 11: 8, 16: 8, 32: 5, 40: 4, "tree7": 10}


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def sceneAdjointTree7(bdf2=False):
    """A full binary tree of 7 revolute joints (depth-first listing, axes cycling x, y, z), bodies, stiffness, damping and the task
    constants of sceneAdjointChain; the task point sits on the last leaf."""
    from redmax_amd.redmax import BodyCuboid, JointRevolute, Scene
    from redmax_amd.scenes import _T
    scene = Scene()
    scene.name = "Adjoint tree, 7 joints"
    axes = ([1, 0, 0], [0, 1, 0], [0, 0, 1])

    def add(parent, depth, offset):
        body = BodyCuboid(1.0, [10, 1, 1])
        j = JointRevolute(parent, body, axes[len(scene.joints) % 3])
        j.setJointTransform(np.eye(4) if parent is None else _T(offset))
        j.q[0] = 0.3 if parent is None else 0.2
        j.qdot[0] = 1.0
        j.setStiffness(1e4)
        j.setDamping(1e4)
        body.setBodyTransform(_T([5, 0, 0]))
        scene.bodies.append(body)
        scene.joints.append(j)
        if depth < 2:
            add(j, depth + 1, [10, -3, 0])
            add(j, depth + 1, [10, 3, 0])

    add(None, 0, [0, 0, 0])
    scene.task = {"body": 6, "xlocal": [5.0, 0.0, 0.0], "xtarget": [-10.0 if bdf2 else 10.0, 5.0, -10.0], "t": scene.tEnd,
                  "pscale": 1e5, "wreg": 1e-2, "wpos": 1e2}
    return scene


def _scene(size, integ):
    from redmax_amd.scenes import sceneAdjointChain
    sc = sceneAdjointTree7(bdf2=integ == 2) if size == "tree7" else sceneAdjointChain(size, bdf2=integ == 2)
    sc.init()
    return sc


def _run(sim, sc, fn, *args, **kw):
    """One call from the scene's initial state: (P, gradient, info, q, qdot)."""
    q0, qd0 = sc.getQ()
    sim.set_state(q0[None, :], qd0[None, :])
    P, dP, info = fn(*args, **kw)
    return (P, dP, info) + sim.get_state()


# ---------------------------------------------------------------- 1. reduces to the constant call

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, 11, 16, "16-one-wave", 32, 40, "tree7"])
def test_constant_controls_are_the_constant_call(oracle_lib, size, integ, monkeypatch):
    from redmax_amd import BatchSim
    if size == "16-one-wave":          # the full 16-link chain without its helper wave: FullChain16
        monkeypatch.setenv("RMX_ADJ_HELP", "0")
        size = 16
    sc = _scene(size, integ)
    B, nsteps = 3, STEPS[size]
    p = 0.1 * np.random.default_rng(31).standard_normal((B, sc.nr))
    p[0] = 0.0
    u = np.repeat(p[:, None, :], nsteps, axis=1)
    task = dict(sc.task, t=nsteps * sc.h)
    task0 = dict(task, wreg=0.0)
    sim = BatchSim(sc, batch=B)
    const = sim.adjoint_bdf1 if integ == 1 else sim.adjoint_bdf2
    Pc, dPc, ic, qc, qdc = _run(sim, sc, const, nsteps, sc.h, task, p, stats=True)
    Pc0, _, _, _, _ = _run(sim, sc, const, nsteps, sc.h, task0, p, stats=True)
    Pu0, dPu0, iu0, qu0, qdu0 = _run(sim, sc, sim.adjoint_controls, nsteps, sc.h, task0, u, integrator=integ, stats=True)
    Pu, dPu, iu, qu, qdu = _run(sim, sc, sim.adjoint_controls, nsteps, sc.h, dict(task, wreg=task["wreg"] / nsteps), u, integrator=integ,
                                stats=True)
    sim.close()
    assert (ic["status"] == 0).all()
    # bit for bit: P without the regulariser, the final state and both counters (the regulariser enters none of the last three)
    assert np.array_equal(Pu0, Pc0)
    for q, qd, info in ((qu0, qdu0, iu0), (qu, qdu, iu)):
        assert np.array_equal(q, qc) and np.array_equal(qd, qdc)
        assert np.array_equal(info["newton_iters"], ic["newton_iters"]) and np.array_equal(info["status"], ic["status"])
    # the rows sum to the constant call's gradient (summation order only), with and without the regulariser
    assert dPu.shape == (B, nsteps, sc.nr)
    for b in range(B):
        print("size %s integ %d b %d: |sum_k dPdu - dPdp| / |dPdp| = %.3e" % (size, integ, b, _rel(dPu[b].sum(axis=0), dPc[b])))
        assert _rel(dPu[b].sum(axis=0), dPc[b]) <= 1e-12, (size, integ, b)
        assert abs(Pu[b] - Pc[b]) <= 1e-12 * abs(Pc[b])
    for b in range(B):
        o = oracle_lib.Oracle(sc.desc())
        Po, dPo, st = (o.adjoint_bdf1 if integ == 1 else o.adjoint_bdf2)(sc.h, nsteps, task, p[b])
        assert _rel(dPu[b].sum(axis=0), dPo) <= 1e-7, (size, integ, b, _rel(dPu[b].sum(axis=0), dPo))
        assert abs(Pu[b] - Po) <= 1e-9 * abs(Po), (size, integ, b, Pu[b], Po)
        assert iu["newton_iters"][b] == st.newton_iters


# ---------------------------------------------------------------- 2. forward parity with truly varying controls

def oracle_rollout_per_step(orc, sc, h, nsteps, task, u):
    """The oracle's BDF1 adjoint rollout under a torque per step.  Its adjoint call resets to the scene's initial state and takes one p,
    so every step is a call of its own: an Oracle whose initial state is the current one (the rest positions stay the scene's), one
    step under p = u[k-1], measured only at the task step, no regulariser.  Returns (q, qdot, position term of P, Newton iterations)."""
    d0 = sc.desc()
    idx = orc.Oracle(d0).idxR()
    q, qd = (np.array(a, dtype=np.float64) for a in sc.getQ())
    kt = int(round(float(task["t"]) / h))
    P, iters = 0.0, 0
    for k in range(1, nsteps + 1):
        d = dict(d0)
        d["q"] = np.array([q[i] if i >= 0 else 0.0 for i in idx])
        d["qdot"] = np.array([qd[i] if i >= 0 else 0.0 for i in idx])
        d["qR"], d["qdotR"] = q.copy(), qd.copy()
        o = orc.Oracle(d)
        o.set_qrest_joint_order(d0["qRest"])
        Pk, _, st = o.adjoint_bdf1(h, 1, dict(task, t=h if k == kt else 2 * h, wreg=0.0), u[k - 1])
        assert st.not_converged == 0 and st.diverged == 0
        q, qd = o.get_state()
        P += Pk
        iters += st.newton_iters
    return q, qd, P, iters


@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, "tree7"])
def test_varying_controls_forward_matches_oracle(oracle_lib, size):
    from redmax_amd import BatchSim
    sc = _scene(size, 1)
    B, nsteps = 3, STEPS[size]
    u = 0.1 * np.random.default_rng(41).standard_normal((B, nsteps, sc.nr))
    u[0, ::2] = 0.0
    task = dict(sc.task, t=(nsteps - 3) * sc.h)
    sim = BatchSim(sc, batch=B)
    P, dPdu, info, q, qd = _run(sim, sc, sim.adjoint_controls, nsteps, sc.h, task, u, stats=True)
    sim.close()
    assert (info["status"] == 0).all() and np.isfinite(dPdu).all()
    for b in range(B):
        qo, qdo, Ppos, iters = oracle_rollout_per_step(oracle_lib, sc, sc.h, nsteps, task, u[b])
        Po = Ppos + 0.5 * task["wreg"] * float((u[b] ** 2).sum())
        assert _rel(q[b], qo) <= 1e-9, (size, b, _rel(q[b], qo))
        assert abs(P[b] - Po) <= 1e-9 * abs(Po), (size, b, P[b], Po)
        assert info["newton_iters"][b] == iters


# ---------------------------------------------------------------- 3. the gradient by the reference's testGrad identity

def _fd_errors(sc, nsteps, kt, integ, controls):
    """testGrad on the device: central differences of P along 3 random directions (eps = 1e-5, one batch of 6 rollouts) against
    direction . gradient.  controls: directions in the full [nsteps][nr] space through rmx_adjoint_controls (for BDF2 zero in the
    k = 1 rows: that row carries the reference's start-step approximation); else in the [nr] space of the constant call."""
    from redmax_amd import BatchSim
    nd, eps = 3, 1e-5
    rng = np.random.default_rng(53)
    task = dict(sc.task, t=kt * sc.h)
    base = 0.1 * rng.standard_normal((nsteps, sc.nr) if controls else (sc.nr,))
    d = rng.standard_normal((nd,) + base.shape)
    if controls and integ == 2:
        d[:, 0, :] = 0.0
    one, fd = BatchSim(sc, batch=1), BatchSim(sc, batch=2 * nd)
    pp = np.repeat(base[None], 2 * nd, axis=0)
    pp[0::2] += eps * d
    pp[1::2] -= eps * d
    if controls:
        _, grad, _, _, _ = _run(one, sc, one.adjoint_controls, nsteps, sc.h, task, base[None], integrator=integ)
        Pf, none, _, _, _ = _run(fd, sc, fd.adjoint_controls, nsteps, sc.h, task, pp, integrator=integ, gradient=False)
        assert none is None
    else:
        _, grad, _, _, _ = _run(one, sc, one.adjoint_bdf1 if integ == 1 else one.adjoint_bdf2, nsteps, sc.h, task, base[None])
        Pf, _, _, _, _ = _run(fd, sc, fd.adjoint_bdf1 if integ == 1 else fd.adjoint_bdf2, nsteps, sc.h, task, pp)
    one.close()
    fd.close()
    num = (Pf[0::2] - Pf[1::2]) / (2 * eps)
    ana = (d.reshape(nd, -1) * grad.reshape(1, -1)).sum(axis=1)
    return num, ana


@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n,nsteps,kt", [(5, 10, 5), (16, 6, 3)])
def test_gradient_meets_the_testgrad_identity(n, nsteps, kt, integ):
    """Tolerance: twice the error the oracle-pinned constant-parameter call shows in the same identity on the same scene, horizon, task
    step and eps = 1e-5 - measured here, in the same run - and never tighter than the rtol = 2e-5, atol = 1e-6 max|ana| of
    test_adjoint_scene100_at_its_own_horizon.  Under BDF2 the constant call's figure is the reference's start-step approximation
    (17 - 20 % of the gradient at these horizons), which the directions here leave out by being zero in the k = 1 rows: it says
    nothing about the rows k >= 2, which are exact, so there the bound is that floor alone.

    Measured on MI355X, max over the 3 directions of |num - ana| / max|ana|:
        n  nsteps  integrator   constant call   this call
        5    10      BDF1         3.4e-10        5.0e-10
        5    10      BDF2         1.7e-01        7.5e-09
       16     6      BDF1         8.5e-10        1.8e-09
       16     6      BDF2         2.0e-01        1.6e-09
    so the floor is what binds in every case."""
    sc = _scene(n, integ)
    num_c, ana_c = _fd_errors(sc, nsteps, kt, integ, controls=False)
    err_c = np.abs(num_c - ana_c)
    num, ana = _fd_errors(sc, nsteps, kt, integ, controls=True)
    err = np.abs(num - ana)
    print("testgrad n %d integ %d: constant call %.3e, controls %.3e (of max|ana|)"
          % (n, integ, err_c.max() / np.abs(ana_c).max(), err.max() / np.abs(ana).max()))
    assert np.abs(ana).max() > 0
    measured = float(err_c.max() / np.abs(ana_c).max())
    floor = 2e-5 * np.abs(ana) + 1e-6 * np.abs(ana).max()
    tol = np.maximum(2.0 * measured * np.abs(ana).max(), floor) if integ == 1 else floor
    assert (err <= tol).all(), (num, ana, err, tol)


# ---------------------------------------------------------------- 4. exact structure

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, 16, 40])
def test_rows_behind_the_task_step_and_the_zero_rollout(size, integ):
    from redmax_amd import BatchSim
    sc = _scene(size, integ)
    B, nsteps = 3, STEPS[size]
    kt = nsteps // 2
    u = 0.1 * np.random.default_rng(61).standard_normal((B, nsteps, sc.nr))
    u[0] = 0.0
    task = dict(sc.task, t=kt * sc.h)
    sim = BatchSim(sc, batch=B)
    P, dPdu, info, q, qd = _run(sim, sc, sim.adjoint_controls, nsteps, sc.h, task, u, integrator=integ, stats=True)
    P0, dPdu0, _, _, _ = _run(sim, sc, sim.adjoint_controls, nsteps, sc.h, dict(task, wreg=0.0), u, integrator=integ)
    const = sim.adjoint_bdf1 if integ == 1 else sim.adjoint_bdf2
    Pc, dPc, ic, qc, qdc = _run(sim, sc, const, nsteps, sc.h, task, np.zeros((B, sc.nr)), stats=True)
    sim.close()
    # z_k is exactly 0 behind the task step
    assert np.array_equal(dPdu[:, kt:, :], task["wreg"] * u[:, kt:, :])
    assert not dPdu0[:, kt:, :].any()
    assert np.abs(dPdu0[1:, :kt, :]).max(axis=2).min() > 0
    # rollout 0, u = 0: the plain adjoint call with p = 0 (wreg * 0 adds nothing on either side)
    assert P[0] == Pc[0] and np.array_equal(q[0], qc[0]) and np.array_equal(qd[0], qdc[0])
    assert info["newton_iters"][0] == ic["newton_iters"][0] and info["status"][0] == ic["status"][0]
    assert _rel(dPdu[0].sum(axis=0), dPc[0]) <= 1e-12


# ---------------------------------------------------------------- 5. plumbing

@pytest.mark.gpu
@pytest.mark.parametrize("n,integ", [(16, 1), (16, 2), (11, 1)])
def test_helper_wave_on_and_off_agree(n, integ, monkeypatch):
    from redmax_amd import BatchSim
    sc = _scene(n, integ)
    B, nsteps = 4, STEPS[n]
    u = 0.1 * np.random.default_rng(71).standard_normal((B, nsteps, sc.nr))
    task = dict(sc.task, t=(nsteps - 1) * sc.h)
    res = []
    for helper in ("0", "1"):
        monkeypatch.setenv("RMX_ADJ_HELP", helper)
        sim = BatchSim(sc, batch=B)
        P, dPdu, info, q, qd = _run(sim, sc, sim.adjoint_controls, nsteps, sc.h, task, u, integrator=integ, stats=True)
        res.append((P, dPdu, info["newton_iters"], info["status"], q, qd))
        sim.close()
    assert np.isfinite(res[0][0]).all() and np.abs(res[0][1]).sum() > 0
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


class _DevArray:
    """A device array through the HIP runtime the library itself is linked against (as in tests/test_gpu_parity.py)."""
    _hip = None

    def __init__(self, host):
        if _DevArray._hip is None:
            _DevArray._hip = C.CDLL("libamdhip64.so")
        self.host = np.ascontiguousarray(host, dtype=np.float64)
        self.ptr = C.c_void_p()
        assert self._hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.host.nbytes)) == 0
        assert self._hip.hipMemcpy(self.ptr, self.host.ctypes.data_as(C.c_void_p), C.c_size_t(self.host.nbytes), 1) == 0

    def get(self):
        out = np.empty_like(self.host)
        assert self._hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        self._hip.hipFree(self.ptr)


@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
def test_device_form_and_forward_only(integ):
    """The _device form equals the host form bit for bit and leaves u untouched; gradient=False (host) and a null dPdu pointer (device)
    leave the same state, P and counters."""
    from redmax_amd import BatchSim
    sc = _scene(16, integ)
    B, nsteps = 4, 6
    u = 0.1 * np.random.default_rng(81).standard_normal((B, nsteps, sc.nr))
    task = dict(sc.task, t=4 * sc.h)
    sim = BatchSim(sc, batch=B)
    P, dPdu, info, q, qd = _run(sim, sc, sim.adjoint_controls, nsteps, sc.h, task, u, integrator=integ, stats=True)
    Pf, none, info_f, qf, qdf = _run(sim, sc, sim.adjoint_controls, nsteps, sc.h, task, u, integrator=integ, stats=True, gradient=False)
    assert none is None and np.array_equal(Pf, P) and np.array_equal(qf, q) and np.array_equal(qdf, qd)
    assert np.array_equal(info_f["newton_iters"], info["newton_iters"]) and np.array_equal(info_f["status"], info["status"])
    # a (nsteps, nr) array holds for every trajectory
    Pb, dPb, _, _, _ = _run(sim, sc, sim.adjoint_controls, nsteps, sc.h, task, u[1], integrator=integ)
    assert (Pb == P[1]).all() and all(np.array_equal(dPb[b], dPdu[1]) for b in range(B))
    u_d, P_d, dP_d = _DevArray(u), _DevArray(np.full(B, np.nan)), _DevArray(np.full(u.shape, np.nan))
    q0, qd0 = sc.getQ()
    for grad_ptr in (dP_d.ptr.value, None):
        sim.set_state(q0[None, :], qd0[None, :])
        info_d = sim.adjoint_controls_device(nsteps, sc.h, task, u_d.ptr.value, P_d.ptr.value, grad_ptr, integrator=integ, stats=True)
        qb, qdb = sim.get_state()
        assert np.array_equal(P_d.get(), P) and np.array_equal(dP_d.get(), dPdu)
        assert np.array_equal(qb, q) and np.array_equal(qdb, qd)
        assert np.array_equal(info_d["newton_iters"], info["newton_iters"]) and np.array_equal(info_d["status"], info["status"])
        assert np.array_equal(u_d.get(), u)
    for d in (u_d, P_d, dP_d):
        d.free()
    sim.close()


@pytest.mark.gpu
def test_bad_arguments_raise_cleanly():
    from redmax_amd import BatchSim, _abi
    from redmax_amd.scenes import scenesRedMax
    sc = _scene(5, 1)
    B, nsteps = 2, 4
    task = dict(sc.task, t=nsteps * sc.h)
    u = np.zeros((B, nsteps, sc.nr))
    sim = BatchSim(sc, batch=B)
    for bad in (np.zeros((B, nsteps + 1, sc.nr)), np.zeros((B, sc.nr)), np.zeros((B + 1, nsteps, sc.nr)), np.zeros((nsteps, sc.nr + 1))):
        with pytest.raises(ValueError, match="shape"):
            sim.adjoint_controls(nsteps, sc.h, task, bad)
    with pytest.raises(ValueError):
        sim.adjoint_controls(nsteps, sc.h, task, None)
    with pytest.raises(_abi.RedMaxHipError, match="null"):
        sim.adjoint_controls_device(nsteps, sc.h, task, None, None, None)
    with pytest.raises(_abi.RedMaxHipError, match="integrator"):
        sim.adjoint_controls(nsteps, sc.h, task, u, integrator=3)
    with pytest.raises(_abi.RedMaxHipError, match="task step"):
        sim.adjoint_controls(nsteps, sc.h, dict(task, t=(nsteps + 1) * sc.h), u)
    P, dPdu, _ = sim.adjoint_controls(nsteps, sc.h, task, u)          # ... and the batch is still usable
    assert np.isfinite(P).all() and np.isfinite(dPdu).all()
    sim.close()
    ground = scenesRedMax(11)
    ground.init()
    gsim = BatchSim(ground, batch=1)
    with pytest.raises(_abi.RedMaxHipError, match="ground contact"):
        gsim.adjoint_controls(2, ground.h, dict(sc.task, body=0, step=2), np.zeros((1, 2, ground.nr)))
    gsim.close()


@pytest.mark.gpu
def test_mex_command_equals_the_ctypes_call(gw):  # noqa: F811
    """'adjoint_controls' through the gateway (stub): MATLAB's nr x nsteps x B column-major array is the ABI's [B][nsteps][nr]."""
    from redmax_amd import BatchSim
    sc = _scene(5, 1)
    B, nsteps = 3, 6
    u = 0.1 * np.random.default_rng(91).standard_normal((B, nsteps, sc.nr))
    task = dict(sc.task, t=4 * sc.h)
    q0, qd0 = sc.getQ()
    mtask = {"body": float(task["body"] + 1), "xlocal": np.array(task["xlocal"]), "xtarget": np.array(task["xtarget"]), "step": 4.0,
             "pscale": task["pscale"], "wreg": task["wreg"], "wpos": task["wpos"]}
    um = u.transpose(2, 1, 0)                                  # nr x nsteps x B
    for integ in (1, 2):
        sim = BatchSim(sc, batch=B)
        P, dPdu, info, q, qd = _run(sim, sc, sim.adjoint_controls, nsteps, sc.h, task, u, integrator=integ, stats=True)
        sim.close()
        h = gw.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))          # two shards: the arrays advance per shard
        gw.call(0, "set", h, np.repeat(q0[:, None], B, axis=1), np.repeat(qd0[:, None], B, axis=1))
        Pm, dPm, st = gw.call(3, "adjoint_controls", h, sc.h, float(nsteps), mtask, um, float(integ))
        qm, qdm = gw.call(2, "get", h)
        assert dPm.shape == (sc.nr, nsteps, B) and np.array_equal(dPm.transpose(2, 1, 0), dPdu)
        assert np.array_equal(Pm[0], P) and np.array_equal(qm.T, q) and np.array_equal(qdm.T, qd)
        assert np.array_equal(st[:, 0], info["newton_iters"]) and np.array_equal(st[:, 1], info["status"])
        gw.call(0, "set", h, np.repeat(q0[:, None], B, axis=1), np.repeat(qd0[:, None], B, axis=1))
        Pf = gw.call(1, "adjoint_controls", h, sc.h, float(nsteps), mtask, um, float(integ))      # one output: forward only
        assert np.array_equal(Pf[0], P)
        with pytest.raises(MexError, match="nr x nsteps x batch"):
            gw.call(1, "adjoint_controls", h, sc.h, float(nsteps), mtask, um[:, :-1, :])
        with pytest.raises(MexError, match="integrator"):
            gw.call(1, "adjoint_controls", h, sc.h, float(nsteps), mtask, um, 3.0)
        gw.call(0, "destroy", h)
