"""rmx_rollout_tape_bdf2 / rmx_rollout_vjp: the differentiable controlled BDF2 rollout - the SDIRK2 start step on the tape, every
solve differentiated exactly.

The checks, in the order of the sections below:
  1. the forward sweep: its record against the proto's rollout (tests/proto_rollout_vjp_bdf2.py: a Newton iteration of its own on the
     oracle's residual, pinned against central differences on the CPU by tests/test_rollout_vjp_bdf2_proto.py), its final state against
     rmx_adjoint_controls with integrator 2, the BDF2 history it leaves behind;
  2. du, dq0, dqd0 against the proto's recursion, also for the one- and two-step rollouts (start step alone; first BDF2 step);
  3. the reference's testGrad identity on the device, in u, q0 and qdot0, separately and jointly;
  4. exact structure: zeros, causality, batch independence, repeatability, device pointers, no helper wave;
  5. tape bookkeeping and refusals; 6. the torch.autograd.Function; 7. the MEX command.

Sizes by the path each takes: 5-link chain and tree7 NP 8 (chain and branching); 16-link chain the full-chain form, one wavefront per
rollout where the BDF1 tape takes a helper wave; 32-link chain M, D from the matrix cores, also for the SDIRK2a stage; 40-link chain
the 64-lane path, whose H goes to the tape at every iterate - the SDIRK2a stage to its own slot.  "tree16": a branching tree of
exactly 16 joints - the generic 16-lane pair, which the full chain does not run, with every column of H a real one (at 16 lanes the
backward kernel's guarded solve starts with DPP broadcasts of the rows it has just loaded).
"""
import numpy as np
import pytest

import proto_rollout_vjp_bdf2 as proto
from test_gpu_adjoint_controls import _DevArray, _rel, _scene
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)
from test_rollout_vjp_proto import case

B = 3
STEPS = {5: 6, 16: 5, 32: 4, 40: 4, "tree7": 6, "tree16": 5}        # (the steps of tests/test_gpu_rollout_vjp.py; tree16 as 16)
SIZES = [5, "tree7", 16, "tree16", 32, 40]
_CACHE = {}


def sceneAdjointTree16():
    """sceneAdjointTree7's binary tree one level deeper (15 joints) with a 16th joint on its last leaf: depth-first listing, axes
    cycling x, y, z, the bodies, stiffness, damping and task constants of sceneAdjointChain."""
    from redmax_amd.redmax import BodyCuboid, JointRevolute, Scene
    from redmax_amd.scenes import _T
    scene = Scene()
    scene.name = "Adjoint tree, 16 joints"
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
        if depth < 3:
            add(j, depth + 1, [10, -3, 0])
            add(j, depth + 1, [10, 3, 0])
        elif len(scene.joints) == 15:
            add(j, depth + 1, [10, 0, 0])

    add(None, 0, [0, 0, 0])
    assert len(scene.joints) == 16
    scene.task = {"body": 15, "xlocal": [5.0, 0.0, 0.0], "xtarget": [-10.0, 5.0, -10.0], "t": scene.tEnd,
                  "pscale": 1e5, "wreg": 1e-2, "wpos": 1e2}
    return scene


def _scene2(size):
    if size != "tree16":
        return _scene(size, 2)
    sc = sceneAdjointTree16()
    sc.init()
    return sc


def _setup(size, nsteps=None):
    """(scene, case, nsteps) of a size under BDF2; nsteps None: the table's."""
    nsteps = STEPS[size] if nsteps is None else nsteps
    key = (size, nsteps)
    if key not in _CACHE:
        if ("scene", size) not in _CACHE:
            _CACHE[("scene", size)] = _scene2(size)
        sc = _CACHE[("scene", size)]
        _CACHE[key] = (sc, case(sc, 17, nsteps=nsteps, B=B), nsteps)
    return _CACHE[key]


def _reference(orc, size, b, nsteps=None):
    """The proto's answer for rollout b of a size, computed once and left unchanged."""
    sc, cs, nsteps = _setup(size, nsteps)
    key = ("ref", size, nsteps, b)
    if key not in _CACHE:
        _CACHE[key] = proto.reference(orc, sc, cs["q0"][b], cs["qd0"][b], cs["u"][b], sc.h, sc.task["pscale"], cs["c"][b], cs["d"][b])
    return _CACHE[key]


def _tape(sim, sc, cs, sel=slice(None), integrator=2, **kw):
    sim.set_state(cs["q0"][sel], cs["qd0"][sel])
    return sim.rollout_tape(cs["u"].shape[1], sc.h, cs["u"][sel], pscale=sc.task["pscale"], integrator=integrator, **kw)


def _tape_and_vjp(sim, sc, cs, sel=slice(None), integrator=2):
    """(qtraj, qdtraj, du, dq0, dqd0) under the loss of the proto test."""
    qt, qdt, info = _tape(sim, sc, cs, sel, integrator, stats=True)
    assert (info["status"] & 15 == 0).all()
    du, dq0, dqd0 = sim.rollout_vjp(qt.shape[1], cs["c"][sel] + qt, cs["d"][sel])
    return qt, qdt, du, dq0, dqd0


def _full(size):
    return B if size in (5, "tree7", 16, "tree16") else 1


# ---------------------------------------------------------------- 1. the forward sweep

@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_forward_sweep_is_the_protos_rollout_and_the_controls_call(oracle_lib, size):
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size)
    sim = BatchSim(sc, batch=B)
    sim.set_state(cs["q0"], cs["qd0"])
    _, none, ic = sim.adjoint_controls(nsteps, sc.h, dict(sc.task, t=nsteps * sc.h), cs["u"], integrator=2, stats=True, gradient=False)
    qc, qdc = sim.get_state()
    sim.step_bdf2(2, h=sc.h)
    qc2, qdc2 = sim.get_state()
    qt, qdt, info = _tape(sim, sc, cs, stats=True)
    q, qd = sim.get_state()
    sim.step_bdf2(2, h=sc.h)            # continues from the history the tape call left behind
    q2, qd2 = sim.get_state()
    sim.close()
    # the sweep is rmx_adjoint_controls' with integrator 2 plus stores (measured bit-identical on every scene here); asserted below,
    # behind the bounds the issue sets, so that the exact half of the continuation check cannot drop out unnoticed
    same = np.array_equal(q, qc) and np.array_equal(qd, qdc)
    print("size %s: final state bit-identical to adjoint_controls(integrator=2): %s; Newton counts tape %s controls %s"
          % (size, same, info["newton_iters"].tolist(), ic["newton_iters"].tolist()))
    print("size %s: |q - controls| %.3e |qd - controls| %.3e; two more BDF2 steps %.3e %.3e"
          % (size, _rel(q, qc), _rel(qd, qdc), _rel(q2, qc2), _rel(qd2, qdc2)))
    assert none is None and (info["status"] & 15 == 0).all()
    assert np.array_equal(info["status"], ic["status"])
    for b in range(B):
        assert _rel(q[b], qc[b]) <= 1e-9 and _rel(qd[b], qdc[b]) <= 1e-9, (size, b, _rel(q[b], qc[b]), _rel(qd[b], qdc[b]))
        # rmx_step_bdf2 goes on from either call alike: from equal bits to equal bits, and to the forward bound in any case
        assert _rel(q2[b], qc2[b]) <= 1e-9 and _rel(qd2[b], qdc2[b]) <= 1e-9, (size, b, _rel(q2[b], qc2[b]), _rel(qd2[b], qdc2[b]))
    assert same, size
    assert np.array_equal(q2, qc2) and np.array_equal(qd2, qdc2)
    assert np.array_equal(qt[:, -1], q) and np.array_equal(qdt[:, -1], qd)
    for b in range(_full(size)):
        ref = _reference(oracle_lib, size, b)
        errs = [(_rel(qt[b, k], ref["qtraj"][k]), _rel(qdt[b, k], ref["qdtraj"][k])) for k in range(nsteps)]
        print("size %s b %d: per step (|q - proto|, |qd - proto|) relative: %s" % (size, b, ", ".join("(%.1e, %.1e)" % e for e in errs)))
        for k in range(nsteps):
            assert max(errs[k]) <= 1e-9, (size, b, k, errs[k])


@pytest.mark.gpu
def test_step_bdf2_after_the_tape_does_not_take_the_start_step_again():
    """The history is in place: two more BDF2 steps after a 4-step tape are rows 5 and 6 of a 6-step tape with zero torques there, to
    the forward bound (rmx_step_bdf2 runs the line-searched Newton, the tape the plain one: the same solutions to tol) - and a start
    step taken again would show at the size of the SDIRK2 / BDF2 truncation difference, orders above it."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(5)
    u = cs["u"].copy()
    u[:, 4:] = 0.0
    sim = BatchSim(sc, batch=B)
    sim.set_state(cs["q0"], cs["qd0"])
    qt6, qdt6, _ = sim.rollout_tape(6, sc.h, u, pscale=sc.task["pscale"], integrator=2)
    sim.set_state(cs["q0"], cs["qd0"])
    qt4, _, _ = sim.rollout_tape(4, sc.h, u[:, :4], pscale=sc.task["pscale"], integrator=2)
    assert np.array_equal(qt4, qt6[:, :4])
    sim.step_bdf2(2, h=sc.h)
    q, qd = sim.get_state()
    sim.close()
    print("continued by step_bdf2: |q - tape| %.3e |qd - tape| %.3e" % (_rel(q, qt6[:, 5]), _rel(qd, qdt6[:, 5])))
    assert _rel(q, qt6[:, 5]) <= 1e-9 and _rel(qd, qdt6[:, 5]) <= 1e-9


# ---------------------------------------------------------------- 2. against the proto

@pytest.mark.gpu
@pytest.mark.parametrize("size,nsteps", [(s, None) for s in SIZES] + [(5, 1), (5, 2)])
def test_gradients_meet_the_proto(oracle_lib, size, nsteps):
    """du, dq0, dqd0 to 1e-7 relative, the bound the suite holds dPdp to against the oracle.  The three smallest scenes in full, the
    32- and 40-link scenes rollout 0; on the 5-link chain also nsteps 1 (the start step alone) and 2 (the first BDF2 step)."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, nsteps)
    sim = BatchSim(sc, batch=B)
    _, _, du, dq0, dqd0 = _tape_and_vjp(sim, sc, cs)
    sim.close()
    for b in range(_full(size)):
        ref = _reference(oracle_lib, size, b, nsteps)
        errs = (_rel(du[b], ref["du"]), _rel(dq0[b], ref["dq0"]), _rel(dqd0[b], ref["dqd0"]))
        print("size %s nsteps %d b %d: du %.3e dq0 %.3e dqd0 %.3e (relative to the proto)" % ((size, nsteps, b) + errs))
        assert max(errs) <= 1e-7, (size, nsteps, b, errs)


# ---------------------------------------------------------------- 3. the testGrad identity on the device

@pytest.mark.gpu
@pytest.mark.parametrize("n,nsteps", [(5, 6), (16, 5)])
def test_gradients_meet_the_testgrad_identity(n, nsteps):
    """Central differences (eps = 1e-5, 3 random directions per group, one batch of 24 rollouts) of the proto test's loss along
    directions in u - the k = 1 row included, which the adjoint calls only approximate -, in q0, in qdot0 and in all three jointly,
    against direction . gradient.  Tolerance: rtol 2e-5, atol 1e-6 max|ana|, the floor of the BDF1 file's rule and, as in
    test_gpu_adjoint_controls.py under BDF2 (where the constant-parameter call's own figure is the reference's start-step
    approximation and says nothing), the whole of it."""
    from redmax_amd import BatchSim
    sc = _scene(n, 2)
    cs = {k: v[0] for k, v in case(sc, 23, nsteps=nsteps).items()}
    one = BatchSim(sc, batch=1)
    _, _, du, dq0, dqd0 = _tape_and_vjp(one, sc, {k: v[None] for k, v in cs.items()})
    one.close()
    grads = {"u": du[0], "q0": dq0[0], "qd0": dqd0[0]}
    nd, eps = 3, 1e-5
    rng = np.random.default_rng(29)
    groups = [("u",), ("q0",), ("qd0",), ("u", "q0", "qd0")]
    dirs, pert = [], {k: [] for k in grads}
    for g in groups:
        for _ in range(nd):
            d = {k: (rng.standard_normal(grads[k].shape) if k in g else np.zeros(grads[k].shape)) for k in grads}
            dirs.append(d)
            for sgn in (1.0, -1.0):
                for k in grads:
                    pert[k].append(cs[k] + sgn * eps * d[k])
    nb = len(pert["u"])
    fd = BatchSim(sc, batch=nb)
    fd.set_state(np.array(pert["q0"]), np.array(pert["qd0"]))
    qt, qdt, info = fd.rollout_tape(nsteps, sc.h, np.array(pert["u"]), pscale=sc.task["pscale"], stats=True, integrator=2)
    fd.close()
    assert (info["status"] & 15 == 0).all()
    L = np.array([proto.loss_and_cotangents(qt[i], qdt[i], cs["c"], cs["d"])[0] for i in range(nb)])
    num = (L[0::2] - L[1::2]) / (2 * eps)
    ana = np.array([sum(float((d[k] * grads[k]).sum()) for k in grads) for d in dirs])
    shown = []
    for i, g in enumerate(groups):
        a, e = ana[i * nd:(i + 1) * nd], np.abs(num - ana)[i * nd:(i + 1) * nd]
        shown.append(e.max() / np.abs(a).max())
    print("bdf2 testgrad n %d nsteps %d: u %.3e, q0 %.3e, qdot0 %.3e, jointly %.3e (of max|ana|)" % ((n, nsteps) + tuple(shown)))
    for i, g in enumerate(groups):
        a, e = ana[i * nd:(i + 1) * nd], np.abs(num - ana)[i * nd:(i + 1) * nd]
        assert np.abs(a).max() > 0
        assert (e <= 2e-5 * np.abs(a) + 1e-6 * np.abs(a).max()).all(), (g, num[i * nd:(i + 1) * nd], a, e)


# ---------------------------------------------------------------- 4. exact structure

@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, 16, "tree16", 32, 40])
def test_zeros_causality_batch_independence_and_repeatability(size):
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size)
    sim = BatchSim(sc, batch=B)
    qt, qdt, du, dq0, dqd0 = _tape_and_vjp(sim, sc, cs)
    state = sim.get_state()
    assert np.abs(du).min(axis=2).min() > 0 and np.abs(dq0).max() > 0 and np.abs(dqd0).max() > 0
    gq, gqd = cs["c"] + qt, cs["d"]
    # a second call on the same tape: the same bits, and the state is where the rollout left it
    for a, b in zip(sim.rollout_vjp(nsteps, gq, gqd), (du, dq0, dqd0)):
        assert np.array_equal(a, b)
    assert all(np.array_equal(a, b) for a, b in zip(sim.get_state(), state))
    # zero cotangents: exactly zero
    for a in sim.rollout_vjp(nsteps, np.zeros_like(gq), np.zeros_like(gqd)):
        assert not a.any()
    # cotangents that are zero behind step k: du rows behind k are exactly zero, the ones up to k are not
    for k in (nsteps // 2, 1):
        gq_k, gqd_k = gq.copy(), gqd.copy()
        gq_k[:, k:], gqd_k[:, k:] = 0.0, 0.0
        du_k, dq0_k, _ = sim.rollout_vjp(nsteps, gq_k, gqd_k)
        assert not du_k[:, k:].any() and np.abs(du_k[:, :k]).max(axis=2).min() > 0 and dq0_k.any()
    # du alone (dq0, dqd0 not requested): the same du
    du_only, none0, none1 = sim.rollout_vjp(nsteps, gq, gqd, initial_state=False)
    assert none0 is None and none1 is None and np.array_equal(du_only, du)
    # step calls and set_state leave the tape alone
    sim.set_state(cs["q0"], cs["qd0"])
    sim.step_bdf2(2, h=sc.h)
    for a, b in zip(sim.rollout_vjp(nsteps, gq, gqd), (du, dq0, dqd0)):
        assert np.array_equal(a, b)
    # no record asked for: the same rollout
    none0, none1, _ = _tape(sim, sc, cs, trajectory=False)
    assert none0 is None and none1 is None and np.array_equal(sim.get_state()[0], qt[:, -1])
    assert np.array_equal(sim.rollout_vjp(nsteps, gq, gqd)[0], du)
    sim.close()
    # rollout b of the batch is a batch-of-one call, bit for bit
    one = BatchSim(sc, batch=1)
    for b in range(B):
        for a, ref in zip(_tape_and_vjp(one, sc, cs, slice(b, b + 1)), (qt, qdt, du, dq0, dqd0)):
            assert np.array_equal(a[0], ref[b]), (size, b)
    one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [16, "tree16", 5])
def test_no_helper_wave_runs(size, monkeypatch):
    """Batches this small give the BDF1 tape of the 16-link chain its helper wave; the BDF2 tape runs one wavefront per rollout whatever
    RMX_ADJ_HELP says - the full-chain form at 16 links -, with the same bits."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size)
    res = []
    for helper in ("1", "0"):
        monkeypatch.setenv("RMX_ADJ_HELP", helper)
        sim = BatchSim(sc, batch=B)
        res.append(_tape_and_vjp(sim, sc, cs))
        assert sim.last_step_kernel() == ("k_adjoint_fwd<16,bdf2,tape,fullchain>" if size == 16 else "k_adjoint_fwd<bdf2,tape>")
        sim.close()
    assert np.abs(res[0][2]).sum() > 0
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_device_form_equals_the_host_form():
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(16)
    sim = BatchSim(sc, batch=B)
    qt, qdt, du, dq0, dqd0 = _tape_and_vjp(sim, sc, cs)
    nan = np.full(qt.shape, np.nan)
    u_d, qt_d, qdt_d = _DevArray(cs["u"]), _DevArray(nan), _DevArray(nan)
    sim.set_state(cs["q0"], cs["qd0"])
    info = sim.rollout_tape_device(nsteps, sc.h, u_d.ptr.value, qt_d.ptr.value, qdt_d.ptr.value, pscale=sc.task["pscale"], stats=True,
                                   integrator=2)
    assert (info["status"] & 15 == 0).all()
    assert np.array_equal(qt_d.get(), qt) and np.array_equal(qdt_d.get(), qdt) and np.array_equal(u_d.get(), cs["u"])
    gq_d, gqd_d, du_d = _DevArray(cs["c"] + qt), _DevArray(cs["d"]), _DevArray(nan)
    dq0_d, dqd0_d = _DevArray(np.full(dq0.shape, np.nan)), _DevArray(np.full(dq0.shape, np.nan))
    sim.rollout_vjp_device(nsteps, gq_d.ptr.value, gqd_d.ptr.value, du_d.ptr.value, dq0_d.ptr.value, dqd0_d.ptr.value)
    assert np.array_equal(du_d.get(), du) and np.array_equal(dq0_d.get(), dq0) and np.array_equal(dqd0_d.get(), dqd0)
    assert np.array_equal(gq_d.get(), cs["c"] + qt) and np.array_equal(gqd_d.get(), cs["d"])
    du2_d = _DevArray(nan)
    sim.rollout_vjp_device(nsteps, gq_d.ptr.value, gqd_d.ptr.value, du2_d.ptr.value)       # dq0, dqd0 not requested
    assert np.array_equal(du2_d.get(), du)
    for d in (u_d, qt_d, qdt_d, gq_d, gqd_d, du_d, dq0_d, dqd0_d, du2_d):
        d.free()
    sim.close()


# ---------------------------------------------------------------- 5. tape bookkeeping and refusals

@pytest.mark.gpu
def test_tape_bookkeeping():
    from redmax_amd import BatchSim, _abi
    sc, cs, nsteps = _setup(5)
    sim = BatchSim(sc, batch=B)
    z = np.zeros((B, nsteps, sc.nr))
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        sim.rollout_vjp(nsteps, z, z)
    qt2, qdt2, du2, dq02, dqd02 = _tape_and_vjp(sim, sc, cs)
    with pytest.raises(_abi.RedMaxHipError, match="nsteps differs"):
        sim.rollout_vjp(nsteps - 1, z[:, 1:], z[:, 1:])
    assert np.array_equal(sim.rollout_vjp(nsteps, cs["c"] + qt2, cs["d"])[0], du2)        # (the refused call left the tape alone)
    # a BDF1 tape replaces the BDF2 tape: the vjp follows the last one
    qt1, qdt1, du1, dq01, dqd01 = _tape_and_vjp(sim, sc, cs, integrator=1)
    fresh = BatchSim(sc, batch=B)
    for a, b in zip(_tape_and_vjp(fresh, sc, cs, integrator=1), (qt1, qdt1, du1, dq01, dqd01)):
        assert np.array_equal(a, b)
    fresh.close()
    assert not np.array_equal(qt1, qt2) and not np.array_equal(du1, du2)
    assert np.array_equal(sim.rollout_vjp(nsteps, cs["c"] + qt1, cs["d"])[0], du1)
    # ... and the reverse
    for a, b in zip(_tape_and_vjp(sim, sc, cs), (qt2, qdt2, du2, dq02, dqd02)):
        assert np.array_equal(a, b)
    # a shorter BDF2 tape after a longer one, then its vjp
    sc3, cs3, n3 = _setup(5, 2)
    short = _tape_and_vjp(sim, sc3, cs3)
    fresh = BatchSim(sc, batch=B)
    for a, b in zip(_tape_and_vjp(fresh, sc3, cs3), short):
        assert np.array_equal(a, b)
    fresh.close()
    with pytest.raises(_abi.RedMaxHipError, match="nsteps differs"):
        sim.rollout_vjp(nsteps, z, z)
    # an adjoint call reuses the workspace: the tape is gone
    _tape_and_vjp(sim, sc, cs)
    sim.adjoint_controls(nsteps, sc.h, dict(sc.task, t=nsteps * sc.h), cs["u"], integrator=2)
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        sim.rollout_vjp(nsteps, z, z)
    # arguments
    for bad in (3, 0, "2", None):
        with pytest.raises(ValueError, match="integrator"):
            sim.rollout_tape(nsteps, sc.h, cs["u"], integrator=bad)
        with pytest.raises(ValueError, match="integrator"):
            sim.rollout_tape_device(nsteps, sc.h, 0, 0, 0, integrator=bad)
    d = _DevArray(z)
    with pytest.raises(_abi.RedMaxHipError, match="null"):
        sim.rollout_tape_device(nsteps, sc.h, None, None, None, integrator=2)
    with pytest.raises(_abi.RedMaxHipError, match="together"):
        sim.rollout_tape_device(nsteps, sc.h, d.ptr.value, d.ptr.value, None, integrator=2)
    d.free()
    with pytest.raises(_abi.RedMaxHipError, match="nsteps < 1"):
        sim.rollout_tape(0, sc.h, np.zeros((B, 0, sc.nr)), integrator=2)
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["chart", "point forces", "ground", "big"])
def test_models_outside_the_adjoint_path_are_refused(kind):
    """Scene 7 (Euler charts), scene 12 (point forces), scene 11 (ground contact) and a 100-link chain: rmx_rollout_tape_bdf2 refuses
    them with the words of rmx_rollout_tape, host and device form, and the batch still steps afterwards as one that was never asked."""
    from redmax_amd import BatchSim, _abi
    from redmax_amd.scenes import sceneChain, scenesRedMax
    sc = {"chart": lambda: scenesRedMax(7), "point forces": lambda: scenesRedMax(12), "ground": lambda: scenesRedMax(11),
          "big": lambda: sceneChain(100)}[kind]()
    sc.init()
    words = {"chart": "spherical joints", "point forces": "point forces", "ground": "ground contact", "big": "more than 64 nodes"}[kind]
    nsteps, Bs = 2, 2
    u = np.zeros((Bs, nsteps, sc.nr))
    q0, qd0 = sc.getQ()
    fresh, sim = BatchSim(sc, batch=Bs), BatchSim(sc, batch=Bs)
    for s in (fresh, sim):
        s.set_state(q0[None, :], qd0[None, :])
    with pytest.raises(_abi.RedMaxHipError, match=words) as bdf1:
        sim.rollout_tape(nsteps, sc.h, u)
    with pytest.raises(_abi.RedMaxHipError, match=words) as bdf2:
        sim.rollout_tape(nsteps, sc.h, u, integrator=2)
    assert str(bdf2.value).split(": ", 1)[1] == str(bdf1.value).split(": ", 1)[1]        # (behind the name of the entry point)
    u_d = _DevArray(u)
    with pytest.raises(_abi.RedMaxHipError, match=words):
        sim.rollout_tape_device(nsteps, sc.h, u_d.ptr.value, None, None, integrator=2)
    u_d.free()
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        sim.rollout_vjp(nsteps, u, u)
    out, ref = sim.step_bdf2(3, h=sc.h, stats=True), fresh.step_bdf2(3, h=sc.h, stats=True)
    qa, qda = sim.get_state()
    qb, qdb = fresh.get_state()
    sim.close()
    fresh.close()
    assert (out["status"] & 15 == 0).all() and np.isfinite(qa).all()
    assert np.array_equal(qa, qb) and np.array_equal(qda, qdb) and np.array_equal(out["newton_iters"], ref["newton_iters"])


# ---------------------------------------------------------------- 6. torch

@pytest.mark.gpu
def test_torch_backward_is_the_vjp_and_gradcheck_passes():
    import torch
    from redmax_amd import BatchSim, diff
    Bt, nsteps = 2, 3
    sc = _scene(5, 2)
    cs = case(sc, 37, nsteps=nsteps, B=Bt)
    dev = torch.device("cuda", 0)
    t = {k: torch.tensor(cs[k], dtype=torch.float64, device=dev) for k in ("q0", "qd0", "u", "c", "d")}
    pscale = sc.task["pscale"]
    sim = BatchSim(sc, batch=Bt)
    res = {}
    for integ in (2, 1):
        q0, qd0, u = (t[k].clone().requires_grad_(True) for k in ("q0", "qd0", "u"))
        qt, qdt = diff.rollout(sim, q0, qd0, u, h=sc.h, pscale=pscale, integrator=integ)
        loss = (t["c"] * qt).sum() + (t["d"] * qdt).sum() + 0.5 * (qt ** 2).sum()
        loss.backward()
        ref = BatchSim(sc, batch=Bt)
        ref.set_state(cs["q0"], cs["qd0"])
        qtr, qdtr, _ = ref.rollout_tape(nsteps, sc.h, cs["u"], pscale=pscale, integrator=integ)
        du, dq0, dqd0 = ref.rollout_vjp(nsteps, cs["c"] + qtr, cs["d"])
        ref.close()
        assert np.array_equal(qt.detach().cpu().numpy(), qtr) and np.array_equal(qdt.detach().cpu().numpy(), qdtr)
        assert np.array_equal(u.grad.cpu().numpy(), du) and np.array_equal(q0.grad.cpu().numpy(), dq0)
        assert np.array_equal(qd0.grad.cpu().numpy(), dqd0)
        res[integ] = qtr
    # integrator=1 is the default, and still the BDF1 rollout
    qt_default, _ = diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, pscale=pscale)
    assert np.array_equal(qt_default.cpu().numpy(), res[1]) and not np.array_equal(res[1], res[2])
    with pytest.raises(ValueError, match="integrator"):
        diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, pscale=pscale, integrator=3)

    # (a sim holds ONE tape and gradcheck keeps several graphs alive: every call gets a sim of its own, as in the BDF1 file)
    sims = []

    def f(a, b, c):
        sims.append(BatchSim(sc, batch=Bt))
        return diff.rollout(sims[-1], a, b, c, h=sc.h, pscale=pscale, integrator=2)

    assert torch.autograd.gradcheck(f, tuple(t[k].clone().requires_grad_(True) for k in ("q0", "qd0", "u")))
    for s_ in sims:
        s_.close()
    sim.close()


# ---------------------------------------------------------------- 7. the MEX command

@pytest.mark.gpu
def test_mex_command_equals_the_ctypes_call(gw):  # noqa: F811
    """'rollout_tape' with the seventh argument through the gateway (stub): 2 is the BDF2 tape, 1 and none the BDF1 tape; 'rollout_vjp'
    follows the tape."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(5)
    sim = BatchSim(sc, batch=B)
    res = {}
    for integ in (1, 2):
        qt, qdt, info = _tape(sim, sc, cs, integrator=integ, stats=True)
        res[integ] = (qt, qdt, info) + sim.rollout_vjp(nsteps, cs["c"] + qt, cs["d"]) + sim.get_state()
    sim.close()
    ps, ut = float(sc.task["pscale"]), cs["u"].transpose(2, 1, 0)
    h = gw.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    for args, integ in (((2.0,), 2), ((1.0,), 1), ((), 1)):
        qt, qdt, info, du, dq0, dqd0, q, qd = res[integ]
        gw.call(0, "set", h, cs["q0"].T, cs["qd0"].T)
        qtm, qdtm, st = gw.call(3, "rollout_tape", h, sc.h, float(nsteps), ps, ut, *args)
        assert np.array_equal(qtm.transpose(2, 1, 0), qt) and np.array_equal(qdtm.transpose(2, 1, 0), qdt)
        assert np.array_equal(st[:, 0], info["newton_iters"]) and np.array_equal(st[:, 1], info["status"])
        qm, qdm = gw.call(2, "get", h)
        assert np.array_equal(qm.T, q) and np.array_equal(qdm.T, qd)
        gq, gqd = (cs["c"] + qt).transpose(2, 1, 0), cs["d"].transpose(2, 1, 0)
        dum, dq0m, dqd0m = gw.call(3, "rollout_vjp", h, float(nsteps), gq, gqd)
        assert np.array_equal(dum.transpose(2, 1, 0), du) and np.array_equal(dq0m.T, dq0) and np.array_equal(dqd0m.T, dqd0)
    with pytest.raises(MexError, match="integrator"):
        gw.call(1, "rollout_tape", h, sc.h, float(nsteps), ps, ut, 3.0)
    gw.call(0, "destroy", h)
