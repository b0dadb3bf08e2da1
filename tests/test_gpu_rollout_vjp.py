"""rmx_rollout_tape / rmx_rollout_vjp: the differentiable controlled BDF1 rollout - a taped forward sweep, any cotangents back.

The checks, in the order of the sections below:
  1. the forward sweep is rmx_adjoint_controls' (bit for bit) and its record is the oracle's rollout;
  2. du, dq0, dqd0 meet the numpy recursion on the oracle (tests/proto_rollout_vjp.py, pinned against central differences on the CPU
     by tests/test_rollout_vjp_proto.py), which shares no code with the library;
  3. they meet the reference's testGrad identity on the device, in u, q0 and qdot0, separately and jointly;
  4. exact structure: zeros, causality, batch independence, helper wave, device pointers, repeatability, what leaves the tape alone;
  5. refusals; 6. the torch.autograd.Function; 7. the MEX commands.

Sizes by the path each takes: 5-link chain NP 8; tree7 NP 8 with branching; 16-link chain with the helper wave and, under
RMX_ADJ_HELP=0, the full-chain form; 32-link chain M, D on the matrix cores; 40-link chain the 64-lane path with H stored per iterate.
Sections 4 and 5 add an 11-link chain (16 lanes, not a full chain, with and without its helper wave) and a 3-link chain (NP 4).
"""
import numpy as np
import pytest

import proto_rollout_vjp as proto
from test_gpu_adjoint_controls import _DevArray, _fd_errors, _rel, _scene
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)
from test_rollout_vjp_proto import case

B = 3
STEPS = {3: 5, 5: 6, 11: 5, 16: 5, 32: 4, 40: 4, "tree7": 6}
SIZES = [5, "tree7", 16, "16-one-wave", 32, 40]
_CACHE = {}


def _setup(size, monkeypatch=None):
    """(scene, case, nsteps) of a size; "16-one-wave": the full 16-link chain without its helper wave (FullChain16)."""
    if size == "16-one-wave":
        monkeypatch.setenv("RMX_ADJ_HELP", "0")
        size = 16
    if size not in _CACHE:
        sc = _scene(size, 1)
        _CACHE[size] = (sc, case(sc, 17, nsteps=STEPS[size], B=B), STEPS[size])
    return _CACHE[size]


def _reference(orc, size, b):
    """The proto's answer for rollout b of a size, computed once and left unchanged."""
    key = ("ref", size, b)
    if key not in _CACHE:
        sc, cs, _ = _setup(size)
        _CACHE[key] = proto.reference(orc, sc, cs["q0"][b], cs["qd0"][b], cs["u"][b], sc.h, sc.task["pscale"], cs["c"][b], cs["d"][b])
    return _CACHE[key]


def _tape(sim, sc, cs, sel=slice(None), **kw):
    sim.set_state(cs["q0"][sel], cs["qd0"][sel])
    return sim.rollout_tape(cs["u"].shape[1], sc.h, cs["u"][sel], pscale=sc.task["pscale"], **kw)


def _tape_and_vjp(sim, sc, cs, sel=slice(None)):
    """(qtraj, qdtraj, du, dq0, dqd0) under the loss of the proto test."""
    qt, qdt, info = _tape(sim, sc, cs, sel, stats=True)
    assert (info["status"] & 15 == 0).all()
    du, dq0, dqd0 = sim.rollout_vjp(qt.shape[1], cs["c"][sel] + qt, cs["d"][sel])
    return qt, qdt, du, dq0, dqd0


# ---------------------------------------------------------------- 1. the forward sweep

@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_forward_sweep_is_the_controls_call_and_the_oracles_rollout(oracle_lib, size, monkeypatch):
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, monkeypatch)
    size = 16 if size == "16-one-wave" else size
    sim = BatchSim(sc, batch=B)
    sim.set_state(cs["q0"], cs["qd0"])
    _, none, ic = sim.adjoint_controls(nsteps, sc.h, dict(sc.task, t=nsteps * sc.h), cs["u"], stats=True, gradient=False)
    qc, qdc = sim.get_state()
    qt, qdt, info = _tape(sim, sc, cs, stats=True)
    q, qd = sim.get_state()
    sim.close()
    assert none is None and (info["status"] & 15 == 0).all()
    assert np.array_equal(q, qc) and np.array_equal(qd, qdc)
    assert np.array_equal(info["newton_iters"], ic["newton_iters"]) and np.array_equal(info["status"], ic["status"])
    assert np.array_equal(qt[:, -1], q) and np.array_equal(qdt[:, -1], qd)
    for b in range(B if size in (5, "tree7", 16) else 1):
        ref = _reference(oracle_lib, size, b)
        for k in range(nsteps):
            assert _rel(qt[b, k], ref["qtraj"][k]) <= 1e-9, (size, b, k, _rel(qt[b, k], ref["qtraj"][k]))
        print("size %s b %d: |qdtraj - oracle| / |oracle| = %.3e" % (size, b, _rel(qdt[b], ref["qdtraj"])))
    # the recorded qdot is (q_k - q_{k-1}) / h of the recorded q, up to the rounding of that difference: two roundings of q over h
    qprev = np.concatenate([cs["q0"][:, None], qt[:, :-1]], axis=1)
    assert (np.abs(qdt - (qt - qprev) / sc.h) <= 4 * np.finfo(float).eps * np.abs(qt).max() / sc.h).all()


# ---------------------------------------------------------------- 2. against the proto

@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_gradients_meet_the_proto(oracle_lib, size, monkeypatch):
    """du, dq0, dqd0 to 1e-7 relative, the bound the suite holds dPdp to against the oracle.  The three smallest scenes in full, the
    32- and 40-link scenes rollout 0."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, monkeypatch)
    size = 16 if size == "16-one-wave" else size
    sim = BatchSim(sc, batch=B)
    _, _, du, dq0, dqd0 = _tape_and_vjp(sim, sc, cs)
    sim.close()
    for b in range(B if size in (5, "tree7", 16) else 1):
        ref = _reference(oracle_lib, size, b)
        errs = (_rel(du[b], ref["du"]), _rel(dq0[b], ref["dq0"]), _rel(dqd0[b], ref["dqd0"]))
        print("size %s b %d: du %.3e dq0 %.3e dqd0 %.3e (relative to the proto)" % ((size, b) + errs))
        assert max(errs) <= 1e-7, (size, b, errs)


# ---------------------------------------------------------------- 3. the testGrad identity on the device

@pytest.mark.gpu
@pytest.mark.parametrize("n,nsteps", [(5, 6), (16, 5)])
def test_gradients_meet_the_testgrad_identity(n, nsteps):
    """Central differences (eps = 1e-5, 3 random directions per group, one batch of 24 rollouts) of the proto test's loss along
    directions in u, in q0, in qdot0 and in all three jointly, against direction . gradient.  Tolerance as in
    test_gpu_adjoint_controls.py::test_gradient_meets_the_testgrad_identity: twice what the constant-parameter call shows in the same
    run, never tighter than rtol 2e-5, atol 1e-6 max|ana|.

    Measured on MI355X, max over the 3 directions of |num - ana| / max|ana|:
        n  nsteps   constant call      u         q0        qdot0     jointly
        5     6       7.2e-10       8.1e-11   1.8e-10   5.7e-10   8.8e-11
       16     5       1.5e-09       6.8e-10   1.6e-10   3.7e-10   1.7e-10
    so the floor is what binds in every case.
    """
    from redmax_amd import BatchSim
    sc = _scene(n, 1)
    num_c, ana_c = _fd_errors(sc, nsteps, nsteps // 2, 1, controls=False)
    measured = float(np.abs(num_c - ana_c).max() / np.abs(ana_c).max())
    cs = {k: v[0] for k, v in case(sc, 23, nsteps=nsteps).items()}
    one = BatchSim(sc, batch=1)
    one1 = {k: v[None] for k, v in cs.items()}
    _, _, du, dq0, dqd0 = _tape_and_vjp(one, sc, one1)
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
    qt, qdt, info = fd.rollout_tape(nsteps, sc.h, np.array(pert["u"]), pscale=sc.task["pscale"], stats=True)
    fd.close()
    assert (info["status"] & 15 == 0).all()
    L = np.array([proto.loss_and_cotangents(qt[i], qdt[i], cs["c"], cs["d"])[0] for i in range(nb)])
    num = (L[0::2] - L[1::2]) / (2 * eps)
    ana = np.array([sum(float((d[k] * grads[k]).sum()) for k in grads) for d in dirs])
    shown = []
    for i, g in enumerate(groups):
        a, e = ana[i * nd:(i + 1) * nd], np.abs(num - ana)[i * nd:(i + 1) * nd]
        shown.append(e.max() / np.abs(a).max())
        assert np.abs(a).max() > 0
        floor = 2e-5 * np.abs(a) + 1e-6 * np.abs(a).max()
        tol = np.maximum(2.0 * measured * np.abs(a).max(), floor)
        assert (e <= tol).all(), (g, num[i * nd:(i + 1) * nd], a, e, tol)
    print("testgrad n %d nsteps %d: constant call %.3e; u %.3e, q0 %.3e, qdot0 %.3e, jointly %.3e (of max|ana|)"
          % ((n, nsteps, measured) + tuple(shown)))


# ---------------------------------------------------------------- 4. exact structure

@pytest.mark.gpu
@pytest.mark.parametrize("size", [3, 5, 16, 32, 40])
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
    k = nsteps // 2
    gq_k, gqd_k = gq.copy(), gqd.copy()
    gq_k[:, k:], gqd_k[:, k:] = 0.0, 0.0
    du_k, dq0_k, _ = sim.rollout_vjp(nsteps, gq_k, gqd_k)
    assert not du_k[:, k:].any() and np.abs(du_k[:, :k]).max(axis=2).min() > 0 and dq0_k.any()
    # du alone (dq0, dqd0 not requested): the same du
    du_only, none0, none1 = sim.rollout_vjp(nsteps, gq, gqd, initial_state=False)
    assert none0 is None and none1 is None and np.array_equal(du_only, du)
    # step calls and set_state leave the tape alone
    sim.set_state(cs["q0"], cs["qd0"])
    sim.step_bdf1(2, h=sc.h)
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
@pytest.mark.parametrize("size", [16, 11])
def test_helper_wave_on_and_off_agree(size, monkeypatch):
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size)
    res = []
    for helper in ("0", "1"):
        monkeypatch.setenv("RMX_ADJ_HELP", helper)
        sim = BatchSim(sc, batch=B)
        res.append(_tape_and_vjp(sim, sc, cs))
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
    info = sim.rollout_tape_device(nsteps, sc.h, u_d.ptr.value, qt_d.ptr.value, qdt_d.ptr.value, pscale=sc.task["pscale"], stats=True)
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


# ---------------------------------------------------------------- 5. refusals

@pytest.mark.gpu
def test_refusals():
    from redmax_amd import BatchSim, _abi
    sc, cs, nsteps = _setup(5)
    sim = BatchSim(sc, batch=B)
    z = np.zeros((B, nsteps, sc.nr))
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        sim.rollout_vjp(nsteps, z, z)
    qt, qdt, du, dq0, dqd0 = _tape_and_vjp(sim, sc, cs)
    with pytest.raises(_abi.RedMaxHipError, match="nsteps differs"):
        sim.rollout_vjp(nsteps - 1, z[:, 1:], z[:, 1:])
    with pytest.raises(_abi.RedMaxHipError, match="null"):
        sim.rollout_vjp_device(nsteps, None, None, None)
    d = _DevArray(z)
    with pytest.raises(_abi.RedMaxHipError, match="together"):
        sim.rollout_vjp_device(nsteps, d.ptr.value, d.ptr.value, d.ptr.value, d.ptr.value, None)
    with pytest.raises(_abi.RedMaxHipError, match="null"):
        sim.rollout_tape_device(nsteps, sc.h, None, None, None)
    with pytest.raises(_abi.RedMaxHipError, match="together"):
        sim.rollout_tape_device(nsteps, sc.h, d.ptr.value, d.ptr.value, None)
    d.free()
    with pytest.raises(_abi.RedMaxHipError, match="nsteps < 1"):
        sim.rollout_tape(0, sc.h, np.zeros((B, 0, sc.nr)))
    for bad in (np.zeros((B, nsteps + 1, sc.nr)), np.zeros((B, sc.nr)), np.zeros((nsteps, sc.nr + 1))):
        with pytest.raises(ValueError, match="shape"):
            sim.rollout_tape(nsteps, sc.h, bad)
    with pytest.raises(ValueError, match="shape"):
        sim.rollout_vjp(nsteps, z[:, 1:], z)
    # the refused calls left the tape alone (the refused rollout_tape calls never reached the workspace)
    assert np.array_equal(sim.rollout_vjp(nsteps, cs["c"] + qt, cs["d"])[0], du)
    # an adjoint call reuses the workspace: the tape is gone
    sim.adjoint_controls(nsteps, sc.h, dict(sc.task, t=nsteps * sc.h), cs["u"])
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        sim.rollout_vjp(nsteps, z, z)
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["chart", "point forces", "ground", "big"])
def test_models_outside_the_adjoint_path_are_refused(kind):
    """Scene 7 (Euler charts), scene 12 (point forces), scene 11 (ground contact) and a 100-link chain: rmx_rollout_tape refuses them
    with the words of rmx_adjoint_controls, host and device form, and the batch still steps afterwards as one that was never asked."""
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
    with pytest.raises(_abi.RedMaxHipError, match=words) as ctl:
        sim.adjoint_controls(nsteps, sc.h, dict(body=0, xlocal=[0.0, 0.0, 0.0], xtarget=[0.0, 0.0, 0.0], step=nsteps, pscale=1.0, wreg=0.0,
                                                wpos=1.0), u)
    with pytest.raises(_abi.RedMaxHipError, match=words) as tape:
        sim.rollout_tape(nsteps, sc.h, u)
    assert str(tape.value).split(": ", 1)[1] == str(ctl.value).split(": ", 1)[1]        # (behind the name of the entry point)
    u_d = _DevArray(u)
    with pytest.raises(_abi.RedMaxHipError, match=words):
        sim.rollout_tape_device(nsteps, sc.h, u_d.ptr.value, None, None)
    u_d.free()
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        sim.rollout_vjp(nsteps, u, u)
    out, ref = sim.step_bdf1(3, h=sc.h, stats=True), fresh.step_bdf1(3, h=sc.h, stats=True)
    qa, qda = sim.get_state()
    qb, qdb = fresh.get_state()
    sim.close()
    fresh.close()
    assert (out["status"] & 15 == 0).all() and np.isfinite(qa).all()
    assert np.array_equal(qa, qb) and np.array_equal(qda, qdb) and np.array_equal(out["newton_iters"], ref["newton_iters"])


# ---------------------------------------------------------------- 6. torch

def _torch_case(Bt, nsteps):
    import torch
    sc = _scene(5, 1)
    cs = case(sc, 37, nsteps=nsteps, B=Bt)
    dev = torch.device("cuda", 0)
    t = {k: torch.tensor(cs[k], dtype=torch.float64, device=dev) for k in ("q0", "qd0", "u", "c", "d")}
    return sc, cs, t


@pytest.mark.gpu
def test_torch_backward_is_the_vjp_and_gradcheck_passes():
    import torch
    from redmax_amd import BatchSim, diff
    Bt, nsteps = 2, 3
    sc, cs, t = _torch_case(Bt, nsteps)
    pscale = sc.task["pscale"]
    sim = BatchSim(sc, batch=Bt)
    q0, qd0, u = (t[k].clone().requires_grad_(True) for k in ("q0", "qd0", "u"))
    qt, qdt = diff.rollout(sim, q0, qd0, u, h=sc.h, pscale=pscale)
    loss = (t["c"] * qt).sum() + (t["d"] * qdt).sum() + 0.5 * (qt ** 2).sum()
    loss.backward()
    ref = BatchSim(sc, batch=Bt)
    qtr, qdtr, du, dq0, dqd0 = _tape_and_vjp(ref, sc, cs)
    ref.close()
    assert np.array_equal(qt.detach().cpu().numpy(), qtr) and np.array_equal(qdt.detach().cpu().numpy(), qdtr)
    assert np.array_equal(u.grad.cpu().numpy(), du) and np.array_equal(q0.grad.cpu().numpy(), dq0)
    assert np.array_equal(qd0.grad.cpu().numpy(), dqd0)
    # a loss on qtraj alone: the missing cotangent is zeros
    q0b, qd0b, ub = (t[k].clone().requires_grad_(True) for k in ("q0", "qd0", "u"))
    qt2, _ = diff.rollout(sim, q0b, qd0b, ub, h=sc.h, pscale=pscale)
    qt2.sum().backward()
    assert torch.isfinite(ub.grad).all() and ub.grad.abs().sum() > 0

    # gradcheck keeps the graphs of several of its calls alive while it makes further ones (the first call's through all the
    # finite-difference calls, and one per output in its undefined-gradient check); a sim holds ONE tape, so every call gets a sim
    # of its own here
    sims = []

    def f(a, b, c):
        sims.append(BatchSim(sc, batch=Bt))
        return diff.rollout(sims[-1], a, b, c, h=sc.h, pscale=pscale)

    assert torch.autograd.gradcheck(f, tuple(t[k].clone().requires_grad_(True) for k in ("q0", "qd0", "u")))
    for s_ in sims:
        s_.close()
    sim.close()


@pytest.mark.gpu
def test_torch_rejects_what_it_cannot_take():
    import torch
    from redmax_amd import BatchSim, diff
    Bt, nsteps = 2, 3
    sc, cs, t = _torch_case(Bt, nsteps)
    sim = BatchSim(sc, batch=Bt)
    with pytest.raises(ValueError, match="float64"):
        diff.rollout(sim, t["q0"].float(), t["qd0"], t["u"], h=sc.h)
    with pytest.raises(ValueError, match="device"):
        diff.rollout(sim, t["q0"], t["qd0"], t["u"].cpu(), h=sc.h)
    with pytest.raises(ValueError, match="torch.Tensor"):
        diff.rollout(sim, cs["q0"], t["qd0"], t["u"], h=sc.h)
    with pytest.raises(ValueError, match="shape"):
        diff.rollout(sim, t["q0"][:1], t["qd0"], t["u"], h=sc.h)
    with pytest.raises(ValueError, match="shape"):
        diff.rollout(sim, t["q0"], t["qd0"], t["u"][:, :, :-1], h=sc.h)
    # backward() after a second rollout on the same sim: the tape has been replaced
    u1 = t["u"].clone().requires_grad_(True)
    qt1, _ = diff.rollout(sim, t["q0"], t["qd0"], u1, h=sc.h, pscale=sc.task["pscale"])
    diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, pscale=sc.task["pscale"])
    with pytest.raises(RuntimeError, match="the tape of this rollout has been replaced"):
        qt1.sum().backward()
    # ... and after an adjoint call
    u2 = t["u"].clone().requires_grad_(True)
    qt2, _ = diff.rollout(sim, t["q0"], t["qd0"], u2, h=sc.h, pscale=sc.task["pscale"])
    sim.adjoint_controls(nsteps, sc.h, dict(sc.task, t=nsteps * sc.h), cs["u"])
    with pytest.raises(RuntimeError, match="the tape of this rollout has been replaced"):
        qt2.sum().backward()
    # check=True: a rollout driven to "Newton diverged" (a status bit, not a fault) raises; check=False returns
    sim.opts.dxMax = 1e-12
    with pytest.raises(RuntimeError, match="Newton"):
        diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, pscale=sc.task["pscale"])
    qt3, _ = diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, pscale=sc.task["pscale"], check=False)
    assert qt3.shape == (Bt, nsteps, sc.nr)
    sim.close()


# ---------------------------------------------------------------- 7. the MEX commands

@pytest.mark.gpu
def test_mex_commands_equal_the_ctypes_calls(gw):  # noqa: F811
    """'rollout_tape' / 'rollout_vjp' through the gateway (stub), over two shards: MATLAB's nr x nsteps x B column-major arrays are
    the ABI's [B][nsteps][nr]."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(5)
    sim = BatchSim(sc, batch=B)
    qt, qdt, info = _tape(sim, sc, cs, stats=True)
    gq, gqd = cs["c"] + qt, cs["d"]
    du, dq0, dqd0 = sim.rollout_vjp(nsteps, gq, gqd)
    q, qd = sim.get_state()
    sim.close()
    h = gw.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    with pytest.raises(MexError, match="no tape"):
        gw.call(3, "rollout_vjp", h, float(nsteps), gq.transpose(2, 1, 0), gqd.transpose(2, 1, 0))
    gw.call(0, "set", h, cs["q0"].T, cs["qd0"].T)
    qtm, qdtm, st = gw.call(3, "rollout_tape", h, sc.h, float(nsteps), float(sc.task["pscale"]), cs["u"].transpose(2, 1, 0))
    assert qtm.shape == (sc.nr, nsteps, B)
    assert np.array_equal(qtm.transpose(2, 1, 0), qt) and np.array_equal(qdtm.transpose(2, 1, 0), qdt)
    assert np.array_equal(st[:, 0], info["newton_iters"]) and np.array_equal(st[:, 1], info["status"])
    qm, qdm = gw.call(2, "get", h)
    assert np.array_equal(qm.T, q) and np.array_equal(qdm.T, qd)
    dum, dq0m, dqd0m = gw.call(3, "rollout_vjp", h, float(nsteps), gq.transpose(2, 1, 0), gqd.transpose(2, 1, 0))
    assert dum.shape == (sc.nr, nsteps, B) and np.array_equal(dum.transpose(2, 1, 0), du)
    assert np.array_equal(dq0m.T, dq0) and np.array_equal(dqd0m.T, dqd0)
    with pytest.raises(MexError, match="nr x nsteps x batch"):
        gw.call(1, "rollout_tape", h, sc.h, float(nsteps), 1.0, cs["u"].transpose(2, 1, 0)[:, :-1, :])
    with pytest.raises(MexError, match="nr x nsteps x batch"):
        gw.call(1, "rollout_vjp", h, float(nsteps), gq.transpose(2, 1, 0), gqd.transpose(2, 1, 0)[:, :-1, :])
    with pytest.raises(MexError, match="nsteps differs"):
        gw.call(1, "rollout_vjp", h, float(nsteps - 1), gq.transpose(2, 1, 0)[:, 1:, :], gqd.transpose(2, 1, 0)[:, 1:, :])
    gw.call(0, "destroy", h)
