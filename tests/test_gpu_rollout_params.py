"""rmx_rollout_vjp_params: the gradient of a loss on the taped rollout with respect to the model's parameters - joint stiffness,
damping and rest position, body inertia and mass, gravity.

The checks, in the order of the sections below:
  1. every array against the numpy proto on the oracle's tape (tests/proto_rollout_params.py, pinned against central differences on
     the CPU by tests/test_rollout_params_proto.py), BDF1 and BDF2, to 1e-7 relative (norm over the array) - the bound the suite
     holds tape-derived gradients to (tests/test_gpu_rollout_linearize.py, section 1);
  2. - 5. one test per size and integrator: du, dq0, dqd0 are rollout_vjp's bits; dL/dqRest_j = (k_j / pscale) sum_k du_k[j] to 1e-12
     relative; batch independence, repeatability, one output alone, device pointers, what the call leaves alone (state, tape,
     rollout_vjp, rollout_linearize), and the forward sweep is still rmx_adjoint_controls' bit for bit;
  4. the testGrad identity on the device: central differences of rollout_tape on sims built from perturbed scenes;
  6. refusals; 7. redmax_amd.diff (model_params, rollout(params=...)); 8. the MEX command.

Sizes by the path each takes: 3 (NP 4); 5 and tree7 (NP 8, a chain and a branching tree); 16 (NP 16; under BDF1 rollout_vjp's plan is
the full-chain instantiation); 32 (NP 32); 40 (NP 64).  Inputs: case(sc, 17) and the step counts of tests/test_gpu_rollout_vjp.py.
"""
import ctypes as C

import numpy as np
import pytest

import proto_rollout_params as pp
import proto_rollout_vjp as proto1
from test_gpu_adjoint_controls import _DevArray, _fd_errors, _rel, _scene
from test_gpu_rollout_vjp import B, STEPS
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)
from test_rollout_vjp_proto import case

SIZES = [3, 5, "tree7", 16, 32, 40]
NAMES = pp.GROUPS
_CACHE = {}


def _setup(size, integ=1):
    """(scene, case, nsteps) of a size under an integrator."""
    key = (size, integ)
    if key not in _CACHE:
        sc = _scene(size, integ)
        _CACHE[key] = (sc, case(sc, 17, nsteps=STEPS[size], B=B), STEPS[size])
    return _CACHE[key]


def _reference(orc, size, integ, b):
    """The proto's answer for rollout b, computed once and left unchanged."""
    key = ("ref", size, integ, b)
    if key not in _CACHE:
        sc, cs, _ = _setup(size, integ)
        _CACHE[key] = pp.reference(orc, sc, cs["q0"][b], cs["qd0"][b], cs["u"][b], sc.h, sc.task["pscale"], cs["c"][b], cs["d"][b], integ)
    return _CACHE[key]


def _tape(sim, sc, cs, integ=1, sel=slice(None), **kw):
    sim.set_state(cs["q0"][sel], cs["qd0"][sel])
    qt, qdt, info = sim.rollout_tape(cs["u"].shape[1], sc.h, cs["u"][sel], pscale=sc.task["pscale"], integrator=integ, stats=True, **kw)
    assert (info["status"] & 15 == 0).all()
    return qt, qdt


def _tape_and_grads(sim, sc, cs, integ=1, sel=slice(None), **kw):
    """(qt, gq, gqd, du, dq0, dqd0, grads) under the loss of the proto test."""
    qt, _ = _tape(sim, sc, cs, integ, sel)
    gq, gqd = cs["c"][sel] + qt, cs["d"][sel]
    return (qt, gq, gqd) + sim.rollout_vjp_params(qt.shape[1], gq, gqd, **kw)


# ---------------------------------------------------------------- 1. against the proto on the oracle's tape

@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", [(s, 1) for s in SIZES] + [(5, 2), ("tree7", 2), (16, 2), (40, 2)])
def test_parameter_gradients_meet_the_proto(oracle_lib, size, integ):
    """All rollouts up to 16 links, rollout 0 for 32 and 40.  Measured on MI355X, over the five arrays: 2e-15 .. 1e-13
    up to 8 nodes, 1e-13 .. 2.4e-12 at 16, 32 and 40 links, BDF1 and BDF2 alike."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, integ)
    sim = BatchSim(sc, batch=B)
    grads = _tape_and_grads(sim, sc, cs, integ)[-1]
    sim.close()
    assert set(grads) == set(NAMES)
    for b in range(B if size in (3, 5, "tree7", 16) else 1):
        ref = _reference(oracle_lib, size, integ, b)["grads"]
        errs = {}
        for name in NAMES:
            assert grads[name][b].shape == ref[name].shape, name
            assert np.linalg.norm(ref[name]) > 0, name
            errs[name] = _rel(grads[name][b], ref[name])
        print("size %s integ %d b %d: " % (size, integ, b) + " ".join("%s %.3e" % (k, v) for k, v in errs.items()) + " (relative to the proto)")
        assert max(errs.values()) <= 1e-7, (size, integ, b, errs)


# ---------------------------------------------------------------- 2, 3, 5. the same bits, the qrest identity, exact structure

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_same_bits_as_the_vjp_the_qrest_identity_and_exact_structure(oracle_lib, size, integ):
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, integ)
    pscale = sc.task["pscale"]
    sim = BatchSim(sc, batch=B)
    # the forward sweep is still rmx_adjoint_controls' (which rewrites the workspace: it comes first)
    sim.set_state(cs["q0"], cs["qd0"])
    sim.adjoint_controls(nsteps, sc.h, dict(sc.task, t=nsteps * sc.h), cs["u"], integrator=integ, gradient=False)
    qc, qdc = sim.get_state()
    qt, gq, gqd, du, dq0, dqd0, grads = _tape_and_grads(sim, sc, cs, integ)
    state = sim.get_state()
    assert np.array_equal(state[0], qc) and np.array_equal(state[1], qdc)
    assert np.array_equal(qt[:, -1], qc)
    assert all(np.isfinite(grads[n]).all() and np.abs(grads[n]).max() > 0 for n in NAMES)
    # 2. du, dq0, dqd0: the bits of rollout_vjp, before and after
    count = sim.tape_count
    vjp = sim.rollout_vjp(nsteps, gq, gqd)
    assert all(np.array_equal(a, b) for a, b in zip((du, dq0, dqd0), vjp))
    X = sim.rollout_linearize(nsteps)
    # 3. dL/dqRest = k / pscale * sum_k du_k
    k = pp.values(oracle_lib, sc)["stiffness"]
    want = k[None] / pscale * du.sum(axis=1)
    err = _rel(grads["qrest"], want)
    print("size %s integ %d: qrest identity %.3e" % (size, integ, err))
    assert np.linalg.norm(want) > 0 and err <= 1e-12
    # 5. a second call: the same bits; state, tape, rollout_vjp and rollout_linearize where they were
    again = sim.rollout_vjp_params(nsteps, gq, gqd)
    assert all(np.array_equal(a, b) for a, b in zip(again[:3], (du, dq0, dqd0)))
    assert all(np.array_equal(again[3][n], grads[n]) for n in NAMES)
    assert sim.tape_count == count
    assert all(np.array_equal(a, b) for a, b in zip(sim.get_state(), state))
    assert all(np.array_equal(a, b) for a, b in zip(sim.rollout_vjp(nsteps, gq, gqd), vjp))
    assert all(np.array_equal(a, b) for a, b in zip(sim.rollout_linearize(nsteps), X))
    # one output alone, and two, without the initial state: the bits they have among all five
    for n in NAMES:
        d1, none0, none1, g1 = sim.rollout_vjp_params(nsteps, gq, gqd, want=(n,), initial_state=False)
        assert none0 is None and none1 is None and list(g1) == [n]
        assert np.array_equal(d1, du) and np.array_equal(g1[n], grads[n]), n
    g2 = sim.rollout_vjp_params(nsteps, gq, gqd, want=("grav", "stiffness"))[3]
    assert np.array_equal(g2["grav"], grads["grav"]) and np.array_equal(g2["stiffness"], grads["stiffness"])
    # the device form
    shapes = sim._param_shapes()
    dev = {n: _DevArray(np.full((B,) + shapes[n], np.nan)) for n in NAMES}
    io = [_DevArray(a) for a in (gq, gqd, np.full(du.shape, np.nan), np.full(dq0.shape, np.nan), np.full(dq0.shape, np.nan))]
    sim.rollout_vjp_params_device(nsteps, *[a.ptr.value for a in io], **{n + "_ptr": dev[n].ptr.value for n in NAMES})
    assert all(np.array_equal(io[2 + i].get().reshape(ref.shape), ref) for i, ref in enumerate((du, dq0, dqd0)))
    for n in NAMES:
        assert np.array_equal(dev[n].get().reshape(grads[n].shape), grads[n]), n
    only = _DevArray(np.full((B,) + shapes["inertia"], np.nan))
    sim.rollout_vjp_params_device(nsteps, io[0].ptr.value, io[1].ptr.value, io[2].ptr.value, inertia_ptr=only.ptr.value)
    assert np.array_equal(only.get().reshape(grads["inertia"].shape), grads["inertia"])
    for a in list(dev.values()) + io + [only]:
        a.free()
    # step calls and set_state between the tape and the call leave the result alone
    sim.set_state(cs["q0"], cs["qd0"])
    sim.step_bdf1(2, h=sc.h)
    assert all(np.array_equal(sim.rollout_vjp_params(nsteps, gq, gqd)[3][n], grads[n]) for n in NAMES)
    # a tape recorded without a trajectory of the caller's keeps the same states
    sim.set_state(cs["q0"], cs["qd0"])
    sim.rollout_tape(nsteps, sc.h, cs["u"], pscale=pscale, integrator=integ, trajectory=False)
    quiet = sim.rollout_vjp_params(nsteps, gq, gqd)
    assert np.array_equal(quiet[0], du) and all(np.array_equal(quiet[3][n], grads[n]) for n in NAMES)
    sim.close()
    # rollout b of the batch is a batch-of-one call, bit for bit
    one = BatchSim(sc, batch=1)
    for b in range(B):
        g1 = _tape_and_grads(one, sc, cs, integ, slice(b, b + 1))[-1]
        for n in NAMES:
            assert np.array_equal(g1[n][0], grads[n][b]), (size, b, n)
    one.close()


# ---------------------------------------------------------------- 4. the testGrad identity on the device

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n,nsteps", [(5, 6), (16, 5)])
def test_parameter_gradients_meet_the_testgrad_identity(oracle_lib, n, nsteps, integ):
    """Central differences (eps = 1e-5) of the proto test's loss over rollout_tape on sims built from perturbed scenes, one random
    direction per parameter group, against direction . gradient.  The direction is scaled to the group's magnitude, as in
    tests/test_rollout_params_proto.py.  Tolerance as tests/test_gpu_rollout_vjp.py::test_gradients_meet_the_testgrad_identity: twice
    what the constant-parameter call shows in the same run, never tighter than rtol 2e-5, atol 1e-6 |ana|."""
    from redmax_amd import BatchSim
    from test_rollout_params_proto import directions
    sc = _scene(n, integ)
    num_c, ana_c = _fd_errors(sc, nsteps, nsteps // 2, 1, controls=False)
    measured = float(np.abs(num_c - ana_c).max() / np.abs(ana_c).max())
    cs = {k: v[:1] for k, v in case(sc, 23, nsteps=nsteps).items()}
    one = BatchSim(sc, batch=1)
    grads = _tape_and_grads(one, sc, cs, integ)[-1]
    one.close()
    dirs = directions(pp.values(oracle_lib, sc), 29)
    dirs["inertia"][:, 4:] = dirs["inertia"][:, 3:4]      # (the library takes one mass per body: I_i(4:6) move together)
    eps, shown = 1e-5, {}
    for group in NAMES:
        L = []
        for sgn in (1.0, -1.0):
            fd = BatchSim(pp.perturbed(oracle_lib, sc, group, sgn * eps * dirs[group]), batch=1)
            qt, qdt = _tape(fd, sc, cs, integ)
            fd.close()
            L.append(proto1.loss_and_cotangents(qt[0], qdt[0], cs["c"][0], cs["d"][0])[0])
        num, ana = (L[0] - L[1]) / (2 * eps), float((grads[group][0] * dirs[group]).sum())
        shown[group] = abs(num - ana) / abs(ana)
        assert abs(ana) > 0
        assert abs(num - ana) <= max(2.0 * measured * abs(ana), 2e-5 * abs(ana) + 1e-6 * abs(ana)), (group, num, ana)
    print("testgrad n %d nsteps %d integ %d: constant call %.3e; " % (n, nsteps, integ, measured)
          + " ".join("%s %.3e" % kv for kv in shown.items()) + " (of |ana|)")


# ---------------------------------------------------------------- 6. refusals

@pytest.mark.gpu
def test_refusals():
    from redmax_amd import BatchSim, _abi
    sc, cs, nsteps = _setup(5)
    sim = BatchSim(sc, batch=B)
    z = np.zeros((B, nsteps, sc.nr))
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        sim.rollout_vjp_params(nsteps, z, z)
    qt, gq, gqd, du, dq0, dqd0, grads = _tape_and_grads(sim, sc, cs)
    with pytest.raises(_abi.RedMaxHipError, match="nsteps differs"):
        sim.rollout_vjp_params(nsteps - 1, z[:, :-1], z[:, :-1])
    io = [_DevArray(a) for a in (gq, gqd, du)]
    with pytest.raises(_abi.RedMaxHipError, match="all outputs are null"):
        sim.rollout_vjp_params_device(nsteps, *[a.ptr.value for a in io])
    for a in io:
        a.free()
    with pytest.raises(ValueError, match="want"):
        sim.rollout_vjp_params(nsteps, gq, gqd, want=("stiffness", "mass"))
    with pytest.raises(ValueError, match="want"):
        sim.rollout_vjp_params(nsteps, gq, gqd, want=())
    with pytest.raises(ValueError, match="shape"):
        sim.rollout_vjp_params(nsteps, gq[:, :-1], gqd)
    # null batch, gq, gqd, du, out: "null argument", straight through the C ABI
    L, pg = sim._L, _abi.ParamGrads(None, None, None, None, grads["grav"].ctypes.data)
    p = [_abi.dptr(a) for a in (gq, gqd, du, dq0, dqd0)]
    for hole in range(4):
        args = [sim._batch, nsteps] + p[:3] + p[3:] + [C.byref(pg)]
        args[0 if hole == 0 else hole + 1] = None
        assert L.rmx_rollout_vjp_params(*args) != 0 and b"null argument" in L.rmx_last_error()
    assert L.rmx_rollout_vjp_params(sim._batch, nsteps, p[0], p[1], p[2], p[3], p[4], None) != 0 and b"null argument" in L.rmx_last_error()
    assert L.rmx_rollout_vjp_params(sim._batch, nsteps, p[0], p[1], p[2], p[3], None, C.byref(pg)) != 0 and b"together" in L.rmx_last_error()
    # the refused calls left the tape alone
    assert all(np.array_equal(sim.rollout_vjp_params(nsteps, gq, gqd)[3][n], grads[n]) for n in NAMES)
    # an adjoint call reuses the workspace: the tape is gone
    sim.adjoint_controls(nsteps, sc.h, dict(sc.task, t=nsteps * sc.h), cs["u"])
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        sim.rollout_vjp_params(nsteps, gq, gqd)
    sim.close()


# ---------------------------------------------------------------- 7. torch

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
def test_torch_params_gradients_are_the_batch_sum_of_the_call(oracle_lib, integ):
    import torch
    from redmax_amd import BatchSim, diff
    Bt, nsteps = 2, 3
    sc = _scene(5, integ)
    cs = case(sc, 37, nsteps=nsteps, B=Bt)
    dev = torch.device("cuda", 0)
    t = {k: torch.tensor(cs[k], dtype=torch.float64, device=dev) for k in ("q0", "qd0", "u", "c", "d")}
    pscale = sc.task["pscale"]
    sim = BatchSim(sc, batch=Bt)
    p = diff.model_params(sim)
    assert set(p) == set(NAMES) and all(v.is_leaf and v.requires_grad and v.dtype == torch.float64 and v.device == dev for v in p.values())
    vals = pp.values(oracle_lib, sc)
    assert all(np.array_equal(p[n].detach().cpu().numpy(), vals[n]) for n in NAMES)

    def run(params):
        q0, qd0, u = (t[k].clone().requires_grad_(True) for k in ("q0", "qd0", "u"))
        qt, qdt = diff.rollout(sim, q0, qd0, u, h=sc.h, pscale=pscale, integrator=integ, **({} if params is None else {"params": params}))
        ((t["c"] * qt).sum() + (t["d"] * qdt).sum() + 0.5 * (qt ** 2).sum()).backward()
        return qt.detach().cpu().numpy(), qdt.detach().cpu().numpy(), [x.grad.cpu().numpy() for x in (q0, qd0, u)]

    qt0, qdt0, g0 = run(None)
    qt1, qdt1, g1 = run(p)
    # params=None: as before; with params the same tensors and input gradients
    assert np.array_equal(qt0, qt1) and np.array_equal(qdt0, qdt1) and all(np.array_equal(a, b) for a, b in zip(g0, g1))
    ref = BatchSim(sc, batch=Bt)
    qt, gq, gqd, du, dq0, dqd0, grads = _tape_and_grads(ref, sc, cs, integ)
    ref.close()
    assert np.array_equal(qt, qt1) and np.array_equal(g1[2], du) and np.array_equal(g1[0], dq0) and np.array_equal(g1[1], dqd0)
    for n in NAMES:
        got, want = p[n].grad.cpu().numpy(), grads[n].sum(axis=0)
        assert got.shape == want.shape and _rel(got, want) <= 1e-14, n
    # a subset: only the named tensors receive a gradient, and backward accumulates
    sub = {"grav": p["grav"], "damping": p["damping"]}
    before = {n: p[n].grad.clone() for n in NAMES}
    run(sub)
    for n in NAMES:
        want = 2.0 * before[n] if n in sub else before[n]
        assert torch.allclose(p[n].grad, want, rtol=1e-14, atol=0.0), n
    # what it cannot take
    with pytest.raises(ValueError, match="unknown model parameter"):
        diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, params={"mass": p["grav"]})
    with pytest.raises(ValueError, match="shape"):
        diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, params={"grav": p["stiffness"]})
    with pytest.raises(ValueError, match="float64"):
        diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, params={"grav": p["grav"].detach().float()})
    with pytest.raises(ValueError, match="device"):
        diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, params={"grav": p["grav"].detach().cpu()})
    with pytest.raises(ValueError, match="torch.Tensor"):
        diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, params={"grav": vals["grav"]})
    with pytest.raises(ValueError, match="dict"):
        diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, params=[p["grav"]])
    sim.close()


# ---------------------------------------------------------------- 8. MEX

@pytest.mark.gpu
def test_mex_command_equals_the_ctypes_call(gw):  # noqa: F811
    """'rollout_vjp_params' through the gateway (stub), over two shards: MATLAB's column-major nr x B, 6 x njoints x B and 3 x B arrays
    are the ABI's rows."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(5)
    sim = BatchSim(sc, batch=B)
    qt, gq, gqd, du, dq0, dqd0, grads = _tape_and_grads(sim, sc, cs)
    sim.close()
    h = gw.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    gqm, gqdm = gq.transpose(2, 1, 0), gqd.transpose(2, 1, 0)
    with pytest.raises(MexError, match="no tape"):
        gw.call(8, "rollout_vjp_params", h, float(nsteps), gqm, gqdm)
    gw.call(0, "set", h, cs["q0"].T, cs["qd0"].T)
    gw.call(3, "rollout_tape", h, sc.h, float(nsteps), float(sc.task["pscale"]), cs["u"].transpose(2, 1, 0))
    out = gw.call(8, "rollout_vjp_params", h, float(nsteps), gqm, gqdm)
    assert np.array_equal(np.asarray(out[0]).transpose(2, 1, 0), du)
    assert np.array_equal(np.asarray(out[1]).T, dq0) and np.array_equal(np.asarray(out[2]).T, dqd0)
    for i, n in enumerate(("stiffness", "damping", "qrest")):
        assert np.array_equal(np.asarray(out[3 + i]).T, grads[n]), n
    assert np.asarray(out[6]).shape == (6, len(sc.joints), B)
    assert np.array_equal(np.asarray(out[6]).transpose(2, 1, 0), grads["inertia"])
    assert np.array_equal(np.asarray(out[7]).T, grads["grav"])
    (only,) = (gw.call(1, "rollout_vjp_params", h, float(nsteps), gqm, gqdm),)
    assert np.array_equal(np.asarray(only).transpose(2, 1, 0), du)
    with pytest.raises(MexError, match="nsteps differs"):
        gw.call(8, "rollout_vjp_params", h, float(nsteps - 1), gqm[:, :-1], gqdm[:, :-1])
    gw.call(0, "destroy", h)
