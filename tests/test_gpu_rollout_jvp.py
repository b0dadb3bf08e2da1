"""rmx_rollout_jvp: forward-mode tangents of the taped rollout - tangents of the controls and of the initial state in, the tangents of
the whole trajectory out, several directions per sweep.

The checks, in the order of the sections below:
  1. every direction's tq, tqd against the numpy proto on the oracle's tape (tests/proto_rollout_jvp.py, pinned on the CPU by
     tests/test_rollout_jvp_proto.py), BDF1 and BDF2, to 1e-7 relative Frobenius - the bound the suite holds tape-derived gradients
     to: the GPU's H, M, D are those of the last evaluated iterate;
  2. the forward recursion done in numpy on rollout_linearize's XA, XB, XU of the same tape, to 1e-10 relative (the bound of
     test_gpu_rollout_linearize.py::test_chain_reproduces_the_vjp_of_the_same_tape);
  3. the pairing <gq, tq> + <gqd, tqd> = <du, tu> + <dq0, tq0> + <dqd0, tqd0> with rollout_vjp of the same tape;
  4. the testGrad identity on the device: central differences of rollout_tape against the JVP;
  5. exact structure, bit for bit: zeros, causality, a direction's independence of its neighbours and of ntan, NULL against zeros,
     batch independence, repeatability, the device form, what the call leaves alone;
  6. refusals; 7. torch (torch.func.jvp, forward_ad, gradcheck, jacfwd, diff.jvp); 8. the MEX command.

Sizes by the path each takes: 3 (NP 4); 5 and tree7 (NP 8); 11 and 16 (NP 16); 32 (NP 32); 40 (NP 64); BDF2 on 5, tree7, 16 and 40.
ntan in {1, 3, 9}: a part chunk of the 8 directions a wavefront carries, and a call that crosses a chunk boundary.  Inputs: case(sc, 17)
and the step counts of tests/test_gpu_rollout_vjp.py, standard-normal tangents of a fixed seed.
"""
import numpy as np
import pytest

import proto_rollout_jvp as pj
from test_gpu_adjoint_controls import _DevArray, _scene
from test_gpu_rollout_linearize import _setup, _tape
from test_gpu_rollout_vjp import B, STEPS
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)
from test_rollout_jvp_proto import TSEED, oracle_tape, tangent0
from test_rollout_vjp_proto import case

SIZES = [3, 5, "tree7", 11, 16, 32, 40]
BDF2_SIZES = [5, "tree7", 16, 40]
CASES = [(s, 1) for s in SIZES] + [(s, 2) for s in BDF2_SIZES]
# the largest pairing error tests/test_rollout_jvp_proto.py prints (numpy / LAPACK on the oracle's tape of rollout 0, direction tangent0;
# 5, tree7, 16, 32 under BDF1, 5, tree7, 16 under BDF2; all three groups of tangents and each alone): 7.32e-11, the 16-link chain
# under BDF2 with tq0 alone (5.4e-12 under BDF1)
PAIRING_CPU = 7.32e-11
KEYS = ("tu", "tq0", "tqd0")


def _tangents(sc, nsteps, ntan, nb=B):
    return pj.tangents(TSEED, nb, ntan, nsteps, sc.nr)


def _jvp(sim, nsteps, t, keys=KEYS):
    return sim.rollout_jvp(nsteps, **{k: (t[k] if k in keys else None) for k in KEYS})


# ---------------------------------------------------------------- 1. against the proto on the oracle's tape

@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", CASES)
def test_tangents_meet_the_proto(oracle_lib, size, integ):
    """9 directions (two chunks, the second with one direction).  All rollouts up to 16 links, rollout 0 for 32 and 40."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, integ)
    t = _tangents(sc, nsteps, 9)
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs, integ)
    tq, tqd = _jvp(sim, nsteps, t)
    sim.close()
    assert tq.shape == (B, 9, nsteps, sc.nr) and tqd.shape == tq.shape
    worst = 0.0
    for b in range(B if size not in (32, 40) else 1):
        _, _, _, _, H, M, D = oracle_tape(oracle_lib, size, integ, b, B)
        for d in range(9):
            rq, rqd = pj.jvp(integ, H, M, D, sc.h, sc.task["pscale"], t["tu"][b, d], t["tq0"][b, d], t["tqd0"][b, d])
            worst = max(worst, pj.rel(tq[b, d], rq), pj.rel(tqd[b, d], rqd))
        print("size %s bdf%d b %d: worst direction so far %.3e (relative Frobenius to the proto)" % (size, integ, b, worst))
    assert worst <= 1e-7, (size, integ, worst)


# ---------------------------------------------------------------- 2. the linearisation of the same tape

@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", CASES)
def test_tangents_are_the_recursion_on_the_linearisation_of_the_same_tape(size, integ):
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, integ)
    t = _tangents(sc, nsteps, 3)
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs, integ)
    tq, tqd = _jvp(sim, nsteps, t)
    XA, XB, XU = sim.rollout_linearize(nsteps)
    sim.close()
    worst = 0.0
    for b in range(B):
        for d in range(3):
            rq, rqd = pj.jvp_on_sensitivities(integ, XA[b], XB[b], XU[b], sc.h, t["tu"][b, d], t["tq0"][b, d], t["tqd0"][b, d])
            errs = (pj.rel(tq[b, d], rq), pj.rel(tqd[b, d], rqd))
            print("size %s bdf%d b %d direction %d: tq %.3e tqd %.3e (relative to the recursion on XA, XB, XU)" % ((size, integ, b, d) + errs))
            worst = max(worst, max(errs))
    assert worst <= 1e-10, (size, integ, worst)


# ---------------------------------------------------------------- 3. the pairing with rollout_vjp of the same tape

@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", [(5, 1), ("tree7", 1), (16, 1), (32, 1), (5, 2), ("tree7", 2), (16, 2)])
def test_pairing_with_the_vjp_of_the_same_tape(size, integ):
    """|<gq, tq> + <gqd, tqd> - <du, tu> - <dq0, tq0> - <dqd0, tqd0>| relative to |<du, tu>| + |<dq0, tq0>| + |<dqd0, tqd0>|, for all
    three groups of tangents together and each alone.  The normaliser is a sum of single inner products, each of which may nearly
    cancel, so the figure belongs to its rollout and direction: the check is made on the rollout and direction the reference figure
    was measured on (rollout 0, direction 0 of a 3-direction call; tests/test_rollout_jvp_proto.py::tangent0), where numpy / LAPACK
    on the oracle's tape gives at most PAIRING_CPU.  The bound is 50 x that figure: the margin the linearize suite took over its
    LAPACK figure, for the kernels' different elimination orders.
    Measured on MI355X, the largest of all sizes and groups: 4.75e-11 (the 16-link chain, BDF2, tq0 alone; 1.8e-12 under BDF1)."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, integ)
    t = _tangents(sc, nsteps, 3)
    assert all(np.array_equal(t[k][0, 0], tangent0(nsteps, sc.nr)[k]) for k in KEYS)
    sim = BatchSim(sc, batch=B)
    qt, _ = _tape(sim, sc, cs, integ)
    gq, gqd = cs["c"] + qt, cs["d"]
    grads = sim.rollout_vjp(nsteps, gq, gqd)
    worst = 0.0
    for keys in (KEYS, ("tu",), ("tq0",), ("tqd0",)):
        tq, tqd = _jvp(sim, nsteps, t, keys)
        tans = tuple(t[k][0, 0] if k in keys else None for k in KEYS)
        e = pj.pairing((gq[0], gqd[0]), (tq[0, 0], tqd[0, 0]), tuple(g[0] for g in grads), tans)
        print("size %s bdf%d %s: pairing error %.3e" % (size, integ, "+".join(keys), e))
        worst = max(worst, e)
    sim.close()
    assert worst <= 50 * PAIRING_CPU, (size, integ, worst)


# ---------------------------------------------------------------- 4. the testGrad identity on the device

@pytest.mark.gpu
@pytest.mark.parametrize("n,integ", [(5, 1), (16, 1), (5, 2), (16, 2)])
def test_tangents_meet_the_testgrad_identity(n, integ):
    """Central differences (eps = 1e-6) of rollout_tape along 3 directions in (u, q0, qdot0) jointly, one batch of 6 rollouts, against
    the 3 directions of one rollout_jvp call.  Elementwise rtol 2e-5, atol 1e-6 max|ana|, for tq and for tqd."""
    from redmax_amd import BatchSim
    sc = _scene(n, integ)
    nsteps, h, pscale = STEPS[n], sc.h, sc.task["pscale"]
    cs = {k: v[0] for k, v in case(sc, 23, nsteps=nsteps).items()}
    nd, eps = 3, 1e-6
    t = {k: v[0] for k, v in pj.tangents(29, 1, nd, nsteps, sc.nr).items()}
    one = BatchSim(sc, batch=1)
    one.set_state(cs["q0"][None], cs["qd0"][None])
    one.rollout_tape(nsteps, h, cs["u"][None], pscale=pscale, integrator=integ)
    ana = one.rollout_jvp(nsteps, t["tu"][None], t["tq0"][None], t["tqd0"][None])
    one.close()
    sgn = np.tile([1.0, -1.0], nd)
    pert = {k: cs[k][None] + eps * sgn.reshape((-1,) + (1,) * cs[k].ndim) * np.repeat(t[tk], 2, axis=0)
            for k, tk in (("u", "tu"), ("q0", "tq0"), ("qd0", "tqd0"))}
    fd = BatchSim(sc, batch=2 * nd)
    fd.set_state(pert["q0"], pert["qd0"])
    qt, qdt, info = fd.rollout_tape(nsteps, h, pert["u"], pscale=pscale, integrator=integ, stats=True)
    fd.close()
    assert (info["status"] & 15 == 0).all()
    for name, a, x in (("tq", ana[0][0], qt), ("tqd", ana[1][0], qdt)):
        num = (x[0::2] - x[1::2]) / (2 * eps)
        err = np.abs(num - a)
        print("testgrad n %d bdf%d %s: max |num - ana| / max|ana| = %.3e" % (n, integ, name, err.max() / np.abs(a).max()))
        assert np.abs(a).max() > 0
        assert (err <= 2e-5 * np.abs(a) + 1e-6 * np.abs(a).max()).all(), (name, err.max(), np.abs(a).max())


# ---------------------------------------------------------------- 5. exact structure

@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", [(3, 1), (5, 1), (11, 1), (16, 1), (32, 1), (40, 1), (5, 2), (16, 2), (40, 2)])
def test_zeros_causality_and_a_direction_alone(size, integ):
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, integ)
    t9 = _tangents(sc, nsteps, 9)
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs, integ)
    tq9, tqd9 = _jvp(sim, nsteps, t9)
    assert np.isfinite(tq9).all() and np.isfinite(tqd9).all() and np.abs(tq9).max() > 0
    # zero tangents of one rollout give exactly zero rows, whatever the other rollouts carry
    tz = {k: v.copy() for k, v in t9.items()}
    for k in KEYS:
        tz[k][1] = 0.0
    zq, zqd = _jvp(sim, nsteps, tz)
    assert (zq[1] == 0).all() and (zqd[1] == 0).all()
    assert np.array_equal(zq[0], tq9[0]) and np.array_equal(zqd[2], tqd9[2])
    # tu alone, non-zero only at step k: rows 0 .. k-2 are exactly zero, row k-1 is not (under BDF2 k = 2 is the first BDF2 solve
    # behind the start step)
    for k in (2, nsteps):
        tk = np.zeros_like(t9["tu"])
        tk[:, :, k - 1] = t9["tu"][:, :, k - 1]
        cq, cqd = sim.rollout_jvp(nsteps, tu=tk)
        assert (cq[:, :, :k - 1] == 0).all() and (cqd[:, :, :k - 1] == 0).all(), k
        assert (np.abs(cq[:, :, k - 1]).max(axis=-1) > 0).all(), k
    # a direction alone (ntan 1) equals the same direction at positions 0, 7 and 8 of a 9-direction call
    for pos in (0, 7, 8):
        aq, aqd = sim.rollout_jvp(nsteps, *(t9[k][:, pos:pos + 1] for k in KEYS))
        assert np.array_equal(aq[:, 0], tq9[:, pos]) and np.array_equal(aqd[:, 0], tqd9[:, pos]), pos
        # ... and the form without the direction axis
        sq, sqd = sim.rollout_jvp(nsteps, *(t9[k][:, pos] for k in KEYS))
        assert sq.shape == (B, nsteps, sc.nr) and np.array_equal(sq, tq9[:, pos]) and np.array_equal(sqd, tqd9[:, pos]), pos
    # the same direction elsewhere in a 3-direction call
    mq, mqd = sim.rollout_jvp(nsteps, *(t9[k][:, [4, 8, 0]] for k in KEYS))
    assert np.array_equal(mq, tq9[:, [4, 8, 0]]) and np.array_equal(mqd, tqd9[:, [4, 8, 0]])
    # NULL equals an array of zeros
    for keys in (("tu",), ("tq0",), ("tqd0",), ("tu", "tqd0")):
        nq, nqd = _jvp(sim, nsteps, t9, keys)
        fq, fqd = _jvp(sim, nsteps, {k: (t9[k] if k in keys else np.zeros_like(t9[k])) for k in KEYS})
        assert np.array_equal(nq, fq) and np.array_equal(nqd, fqd), keys
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", [(3, 1), (5, 1), (16, 1), (32, 1), (40, 1), (5, 2), (40, 2)])
def test_batch_independence_repeatability_and_what_the_call_leaves_alone(size, integ):
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, integ)
    t = _tangents(sc, nsteps, 3)
    sim = BatchSim(sc, batch=B)
    qt, _ = _tape(sim, sc, cs, integ)
    gq, gqd = cs["c"] + qt, cs["d"]
    state = sim.get_state()
    vjp = sim.rollout_vjp(nsteps, gq, gqd)
    X = sim.rollout_linearize(nsteps)
    count = sim.tape_count
    tq, tqd = _jvp(sim, nsteps, t)
    assert sim.tape_count == count
    # the state and the tape are where they were
    assert all(np.array_equal(a, b) for a, b in zip(sim.get_state(), state))
    assert all(np.array_equal(a, b) for a, b in zip(sim.rollout_vjp(nsteps, gq, gqd), vjp))
    assert all(np.array_equal(a, b) for a, b in zip(sim.rollout_linearize(nsteps), X))
    # a second call: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(_jvp(sim, nsteps, t), (tq, tqd)))
    # the device form, all three inputs and one alone
    nan = np.full((B, 3, nsteps, sc.nr), np.nan)
    din = {k: _DevArray(t[k]) for k in KEYS}
    dq, dqd = _DevArray(nan), _DevArray(nan)
    sim.rollout_jvp_device(nsteps, 3, din["tu"].ptr.value, din["tq0"].ptr.value, din["tqd0"].ptr.value, dq.ptr.value, dqd.ptr.value)
    assert np.array_equal(dq.get(), tq) and np.array_equal(dqd.get(), tqd)
    sim.rollout_jvp_device(nsteps, 3, None, din["tq0"].ptr.value, None, dq.ptr.value, dqd.ptr.value)
    assert all(np.array_equal(a, b) for a, b in zip((dq.get(), dqd.get()), _jvp(sim, nsteps, t, ("tq0",))))
    assert all(np.array_equal(din[k].get(), t[k]) for k in KEYS)
    for a in list(din.values()) + [dq, dqd]:
        a.free()
    # step calls and set_state between tape and sweep leave the result alone
    sim.set_state(cs["q0"], cs["qd0"])
    sim.step_bdf1(2, h=sc.h)
    assert all(np.array_equal(a, b) for a, b in zip(_jvp(sim, nsteps, t), (tq, tqd)))
    sim.close()
    # rollout b of the batch is a batch-of-one call, bit for bit
    one = BatchSim(sc, batch=1)
    for b in range(B):
        _tape(one, sc, cs, integ, slice(b, b + 1))
        aq, aqd = one.rollout_jvp(nsteps, *(t[k][b:b + 1] for k in KEYS))
        assert np.array_equal(aq[0], tq[b]) and np.array_equal(aqd[0], tqd[b]), (size, b)
    one.close()


# ---------------------------------------------------------------- 6. refusals

@pytest.mark.gpu
def test_refusals():
    from redmax_amd import BatchSim, _abi
    sc, cs, nsteps = _setup(5)
    t = _tangents(sc, nsteps, 3)
    fresh, sim = BatchSim(sc, batch=B), BatchSim(sc, batch=B)
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        _jvp(sim, nsteps, t)
    _tape(sim, sc, cs)
    ref = _jvp(sim, nsteps, t)
    with pytest.raises(_abi.RedMaxHipError, match="nsteps differs"):
        sim.rollout_jvp(nsteps - 1, t["tu"][:, :, :-1])
    out = _DevArray(np.zeros((B, 3, nsteps, sc.nr)))
    tu = _DevArray(t["tu"])
    with pytest.raises(_abi.RedMaxHipError, match="all tangents are null"):
        sim.rollout_jvp_device(nsteps, 3, None, None, None, out.ptr.value, out.ptr.value)
    with pytest.raises(_abi.RedMaxHipError, match="ntan < 1"):
        sim.rollout_jvp_device(nsteps, 0, tu.ptr.value, None, None, out.ptr.value, out.ptr.value)
    with pytest.raises(_abi.RedMaxHipError, match="null argument"):
        sim.rollout_jvp_device(nsteps, 3, tu.ptr.value, None, None, None, out.ptr.value)
    with pytest.raises(_abi.RedMaxHipError, match="null argument"):
        sim.rollout_jvp_device(nsteps, 3, tu.ptr.value, None, None, out.ptr.value, None)
    with pytest.raises(_abi.RedMaxHipError, match="null argument"):
        _abi.check(sim._L.rmx_rollout_jvp(None, nsteps, 3, None, None, None, None, None), "rmx_rollout_jvp")
    tu.free()
    out.free()
    with pytest.raises(ValueError, match="all tangents are None"):
        sim.rollout_jvp(nsteps)
    with pytest.raises(ValueError, match="shape"):
        sim.rollout_jvp(nsteps, t["tu"], t["tq0"][:, :2])
    with pytest.raises(ValueError, match="shape"):
        sim.rollout_jvp(nsteps, t["tu"][:, 0], t["tq0"])
    # the refused calls left the tape alone
    assert all(np.array_equal(a, b) for a, b in zip(_jvp(sim, nsteps, t), ref))
    # an adjoint call reuses the workspace: the tape is gone
    sim.adjoint_controls(nsteps, sc.h, dict(sc.task, t=nsteps * sc.h), cs["u"])
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        _jvp(sim, nsteps, t)
    # the batch still steps afterwards as one that was never asked
    for s in (fresh, sim):
        s.set_state(cs["q0"], cs["qd0"])
    out, want = sim.step_bdf1(3, h=sc.h, stats=True), fresh.step_bdf1(3, h=sc.h, stats=True)
    qa, qda = sim.get_state()
    qb, qdb = fresh.get_state()
    sim.close()
    fresh.close()
    assert (out["status"] & 15 == 0).all() and np.isfinite(qa).all()
    assert np.array_equal(qa, qb) and np.array_equal(qda, qdb) and np.array_equal(out["newton_iters"], want["newton_iters"])


# ---------------------------------------------------------------- 7. torch

def _torch_case(Bt, nsteps, ntan, integ=1):
    import torch
    sc = _scene(5, integ)
    cs = case(sc, 37, nsteps=nsteps, B=Bt)
    dev = torch.device("cuda", 0)
    tn = pj.tangents(43, Bt, ntan, nsteps, sc.nr)
    t = {k: torch.tensor(v, dtype=torch.float64, device=dev) for k, v in list(cs.items()) + list(tn.items())}
    return sc, cs, tn, t


@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
def test_torch_func_jvp_forward_ad_and_diff_jvp_are_the_library_call(integ):
    import torch
    import torch.autograd.forward_ad as fwAD
    from redmax_amd import BatchSim, diff
    Bt, nsteps = 2, 3
    sc, cs, tn, t = _torch_case(Bt, nsteps, 3, integ)
    pscale = sc.task["pscale"]
    ref = BatchSim(sc, batch=Bt)
    ref.set_state(cs["q0"], cs["qd0"])
    qtr, qdtr, _ = ref.rollout_tape(nsteps, sc.h, cs["u"], pscale=pscale, integrator=integ)
    want = ref.rollout_jvp(nsteps, tn["tu"], tn["tq0"], tn["tqd0"])
    want_u = ref.rollout_jvp(nsteps, tu=tn["tu"])
    ref.close()
    sim = BatchSim(sc, batch=Bt)

    def f(q0, qd0, u):
        return diff.rollout(sim, q0, qd0, u, h=sc.h, pscale=pscale, integrator=integ)

    # torch.func.jvp, one direction at a time: BatchSim.rollout_jvp's bits
    for d in range(3):
        (qt, qdt), (tq, tqd) = torch.func.jvp(f, (t["q0"], t["qd0"], t["u"]), (t["tq0"][:, d], t["tqd0"][:, d], t["tu"][:, d]))
        assert np.array_equal(qt.cpu().numpy(), qtr) and np.array_equal(qdt.cpu().numpy(), qdtr)
        assert np.array_equal(tq.cpu().numpy(), want[0][:, d]) and np.array_equal(tqd.cpu().numpy(), want[1][:, d]), d
    # forward_ad with a tangent on u alone: the other two are NULL
    with fwAD.dual_level():
        qt, qdt = f(t["q0"], t["qd0"], fwAD.make_dual(t["u"], t["tu"][:, 1].contiguous()))
        tq, tqd = fwAD.unpack_dual(qt).tangent, fwAD.unpack_dual(qdt).tangent
    assert np.array_equal(tq.cpu().numpy(), want_u[0][:, 1]) and np.array_equal(tqd.cpu().numpy(), want_u[1][:, 1])
    # diff.jvp: one tape, all directions in one call; no graph
    qt, qdt, tq, tqd = diff.jvp(sim, t["q0"], t["qd0"], t["u"], tq0=t["tq0"], tqdot0=t["tqd0"], tu=t["tu"], h=sc.h, pscale=pscale,
                                integrator=integ)
    assert tq.shape == (Bt, 3, nsteps, sc.nr) and not tq.requires_grad and tq.device == t["u"].device
    assert np.array_equal(qt.cpu().numpy(), qtr) and np.array_equal(qdt.cpu().numpy(), qdtr)
    assert np.array_equal(tq.cpu().numpy(), want[0]) and np.array_equal(tqd.cpu().numpy(), want[1])
    _, _, tq, tqd = diff.jvp(sim, t["q0"], t["qd0"], t["u"], tu=t["tu"][:, 2], h=sc.h, pscale=pscale, integrator=integ)
    assert tq.shape == (Bt, nsteps, sc.nr)
    assert np.array_equal(tq.cpu().numpy(), want_u[0][:, 2]) and np.array_equal(tqd.cpu().numpy(), want_u[1][:, 2])
    with pytest.raises(ValueError, match="all tangents are None"):
        diff.jvp(sim, t["q0"], t["qd0"], t["u"], h=sc.h)
    with pytest.raises(ValueError, match="shape"):
        diff.jvp(sim, t["q0"], t["qd0"], t["u"], tu=t["tu"], tq0=t["tq0"][:, :2], h=sc.h)
    with pytest.raises(ValueError, match="float64"):
        diff.jvp(sim, t["q0"], t["qd0"], t["u"], tu=t["tu"].float(), h=sc.h)
    sim.close()


@pytest.mark.gpu
def test_torch_jacfwd_runs_all_directions_in_one_sweep():
    """torch.func.jacfwd is vmap over jvp: the mapped axis becomes the directions of one rollout_jvp call.  Column j of the Jacobian in
    u is the tangent of the unit direction e_j."""
    import torch
    from redmax_amd import BatchSim, diff
    Bt, nsteps = 2, 3
    sc, cs, tn, t = _torch_case(Bt, nsteps, 1)
    pscale = sc.task["pscale"]
    sim = BatchSim(sc, batch=Bt)
    J = torch.func.jacfwd(lambda u: diff.rollout(sim, t["q0"], t["qd0"], u, h=sc.h, pscale=pscale)[0])(t["u"])
    assert J.shape == (Bt, nsteps, sc.nr) + (Bt, nsteps, sc.nr)
    ref = BatchSim(sc, batch=Bt)
    ref.set_state(cs["q0"], cs["qd0"])
    ref.rollout_tape(nsteps, sc.h, cs["u"], pscale=pscale)
    eye = np.zeros((Bt, nsteps * sc.nr, nsteps, sc.nr))
    eye[:] = np.eye(nsteps * sc.nr).reshape(nsteps * sc.nr, nsteps, sc.nr)
    tq, _ = ref.rollout_jvp(nsteps, tu=eye)
    ref.close()
    sim.close()
    Jn = J.cpu().numpy()
    for b in range(Bt):
        # rollout b depends on its own u alone, and there on the unit directions
        assert np.array_equal(Jn[b, :, :, b].reshape(nsteps, sc.nr, -1), tq[b].transpose(1, 2, 0)), b
        assert (Jn[b, :, :, 1 - b] == 0).all()


@pytest.mark.gpu
def test_torch_gradcheck_with_forward_ad():
    """gradcheck's defaults (eps 1e-6, atol 1e-5, rtol 1e-3), reverse and forward mode, one sim per call as in
    tests/test_gpu_rollout_vjp.py."""
    import torch
    from redmax_amd import BatchSim, diff
    Bt, nsteps = 2, 3
    sc, cs, tn, t = _torch_case(Bt, nsteps, 1)
    pscale = sc.task["pscale"]
    sims = []

    def f(a, b, c):      # (a sim holds ONE tape and gradcheck keeps the graphs of several of its calls alive: a sim per call)
        sims.append(BatchSim(sc, batch=Bt))
        return diff.rollout(sims[-1], a, b, c, h=sc.h, pscale=pscale)

    assert torch.autograd.gradcheck(f, tuple(t[k].clone().requires_grad_(True) for k in ("q0", "qd0", "u")), check_forward_ad=True)
    for s_ in sims:
        s_.close()


@pytest.mark.gpu
def test_torch_forward_mode_refuses_parameter_tangents_and_a_replaced_tape():
    import torch
    import torch.autograd.forward_ad as fwAD
    from redmax_amd import BatchSim, diff
    Bt, nsteps = 2, 3
    sc, cs, tn, t = _torch_case(Bt, nsteps, 1)
    pscale = sc.task["pscale"]
    sim = BatchSim(sc, batch=Bt)
    params = {k: v.detach() for k, v in diff.model_params(sim).items() if k in ("stiffness",)}
    with fwAD.dual_level():
        dual = {"stiffness": fwAD.make_dual(params["stiffness"], torch.ones_like(params["stiffness"]))}
        with pytest.raises(RuntimeError, match="tangents of the model parameters"):
            diff.rollout(sim, t["q0"], t["qd0"], fwAD.make_dual(t["u"], t["tu"][:, 0].contiguous()), h=sc.h, pscale=pscale, params=dual)
    # the jvp of a rollout whose tape another rollout has replaced
    Fn = diff._function()

    class _Ctx:
        pass

    ctx = _Ctx()
    Fn.setup_context(ctx, (t["q0"], t["qd0"], t["u"], sim, sc.h, pscale, True, 1), None)
    diff.rollout(sim, t["q0"], t["qd0"], t["u"], h=sc.h, pscale=pscale)
    with pytest.raises(RuntimeError, match="the tape of this rollout has been replaced"):
        Fn.jvp(ctx, None, None, t["tu"][:, 0].contiguous())
    sim.close()


# ---------------------------------------------------------------- 8. the MEX command

@pytest.mark.gpu
def test_mex_command_equals_the_ctypes_call(gw):  # noqa: F811
    """'rollout_jvp' through the gateway (stub), over two shards: MATLAB's nr x nsteps x ntan x B column-major arrays are the ABI's
    [B][ntan][nsteps][nr]; [] is NULL."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(5)
    t = _tangents(sc, nsteps, 3)
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    want = _jvp(sim, nsteps, t)
    want_u = _jvp(sim, nsteps, t, ("tu",))
    sim.close()
    empty = np.zeros((0, 0))
    tu, tq0, tqd0 = t["tu"].transpose(3, 2, 1, 0), t["tq0"].transpose(2, 1, 0), t["tqd0"].transpose(2, 1, 0)
    h = gw.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    with pytest.raises(MexError, match="no tape"):
        gw.call(2, "rollout_jvp", h, float(nsteps), tu, tq0, tqd0)
    gw.call(0, "set", h, cs["q0"].T, cs["qd0"].T)
    gw.call(3, "rollout_tape", h, sc.h, float(nsteps), float(sc.task["pscale"]), cs["u"].transpose(2, 1, 0))
    tq, tqd = gw.call(2, "rollout_jvp", h, float(nsteps), tu, tq0, tqd0)
    assert tq.shape == (sc.nr, nsteps, 3, B)
    assert np.array_equal(tq.transpose(3, 2, 1, 0), want[0]) and np.array_equal(tqd.transpose(3, 2, 1, 0), want[1])
    tq, tqd = gw.call(2, "rollout_jvp", h, float(nsteps), tu, empty, empty)
    assert np.array_equal(tq.transpose(3, 2, 1, 0), want_u[0]) and np.array_equal(tqd.transpose(3, 2, 1, 0), want_u[1])
    with pytest.raises(MexError, match="all tangents are null"):
        gw.call(2, "rollout_jvp", h, float(nsteps), empty, empty, empty)
    with pytest.raises(MexError, match="same ntan"):
        gw.call(2, "rollout_jvp", h, float(nsteps), tu, tq0[:, :2], empty)
    with pytest.raises(MexError, match="nsteps differs"):
        gw.call(2, "rollout_jvp", h, float(nsteps - 1), tu[:, :-1], empty, empty)
    gw.call(0, "destroy", h)
