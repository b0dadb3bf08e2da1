"""rmx_rollout_jvp_params: forward-mode tangents of the taped rollout with respect to the model's parameters - directions in joint
stiffness, damping and rest position, body inertia and mass, and gravity in, the tangents of the whole trajectory out.

The checks, in the order of the sections below:
  1. every direction's tq, tqd against the numpy proto on the oracle's tape (tests/proto_rollout_jvp_params.py, pinned on the CPU by
     tests/test_rollout_jvp_params_proto.py), BDF1 and BDF2, to 1e-7 relative Frobenius - the bound the suite holds tape-derived
     quantities to;
  2. the pairing with rollout_vjp_params of the same tape, each group alone and all together;
  3. the same pairing on a tape with point forces, against rollout_vjp_forces(model=PARAM_NAMES);
  4. the testGrad identity on the device: central differences of rollout_tape over sims rebuilt from perturbed scenes;
  5. exact structure, np.array_equal; 6. refusals; 7. redmax_amd.diff (jvp_params, param_jacobian); 8. the MEX command.

Sizes by the path each takes: 3 (NP 4); 5 and tree7 (NP 8, a chain and a branching tree); 16 (NP 16); 32 (NP 32); 40 (NP 64); BDF2 on
5, tree7, 16 and 40.  Inputs: case(sc, 17), the step counts and B = 3 of tests/test_gpu_rollout_vjp.py; the directions of
tests/test_rollout_jvp_params_proto.py tangents().
"""
import ctypes as C

import numpy as np
import pytest

import proto_rollout_jvp as pj
import proto_rollout_jvp_params as pjp
import proto_rollout_params as pp
import proto_rollout_pf as P
from test_gpu_adjoint_controls import _DevArray, _scene
from test_gpu_rollout_linearize import _setup, _tape
from test_gpu_rollout_vjp import B, STEPS
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)
from test_rollout_jvp_params_proto import KEYS, PSEED, oracle_case, tangents
from test_rollout_vjp_proto import case

GROUPS = pp.GROUPS
SIZES = [3, 5, "tree7", 16, 32, 40]
BDF2_SIZES = [5, "tree7", 16, 40]
CASES = [(s, 1) for s in SIZES] + [(s, 2) for s in BDF2_SIZES]
# the largest pairing error tests/test_rollout_jvp_params_proto.py prints (numpy / LAPACK on the oracle's tape of rollout 0, direction
# 0 of tangents(.., 3); 5, tree7, 16, 32 under BDF1, 5, tree7, 16 under BDF2; each group alone and all together): 6.624e-12, the
# 32-link chain under BDF1 with stiffness alone (1.207e-12 under BDF2: the 16-link chain, stiffness alone)
PAIRING_CPU = 6.624e-12
# the proto's own central-difference error per group, in units of the testGrad bound 2e-5 |ana| + 1e-6 max|ana|
# (tests/test_rollout_jvp_params_proto.py::test_parameter_jvp_meets_central_differences, the worst of 5 and tree7; BDF1, BDF2):
CD_CPU = {"stiffness": (2.599e-02, 2.379e-01), "damping": (1.774e-04, 2.495e-03), "qrest": (3.192e-04, 9.449e-04),
          "inertia": (2.247e-04, 5.709e-04), "grav": (4.842e-04, 6.324e-03)}


def _call(sim, nsteps, t, groups=GROUPS, keys=KEYS):
    return sim.rollout_jvp_params(nsteps, {g: t[g] for g in groups}, **{k: (t[k] if k in keys else None) for k in KEYS})


def _pairing(gq, gqd, tq, tqd, grads, pgrads, t, groups, keys, b=0, d=0):
    """The pairing error of rollout b, direction d (tests/proto_rollout_jvp_params.py pairing: relative to the sum of the magnitudes
    of the terms on the right)."""
    return pjp.pairing((gq[b], gqd[b]), (tq[b, d], tqd[b, d]), tuple(g[b] for g in grads), tuple(t[k][b, d] if k in keys else None for k in KEYS),
                       {g: pgrads[g][b] for g in groups}, {g: t[g][b, d] for g in groups})


# ---------------------------------------------------------------- 1. against the proto on the oracle's tape

@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", CASES)
def test_tangents_meet_the_proto(oracle_lib, size, integ):
    """9 directions (two chunks of the sweep, the second with one direction), all five groups plus tu, tq0, tqd0.  All rollouts up to
    16 links, rollout 0 for 32 and 40.
    Measured on MI355X, the worst direction of every case: 6.98e-12 at the worst (the 16-link chain, BDF2), 7.5e-14 .. 2.4e-12 on the
    BDF1 cases, 1.2e-13 .. 4.6e-12 on the other BDF2 cases."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, integ)
    t = tangents(oracle_lib, sc, nsteps, 9)
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs, integ)
    tq, tqd = _call(sim, nsteps, t)
    sim.close()
    assert tq.shape == (B, 9, nsteps, sc.nr) and tqd.shape == tq.shape
    worst = 0.0
    idx = oracle_lib.Oracle(sc.desc()).idxR()
    for b in range(B if size not in (32, 40) else 1):
        _, _, tp = oracle_case(oracle_lib, size, integ, b, B)
        g0 = pp.residuals(oracle_lib, sc, tp["slots"])
        for d in range(9):
            rq, rqd = pjp.jvp_params(oracle_lib, sc, integ, tp, sc.h, sc.task["pscale"], {g: t[g][b, d] for g in GROUPS},
                                     t["tu"][b, d], t["tq0"][b, d], t["tqd0"][b, d], g0=g0, idx=idx)
            worst = max(worst, pj.rel(tq[b, d], rq), pj.rel(tqd[b, d], rqd))
        print("size %s bdf%d b %d: worst direction so far %.3e (relative Frobenius to the proto)" % (size, integ, b, worst))
    assert worst <= 1e-7, (size, integ, worst)


# ---------------------------------------------------------------- 2. the pairing with rollout_vjp_params of the same tape

@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", [(5, 1), ("tree7", 1), (16, 1), (32, 1), (5, 2), ("tree7", 2), (16, 2)])
def test_pairing_with_the_parameter_gradients_of_the_same_tape(oracle_lib, size, integ):
    """|<gq, tq> + <gqd, tqd> - <du, tu> - <dq0, tq0> - <dqd0, tqd0> - sum_groups <grad, ttheta>| relative to the sum of the magnitudes
    of the terms on the right, each group alone and all five together with tu, tq0, tqd0, on rollout 0, direction 0 of a 3-direction
    call - where numpy / LAPACK on the oracle's tape gives at most PAIRING_CPU.  The bound is 50 x that figure, the margin
    tests/test_gpu_rollout_jvp.py took over its LAPACK figure.
    Measured on MI355X, the largest of all sizes and groups: 7.08e-13 (the 32-link chain, BDF1, stiffness alone; 2.3e-13 under BDF2:
    the 16-link chain, damping alone)."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, integ)
    t = tangents(oracle_lib, sc, nsteps, 3)
    sim = BatchSim(sc, batch=B)
    qt, _ = _tape(sim, sc, cs, integ)
    gq, gqd = cs["c"] + qt, cs["d"]
    du, dq0, dqd0, pgrads = sim.rollout_vjp_params(nsteps, gq, gqd)
    worst = 0.0
    for groups, keys in [((g,), ()) for g in GROUPS] + [(GROUPS, KEYS)]:
        tq, tqd = _call(sim, nsteps, t, groups, keys)
        e = _pairing(gq, gqd, tq, tqd, (du, dq0, dqd0), pgrads, t, groups, keys)
        print("size %s bdf%d %s: pairing error %.3e" % (size, integ, "+".join(groups + keys), e))
        worst = max(worst, e)
    sim.close()
    assert worst <= 50 * PAIRING_CPU, (size, integ, worst)


# ---------------------------------------------------------------- 3. the pairing on a tape with point forces

@pytest.mark.gpu
@pytest.mark.parametrize("n,integ", [(8, 1), (32, 1), (8, 2)])
def test_pairing_on_a_tape_with_point_forces(oracle_lib, n, integ):
    """tests/proto_rollout_pf.py case(n) on BatchSim(..., tape_forces=True): the five groups' dg/dtheta does not involve the forces, H
    and D on the tape carry them.  Paired against rollout_vjp_forces(model=PARAM_NAMES); the bound of section 2.
    Measured on MI355X, the largest of the three cases and all groups: 9.46e-13 (n = 32, BDF1, inertia alone)."""
    from redmax_amd import BatchSim, _abi
    cs = P.case(n)
    sc, N, h, ps = cs["sc"], cs["nsteps"], cs["h"], cs["pscale"]
    t = pj.tangents(53, 2, 3, N, sc.nr)
    t.update(pjp.directions(_values(sc), PSEED, (2, 3)))
    sim = BatchSim(sc, batch=2, tape_forces=True)
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, info = sim.rollout_tape(N, h, cs["u"], pscale=ps, integrator=integ, stats=True)
    assert (info["status"] & 15 == 0).all()
    gq, gqd = cs["c"] + qt, cs["d"]
    du, dq0, dqd0, grads = sim.rollout_vjp_forces(N, gq, gqd, want=(), model=_abi.PARAM_NAMES)
    worst = 0.0
    for groups, keys in [((g,), ()) for g in GROUPS] + [(GROUPS, KEYS)]:
        tq, tqd = _call(sim, N, t, groups, keys)
        e = _pairing(gq, gqd, tq, tqd, (du, dq0, dqd0), grads, t, groups, keys)
        print("point forces n %d bdf%d %s: pairing error %.3e" % (n, integ, "+".join(groups + keys), e))
        worst = max(worst, e)
    sim.close()
    assert worst <= 50 * PAIRING_CPU, (n, integ, worst)


def _values(sc):
    """The model's parameters in the layout of the tangents, read from the description (joints of at most one DOF, every joint with a
    DOF in these scenes' reduced order as the library reports it)."""
    from redmax_amd import BatchSim, _abi
    d = sc.desc()
    sim = BatchSim(sc, batch=1)
    idx = sim.idxR()
    sim.close()
    out = {g: np.zeros(sc.nr) for g in GROUPS[:3]}
    for j, r in enumerate(idx):
        if r >= 0:
            for g in GROUPS[:3]:
                out[g][r] = np.asarray(d[pp.DESC_KEY[g]], dtype=np.float64)[j]
    out["inertia"] = np.array(d["I_i"], dtype=np.float64).reshape(-1, 6)
    out["grav"] = np.array(d["grav"], dtype=np.float64).reshape(3)
    return out


# ---------------------------------------------------------------- 4. the testGrad identity on the device

@pytest.mark.gpu
@pytest.mark.parametrize("n,integ", [(5, 1), (16, 1), (5, 2), (16, 2)])
def test_tangents_meet_the_testgrad_identity(oracle_lib, n, integ):
    """Central differences (eps = 1e-5) of rollout_tape over sims rebuilt from tests/proto_rollout_params.py perturbed scenes, one
    direction per group, scaled to the group's magnitude, against the single-direction call.  Elementwise rtol 2e-5, atol 1e-6
    max|ana|, for tq and for tqd, every group.
    Measured on MI355X, the largest error in units of that bound (<= 1 passes), per group over the four cases: stiffness 6.3e-02,
    damping 1.2e-02, qrest 1.4e-03, inertia 8.8e-03, grav 1.3e-03 - no group's bound had to be raised (CD_CPU above is the proto's own
    error on the CPU, the figure such a bound would have come from)."""
    from redmax_amd import BatchSim
    from test_rollout_params_proto import directions
    sc = _scene(n, integ)
    nsteps = STEPS[n]
    cs = {k: v[:1] for k, v in case(sc, 23, nsteps=nsteps).items()}
    dirs = directions(pp.values(oracle_lib, sc), 29)
    dirs["inertia"][:, 4:] = dirs["inertia"][:, 3:4]      # (the library takes one mass per body: a mass tangent moves I_i(4:6) together)
    one = BatchSim(sc, batch=1)
    _tape(one, sc, cs, integ)
    ana = {g: one.rollout_jvp_params(nsteps, {g: dirs[g][None]}) for g in GROUPS}
    one.close()
    eps, shown = 1e-5, {}
    for g in GROUPS:
        x = []
        for sgn in (1.0, -1.0):
            fd = BatchSim(pp.perturbed(oracle_lib, sc, g, sgn * eps * dirs[g]), batch=1)
            x.append(_tape(fd, sc, cs, integ))
            fd.close()
        worst = 0.0
        for i in range(2):
            a, num = ana[g][i][0], (x[0][i][0] - x[1][i][0]) / (2 * eps)
            assert np.abs(a).max() > 0
            worst = max(worst, float((np.abs(num - a) / (2e-5 * np.abs(a) + 1e-6 * np.abs(a).max())).max()))
        shown[g] = worst
    print("testgrad n %d bdf%d: " % (n, integ) + " ".join("%s %.3e" % kv for kv in shown.items()) + " (of the testGrad bound)")
    assert all(v <= 1.0 for v in shown.values()), shown


# ---------------------------------------------------------------- 5. exact structure

@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", CASES)
def test_exact_structure(oracle_lib, size, integ):
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(size, integ)
    t9 = tangents(oracle_lib, sc, nsteps, 9)
    zero = {g: np.zeros_like(t9[g]) for g in GROUPS}
    sim = BatchSim(sc, batch=B)
    qt, _ = _tape(sim, sc, cs, integ)
    gq, gqd = cs["c"] + qt, cs["d"]
    state = sim.get_state()
    vjp = sim.rollout_vjp(nsteps, gq, gqd)
    jvp = sim.rollout_jvp(nsteps, t9["tu"], t9["tq0"], t9["tqd0"])
    X = sim.rollout_linearize(nsteps)
    count = sim.tape_count
    tq9, tqd9 = _call(sim, nsteps, t9)
    assert np.isfinite(tq9).all() and np.isfinite(tqd9).all() and np.abs(tq9).max() > 0
    # the state and the tape are where they were
    assert sim.tape_count == count
    assert all(np.array_equal(a, b) for a, b in zip(sim.get_state(), state))
    assert all(np.array_equal(a, b) for a, b in zip(sim.rollout_vjp(nsteps, gq, gqd), vjp))
    assert all(np.array_equal(a, b) for a, b in zip(sim.rollout_jvp(nsteps, t9["tu"], t9["tq0"], t9["tqd0"]), jvp))
    assert all(np.array_equal(a, b) for a, b in zip(sim.rollout_linearize(nsteps), X))
    # a second call: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(_call(sim, nsteps, t9), (tq9, tqd9)))
    # zero-array parameter tangents: rollout_jvp's numbers
    zq, zqd = sim.rollout_jvp_params(nsteps, zero, t9["tu"], t9["tq0"], t9["tqd0"])
    assert np.array_equal(zq, jvp[0]) and np.array_equal(zqd, jvp[1])
    # a NULL group equals an array of zeros, each group left out in turn and each group alone
    for g in GROUPS:
        rest = tuple(x for x in GROUPS if x != g)
        nq, nqd = _call(sim, nsteps, t9, rest)
        fq, fqd = _call(sim, nsteps, dict(t9, **{g: zero[g]}))
        assert np.array_equal(nq, fq) and np.array_equal(nqd, fqd), g
        nq, nqd = _call(sim, nsteps, t9, (g,), ())
        fq, fqd = sim.rollout_jvp_params(nsteps, dict(zero, **{g: t9[g]}), *(np.zeros_like(t9[k]) for k in KEYS))
        assert np.array_equal(nq, fq) and np.array_equal(nqd, fqd), g
    # a direction alone (ntan 1) equals the same direction at positions 0, 4 and 8 of the 9-direction call
    for pos in (0, 4, 8):
        one = {k: v[:, pos:pos + 1] for k, v in t9.items()}
        aq, aqd = _call(sim, nsteps, one)
        assert np.array_equal(aq[:, 0], tq9[:, pos]) and np.array_equal(aqd[:, 0], tqd9[:, pos]), pos
        # ... and the form without the direction axis
        sq, sqd = _call(sim, nsteps, {k: v[:, pos] for k, v in t9.items()})
        assert sq.shape == (B, nsteps, sc.nr) and np.array_equal(sq, tq9[:, pos]) and np.array_equal(sqd, tqd9[:, pos]), pos
    # the same directions elsewhere in a 3-direction call
    mq, mqd = _call(sim, nsteps, {k: v[:, [4, 8, 0]] for k, v in t9.items()})
    assert np.array_equal(mq, tq9[:, [4, 8, 0]]) and np.array_equal(mqd, tqd9[:, [4, 8, 0]])
    # Only the `inertia` rows whose listing index maps to a node are read.  Both constructors of the library give every listed body a
    # node (a lowered multi-DOF joint's body sits on the last node of its chain), so no description reaches a listing row without
    # one, and that rule of the header cannot be exercised through the public interface: no check of it is made here.
    # the device form, everything given and one group alone
    nan = np.full((B, 9, nsteps, sc.nr), np.nan)
    din = {k: _DevArray(v) for k, v in t9.items()}
    dq, dqd = _DevArray(nan), _DevArray(nan)
    sim.rollout_jvp_params_device(nsteps, 9, dq.ptr.value, dqd.ptr.value, *(din[g].ptr.value for g in GROUPS),
                                  tu_ptr=din["tu"].ptr.value, tq0_ptr=din["tq0"].ptr.value, tqd0_ptr=din["tqd0"].ptr.value)
    assert np.array_equal(dq.get(), tq9) and np.array_equal(dqd.get(), tqd9)
    sim.rollout_jvp_params_device(nsteps, 9, dq.ptr.value, dqd.ptr.value, inertia_ptr=din["inertia"].ptr.value)
    assert all(np.array_equal(a, b) for a, b in zip((dq.get(), dqd.get()), _call(sim, nsteps, t9, ("inertia",), ())))
    assert all(np.array_equal(din[k].get(), t9[k]) for k in t9)
    for a in list(din.values()) + [dq, dqd]:
        a.free()
    # a stiffness tangent alone reaches row 0 through the parameter term of slot 0 alone (dqA = dqB = du = 0 there): one hand-made
    # solve on rollout_linearize's XU = eta^2 pscale H^-1
    if integ == 1:
        sq, _ = _call(sim, nsteps, t9, ("stiffness",), ())
        qrest = pp.values(oracle_lib, sc)["qrest"]
        XU = X[2]
        for b in range(B):
            for d in (0, 8):
                r0 = sc.h ** 2 * t9["stiffness"][b, d] * (qt[b, 0] - qrest)
                want = XU[b, 0] @ (-r0) / (sc.h ** 2 * sc.task["pscale"])
                assert pj.rel(sq[b, d, 0], want) <= 1e-10, (b, d, pj.rel(sq[b, d, 0], want))
    # step calls and set_state between tape and sweep leave the result alone
    sim.set_state(cs["q0"], cs["qd0"])
    sim.step_bdf1(2, h=sc.h)
    assert all(np.array_equal(a, b) for a, b in zip(_call(sim, nsteps, t9), (tq9, tqd9)))
    sim.close()
    # the batch permuted [1, 0, 1]: a rollout's rows do not depend on its place in the batch
    perm = [1, 0, 1]
    other = BatchSim(sc, batch=B)
    _tape(other, sc, {k: v[perm] for k, v in cs.items()}, integ)
    pq, pqd = _call(other, nsteps, {k: v[perm] for k, v in t9.items()})
    other.close()
    assert np.array_equal(pq, tq9[perm]) and np.array_equal(pqd, tqd9[perm])


# ---------------------------------------------------------------- 6. refusals

@pytest.mark.gpu
def test_refusals(oracle_lib):
    from redmax_amd import BatchSim, _abi
    sc, cs, nsteps = _setup(5)
    t = tangents(oracle_lib, sc, nsteps, 3)
    fresh, sim = BatchSim(sc, batch=B), BatchSim(sc, batch=B)
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        _call(sim, nsteps, t)
    _tape(sim, sc, cs)
    ref = _call(sim, nsteps, t)
    with pytest.raises(_abi.RedMaxHipError, match="nsteps differs"):
        sim.rollout_jvp_params(nsteps - 1, {"grav": t["grav"]})
    out = _DevArray(np.zeros((B, 3, nsteps, sc.nr)))
    tk, tu = _DevArray(t["stiffness"]), _DevArray(t["tu"])
    with pytest.raises(_abi.RedMaxHipError, match="all parameter tangents are null; rmx_rollout_jvp is the call for it"):
        sim.rollout_jvp_params_device(nsteps, 3, out.ptr.value, out.ptr.value, tu_ptr=tu.ptr.value)
    with pytest.raises(_abi.RedMaxHipError, match="ntan < 1"):
        sim.rollout_jvp_params_device(nsteps, 0, out.ptr.value, out.ptr.value, stiffness_ptr=tk.ptr.value)
    with pytest.raises(_abi.RedMaxHipError, match="null argument"):
        sim.rollout_jvp_params_device(nsteps, 3, None, out.ptr.value, stiffness_ptr=tk.ptr.value)
    with pytest.raises(_abi.RedMaxHipError, match="null argument"):
        sim.rollout_jvp_params_device(nsteps, 3, out.ptr.value, None, stiffness_ptr=tk.ptr.value)
    L = sim._L
    tp = _abi.ParamTangents(t["stiffness"].ctypes.data, None, None, None, None)
    o = np.zeros((B, 3, nsteps, sc.nr))
    assert L.rmx_rollout_jvp_params(None, nsteps, 3, C.byref(tp), None, None, None, _abi.dptr(o), _abi.dptr(o)) != 0
    assert b"rmx_rollout_jvp_params: null argument" in L.rmx_last_error()
    assert L.rmx_rollout_jvp_params(sim._batch, nsteps, 3, None, None, None, None, _abi.dptr(o), _abi.dptr(o)) != 0
    assert b"null argument" in L.rmx_last_error()
    for a in (out, tk, tu):
        a.free()
    # the refused calls left the tape alone
    assert all(np.array_equal(a, b) for a, b in zip(_call(sim, nsteps, t), ref))
    # an adjoint call reuses the workspace: the tape is gone
    sim.adjoint_controls(nsteps, sc.h, dict(sc.task, t=nsteps * sc.h), cs["u"])
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        _call(sim, nsteps, t)
    # the batch still steps afterwards exactly like one never asked
    for s in (fresh, sim):
        s.set_state(cs["q0"], cs["qd0"])
    got, want = sim.step_bdf1(3, h=sc.h, stats=True), fresh.step_bdf1(3, h=sc.h, stats=True)
    qa, qda = sim.get_state()
    qb, qdb = fresh.get_state()
    sim.close()
    fresh.close()
    assert (got["status"] & 15 == 0).all() and np.isfinite(qa).all()
    assert np.array_equal(qa, qb) and np.array_equal(qda, qdb) and np.array_equal(got["newton_iters"], want["newton_iters"])


# ---------------------------------------------------------------- 7. redmax_amd.diff

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
def test_diff_jvp_params_and_param_jacobian(oracle_lib, integ):
    """diff.jvp_params is the library call on the tape it records; a column of diff.param_jacobian is the single-direction call, bit
    for bit; J' (gq, gqd) summed over the trajectory is rollout_vjp_params' row, to the bound of section 2 (relative to the sum of
    the magnitudes of the right-hand terms of a group's unit directions: the entries of its gradient row).
    Measured on MI355X: 8.4e-15 (BDF1), 1.4e-14 (BDF2)."""
    import torch
    from redmax_amd import BatchSim, diff
    Bt, nsteps = 2, 3
    sc = _scene(5, integ)
    cs = case(sc, 37, nsteps=nsteps, B=Bt)
    pscale = sc.task["pscale"]
    dev = torch.device("cuda", 0)
    tn = tangents(oracle_lib, sc, nsteps, 3, nb=Bt)
    tt = {k: torch.tensor(v, dtype=torch.float64, device=dev) for k, v in list(cs.items()) + list(tn.items())}
    ref = BatchSim(sc, batch=Bt)
    ref.set_state(cs["q0"], cs["qd0"])
    qtr, qdtr, _ = ref.rollout_tape(nsteps, sc.h, cs["u"], pscale=pscale, integrator=integ)
    want = _call(ref, nsteps, tn)
    want_g = _call(ref, nsteps, tn, ("grav",), ())
    gq, gqd = cs["c"] + qtr, cs["d"]
    pgrads = ref.rollout_vjp_params(nsteps, gq, gqd)[3]
    sim = BatchSim(sc, batch=Bt)
    qt, qdt, tq, tqd = diff.jvp_params(sim, tt["q0"], tt["qd0"], tt["u"], {g: tt[g] for g in GROUPS}, tq0=tt["tq0"], tqdot0=tt["tqd0"],
                                       tu=tt["tu"], h=sc.h, pscale=pscale, integrator=integ)
    assert tq.shape == (Bt, 3, nsteps, sc.nr) and not tq.requires_grad and tq.device == tt["u"].device
    assert np.array_equal(qt.cpu().numpy(), qtr) and np.array_equal(qdt.cpu().numpy(), qdtr)
    assert np.array_equal(tq.cpu().numpy(), want[0]) and np.array_equal(tqd.cpu().numpy(), want[1])
    _, _, tq, tqd = diff.jvp_params(sim, tt["q0"], tt["qd0"], tt["u"], {"grav": tt["grav"][:, 1]}, h=sc.h, pscale=pscale, integrator=integ)
    assert tq.shape == (Bt, nsteps, sc.nr)
    assert np.array_equal(tq.cpu().numpy(), want_g[0][:, 1]) and np.array_equal(tqd.cpu().numpy(), want_g[1][:, 1])
    # the Jacobian on the tape diff.jvp_params left
    J = diff.param_jacobian(sim, nsteps)
    shapes = sim._param_shapes()
    assert set(J) == set(GROUPS)
    worst = 0.0
    for g in GROUPS:
        Jq, Jqd = (x.cpu().numpy() for x in J[g])
        assert Jq.shape == (Bt, nsteps, sc.nr) + shapes[g] and Jqd.shape == Jq.shape
        for i in list(np.ndindex(shapes[g]))[::3]:
            unit = np.zeros((Bt,) + shapes[g])
            unit[(slice(None),) + i] = 1.0
            cq, cqd = ref.rollout_jvp_params(nsteps, {g: unit})
            assert np.array_equal(Jq[(Ellipsis,) + i], cq) and np.array_equal(Jqd[(Ellipsis,) + i], cqd), (g, i)
        for b in range(Bt):      # (the group's unit directions together: the right-hand terms are the entries of its gradient row)
            lhs = np.tensordot(gq[b], Jq[b], axes=2) + np.tensordot(gqd[b], Jqd[b], axes=2)
            assert lhs.shape == shapes[g]
            worst = max(worst, float(np.abs(lhs - pgrads[g][b]).max() / np.abs(pgrads[g][b]).sum()))
    print("diff bdf%d: J'(gq, gqd) against rollout_vjp_params, worst entry %.3e" % (integ, worst))
    assert worst <= 50 * PAIRING_CPU, worst
    only = diff.param_jacobian(sim, nsteps, names=("grav",))
    assert list(only) == ["grav"] and torch.equal(only["grav"][0], J["grav"][0]) and torch.equal(only["grav"][1], J["grav"][1])
    ref.close()
    sim.close()


# ---------------------------------------------------------------- 8. the MEX command

@pytest.mark.gpu
def test_mex_command_equals_the_ctypes_call(oracle_lib, gw):  # noqa: F811
    """'rollout_jvp_params' through the gateway (stub), over two shards: MATLAB's column-major arrays are the ABI's rows; [] is NULL."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = _setup(5)
    t = tangents(oracle_lib, sc, nsteps, 3)
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    want = _call(sim, nsteps, t)
    want_i = _call(sim, nsteps, t, ("inertia",), ())
    sim.close()
    e = np.zeros((0, 0))
    m = {k: v.transpose(tuple(range(v.ndim))[::-1]) for k, v in t.items()}
    h = gw.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    args = [m[g] for g in GROUPS] + [m[k] for k in KEYS]
    with pytest.raises(MexError, match="no tape"):
        gw.call(2, "rollout_jvp_params", h, float(nsteps), *args)
    gw.call(0, "set", h, cs["q0"].T, cs["qd0"].T)
    gw.call(3, "rollout_tape", h, sc.h, float(nsteps), float(sc.task["pscale"]), cs["u"].transpose(2, 1, 0))
    tq, tqd = gw.call(2, "rollout_jvp_params", h, float(nsteps), *args)
    assert tq.shape == (sc.nr, nsteps, 3, B)
    assert np.array_equal(tq.transpose(3, 2, 1, 0), want[0]) and np.array_equal(tqd.transpose(3, 2, 1, 0), want[1])
    tq, tqd = gw.call(2, "rollout_jvp_params", h, float(nsteps), e, e, e, m["inertia"], e, e, e, e)
    assert np.array_equal(tq.transpose(3, 2, 1, 0), want_i[0]) and np.array_equal(tqd.transpose(3, 2, 1, 0), want_i[1])
    with pytest.raises(MexError, match="rmx_rollout_jvp is the call for it"):
        gw.call(2, "rollout_jvp_params", h, float(nsteps), e, e, e, e, e, m["tu"], e, e)
    with pytest.raises(MexError, match="same ntan"):
        gw.call(2, "rollout_jvp_params", h, float(nsteps), m["stiffness"], m["damping"][:, :2], e, e, e, e, e, e)
    gw.call(0, "destroy", h)
