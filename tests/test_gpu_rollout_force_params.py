"""rmx_rollout_vjp_forces: the gradient of a loss on the taped rollout of a model with body-to-body forces with respect to the
constants of the force table (stiffness, damping, rest length of every point-point force, spring-damper and cable), and
rmx_rollout_vjp_params' five arrays on such a tape.

The checks, in the order of the sections below:
  1. every entry against the numpy proto evaluated ON THE GPU'S OWN RECORD (tests/proto_rollout_force_params.py, pinned against
     central differences of whole rollouts by tests/test_rollout_force_params_proto.py) at every size and both integrators:
     |gpu - proto| <= 1e-7 S per entry, S = sum_s |z_s' dg_s/dtheta| - the 1e-7 this suite holds every taped gradient to, per force
     and proof against cancellation between the slots; the point-point force's L entry is exactly +0.0; the `model` arrays on the
     same tape to 1e-7 relative against tests/proto_rollout_params.py's differences of the oracle's residual, fed with this tape's z;
  2. the testGrad identity on the device at n = 4 and 16: central differences over rollouts of sims built from scenes with perturbed
     force constants, and one direction in the joint stiffness through `model`;
  3. the switching scene against the proto; a cable that is slack throughout has exact zeros in its three entries;
  4. the call on a closed-loop tape equals the call on the open-loop tape under uapp, bit for bit;
  5. exact structure at n = 5 and 64; 6. refusals.
Inputs: proto_rollout_pf.case(n) (B = 2, 4 steps, 3 at 64 lanes) and switching_case(); the CPU test asserts on them that every entry
but the point-point L has |G| >= 1e-3 S, so the 1e-7 S is at most 1e-4 of any entry.

Measured on an MI355X, worst |gpu - proto| / S over the entries and the two rollouts (BDF1 / BDF2), and the worst relative error of
the five `model` arrays:
  n      force entries            model arrays
  4      2.1e-14 / 2.2e-12        9.1e-14 / 1.3e-12
  5      4.6e-13 / 3.6e-13        1.5e-13 / 1.8e-13
  8      6.7e-12 / 2.2e-13        5.4e-12 / 4.9e-14
  16     2.0e-13 / 1.1e-13        5.2e-14 / 7.4e-14
  32     2.6e-13 / 2.3e-12        1.2e-12 / 9.6e-13
  33     1.6e-11 / 9.2e-12        8.1e-13 / 4.4e-12
  64     1.4e-12 / 1.8e-13        2.7e-13 / 4.4e-13
  switching scene: 1.6e-12 / 2.7e-12.  testGrad, |num - ana| / max|ana| over the force constants: 5.9e-9 / 3.6e-9 at n = 4,
  1.5e-9 / 8.4e-10 at n = 16; the joint-stiffness direction agrees to 1.1e-7 relative or better.
No size comes within three decades of the 1e-7.
"""
import functools

import numpy as np
import pytest

import proto_point_forces as ppf
import proto_rollout_force_params as F
import proto_rollout_params as prm
import proto_rollout_pf as P
from test_gpu_adjoint_controls import _DevArray

pytestmark = pytest.mark.gpu

FN = F.NAMES
MN = prm.GROUPS


@functools.lru_cache(maxsize=None)
def _case(n):
    """Inputs and the numpy evaluator of a size ("switch": the switching scene) - built once, shared by the tests, never changed."""
    cs = P.switching_case() if n == "switch" else P.case(n)
    return cs, P.World(cs["sc"])


def _sim(cs, batch=2, desc=None):
    from redmax_amd import BatchSim
    return BatchSim(cs["sc"] if desc is None else desc, batch=batch, tape_forces=True)


def _tape(sim, cs, integ, sel=slice(None)):
    sim.set_state(cs["q0"][sel], cs["qd0"][sel])
    qt, qdt, info = sim.rollout_tape(cs["nsteps"], cs["h"], cs["u"][sel], pscale=cs["pscale"], integrator=integ, stats=True)
    assert (info["status"] & 15 == 0).all(), info["status"]
    return qt, qdt


def _grads(sim, cs, integ, sel=slice(None), **kw):
    """(qt, qdt, gq, gqd, du, dq0, dqd0, grads) under the loss of the proto."""
    qt, qdt = _tape(sim, cs, integ, sel)
    gq, gqd = cs["c"][sel] + qt, cs["d"][sel]
    return (qt, qdt, gq, gqd) + sim.rollout_vjp_forces(cs["nsteps"], gq, gqd, **kw)


class _OracleScene:
    """A scene of proto_point_forces as proto_rollout_params reads one (desc, getQ, h, nr and a task, which these scenes lack)."""

    def __init__(self, sc):
        self.task, self.h, self.nr, self.desc, self.getQ = None, sc.h, sc.nr, sc.desc, sc.getQ


def _stack(grads):
    """[B][nforces][3] from the three force arrays."""
    return np.stack([grads[n] for n in FN], axis=-1)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. every entry against the proto on the GPU's own record

@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", P.SIZES)
def test_every_entry_meets_the_proto_on_the_gpus_record(oracle_lib, n, integ):
    cs, ev = _case(n)
    sim = _sim(cs)
    qt, qdt, gq, gqd, du, dq0, dqd0, grads = _grads(sim, cs, integ, model=MN)
    sim.close()
    G = _stack(grads)
    assert G.shape == (2, len(ev.forces), 3)
    worst, worst_m = 0.0, 0.0
    for b in range(2):
        ref = F.on_record(ev, cs["q0"][b], cs["qd0"][b], qt[b], qdt[b], gq[b], gqd[b], cs["h"], cs["pscale"], integ)
        ratio = np.abs(G[b] - ref["G"]) / np.where(ref["S"] > 0, ref["S"], 1.0)
        worst = max(worst, float(ratio.max()))
        for f, force in enumerate(ev.forces):
            if force[0] == ppf.PP:      # no rest length: +0.0, bit for bit
                assert G[b, f, 2] == 0.0 and not np.signbit(G[b, f, 2])
                assert ref["S"][f, 2] == 0.0
        assert (np.abs(G[b] - ref["G"]) <= 1e-7 * ref["S"]).all(), (n, integ, b, ratio)
        # the five model arrays: proto_rollout_params' differences of the oracle's (force-free) residual with this tape's z
        slots = [(x, qA, qB, eta) for _, eta, qA, qB, x, _, _ in sorted(P.solves(cs["q0"][b], cs["qd0"][b], qt[b], qdt[b], cs["h"], integ),
                                                                       key=lambda s: s[0])]
        want = prm.grads(oracle_lib, _OracleScene(cs["sc"]), slots, ref["z"])
        for name in MN:
            assert grads[name][b].shape == want[name].shape and np.linalg.norm(want[name]) > 0, name
            worst_m = max(worst_m, P.rel(grads[name][b], want[name]))
        assert worst_m <= 1e-7, (n, integ, b, {k: P.rel(grads[k][b], want[k]) for k in MN})
    print("n=%s BDF%d: force entries worst |gpu - proto| / S = %.2e, model arrays worst relative = %.2e" % (n, integ, worst, worst_m))


# ---------------------------------------------------------------- 2. the testGrad identity on the device

def _desc_with(cs, theta=None, jstiff=None):
    d = dict(cs["sc"].desc())
    if theta is not None:
        d["point_forces"] = [dict(f, stiffness=float(t[0]), damping=float(t[1]), L=float(t[2])) for f, t in zip(d["point_forces"], theta)]
    if jstiff is not None:
        d["stiffness"] = np.asarray(jstiff, dtype=np.float64)
    return d


def _loss_of(cs, integ, desc):
    sim = _sim(cs, batch=1, desc=desc)
    qt, qdt = _tape(sim, cs, integ, slice(0, 1))
    sim.close()
    return P.loss_and_cotangents(qt[0], qdt[0], cs["c"][0], cs["d"][0])[0]


@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", [4, 16])
def test_gradients_meet_the_testgrad_identity(n, integ):
    """Central differences with relative step 1e-5 along 3 random directions over all force constants at once (the point-point L, which
    the model does not read, left out), rollouts on sims built from the perturbed tables; and one random direction in the joint
    stiffness against the `model` array.  Floor: the suite's 2e-5 |ana| + 1e-6 max|ana|."""
    from redmax_amd import _abi
    cs, ev = _case(n)
    sim = _sim(cs, batch=1)
    out = _grads(sim, cs, integ, slice(0, 1), model=("stiffness",))
    idx = np.zeros(int(sim._desc.njoints), dtype=np.int32)
    _abi.check(sim._L.rmx_model_idxR(sim._model, _abi.iptr(idx)), "rmx_model_idxR")
    sim.close()
    grads = out[-1]
    G = _stack(grads)[0]
    theta = F.constants(ev)
    mask = np.ones(theta.shape)
    mask[[f[0] == ppf.PP for f in ev.forces], 2] = 0.0
    rng = np.random.default_rng(31)
    eps = 1e-5
    num, ana = [], []
    for _ in range(3):
        dth = rng.standard_normal(theta.shape) * mask * theta
        Lp, Lm = (_loss_of(cs, integ, _desc_with(cs, theta + s * eps * dth)) for s in (1.0, -1.0))
        num.append((Lp - Lm) / (2 * eps))
        ana.append(float((dth * G).sum()))
    num, ana = np.array(num), np.array(ana)
    err = np.abs(num - ana)
    print("testgrad n %d BDF%d: force constants %.3e (of max|ana|)" % (n, integ, err.max() / np.abs(ana).max()))
    assert np.abs(ana).max() > 0
    assert (err <= 2e-5 * np.abs(ana) + 1e-6 * np.abs(ana).max()).all(), (num, ana)
    # the joint stiffness through `model`: per-joint values, one DOF per joint on these trees
    k = np.asarray(cs["sc"].desc()["stiffness"], dtype=np.float64)
    dk = rng.standard_normal(k.shape) * np.maximum(np.abs(k), 1.0) * (idx >= 0)
    Lp, Lm = (_loss_of(cs, integ, _desc_with(cs, jstiff=k + s * eps * dk)) for s in (1.0, -1.0))
    numk = (Lp - Lm) / (2 * eps)
    anak = float(sum(dk[j] * grads["stiffness"][0, idx[j]] for j in range(len(k)) if idx[j] >= 0))
    print("testgrad n %d BDF%d: joint stiffness num %.9e ana %.9e" % (n, integ, numk, anak))
    assert abs(anak) > 0 and abs(numk - anak) <= 2e-5 * abs(anak) + 1e-6 * abs(anak)


# ---------------------------------------------------------------- 3. cables

@pytest.mark.parametrize("integ", [1, 2])
def test_cables_that_switch_within_the_rollout(integ):
    """proto_point_forces.switchingScene(): two cables (no damping) that go slack and taut again within the twenty steps."""
    cs, ev = _case("switch")
    sim = _sim(cs)
    qt, qdt, gq, gqd, du, dq0, dqd0, grads = _grads(sim, cs, integ)
    sim.close()
    G = _stack(grads)
    for b in range(2):
        taut = P.cable_strains(ev, qt[b], qdt[b]) > 0
        assert all(taut[:, c].any() and not taut[:, c].all() for c in range(taut.shape[1]))
        ref = F.on_record(ev, cs["q0"][b], cs["qd0"][b], qt[b], qdt[b], gq[b], gqd[b], cs["h"], cs["pscale"], integ)
        ratio = np.abs(G[b] - ref["G"]) / np.where(ref["S"] > 0, ref["S"], 1.0)
        print("switching BDF%d b=%d: worst |gpu - proto| / S = %.2e" % (integ, b, ratio.max()))
        assert (ref["S"] > 0).all() and np.abs(ref["G"]).max() > 0
        assert (np.abs(G[b] - ref["G"]) <= 1e-7 * ref["S"]).all(), (integ, b, ratio)


@pytest.mark.parametrize("integ", [1, 2])
def test_a_cable_that_is_slack_throughout_has_exact_zeros(integ):
    """sizedSceneWithForces(8) with the cable's rest length at 1.5 times its length: +0.0 in the cable's three entries, and the other
    forces' entries are those of the scene without the cable in the table, bit for bit."""
    cs, _ = _case(8)
    res = []
    for drop in (False, True):
        sc = ppf.sizedSceneWithForces(8)
        cable = sc.forces[3]
        cable.setRetLength(1.5 * cable.L / 0.97)
        if drop:
            sc.forces = sc.forces[:3]
        sc.init()
        sim = _sim(dict(cs, sc=sc))
        out = _grads(sim, cs, integ)
        sim.close()
        res.append(_stack(out[-1]))
        if not drop:
            ev = P.World(sc)
            assert all((P.cable_strains(ev, out[0][b], out[1][b]) < 0).all() for b in range(2))
    assert res[0].shape == (2, 4, 3) and res[1].shape == (2, 3, 3)
    assert (res[0][:, 3] == 0.0).all() and not np.signbit(res[0][:, 3]).any()
    assert np.array_equal(res[0][:, :3], res[1]) and np.abs(res[1]).max() > 0


# ---------------------------------------------------------------- 4. the closed-loop tape

@pytest.mark.parametrize("integ", [1, 2])
def test_a_closed_loop_tape_is_the_open_loop_tape_under_uapp(integ):
    cs, _ = _case(8)
    N, h, ps, nr = cs["nsteps"], cs["h"], cs["pscale"], cs["sc"].nr
    rng = np.random.default_rng(61)
    K = 0.3 * rng.standard_normal((N, 2 * nr, nr))
    xref = np.concatenate([cs["q0"][0], cs["qd0"][0]])[None] + 0.05 * rng.standard_normal((N, 2 * nr))
    sim = _sim(cs)
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, ua, info = sim.rollout_feedback(N, h, cs["u"], K=K, xref=xref, pscale=ps, stats=True, integrator=integ)
    assert (info["status"] & 15 == 0).all() and not np.array_equal(ua, cs["u"])
    gq, gqd = cs["c"] + qt, cs["d"]
    closed = sim.rollout_vjp_forces(N, gq, gqd, model=MN)
    sim.set_state(cs["q0"], cs["qd0"])
    qt2, qdt2, _ = sim.rollout_tape(N, h, ua, pscale=ps, integrator=integ)
    assert np.array_equal(qt2, qt) and np.array_equal(qdt2, qdt)
    opened = sim.rollout_vjp_forces(N, gq, gqd, model=MN)
    sim.close()
    assert _same(closed[:3], opened[:3])
    assert set(closed[3]) == set(FN + MN)
    assert all(np.array_equal(closed[3][k], opened[3][k]) and np.abs(closed[3][k]).max() > 0 for k in closed[3])


# ---------------------------------------------------------------- 5. exact structure

@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", [5, 64])
def test_exact_structure(n, integ):
    cs, ev = _case(n)
    N, nf = cs["nsteps"], len(ev.forces)
    sim = _sim(cs)
    qt, qdt = _tape(sim, cs, integ)
    gq, gqd = cs["c"] + qt, cs["d"]
    state, count = sim.get_state(), sim.tape_count
    vjp, lin = sim.rollout_vjp(N, gq, gqd), sim.rollout_linearize(N)
    du, dq0, dqd0, grads = sim.rollout_vjp_forces(N, gq, gqd, model=MN)
    # du, dq0, dqd0 are rollout_vjp's bits
    assert _same((du, dq0, dqd0), vjp)
    assert all(np.isfinite(grads[k]).all() for k in grads)
    # a second call: the same bits; state, tape, rollout_vjp and rollout_linearize where they were
    again = sim.rollout_vjp_forces(N, gq, gqd, model=MN)
    assert _same(again[:3], vjp) and all(np.array_equal(again[3][k], grads[k]) for k in grads)
    assert sim.tape_count == count and _same(sim.get_state(), state)
    assert _same(sim.rollout_vjp(N, gq, gqd), vjp) and _same(sim.rollout_linearize(N), lin)
    # one output alone, without the initial state and without the other struct: the bits it has among all
    for name in FN:
        d1, n0, n1, g1 = sim.rollout_vjp_forces(N, gq, gqd, want=(name,), initial_state=False)
        assert n0 is None and n1 is None and np.array_equal(d1, du) and list(g1) == [name] and np.array_equal(g1[name], grads[name])
    for name in MN:
        g1 = sim.rollout_vjp_forces(N, gq, gqd, want=(), model=(name,))[3]
        assert list(g1) == [name] and np.array_equal(g1[name], grads[name])
    # the device form against the host form
    nan = np.full(qt.shape, np.nan)
    dev = {k: _DevArray(np.full(grads[k].shape, np.nan)) for k in grads}
    gq_d, gqd_d, du_d = _DevArray(gq), _DevArray(gqd), _DevArray(nan)
    dq0_d, dqd0_d = _DevArray(np.full(dq0.shape, np.nan)), _DevArray(np.full(dq0.shape, np.nan))
    sim.rollout_vjp_forces_device(N, gq_d.ptr.value, gqd_d.ptr.value, du_d.ptr.value, dq0_d.ptr.value, dqd0_d.ptr.value,
                                  **{k + "_ptr": dev[k].ptr.value for k in grads})
    assert np.array_equal(du_d.get(), du) and np.array_equal(dq0_d.get(), dq0) and np.array_equal(dqd0_d.get(), dqd0)
    assert all(np.array_equal(dev[k].get(), grads[k]) for k in grads)
    sim.rollout_vjp_forces_device(N, gq_d.ptr.value, gqd_d.ptr.value, du_d.ptr.value, force_L_ptr=dev["force_L"].ptr.value)
    assert np.array_equal(dev["force_L"].get(), grads["force_L"]) and np.array_equal(du_d.get(), du)
    for d in list(dev.values()) + [gq_d, gqd_d, du_d, dq0_d, dqd0_d]:
        d.free()
    assert _same(sim.rollout_vjp(N, gq, gqd), vjp) and _same(sim.rollout_linearize(N), lin)
    sim.close()
    assert grads["force_stiffness"].shape == (2, nf)
    # a rollout's rows depend neither on its place in the batch nor on the batch size
    three = _sim(cs, batch=3)
    order = [1, 0, 1]
    out = _grads(three, cs, integ, order, model=MN)
    three.close()
    assert _same(out[4:7], (du[order], dq0[order], dqd0[order]))
    assert all(np.array_equal(out[7][k], grads[k][order]) for k in grads)


# ---------------------------------------------------------------- 6. refusals

def test_refusals_in_the_librarys_words_leave_the_tape_usable():
    import ctypes as C
    from redmax_amd import BatchSim, _abi
    from redmax_amd.scenes import scenesRedMax
    cs, _ = _case(8)
    N = cs["nsteps"]
    sim = _sim(cs)
    L = sim._L
    nr, nf = sim.nr, sim.nforces
    gq, gqd, du = np.ones((2, N, nr)), np.ones((2, N, nr)), np.empty((2, N, nr))
    dq0, out = np.empty((2, nr)), np.empty((2, nf))
    dp = _abi.dptr
    fg = _abi.ForceGrads(out.ctypes.data, None, None)
    none_f, none_m = _abi.ForceGrads(None, None, None), _abi.ParamGrads(None, None, None, None, None)

    def refused(words, *args):
        rc = L.rmx_rollout_vjp_forces(*args)
        assert rc != 0 and words in L.rmx_last_error().decode(), (rc, L.rmx_last_error())

    refused("rmx_rollout_vjp_forces: no tape", sim._batch, N, dp(gq), dp(gqd), dp(du), None, None, None, C.byref(fg))
    qt, qdt = _tape(sim, cs, 1)
    ok = sim.rollout_vjp_forces(N, gq, gqd)
    vjp = sim.rollout_vjp(N, gq, gqd)
    cases = (("rmx_rollout_vjp_forces: null argument", None, N, dp(gq), dp(gqd), dp(du), None, None, None, C.byref(fg)),
             ("rmx_rollout_vjp_forces: null argument", sim._batch, N, None, dp(gqd), dp(du), None, None, None, C.byref(fg)),
             ("rmx_rollout_vjp_forces: null argument", sim._batch, N, dp(gq), None, dp(du), None, None, None, C.byref(fg)),
             ("rmx_rollout_vjp_forces: null argument", sim._batch, N, dp(gq), dp(gqd), None, None, None, None, C.byref(fg)),
             ("rmx_rollout_vjp_forces: dq0 and dqd0 must be given together", sim._batch, N, dp(gq), dp(gqd), dp(du), dp(dq0), None, None, C.byref(fg)),
             ("rmx_rollout_vjp_forces: all outputs are null", sim._batch, N, dp(gq), dp(gqd), dp(du), None, None, None, None),
             ("rmx_rollout_vjp_forces: all outputs are null", sim._batch, N, dp(gq), dp(gqd), dp(du), None, None, C.byref(none_m), C.byref(none_f)),
             ("rmx_rollout_vjp_forces: nsteps differs from the tape's (%d)" % N, sim._batch, N + 1, dp(gq), dp(gqd), dp(du), None, None, None, C.byref(fg)))
    for c in cases:
        refused(*c)
        # the tape survived the refusal
        again = sim.rollout_vjp_forces(N, gq, gqd)
        assert _same(again[:3], ok[:3]) and all(np.array_equal(again[3][k], ok[3][k]) for k in ok[3])
    # rmx_rollout_vjp_params still refuses such a tape, word for word
    with pytest.raises(_abi.RedMaxHipError, match=r"rmx_rollout_vjp_params: the tape carries point forces \(rmx_model_tape_point_forces\); "
                                                  r"the parameters' contraction does not cover them"):
        sim.rollout_vjp_params(N, gq, gqd)
    assert _same(sim.rollout_vjp(N, gq, gqd), vjp)
    with pytest.raises(ValueError, match="rollout_vjp_forces: want and model name no output"):
        sim.rollout_vjp_forces(N, gq, gqd, want=(), model=())
    with pytest.raises(ValueError, match="rollout_vjp_forces: want must name distinct outputs"):
        sim.rollout_vjp_forces(N, gq, gqd, want=("stiffness",))
    sim.close()
    # a tape without point forces: the message names the call for it
    sc = scenesRedMax(2)
    sc.init()
    plain = BatchSim(sc, batch=1)
    q0, qd0 = sc.getQ()
    plain.set_state(q0[None], qd0[None])
    plain.rollout_tape(2, sc.h, np.zeros((1, 2, sc.nr)))
    g = np.ones((1, 2, sc.nr))
    with pytest.raises(_abi.RedMaxHipError, match="rmx_rollout_vjp_forces: the tape carries no point forces.*rmx_rollout_vjp_params is the call"):
        plain.rollout_vjp_forces(2, g, g, want=(), model=("grav",))
    assert np.isfinite(plain.rollout_vjp_params(2, g, g)[3]["grav"]).all()
    plain.close()
