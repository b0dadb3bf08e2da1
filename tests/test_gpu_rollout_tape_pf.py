"""Taped rollouts of models with body-to-body forces (rmx_model_tape_point_forces): the tape entries take a model with a force
table, the tape they leave carries the forces in H and in D, and every reader of a tape runs on it unchanged.

The checks, in the order of the sections below:
  1. the switch: off, the four tape entries refuse scene 12 in the words they always had; on, they run; off again they refuse again
     and the tape survives; a model without forces has the same bits and the same kernel label either way;
  2. the forward record of both integrators at every size against the numpy rollout of tests/proto_rollout_pf.py: |dq|/|q| <= 1e-8
     per trajectory (the suite's bound for rollouts with these forces, tests/test_gpu_point_forces_edges.py), clean statuses, qdtraj
     the difference quotient of qtraj;
  3. the tape through its readers at every size: du, dq0, dqd0 of rmx_rollout_vjp and XA, XB, XU of rmx_rollout_linearize against
     the proto evaluated ON THE GPU'S OWN RECORD, to 1e-7 relative (the bound the suite holds every taped gradient to);
  4. the testGrad identity on the device at n = 4 and n = 16: central differences of the GPU's own rollout;
  5. the closed loop at n = 8 and n = 33: uapp against its formula, the open-loop tape under uapp bit for bit, rmx_rollout_vjp_feedback
     against the proto recursion at 1e-7;
  6. cables: a cable that is slack throughout has the bits of the scene without it; the switching scene against the proto;
  7. exact structure at n = 5 and n = 64: batch independence, repeatability, device forms, a tape that rmx_rollout_vjp leaves alone;
  8. refusals.

Scenes: proto_point_forces.sizedSceneWithForces(n) - a point-point force, a world-anchored spring, a body-body spring and a four-point
cable on sceneTree(n) - at n = 4, 8, 16, 32, 64 (each fills its padded size) and n = 5, 33 (part-filled at 8 and 64 lanes), B = 2
from sizedStates, 4 steps (3 at 64 lanes); the inputs are proto_rollout_pf.case(n), on which tests/test_rollout_pf_proto.py asserts
that the proto's Newton converges.  On these scenes h |D_pf| / |M| is 0.18 .. 0.39 and |D_pf| / |D0| above 200 (asserted there): a
missing or wrong force block in D cannot hide behind the 1e-7.

Measured on an MI355X (worst over the two rollouts):
  n        record |dq|/|q|  BDF1 / BDF2    du, dq0, dqd0        XA, XB, XU       guard
  4, 5     4.6e-15 / 5.6e-15               8.3e-12 (n=4 BDF2)   1.2e-11          -
  8        7.2e-14 / 4.1e-14               2.8e-12              2.1e-12          -
  16       5.2e-15 / 4.1e-15               7.8e-14              1.7e-13          -
  32       3.9e-14 / 8.3e-14               1.7e-12              1.1e-12          -
  33       9.6e-14 / 1.1e-13               5.1e-12              4.6e-12          RMX_ST_PIVOTED on three of the four rollouts
  64       1.8e-14 / 9.9e-15               3.1e-13              4.0e-13          -
  closed loop (n = 8, 33): duff, dK, dxref, dq0, dqd0 within 1.8e-11 of the proto recursion
  switching scene: record 6.0e-15, gradients 2.1e-11, XA 1.3e-11; the taut / slack sequences are the proto's
No size comes within three decades of the 1e-7.
"""
import functools

import numpy as np
import pytest

import proto_point_forces as ppf
import proto_rollout_linearize as plin
import proto_rollout_pf as P
from test_gpu_adjoint_controls import _DevArray

pytestmark = pytest.mark.gpu

WORDS = r"point forces \(rmx_model_set_point_forces\) are outside the adjoint path"
LABELS = {(1, False): "k_adjoint_fwd<bdf1,tape,pf>", (2, False): "k_adjoint_fwd<bdf2,tape,pf>",
          (1, True): "k_adjoint_fwd<bdf1,tape,feedback,pf>", (2, True): "k_adjoint_fwd<bdf2,tape,feedback,pf>"}


@functools.lru_cache(maxsize=None)
def _case(n):
    """Inputs and the numpy evaluator of a size ("switch": the switching scene) - built once, shared by the tests, never changed."""
    cs = P.switching_case() if n == "switch" else P.case(n)
    return cs, P.World(cs["sc"])


@functools.lru_cache(maxsize=None)
def _proto_rollout(n, integ, b):
    cs, ev = _case(n)
    info = {}
    out = P.rollout(ev, cs["q0"][b], cs["qd0"][b], cs["u"][b], cs["h"], cs["pscale"], integ, info)
    assert info["converged"]
    return out


def _sim(cs, batch=2, on=True):
    from redmax_amd import BatchSim
    return BatchSim(cs["sc"], batch=batch, tape_forces=on)


def _tape(sim, cs, integ, sel=slice(None), **kw):
    sim.set_state(cs["q0"][sel], cs["qd0"][sel])
    return sim.rollout_tape(cs["nsteps"], cs["h"], cs["u"][sel], pscale=cs["pscale"], integrator=integ, **kw)


def _tape_and_vjp(sim, cs, integ, sel=slice(None)):
    qt, qdt, info = _tape(sim, cs, integ, sel, stats=True)
    assert (info["status"] & 15 == 0).all(), info["status"]
    return (qt, qdt) + tuple(sim.rollout_vjp(cs["nsteps"], cs["c"][sel] + qt, cs["d"][sel]))


def _proto_on_record(n, integ, b, qt, qdt):
    """The proto's tape at the GPU's recorded states of rollout b, and what its readers make of it."""
    cs, ev = _case(n)
    H, M, D = P.tape(ev, cs["q0"][b], cs["qd0"][b], qt, qdt, cs["h"], integ)
    du, dq0, dqd0 = P.vjp(H, M, D, cs["c"][b] + qt, cs["d"][b], cs["h"], cs["pscale"], integ)
    XA, XB, XU = P.linearize(H, M, D, cs["h"], cs["pscale"], integ)
    return dict(H=H, M=M, D=D, du=du, dq0=dq0, dqd0=dqd0, XA=XA, XB=XB, XU=XU)


# ---------------------------------------------------------------- 1. the switch

def test_the_switch_opens_and_closes_the_four_tape_entries():
    from redmax_amd import BatchSim, _abi
    from redmax_amd.scenes import scenesRedMax
    sc = scenesRedMax(12)
    sc.init()
    nsteps, Bs = 2, 2
    u = np.zeros((Bs, nsteps, sc.nr))
    K = np.zeros((nsteps, 2 * sc.nr, sc.nr))
    q0, qd0 = sc.getQ()
    sim = BatchSim(sc, batch=Bs)
    assert not sim.tapes_point_forces

    def entries():
        return (lambda: sim.rollout_tape(nsteps, sc.h, u), lambda: sim.rollout_tape(nsteps, sc.h, u, integrator=2),
                lambda: sim.rollout_feedback(nsteps, sc.h, u, K=K), lambda: sim.rollout_feedback(nsteps, sc.h, u, K=K, ulim=(None, None)))

    def refused():
        for call in entries():
            sim.set_state(q0[None, :], qd0[None, :])
            with pytest.raises(_abi.RedMaxHipError, match=WORDS):
                call()

    refused()
    sim.tape_point_forces(True)
    assert sim.tapes_point_forces
    for call, key in zip(entries(), ((1, False), (2, False), (1, True), (1, True))):
        sim.set_state(q0[None, :], qd0[None, :])
        out = call()
        assert np.isfinite(out[0]).all()
        assert sim.last_step_kernel() == LABELS[key], sim.last_step_kernel()
    # the tape of the last call (a BDF1 closed loop without gains that act) survives the switch going off, and the refusals after it
    g = np.ones((Bs, nsteps, sc.nr))
    before = sim.rollout_vjp(nsteps, g, g)
    sim.tape_point_forces(False)
    assert not sim.tapes_point_forces
    refused()
    assert all(np.array_equal(a, b) for a, b in zip(before, sim.rollout_vjp(nsteps, g, g)))
    sim.set_state(q0[None, :], qd0[None, :])
    out = sim.step_bdf1(2, h=sc.h, stats=True)
    assert (out["status"] & 15 == 0).all()
    sim.close()


def test_a_model_without_forces_is_not_affected():
    """Scene 2 (a branching tree, no force table): the four entries return the same bits and report the same kernel, switch on or off."""
    from redmax_amd import BatchSim
    from redmax_amd.scenes import scenesRedMax
    sc = scenesRedMax(2)
    sc.init()
    nsteps, Bs = 3, 2
    rng = np.random.default_rng(8)
    q0, qd0 = sc.getQ()
    q = q0[None] + 0.05 * rng.standard_normal((Bs, sc.nr))
    qd = qd0[None] + 0.2 * rng.standard_normal((Bs, sc.nr))
    u = 0.1 * rng.standard_normal((Bs, nsteps, sc.nr))
    K = 0.1 * rng.standard_normal((nsteps, 2 * sc.nr, sc.nr))
    g = rng.standard_normal((Bs, nsteps, sc.nr))
    res = []
    for on in (False, True):
        sim = BatchSim(sc, batch=Bs, tape_forces=on)
        outs = []
        for call in (lambda: sim.rollout_tape(nsteps, sc.h, u), lambda: sim.rollout_tape(nsteps, sc.h, u, integrator=2),
                     lambda: sim.rollout_feedback(nsteps, sc.h, u, K=K), lambda: sim.rollout_feedback(nsteps, sc.h, u, K=K, integrator=2),
                     lambda: sim.rollout_feedback(nsteps, sc.h, u, K=K, ulim=(np.full(sc.nr, -0.05), None))):
            sim.set_state(q, qd)
            out = call()
            outs.append([np.asarray(a) for a in out[:2]] + [sim.last_step_kernel()] + list(sim.rollout_vjp(nsteps, g, g)))
        res.append(outs)
        sim.close()
    for a, b in zip(*res):
        assert a[2] == b[2] and "pf" not in a[2]
        assert all(np.array_equal(x, y) for x, y in zip(a[:2] + a[3:], b[:2] + b[3:]))


# ---------------------------------------------------------------- 2. the forward record

@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", P.SIZES)
def test_forward_record_meets_the_proto(n, integ):
    cs, ev = _case(n)
    sim = _sim(cs)
    qt, qdt, info = _tape(sim, cs, integ, stats=True)
    label = sim.last_step_kernel()
    q, qd = sim.get_state()
    sim.close()
    assert label == LABELS[(integ, False)], label
    assert (info["status"] & 15 == 0).all(), info["status"]
    assert np.array_equal(qt[:, -1], q) and np.array_equal(qdt[:, -1], qd)
    h, N = cs["h"], cs["nsteps"]
    for b in range(2):
        qo, qdo = _proto_rollout(n, integ, b)
        print("n=%d BDF%d b=%d: |dq|/|q| = %.2e, |dqdot|/|qdot| = %.2e, status %d, %d iterations" % (
            n, integ, b, P.rel(qt[b], qo), P.rel(qdt[b], qdo), info["status"][b], info["newton_iters"][b]))
        assert P.rel(qt[b], qo) <= 1e-8, (n, integ, b, P.rel(qt[b], qo))
    # the recorded qdot is the integrator's difference quotient of the recorded q, up to the rounding of that difference
    qprev = np.concatenate([cs["q0"][:, None], qt[:, :-1]], axis=1)
    bound = 8 * np.finfo(float).eps * max(np.abs(qt).max(), np.abs(cs["q0"]).max()) / h
    if integ == 1:
        assert (np.abs(qdt - (qt - qprev) / h) <= bound).all()
    else:
        qpp = np.concatenate([cs["q0"][:, None], qt[:, :-2]], axis=1)
        quot = (3.0 / (2.0 * h)) * (qt[:, 1:] - (4.0 / 3.0) * qprev[:, 1:] + (1.0 / 3.0) * qpp)
        assert (np.abs(qdt[:, 1:] - quot) <= 2 * bound).all()
        assert N >= 2


# ---------------------------------------------------------------- 3. the tape through its readers

@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", P.SIZES)
def test_the_tape_meets_the_proto_through_its_readers(n, integ):
    """du, dq0, dqd0 and XA, XB, XU to 1e-7 relative to the proto on the GPU's own record.  XA = -eta H^-1 D is where a wrong D
    shows first."""
    cs, ev = _case(n)
    sim = _sim(cs)
    qt, qdt, du, dq0, dqd0 = _tape_and_vjp(sim, cs, integ)
    XA, XB, XU = sim.rollout_linearize(cs["nsteps"])
    sim.close()
    for b in range(2):
        ref = _proto_on_record(n, integ, b, qt[b], qdt[b])
        errs = dict(du=P.rel(du[b], ref["du"]), dq0=P.rel(dq0[b], ref["dq0"]), dqd0=P.rel(dqd0[b], ref["dqd0"]),
                    XA=P.rel(XA[b], ref["XA"]), XB=P.rel(XB[b], ref["XB"]), XU=P.rel(XU[b], ref["XU"]))
        print("n=%d BDF%d b=%d: " % (n, integ, b) + ", ".join("%s %.2e" % kv for kv in errs.items()))
        assert max(errs.values()) <= 1e-7, (n, integ, b, errs)
        # the control: without D_pf the proto's XA is far from the device's
        D0 = np.stack([ev.MD(x, (x - qA) / eta, with_pf=False)[1] for _, eta, qA, _, x, _, _ in
                       sorted(P.solves(cs["q0"][b], cs["qd0"][b], qt[b], qdt[b], cs["h"], integ))])
        XA0 = plin.sens(ref["H"], ref["M"], D0, plin.etas(cs["nsteps"], cs["h"], integ), cs["pscale"])[0]
        assert P.rel(XA[b], XA0) >= 1e-2


# ---------------------------------------------------------------- 4. the testGrad identity on the device

@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", [4, 16])
def test_gradients_meet_the_testgrad_identity(n, integ):
    """Central differences (eps = 1e-5, 3 random directions per group, one batch of 18 rollouts) of the proto's loss over the GPU's
    own rollout, along directions in u, in q0 and in qdot0, against direction . gradient.  Floor: tests/test_gpu_rollout_vjp.py's,
    2e-5 |ana| + 1e-6 max|ana|.

    Measured on an MI355X, max over the 3 directions of |num - ana| / max|ana|:
        n  integrator      u         q0        qdot0
        4     BDF1      1.5e-08   1.5e-10   4.4e-09
        4     BDF2      4.2e-08   7.1e-10   4.8e-09
       16     BDF1      6.4e-09   7.8e-10   6.7e-09
       16     BDF2      2.0e-08   5.2e-08   5.2e-09
    two decades below the floor in every case.
    """
    cs, _ = _case(n)
    nsteps, h, ps = cs["nsteps"], cs["h"], cs["pscale"]
    one = {k: cs[k][:1] for k in ("q0", "qd0", "u", "c", "d")}
    sim = _sim(cs, batch=1)
    _, _, du, dq0, dqd0 = _tape_and_vjp(sim, dict(cs, **one), integ)
    sim.close()
    grads = {"u": du[0], "q0": dq0[0], "qd0": dqd0[0]}
    nd, eps = 3, 1e-5
    rng = np.random.default_rng(29)
    groups = ("u", "q0", "qd0")
    dirs, pert = [], {k: [] for k in grads}
    for g in groups:
        for _ in range(nd):
            d = {k: (rng.standard_normal(grads[k].shape) if k == g else np.zeros(grads[k].shape)) for k in grads}
            dirs.append(d)
            for sgn in (1.0, -1.0):
                for k in grads:
                    pert[k].append(one[k][0] + sgn * eps * d[k])
    nb = len(pert["u"])
    fd = _sim(cs, batch=nb)
    fd.set_state(np.array(pert["q0"]), np.array(pert["qd0"]))
    qt, qdt, info = fd.rollout_tape(nsteps, h, np.array(pert["u"]), pscale=ps, stats=True, integrator=integ)
    fd.close()
    assert (info["status"] & 15 == 0).all()
    L = np.array([P.loss_and_cotangents(qt[i], qdt[i], one["c"][0], one["d"][0])[0] for i in range(nb)])
    num = (L[0::2] - L[1::2]) / (2 * eps)
    ana = np.array([sum(float((d[k] * grads[k]).sum()) for k in grads) for d in dirs])
    shown = []
    for i, g in enumerate(groups):
        a, e = ana[i * nd:(i + 1) * nd], np.abs(num - ana)[i * nd:(i + 1) * nd]
        shown.append(e.max() / np.abs(a).max())
        assert np.abs(a).max() > 0
        assert (e <= 2e-5 * np.abs(a) + 1e-6 * np.abs(a).max()).all(), (g, num[i * nd:(i + 1) * nd], a, e)
    print("testgrad n %d BDF%d: u %.3e, q0 %.3e, qdot0 %.3e (of max|ana|)" % ((n, integ) + tuple(shown)))


# ---------------------------------------------------------------- 5. the closed loop

def _gains(cs, b_scale=0.3):
    nr, N = cs["sc"].nr, cs["nsteps"]
    rng = np.random.default_rng(61)
    K = b_scale * rng.standard_normal((N, 2 * nr, nr))
    xref = np.concatenate([cs["q0"][0], cs["qd0"][0]])[None] + 0.05 * rng.standard_normal((N, 2 * nr))
    return K, xref


@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", [8, 33])
def test_closed_loop_with_and_without_a_box(n, integ):
    import proto_rollout_vjp_feedback as pvf
    cs, ev = _case(n)
    N, h, ps, nr = cs["nsteps"], cs["h"], cs["pscale"], cs["sc"].nr
    K, xref = _gains(cs)
    sim = _sim(cs)
    for ulim in (None, (np.full(nr, -0.08), np.full(nr, 0.08))):
        sim.set_state(cs["q0"], cs["qd0"])
        qt, qdt, ua, info = sim.rollout_feedback(N, h, cs["u"], K=K, xref=xref, pscale=ps, stats=True, integrator=integ, ulim=ulim)
        assert sim.last_step_kernel() == LABELS[(integ, True)]
        assert (info["status"] & 15 == 0).all(), info["status"]
        # uapp against the formula on the returned rows
        x = np.stack([pvf.start_states(cs["q0"][b], cs["qd0"][b], qt[b], qdt[b]) for b in range(2)])      # [B][N][2nr]
        want = cs["u"] + np.einsum("kji,bkj->bki", K, x - xref[None])
        if ulim is not None:
            clamped = (want < ulim[0]) | (want > ulim[1])
            assert clamped.any() and not clamped.all()
            assert np.array_equal(ua[clamped], np.clip(want, ulim[0], ulim[1])[clamped])
            want = np.clip(want, ulim[0], ulim[1])
        assert np.allclose(ua, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        # the tape is the open-loop tape under uapp: the same record, the same readers' output, bit for bit
        gq, gqd = cs["c"] + qt, cs["d"]
        vjp_c, lin_c = sim.rollout_vjp(N, gq, gqd), sim.rollout_linearize(N)
        if ulim is None:
            out = sim.rollout_vjp_feedback(N, gq, gqd, K=K, xref=xref, gu=cs["d"])
        sim.set_state(cs["q0"], cs["qd0"])
        qt2, qdt2, _ = sim.rollout_tape(N, h, ua, pscale=ps, integrator=integ)
        assert np.array_equal(qt2, qt) and np.array_equal(qdt2, qdt)
        assert all(np.array_equal(a, b) for a, b in zip(vjp_c, sim.rollout_vjp(N, gq, gqd)))
        assert all(np.array_equal(a, b) for a, b in zip(lin_c, sim.rollout_linearize(N)))
        if ulim is not None:
            continue
        # the closed-loop adjoint against the proto recursion on the proto's tape at the GPU's record
        for b in range(2):
            H, M, D = P.tape(ev, cs["q0"][b], cs["qd0"][b], qt[b], qdt[b], h, integ)
            ref = pvf.vjp(integ, H, M, D, K, x[b] - xref, gq[b], gqd[b], cs["d"][b], h, ps)
            errs = {k: P.rel(out[k][b], ref[k]) for k in ("duff", "dK", "dxref", "dq0", "dqd0")}
            print("n=%d BDF%d b=%d closed loop: " % (n, integ, b) + ", ".join("%s %.2e" % kv for kv in errs.items()))
            assert max(errs.values()) <= 1e-7, (n, integ, b, errs)
    sim.close()


# ---------------------------------------------------------------- 6. cables

@pytest.mark.parametrize("integ", [1, 2])
def test_a_cable_that_is_slack_throughout_leaves_no_trace(integ):
    """sizedSceneWithForces(8) with the cable's rest length at 1.5 times its length, against the same scene without the cable in the
    table: the same bits in the record and in what the readers make of the tape."""
    from redmax_amd import BatchSim
    cs, _ = _case(8)
    res = []
    for drop in (False, True):
        sc = ppf.sizedSceneWithForces(8)
        cable = sc.forces[3]
        cable.setRetLength(1.5 * cable.L / 0.97)
        if drop:
            sc.forces = sc.forces[:3]
        sc.init()
        sim = BatchSim(sc, batch=2, tape_forces=True)
        assert len(sc.desc()["point_forces"]) == (3 if drop else 4)
        out = _tape_and_vjp(sim, cs, integ) + tuple(sim.rollout_linearize(cs["nsteps"]))
        sim.close()
        res.append(out)
        if not drop:      # slack at every recorded step
            ev = P.World(sc)
            assert all((P.cable_strains(ev, out[0][b], out[1][b]) < 0).all() for b in range(2))
    assert all(np.array_equal(a, b) for a, b in zip(*res))


@pytest.mark.parametrize("integ", [1, 2])
def test_cables_that_switch_within_the_rollout(integ):
    """proto_point_forces.switchingScene(), 20 steps (tests/test_rollout_pf_proto.py: the proto's Newton converges on it and no
    recorded step is within 1e-6 of a cable's rest length): the record against the proto at 1e-8, the gradients against the proto on
    the GPU's record at 1e-7, and the cables' taut / slack sequence equal to the proto's."""
    cs, ev = _case("switch")
    sim = _sim(cs)
    qt, qdt, du, dq0, dqd0 = _tape_and_vjp(sim, cs, integ)
    XA = sim.rollout_linearize(cs["nsteps"], which=("XA",))[0]
    sim.close()
    for b in range(2):
        qo, qdo = _proto_rollout("switch", integ, b)
        assert P.rel(qt[b], qo) <= 1e-8, (b, P.rel(qt[b], qo))
        taut, taut_o = P.cable_strains(ev, qt[b], qdt[b]) > 0, P.cable_strains(ev, qo, qdo) > 0
        assert np.array_equal(taut, taut_o)
        assert all(ppf.switches(list(taut[:, c])) or (taut[:, c].any() and not taut[:, c].all()) for c in range(taut.shape[1]))
        ref = _proto_on_record("switch", integ, b, qt[b], qdt[b])
        errs = dict(du=P.rel(du[b], ref["du"]), dq0=P.rel(dq0[b], ref["dq0"]), dqd0=P.rel(dqd0[b], ref["dqd0"]), XA=P.rel(XA[b], ref["XA"]))
        print("switching BDF%d b=%d: |dq|/|q| %.2e, " % (integ, b, P.rel(qt[b], qo)) + ", ".join("%s %.2e" % kv for kv in errs.items()))
        assert max(errs.values()) <= 1e-7, (integ, b, errs)


# ---------------------------------------------------------------- 7. exact structure

@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", [5, 64])
def test_batch_independence_repeatability_and_device_forms(n, integ):
    cs, _ = _case(n)
    N, h, ps = cs["nsteps"], cs["h"], cs["pscale"]
    sim = _sim(cs)
    ref = _tape_and_vjp(sim, cs, integ)
    qt, qdt, du, dq0, dqd0 = ref
    gq, gqd = cs["c"] + qt, cs["d"]
    # rmx_rollout_vjp does not change the tape: the linearisation before and after it, and a second vjp, have the same bits
    lin = sim.rollout_linearize(N)
    assert all(np.array_equal(a, b) for a, b in zip(sim.rollout_vjp(N, gq, gqd), (du, dq0, dqd0)))
    assert all(np.array_equal(a, b) for a, b in zip(sim.rollout_linearize(N), lin))
    # a repeated call: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(_tape_and_vjp(sim, cs, integ), ref))
    # the device-pointer forms equal the host forms
    nan = np.full(qt.shape, np.nan)
    u_d, qt_d, qdt_d = _DevArray(cs["u"]), _DevArray(nan), _DevArray(nan)
    sim.set_state(cs["q0"], cs["qd0"])
    info = sim.rollout_tape_device(N, h, u_d.ptr.value, qt_d.ptr.value, qdt_d.ptr.value, pscale=ps, stats=True, integrator=integ)
    assert (info["status"] & 15 == 0).all()
    assert np.array_equal(qt_d.get(), qt) and np.array_equal(qdt_d.get(), qdt)
    gq_d, gqd_d, du_d = _DevArray(gq), _DevArray(gqd), _DevArray(nan)
    dq0_d, dqd0_d = _DevArray(np.full(dq0.shape, np.nan)), _DevArray(np.full(dq0.shape, np.nan))
    sim.rollout_vjp_device(N, gq_d.ptr.value, gqd_d.ptr.value, du_d.ptr.value, dq0_d.ptr.value, dqd0_d.ptr.value)
    assert np.array_equal(du_d.get(), du) and np.array_equal(dq0_d.get(), dq0) and np.array_equal(dqd0_d.get(), dqd0)
    ua_d = _DevArray(nan)
    sim.set_state(cs["q0"], cs["qd0"])
    sim.rollout_feedback_device(N, h, u_d.ptr.value, None, None, qt_d.ptr.value, qdt_d.ptr.value, ua_d.ptr.value, pscale=ps, integrator=integ)
    sim.set_state(cs["q0"], cs["qd0"])
    fb = sim.rollout_feedback(N, h, cs["u"], pscale=ps, integrator=integ)
    assert np.array_equal(qt_d.get(), fb[0]) and np.array_equal(qdt_d.get(), fb[1]) and np.array_equal(ua_d.get(), cs["u"])
    for d in (u_d, qt_d, qdt_d, gq_d, gqd_d, du_d, dq0_d, dqd0_d, ua_d):
        d.free()
    sim.close()
    # a rollout's results depend neither on its place in the batch nor on the batch size
    one = _sim(cs, batch=1)
    for b in range(2):
        for a, r in zip(_tape_and_vjp(one, cs, integ, slice(b, b + 1)), ref):
            assert np.array_equal(a[0], r[b]), (n, integ, b)
    one.close()
    three = _sim(cs, batch=3)
    order = [1, 0, 1]
    for a, r in zip(_tape_and_vjp(three, cs, integ, order), ref):
        assert np.array_equal(a, r[order]), (n, integ)
    three.close()


# ---------------------------------------------------------------- 8. refusals

def test_refusals_in_the_librarys_words_leave_the_batch_alone():
    """On a model with forces and the switch ON: rmx_rollout_vjp_params refuses the tape; rmx_rollout_search, rmx_adjoint_controls and
    rmx_adjoint_track refuse the model in the words they always had.  After each the batch steps exactly like one never asked."""
    from redmax_amd import _abi
    cs, _ = _case(8)
    sc, N, nr = cs["sc"], cs["nsteps"], cs["sc"].nr
    fresh, sim = _sim(cs, on=False), _sim(cs)
    fresh.set_state(cs["q0"], cs["qd0"])
    fresh.step_bdf1(2, h=cs["h"])
    want = fresh.get_state()
    fresh.close()
    qt, qdt, du, dq0, dqd0 = _tape_and_vjp(sim, cs, 1)
    gq, gqd = cs["c"] + qt, cs["d"]
    task = dict(body=0, xlocal=[0.0, 0.0, 0.0], xtarget=[0.0, 0.0, 0.0], step=N, pscale=1.0, wreg=0.0, wpos=1.0)
    track = dict(terms=[dict(body=0, xlocal=[0.0, 0.0, 0.0], step=N, wpos=1.0)], xtarget=np.zeros((1, 3)), pscale=1.0, wreg=0.0)
    calls = ((r"rmx_rollout_vjp_params: the tape carries point forces", lambda: sim.rollout_vjp_params(N, gq, gqd)),
             (WORDS, lambda: sim.rollout_search(N, cs["h"], cs["u"], R=np.eye(nr))),
             (WORDS, lambda: sim.adjoint_controls(N, cs["h"], task, cs["u"])),
             (WORDS, lambda: sim.adjoint_track(N, cs["h"], track, cs["u"])))
    for words, call in calls:
        with pytest.raises(_abi.RedMaxHipError, match=words):
            call()
        # the tape survived the refusal
        assert all(np.array_equal(a, b) for a, b in zip(sim.rollout_vjp(N, gq, gqd), (du, dq0, dqd0)))
        sim.set_state(cs["q0"], cs["qd0"])
        sim.step_bdf1(2, h=cs["h"])
        assert all(np.array_equal(a, b) for a, b in zip(sim.get_state(), want))
    sim.close()
