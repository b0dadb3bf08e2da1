"""rmx_rollout_vjp_feedback: the closed-loop adjoint of the taped rollout - dL/duff, dL/dK, dL/dxref, dL/dq0, dL/dqdot0 of a rollout
that ran under rmx_rollout_tape_feedback, for cotangents of its states and of its applied torques.

The checks, in the order of the sections below, BDF1 and BDF2 unless a section says otherwise:
  1. against the numpy recursion of tests/proto_rollout_vjp_feedback.py on the oracle's tape (pinned on the CPU against central
     differences by tests/test_rollout_vjp_feedback_proto.py), 1e-7 relative - the bound tests/test_gpu_rollout_vjp.py holds du, dq0
     and dqd0 to;
  2. against the dense closed-loop costate recursion on rmx_rollout_linearize's A_k, B_k of the same tape (BDF1), the same 1e-7;
  3. the testGrad identity on the GPU's own closed loop: central differences of rmx_rollout_tape_feedback;
  4. without gains: rmx_rollout_vjp's bits, a table of zeros, gu alone;
  5. exact structure: shared against per-rollout tables, a permuted batch, the NULL pattern of the outputs, repetition, the other
     tape readers before and after, device pointers, a NULL reference, one and two steps;
  6. refusals, each by its words, and what a refused call leaves alone;
  7. the torch side: diff.rollout_closed_loop;
  8. the MEX command.

Scenes by the path each takes (feedback_case of tests/test_rollout_feedback_proto.py): 5-link chain and tree7 NP 8, "fixed" NP 8 with
two nodes that have no DOF (lanes with idx < 0 inside the tree), 16-link chain NP 16 (the guarded solve with its DPP sequence),
32-link chain NP 32, 40-link chain the 64-lane path (three chunks of 16 rows of K, the last one partly past the tree).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_adjoint_controls import _DevArray, _rel
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)
from test_rollout_feedback_proto import B, feedback_case
from test_rollout_vjp_feedback_proto import gu_case, reference

SIZES = [5, "tree7", "fixed", 16, 32, 40]
NAMES = ("duff", "dK", "dxref", "dq0", "dqd0")


def _forward(sim, sc, cs, integ, sel=slice(None), K="case", xref="case", uff=None):
    sim.set_state(cs["q0"][sel], cs["qd0"][sel])
    K = cs["K"] if isinstance(K, str) else K
    xref = cs["xref"] if isinstance(xref, str) else xref
    uff = cs["u"][sel] if uff is None else uff
    qt, qdt, ua, info = sim.rollout_feedback(uff.shape[1], sc.h, uff, K=K, xref=xref, pscale=sc.task["pscale"], integrator=integ, stats=True)
    assert (info["status"] & 15 == 0).all()
    return qt, qdt, ua


def _closed(size, integ, batch=B):
    """A sim with the closed loop of feedback_case on its tape, and the cotangents of the proto test's loss."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = feedback_case(size, integ)
    sim = BatchSim(sc, batch=batch)
    qt, qdt, ua = _forward(sim, sc, cs, integ)
    return sim, sc, cs, nsteps, (qt, qdt, ua), (cs["c"] + qt, cs["d"], gu_case(size, integ))


def _bits(a, b, names=NAMES):
    return all(np.array_equal(a[n], b[n]) for n in names)


# ---------------------------------------------------------------- 1. against the proto

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_gradients_meet_the_proto(oracle_lib, size, integ):
    """duff, dK, dxref, dq0, dqd0 to 1e-7 relative against the proto's recursion on the oracle's tape.  The three smallest scenes in
    full, the larger ones rollout 0."""
    sim, sc, cs, nsteps, _, (gq, gqd, gu) = _closed(size, integ)
    out = sim.rollout_vjp_feedback(nsteps, gq, gqd, K=cs["K"], xref=cs["xref"], gu=gu, want=NAMES)
    assert "vjp_feedback" in sim.last_step_kernel()
    sim.close()
    for b in range(B if size in (5, "tree7", "fixed") else 1):
        ref = reference(oracle_lib, size, integ, b)
        errs = tuple(_rel(out[n][b], ref[n]) for n in NAMES)
        print("size %s integ %d b %d: duff %.3e dK %.3e dxref %.3e dq0 %.3e dqd0 %.3e (relative to the proto)" % ((size, integ, b) + errs))
        assert max(errs) <= 1e-7, (size, integ, b, errs)
        assert all(np.abs(out[n][b]).max() > 0 for n in NAMES)


# ---------------------------------------------------------------- 2. against rmx_rollout_linearize of the same tape

@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_gradients_meet_the_costate_recursion_on_the_linearisation(size):
    """BDF1.  With A_k, B_k assembled from XA, XB, XU as diff.linearize does and Kx_k = dU_k/dx_{k-1} ([nr][2nr]):
        lam_{k-1} = g_{k-1} + (A_k + B_k Kx_k)' lam_k + Kx_k' gu_k ;  duff_k = B_k' lam_k + gu_k        (g_0 = 0, lam_N = g_N)
    and dq0, dqd0 = lam_0, dxref_{k-1} = -Kx_k' duff_k, dK_k = dx_{k-1} duff_k'.  The same 1e-7."""
    sim, sc, cs, nsteps, (qt, qdt, ua), (gq, gqd, gu) = _closed(size, 1)
    out = sim.rollout_vjp_feedback(nsteps, gq, gqd, K=cs["K"], xref=cs["xref"], gu=gu, want=NAMES)
    XA, XB, XU = sim.rollout_linearize(nsteps)
    sim.close()
    nr, h = sc.nr, sc.h
    eye = np.eye(nr)
    worst = dict.fromkeys(NAMES, 0.0)
    for b in range(B):
        S = XA[b] + XB[b]
        A = np.concatenate([np.concatenate([S, h * XB[b]], axis=2), np.concatenate([(S - eye) / h, XB[b]], axis=2)], axis=1)
        Bm = np.concatenate([XU[b], XU[b] / h], axis=1)
        g = np.concatenate([gq[b], gqd[b]], axis=1)
        x = np.concatenate([np.concatenate([cs["q0"][b], cs["qd0"][b]])[None], np.concatenate([qt[b], qdt[b]], axis=1)[:-1]])
        dx = x - cs["xref"]
        lam = g[nsteps - 1].copy()
        ref = dict(duff=np.empty((nsteps, nr)), dK=np.empty((nsteps, 2 * nr, nr)), dxref=np.empty((nsteps, 2 * nr)))
        for k in range(nsteps, 0, -1):
            Kx = cs["K"][k - 1].T
            ref["duff"][k - 1] = Bm[k - 1].T @ lam + gu[b, k - 1]
            ref["dxref"][k - 1] = -Kx.T @ ref["duff"][k - 1]
            ref["dK"][k - 1] = np.outer(dx[k - 1], ref["duff"][k - 1])
            lam = (g[k - 2] if k >= 2 else 0.0) + (A[k - 1] + Bm[k - 1] @ Kx).T @ lam + Kx.T @ gu[b, k - 1]
        ref["dq0"], ref["dqd0"] = lam[:nr], lam[nr:]
        for n in NAMES:
            worst[n] = max(worst[n], _rel(out[n][b], ref[n]))
    print("size %s: against the linearisation, worst over the batch: %s" % (size, ", ".join("%s %.3e" % (n, worst[n]) for n in NAMES)))
    assert max(worst.values()) <= 1e-7, worst


# ---------------------------------------------------------------- 3. the testGrad identity on the GPU's own closed loop

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, "fixed", 16])
def test_gradients_meet_the_testgrad_identity(size, integ):
    """Central differences (eps = 1e-5, 3 random directions per group, one batch for all perturbed rollouts, one table per rollout)
    of L = sum_k c_k.q_k + d_k.qdot_k + |q_k|^2/2 + e_k.uapp_k on rmx_rollout_tape_feedback's own record, along directions in uff, K,
    xref, q0, qdot0 and in all five jointly, against direction . gradient of rollout 0.  Tolerance: rtol 2e-5, atol 1e-6 max|ana|, the
    floor of tests/test_gpu_rollout_vjp.py::test_gradients_meet_the_testgrad_identity."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = feedback_case(size, integ)
    e = gu_case(size, integ)[0]
    c, d = cs["c"][0], cs["d"][0]
    base = dict(uff=cs["u"][0], K=cs["K"], xref=cs["xref"], q0=cs["q0"][0], qd0=cs["qd0"][0])

    def run(sim, p):
        sim.set_state(p["q0"], p["qd0"])
        qt, qdt, ua, info = sim.rollout_feedback(nsteps, sc.h, p["uff"], K=p["K"], xref=p["xref"], pscale=sc.task["pscale"], integrator=integ,
                                                 stats=True)
        assert (info["status"] & 15 == 0).all()
        return qt, qdt, ua

    one = BatchSim(sc, batch=1)
    qt, qdt, ua = run(one, {k: v[None] for k, v in base.items()})
    out = one.rollout_vjp_feedback(nsteps, c[None] + qt, d[None], K=base["K"][None], xref=base["xref"][None], gu=e[None], want=NAMES)
    one.close()
    grads = dict(uff=out["duff"][0], K=out["dK"][0], xref=out["dxref"][0], q0=out["dq0"][0], qd0=out["dqd0"][0])
    nd, eps = 3, 1e-5
    rng = np.random.default_rng(29)
    groups = [(k,) for k in grads] + [tuple(grads)]
    dirs, pert = [], {k: [] for k in grads}
    for g in groups:
        for _ in range(nd):
            dv = {k: (rng.standard_normal(grads[k].shape) if k in g else np.zeros(grads[k].shape)) for k in grads}
            dirs.append(dv)
            for sgn in (1.0, -1.0):
                for k in grads:
                    pert[k].append(base[k] + sgn * eps * dv[k])
    nb = len(pert["uff"])
    fd = BatchSim(sc, batch=nb)
    qt, qdt, ua = run(fd, {k: np.array(v) for k, v in pert.items()})
    fd.close()
    L = np.array([(c * qt[i]).sum() + (d * qdt[i]).sum() + 0.5 * (qt[i] ** 2).sum() + (e * ua[i]).sum() for i in range(nb)])
    num = (L[0::2] - L[1::2]) / (2 * eps)
    ana = np.array([sum(float((dv[k] * grads[k]).sum()) for k in grads) for dv in dirs])
    shown = []
    for i, g in enumerate(groups):
        a, err = ana[i * nd:(i + 1) * nd], np.abs(num - ana)[i * nd:(i + 1) * nd]
        shown.append(err.max() / np.abs(a).max())
        assert np.abs(a).max() > 0
        assert (err <= 2e-5 * np.abs(a) + 1e-6 * np.abs(a).max()).all(), (g, num[i * nd:(i + 1) * nd], a, err)
    print("testgrad size %s integ %d: uff %.3e, K %.3e, xref %.3e, q0 %.3e, qdot0 %.3e, jointly %.3e (of max|ana|)" % ((size, integ) + tuple(shown)))


# ---------------------------------------------------------------- 4. without gains

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_without_gains(size, integ):
    """K NULL and gu NULL: rmx_rollout_vjp's bits (the same kernel).  K all zeros: the closed-loop kernel, another arrangement of the
    same sums - 1e-7 relative against rmx_rollout_vjp, the difference printed.  gu alone (K NULL): duff = du + gu to rounding, dq0 and
    dqd0 rmx_rollout_vjp's to the same 1e-7."""
    sim, sc, cs, nsteps, _, (gq, gqd, gu) = _closed(size, integ)
    du, dq0, dqd0 = sim.rollout_vjp(nsteps, gq, gqd)
    vjp_kernel = sim.last_step_kernel()
    none = sim.rollout_vjp_feedback(nsteps, gq, gqd)
    # (the label names the backward kernel of rmx_rollout_vjp's plan, which ran - not the closed-loop kernel)
    assert "vjp_feedback" not in sim.last_step_kernel()
    assert sim.last_step_kernel().startswith("k_adjoint_bwd<" if integ == 1 else "k_rollout_bwd_bdf2")
    assert sorted(none) == ["dq0", "dqd0", "duff"]
    assert np.array_equal(none["duff"], du) and np.array_equal(none["dq0"], dq0) and np.array_equal(none["dqd0"], dqd0)
    only = sim.rollout_vjp_feedback(nsteps, gq, gqd, want=("dq0",))       # (duff not asked for: the same bits still)
    assert np.array_equal(only["dq0"], dq0) and np.array_equal(only["dqd0"], dqd0)
    xr = sim.rollout_vjp_feedback(nsteps, gq, gqd, xref=cs["xref"])        # (a reference without gains is not read)
    assert np.array_equal(xr["duff"], du)
    zero = sim.rollout_vjp_feedback(nsteps, gq, gqd, K=np.zeros_like(cs["K"]), xref=cs["xref"], want=NAMES)
    assert "vjp_feedback" in sim.last_step_kernel() and sim.last_step_kernel() != vjp_kernel
    errs = (_rel(zero["duff"], du), _rel(zero["dq0"], dq0), _rel(zero["dqd0"], dqd0))
    print("size %s integ %d, K zeros against rmx_rollout_vjp: duff %.3e dq0 %.3e dqd0 %.3e" % ((size, integ) + errs))
    assert max(errs) <= 1e-7 and not zero["dxref"].any() and zero["dK"].any()
    g = sim.rollout_vjp_feedback(nsteps, gq, gqd, gu=gu)
    errs = (_rel(g["duff"], du + gu), _rel(g["dq0"], dq0), _rel(g["dqd0"], dqd0))
    print("size %s integ %d, gu alone: duff against du + gu %.3e, dq0 %.3e dqd0 %.3e" % ((size, integ) + errs))
    assert max(errs) <= 1e-7
    sim.close()


# ---------------------------------------------------------------- 5. exact structure

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, "tree7", "fixed", 16, 32, 40])
def test_structure_bit_for_bit(size, integ):
    from redmax_amd import BatchSim
    sim, sc, cs, nsteps, (qt, qdt, ua), (gq, gqd, gu) = _closed(size, integ)
    rng = np.random.default_rng(5)
    tu = rng.standard_normal((B, 2, nsteps, sc.nr))

    def readers():
        return sim.rollout_vjp(nsteps, gq, gqd) + sim.rollout_linearize(nsteps) + sim.rollout_jvp(nsteps, tu=tu)

    before = readers()
    state = sim.get_state()
    kw = dict(K=cs["K"], xref=cs["xref"], gu=gu)
    base = sim.rollout_vjp_feedback(nsteps, gq, gqd, want=NAMES, **kw)
    # a repeated call; the other readers of the tape and the state before and after
    assert _bits(sim.rollout_vjp_feedback(nsteps, gq, gqd, want=NAMES, **kw), base)
    after = readers()
    assert len(before) == 8 and all(np.array_equal(a, b) for a, b in zip(before, after))
    assert all(np.array_equal(a, b) for a, b in zip(sim.get_state(), state))
    # every output alone and in pairs: the same bits whichever others are NULL
    for want in (("duff",), ("dK",), ("dxref",), ("dq0",), ("duff", "dxref"), ("dK", "dq0")):
        part = sim.rollout_vjp_feedback(nsteps, gq, gqd, want=want, **kw)
        assert _bits(part, base, names=tuple(part)), want
    # shared tables against the same tables repeated per rollout
    Kr, xr = np.repeat(cs["K"][None], B, axis=0), np.repeat(cs["xref"][None], B, axis=0)
    assert _bits(sim.rollout_vjp_feedback(nsteps, gq, gqd, K=Kr, xref=xr, gu=gu, want=NAMES), base)
    # a NULL reference is a table of zeros
    z = sim.rollout_vjp_feedback(nsteps, gq, gqd, K=cs["K"], xref=np.zeros_like(cs["xref"]), gu=gu, want=NAMES)
    n = sim.rollout_vjp_feedback(nsteps, gq, gqd, K=cs["K"], xref=None, gu=gu, want=NAMES)
    assert _bits(z, n) and not np.array_equal(z["dK"], base["dK"]) and np.array_equal(z["duff"], base["duff"])
    # device pointers: the host form's bits, shared and per rollout; inputs untouched
    for K, xref, per in ((cs["K"], cs["xref"], False), (Kr, xr, True)):
        din = [_DevArray(a) for a in (gq, gqd, gu, K, xref)]
        dout = [_DevArray(np.full(base[n_].shape, np.nan)) for n_ in NAMES]
        sim.rollout_vjp_feedback_device(nsteps, din[0].ptr.value, din[1].ptr.value, din[2].ptr.value, din[3].ptr.value, din[4].ptr.value,
                                        per_rollout=per, **{n_ + "_ptr": a.ptr.value for n_, a in zip(NAMES, dout)})
        assert all(np.array_equal(a.get(), base[n_]) for n_, a in zip(NAMES, dout))
        assert all(np.array_equal(a.get(), a.host) for a in din)
        for a in din + dout:
            a.free()
    # truly different tables per rollout, and a permuted batch: permuted rows
    Kb = cs["K"][None] * (1.0 + 0.3 * rng.standard_normal((B, 1, 1, 1)))
    xb = cs["xref"][None] + 0.01 * rng.standard_normal((B,) + cs["xref"].shape)
    qt2 = _forward(sim, sc, cs, integ, K=Kb, xref=xb)[0]
    own = sim.rollout_vjp_feedback(nsteps, cs["c"] + qt2, gqd, K=Kb, xref=xb, gu=gu, want=NAMES)
    assert not np.array_equal(own["duff"][1], base["duff"][1])
    perm = np.array([2, 0, 1])
    pcs = {k: cs[k][perm] for k in ("q0", "qd0", "u")}
    qtp = _forward(sim, sc, pcs, integ, K=Kb[perm], xref=xb[perm])[0]
    assert np.array_equal(qtp, qt2[perm])
    pout = sim.rollout_vjp_feedback(nsteps, cs["c"][perm] + qtp, gqd[perm], K=Kb[perm], xref=xb[perm], gu=gu[perm], want=NAMES)
    assert all(np.array_equal(pout[n_], own[n_][perm]) for n_ in NAMES)
    sim.close()
    # rollout 1 of the batch is a batch-of-one call
    one = BatchSim(sc, batch=1)
    q1 = _forward(one, sc, cs, integ, sel=slice(1, 2), K=Kb[1:2], xref=xb[1:2])[0]
    o1 = one.rollout_vjp_feedback(nsteps, cs["c"][1:2] + q1, gqd[1:2], K=Kb[1:2], xref=xb[1:2], gu=gu[1:2], want=NAMES)
    one.close()
    assert all(np.array_equal(o1[n_][0], own[n_][1]) for n_ in NAMES)


@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("nsteps", [1, 2])
def test_one_and_two_steps(oracle_lib, nsteps, integ):
    """Size 5 with 1 and 2 steps - under BDF2 an empty loop and a single pass - against the proto, 1e-7."""
    import proto_rollout_vjp_feedback as protob
    from redmax_amd import BatchSim
    sc, cs, _ = feedback_case(5, integ)
    K, xref, gu = cs["K"][:nsteps], cs["xref"][:nsteps], gu_case(5, integ)[:, :nsteps]
    short = {k: (v[:, :nsteps] if k in ("u", "c", "d") else v) for k, v in cs.items()}
    sim = BatchSim(sc, batch=B)
    qt, qdt, ua = _forward(sim, sc, short, integ, K=K, xref=xref)
    out = sim.rollout_vjp_feedback(nsteps, short["c"] + qt, short["d"], K=K, xref=xref, gu=gu, want=NAMES)
    sim.close()
    ref = protob.reference(oracle_lib, sc, integ, cs["q0"][0], cs["qd0"][0], short["u"][0], K, xref, sc.h, sc.task["pscale"], short["c"][0],
                           short["d"][0], gu[0])
    errs = tuple(_rel(out[n][0], ref[n]) for n in NAMES)
    print("nsteps %d integ %d: duff %.3e dK %.3e dxref %.3e dq0 %.3e dqd0 %.3e (relative to the proto)" % ((nsteps, integ) + errs))
    assert max(errs) <= 1e-7, errs


# ---------------------------------------------------------------- 6. refusals

@pytest.mark.gpu
def test_refusals_leave_the_tape_alone():
    from redmax_amd import BatchSim, _abi
    sc, cs, nsteps = feedback_case(5, 1)
    gu = gu_case(5, 1)
    fresh = BatchSim(sc, batch=B)
    z = np.zeros((B, nsteps, sc.nr))
    with pytest.raises(_abi.RedMaxHipError, match="rmx_rollout_vjp_feedback: no tape"):
        fresh.rollout_vjp_feedback(nsteps, z, z, K=cs["K"])
    fresh.close()
    sim, sc, cs, nsteps, _, (gq, gqd, gu) = _closed(5, 1)
    kw = dict(K=cs["K"], xref=cs["xref"], gu=gu)
    base = sim.rollout_vjp_feedback(nsteps, gq, gqd, want=NAMES, **kw)
    with pytest.raises(_abi.RedMaxHipError, match="nsteps differs from the tape's"):
        sim.rollout_vjp_feedback(nsteps - 1, gq[:, 1:], gqd[:, 1:], K=cs["K"][1:], xref=cs["xref"][1:])
    with pytest.raises(_abi.RedMaxHipError, match="no gains"):
        sim.rollout_vjp_feedback(nsteps, gq, gqd, want=("duff", "dK"))
    with pytest.raises(_abi.RedMaxHipError, match="no gains"):
        sim.rollout_vjp_feedback(nsteps, gq, gqd, gu=gu, want=("dxref",))
    d = _DevArray(gq)
    L, bt = sim._L, sim._batch
    fb = _abi.Feedback(None, None, None, 0)
    fg = _abi.FeedbackGrads(d.ptr.value, None, None, None, None)
    vp = C.c_void_p

    def call(batch, fbp, a, b, outp):
        _abi.check(L.rmx_rollout_vjp_feedback_device(batch, nsteps, fbp, vp(a), vp(b), None, outp), "rmx_rollout_vjp_feedback_device")

    for args in ((None, C.byref(fb), d.ptr.value, d.ptr.value, C.byref(fg)), (bt, None, d.ptr.value, d.ptr.value, C.byref(fg)),
                 (bt, C.byref(fb), None, d.ptr.value, C.byref(fg)), (bt, C.byref(fb), d.ptr.value, None, C.byref(fg)),
                 (bt, C.byref(fb), d.ptr.value, d.ptr.value, None)):
        with pytest.raises(_abi.RedMaxHipError, match="rmx_rollout_vjp_feedback: null argument"):
            call(*args)
    with pytest.raises(_abi.RedMaxHipError, match="all outputs are null"):
        call(bt, C.byref(fb), d.ptr.value, d.ptr.value, C.byref(_abi.FeedbackGrads(None, None, None, None, None)))
    with pytest.raises(_abi.RedMaxHipError, match="dq0 and dqd0 must be given together"):
        call(bt, C.byref(fb), d.ptr.value, d.ptr.value, C.byref(_abi.FeedbackGrads(d.ptr.value, None, None, d.ptr.value, None)))
    fb.per_rollout = 2
    with pytest.raises(_abi.RedMaxHipError, match="per_rollout must be 0 or 1"):
        call(bt, C.byref(fb), d.ptr.value, d.ptr.value, C.byref(fg))
    d.free()
    for bad in (dict(gq=gq[:, :-1]), dict(gu=gu[:, :, :-1]), dict(K=cs["K"][:, :-1]), dict(xref=np.repeat(cs["xref"][None], B, axis=0)),
                dict(want=("duff", "duff")), dict(want=("du",))):
        with pytest.raises(ValueError, match="rollout_vjp_feedback: .*(shape|both|want)"):
            sim.rollout_vjp_feedback(nsteps, **dict(dict(gq=gq, gqd=gqd, **kw), **bad))
    # the refused calls left the tape usable: the same bits
    assert _bits(sim.rollout_vjp_feedback(nsteps, gq, gqd, want=NAMES, **kw), base)
    sim.close()


# ---------------------------------------------------------------- 7. torch

def _torch_case(integ=1, Bt=2, nsteps=3):
    import torch
    sc, cs, _ = feedback_case(5, integ)
    dev = torch.device("cuda", 0)
    np_ = dict(q0=cs["q0"][:Bt], qd0=cs["qd0"][:Bt], u=cs["u"][:Bt, :nsteps], K=cs["K"][:nsteps], xref=cs["xref"][:nsteps],
               c=cs["c"][:Bt, :nsteps], d=cs["d"][:Bt, :nsteps], e=gu_case(5, integ)[:Bt, :nsteps])
    return sc, np_, {k: torch.tensor(v, dtype=torch.float64, device=dev) for k, v in np_.items()}


def _torch_loss(t, qt, qdt, ua):
    return (t["c"] * qt).sum() + (t["d"] * qdt).sum() + 0.5 * (qt ** 2).sum() + (t["e"] * ua).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
def test_torch_backward_is_the_ctypes_call(integ):
    """Backward of diff.rollout_closed_loop is rmx_rollout_vjp_feedback with the cotangent of uapp as gu: the ctypes call's bits for
    per-rollout tables; for shared tables dxref is its rows summed and dK - one einsum of duff with the states - equals the
    per-rollout rows summed to the rounding of that sum."""
    import torch
    from redmax_amd import BatchSim, diff
    Bt, nsteps = 2, 3
    sc, n, t = _torch_case(integ, Bt, nsteps)
    ps = sc.task["pscale"]
    ref = BatchSim(sc, batch=Bt)
    ref.set_state(n["q0"], n["qd0"])
    qt, qdt, ua = ref.rollout_feedback(nsteps, sc.h, n["u"], K=n["K"], xref=n["xref"], pscale=ps, integrator=integ)
    want = ref.rollout_vjp_feedback(nsteps, n["c"] + qt, n["d"], K=n["K"], xref=n["xref"], gu=n["e"], want=NAMES)
    ref.close()
    sim = BatchSim(sc, batch=Bt)
    for per in (False, True):
        leaves = {k: t[k].clone().requires_grad_(True) for k in ("q0", "qd0", "u")}
        K = (t["K"].unsqueeze(0).repeat(Bt, 1, 1, 1) if per else t["K"].clone()).requires_grad_(True)
        xref = (t["xref"].unsqueeze(0).repeat(Bt, 1, 1) if per else t["xref"].clone()).requires_grad_(True)
        out = diff.rollout_closed_loop(sim, leaves["q0"], leaves["qd0"], leaves["u"], K, xref, h=sc.h, pscale=ps, integrator=integ)
        assert all(o.requires_grad for o in out)
        assert all(np.array_equal(o.detach().cpu().numpy(), w) for o, w in zip(out, (qt, qdt, ua)))
        _torch_loss(t, *out).backward()
        got = {k: v.grad.cpu().numpy() for k, v in dict(leaves, K=K, xref=xref).items()}
        assert np.array_equal(got["u"], want["duff"]) and np.array_equal(got["q0"], want["dq0"]) and np.array_equal(got["qd0"], want["dqd0"])
        if per:
            assert np.array_equal(got["K"], want["dK"]) and np.array_equal(got["xref"], want["dxref"])
        else:
            assert got["K"].shape == n["K"].shape and got["xref"].shape == n["xref"].shape
            err = np.abs(got["K"] - want["dK"].sum(axis=0)).max()
            print("integ %d, shared K: max |einsum - rows summed| = %.3e (max |dK| %.3e)" % (integ, err, np.abs(got["K"]).max()))
            # (Bt products summed in some order, fused or not: Bt eps sum_b |row_b| per entry, doubled)
            assert (np.abs(got["K"] - want["dK"].sum(axis=0)) <= 2 * Bt * np.finfo(float).eps * np.abs(want["dK"]).sum(axis=0)).all()
            assert (np.abs(got["xref"] - want["dxref"].sum(axis=0)) <= 2 * Bt * np.finfo(float).eps * np.abs(want["dxref"]).sum(axis=0)).all()
    # a loss on uapp alone, no reference, gains that do not require grad
    u = t["u"].clone().requires_grad_(True)
    out = diff.rollout_closed_loop(sim, t["q0"], t["qd0"], u, t["K"], None, h=sc.h, pscale=ps, integrator=integ)
    out[2].sum().backward()
    assert torch.isfinite(u.grad).all() and u.grad.abs().sum() > 0
    # the tape-replaced check and its words are rollout's
    u1 = t["u"].clone().requires_grad_(True)
    o1 = diff.rollout_closed_loop(sim, t["q0"], t["qd0"], u1, t["K"], t["xref"], h=sc.h, pscale=ps, integrator=integ)
    diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"], t["K"], t["xref"], h=sc.h, pscale=ps, integrator=integ)
    with pytest.raises(RuntimeError, match="the tape of this rollout has been replaced"):
        o1[0].sum().backward()
    # argument checks and words are rollout_feedback's
    with pytest.raises(ValueError, match="rollout: K must have shape"):
        diff.rollout_closed_loop(sim, t["q0"], t["qd0"], t["u"], t["K"].transpose(1, 2), h=sc.h)
    with pytest.raises(ValueError, match="rollout: q0 must be float64"):
        diff.rollout_closed_loop(sim, t["q0"].float(), t["qd0"], t["u"], t["K"], h=sc.h)
    with pytest.raises(ValueError, match="integrator"):
        diff.rollout_closed_loop(sim, t["q0"], t["qd0"], t["u"], t["K"], integrator=3)
    sim.close()


@pytest.mark.gpu
def test_torch_gradcheck_in_all_five_inputs():
    """torch.autograd.gradcheck on diff.rollout_closed_loop at size 5 in q0, qdot0, uff, K and xref, with the settings of
    tests/test_gpu_rollout_vjp.py::test_torch_backward_is_the_vjp_and_gradcheck_passes: gradcheck's defaults.  gradcheck keeps the
    graphs of some of its calls alive while it makes further ones and a sim holds ONE tape, so a call takes a sim whose last
    graph is alive no more (a weak reference to the node the outputs hang on), or a new one: a handful of sims for the few hundred
    calls."""
    import weakref

    import torch
    from redmax_amd import BatchSim, diff
    Bt, nsteps = 2, 3
    sc, n, t = _torch_case(1, Bt, nsteps)
    pool = []      # [sim, a weak reference to the graph node of its last call]

    def f(a, b, c, K, xref):
        slot = next((s_ for s_ in pool if s_[1]() is None), None)
        if slot is None:
            slot = [BatchSim(sc, batch=Bt), None]
            pool.append(slot)
        out = diff.rollout_closed_loop(slot[0], a, b, c, K, xref, h=sc.h, pscale=sc.task["pscale"])
        slot[1] = weakref.ref(out[0].grad_fn)
        return out

    assert torch.autograd.gradcheck(f, tuple(t[k].clone().requires_grad_(True) for k in ("q0", "qd0", "u", "K", "xref")))
    print("gradcheck: %d sims" % len(pool))
    assert len(pool) < 32
    for s_ in pool:
        s_[0].close()


@pytest.mark.gpu
def test_gain_tuning_by_gradient_descent():
    """A use of it: ten steps of gradient descent on a shared K with backtracking, for the cost of tracking the reference of
    feedback_case on size 5.  The accepted costs never rise and the last is below the first."""
    import torch
    from redmax_amd import BatchSim, diff
    sc, cs, nsteps = feedback_case(5, 1)
    dev = torch.device("cuda", 0)
    t = {k: torch.tensor(cs[k], dtype=torch.float64, device=dev) for k in ("q0", "qd0", "u", "K", "xref")}
    nr, ps = sc.nr, sc.task["pscale"]
    sim = BatchSim(sc, batch=B)

    def cost(K):
        qt, qdt, ua = diff.rollout_closed_loop(sim, t["q0"], t["qd0"], t["u"], K, t["xref"], h=sc.h, pscale=ps)
        # the state after step k against the reference the NEXT step's feedback reads, and a small price on the applied torque
        return ((qt[:, :-1] - t["xref"][1:, :nr]) ** 2).sum() + 1e-2 * ((qdt[:, :-1] - t["xref"][1:, nr:]) ** 2).sum() + 1e-3 * (ua ** 2).sum()

    K = t["K"].clone()
    costs, step = [], None
    for it in range(10):
        Kv = K.clone().requires_grad_(True)
        c0 = cost(Kv)
        c0.backward()
        g = Kv.grad
        if step is None:
            costs.append(float(c0.detach()))
            step = 0.05 * float(K.abs().max() / g.abs().max())
        for _ in range(20):
            with torch.no_grad():
                c1 = float(cost(K - step * g))
            if c1 < costs[-1]:
                K = K - step * g
                costs.append(c1)
                step *= 2.0
                break
            step *= 0.5
    sim.close()
    print("gain tuning: accepted costs %s" % " ".join("%.6g" % c for c in costs))
    assert len(costs) > 1 and all(b <= a for a, b in zip(costs, costs[1:])) and costs[-1] < costs[0]


# ---------------------------------------------------------------- 8. the MEX command

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
def test_mex_command_equals_the_python_call(gw, integ):  # noqa: F811
    """'rollout_vjp_feedback' through the gateway (stub), over two shards: dK comes back nr x 2nr x nsteps x B, dxref 2nr x nsteps x B."""
    sim, sc, cs, nsteps, _, (gq, gqd, gu) = _closed(5, integ)
    ps = float(sc.task["pscale"])
    rng = np.random.default_rng(13)
    Kb = cs["K"][None] * (1.0 + 0.3 * rng.standard_normal((B, 1, 1, 1)))
    xb = cs["xref"][None] + 0.01 * rng.standard_normal((B,) + cs["xref"].shape)
    shared = sim.rollout_vjp_feedback(nsteps, gq, gqd, K=cs["K"], xref=cs["xref"], gu=gu, want=NAMES)
    qt2 = _forward(sim, sc, cs, integ, K=Kb, xref=xb)[0]
    own = sim.rollout_vjp_feedback(nsteps, cs["c"] + qt2, gqd, K=Kb, xref=xb, gu=gu, want=NAMES)
    nog = sim.rollout_vjp_feedback(nsteps, cs["c"] + qt2, gqd)
    sim.close()
    h = gw.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    uffm, gqdm, gum = cs["u"].transpose(2, 1, 0), gqd.transpose(2, 1, 0), gu.transpose(2, 1, 0)
    empty = np.zeros((0, 0))
    with pytest.raises(MexError, match="no tape"):
        gw.call(1, "rollout_vjp_feedback", h, float(nsteps), gq.transpose(2, 1, 0), gqdm, empty, empty)
    for K, xref, g, want in ((cs["K"].transpose(2, 1, 0), cs["xref"].T, gq, shared), (Kb.transpose(3, 2, 1, 0), xb.transpose(2, 1, 0), cs["c"] + qt2, own)):
        gw.call(0, "set", h, cs["q0"].T, cs["qd0"].T)
        gw.call(1, "rollout_feedback", h, sc.h, float(nsteps), ps, uffm, K, xref, float(integ))
        duff, dK, dxref, dq0, dqd0 = gw.call(5, "rollout_vjp_feedback", h, float(nsteps), g.transpose(2, 1, 0), gqdm, K, xref, gum)
        assert dK.shape == (sc.nr, 2 * sc.nr, nsteps, B) and dxref.shape == (2 * sc.nr, nsteps, B)
        assert np.array_equal(duff.transpose(2, 1, 0), want["duff"]) and np.array_equal(dK.transpose(3, 2, 1, 0), want["dK"])
        assert np.array_equal(dxref.transpose(2, 1, 0), want["dxref"])
        assert np.array_equal(dq0.T, want["dq0"]) and np.array_equal(dqd0.T, want["dqd0"])
    # without gains (on the tape of the per-rollout tables): rmx_rollout_vjp's outputs, dK and dxref empty
    duff, dK, dxref, dq0, dqd0 = gw.call(5, "rollout_vjp_feedback", h, float(nsteps), (cs["c"] + qt2).transpose(2, 1, 0), gqdm, empty, empty)
    assert np.array_equal(duff.transpose(2, 1, 0), nog["duff"]) and np.array_equal(dq0.T, nog["dq0"]) and dK.size == 0 and dxref.size == 0
    with pytest.raises(MexError, match="nr x nsteps x batch"):
        gw.call(1, "rollout_vjp_feedback", h, float(nsteps), gq.transpose(2, 1, 0)[:, :-1], gqdm, empty, empty)
    with pytest.raises(MexError, match="K and xref alike"):
        gw.call(1, "rollout_vjp_feedback", h, float(nsteps), gq.transpose(2, 1, 0), gqdm, Kb.transpose(3, 2, 1, 0), cs["xref"].T)
    with pytest.raises(MexError, match="nsteps differs"):
        gw.call(1, "rollout_vjp_feedback", h, float(nsteps - 1), gq.transpose(2, 1, 0)[:, 1:], gqdm[:, 1:], empty, empty)
    gw.call(0, "destroy", h)
