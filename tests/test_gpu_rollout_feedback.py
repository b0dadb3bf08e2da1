"""rmx_rollout_tape_feedback: the taped rollout under time-varying affine state feedback, formed on the device inside the one launch.

The checks, in the order of the sections below, BDF1 and BDF2 throughout:
  1. without gains (K NULL, K all zeros) the applied torques are uff bit for bit and the rollout is rmx_rollout_tape's under u = uff;
  2. with gains the record meets the closed loop of tests/proto_rollout_feedback.py (numpy on the oracle, pinned on the CPU by
     tests/test_rollout_feedback_proto.py, which also shows that the oracle's Newton iteration converges for these inputs), and uapp is
     uff + K'(x - xref) on the RETURNED rows to the rounding of that dot product;
  3. the tape is the open-loop tape under uapp: a replay with uff = uapp and no gains returns the same bits, and rmx_rollout_vjp,
     _linearize and _jvp return the same bits on both tapes; the vjp meets the proto's recursion on the oracle's tape under uapp;
  4. exact structure: shared tables against one table per rollout, a permuted batch, device pointers, a NULL reference;
  5. refusals, what a refused call leaves alone, stepping on from the state the call left, the torch side;
  6. the MEX command.

Sizes by the path each takes (tests/test_rollout_feedback_proto.py feedback_case): 5-link chain and tree7 NP 8 (chain and branching),
"fixed" NP 8 with two nodes that have no DOF (lanes with idx < 0 inside the tree), 16-link chain NP 16, 32-link chain M, D on the
matrix cores, 40-link chain the 64-lane path (three chunks of 16 columns, the last one partly past the tree).
"""
import numpy as np
import pytest

import proto_rollout_vjp as proto1
import proto_rollout_vjp_bdf2 as proto2
from test_gpu_adjoint_controls import _DevArray, _rel
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)
from test_rollout_feedback_proto import B, closed_loop, feedback_case

SIZES = [5, "tree7", "fixed", 16, 32, 40]
EPS = np.finfo(float).eps
_ORACLE = {}      # the oracle's open-loop rollouts of section 1, computed once


def _feedback(sim, sc, cs, sel=slice(None), integ=1, K="case", xref="case", uff=None, **kw):
    sim.set_state(cs["q0"][sel], cs["qd0"][sel])
    K = cs["K"] if isinstance(K, str) else K
    xref = cs["xref"] if isinstance(xref, str) else xref
    uff = cs["u"][sel] if uff is None else uff
    return sim.rollout_feedback(uff.shape[1], sc.h, uff, K=K, xref=xref, pscale=sc.task["pscale"], integrator=integ, **kw)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. without gains

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, "tree7", "fixed", 11, 16, 32, 40])
def test_without_gains_it_is_the_taped_rollout(oracle_lib, size, integ):
    """uapp == uff bit for bit, and qtraj, qdtraj, Newton counts, status and the final state are rmx_rollout_tape's under u = uff, bit
    for bit - in every scene but the full 16-link chain.  There rmx_rollout_tape runs the FULL-CHAIN instantiation of the forward
    kernel (with its helper wave under BDF1), whose front has the chain's two model facts as compile-time constants, and the feedback
    call - always the generic kernel - contracts a few products of the front differently.  Measured on MI355X between the two kernels
    over the 5 steps: max |q - q_tape| = 5.6e-16 and max |qd - qd_tape| = 2.3e-14 under BDF1, 1.3e-15 and 1.3e-13 under BDF2 (1 to
    2 ulp of q; qd is a difference of q over h), Newton counts and status equal.  For that scene the record is held to the oracle's
    open-loop rollout instead, 1e-9 relative per step - the bound test_forward_sweep_is_the_controls_call_and_the_oracles_rollout holds
    rmx_rollout_tape's own record to.  The 11-link chain is the 16-lane kernel on a tree that does not fill its slots, where
    rmx_rollout_tape runs the generic instantiation (with the helper wave under BDF1): bit for bit."""
    from redmax_amd import BatchSim
    bits = size != 16
    sc, cs, nsteps = feedback_case(size, integ)
    sim = BatchSim(sc, batch=B)
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, info = sim.rollout_tape(nsteps, sc.h, cs["u"], pscale=sc.task["pscale"], stats=True, integrator=integ)
    tape_kernel = sim.last_step_kernel()
    state = sim.get_state()
    assert (info["status"] & 15 == 0).all()
    for name, K, xref in (("K NULL", None, None), ("K NULL, xref given", None, cs["xref"]), ("K zeros", np.zeros_like(cs["K"]), cs["xref"])):
        q1, qd1, ua, i1 = _feedback(sim, sc, cs, integ=integ, K=K, xref=xref, stats=True)
        assert "feedback" in sim.last_step_kernel() and sim.last_step_kernel() != tape_kernel
        print("size %s integ %d, %s: max |q - q_tape| = %.3e, max |qd - qd_tape| = %.3e, Newton iterations %s against %s"
              % (size, integ, name, np.abs(q1 - qt).max(), np.abs(qd1 - qdt).max(), i1["newton_iters"], info["newton_iters"]))
        assert np.array_equal(ua, cs["u"])
        assert np.array_equal(i1["newton_iters"], info["newton_iters"]) and np.array_equal(i1["status"], info["status"])
        assert np.array_equal(q1[:, -1], sim.get_state()[0]) and np.array_equal(qd1[:, -1], sim.get_state()[1])
        if bits:
            assert np.array_equal(q1, qt) and np.array_equal(qd1, qdt)
            assert _same(sim.get_state(), state)
        else:
            for b in range(B):
                key = ("open loop", size, integ, b)
                if key not in _ORACLE:
                    _ORACLE[key] = (proto1 if integ == 1 else proto2).rollout(oracle_lib, sc, cs["q0"][b], cs["qd0"][b], cs["u"][b], sc.h,
                                                                              sc.task["pscale"])[0]
                for k in range(nsteps):
                    assert _rel(q1[b, k], _ORACLE[key][k]) <= 1e-9, (size, integ, b, k, _rel(q1[b, k], _ORACLE[key][k]))
    sim.close()


# ---------------------------------------------------------------- 2. with gains: against the proto

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_closed_loop_meets_the_proto(oracle_lib, size, integ):
    """qtraj per step to 1e-9 relative against the oracle's closed loop (the bound the open-loop record is held to), uapp element-wise
    to (2nr + 2) eps (|uff| + |K|'|x - xref|) against the formula on the returned rows: 2nr products and 2nr additions in some order,
    the differences x - xref themselves rounded once.  The three smallest scenes in full, the larger ones rollout 0."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = feedback_case(size, integ)
    nr = sc.nr
    sim = BatchSim(sc, batch=B)
    qt, qdt, ua, info = _feedback(sim, sc, cs, integ=integ, stats=True)
    q, qd = sim.get_state()
    sim.close()
    assert (info["status"] & 15 == 0).all()
    assert np.array_equal(qt[:, -1], q) and np.array_equal(qdt[:, -1], qd)
    x = np.concatenate([np.concatenate([cs["q0"], cs["qd0"]], axis=1)[:, None], np.concatenate([qt, qdt], axis=2)[:, :-1]], axis=1)
    dx = x - cs["xref"][None]
    fb = np.einsum("kji,bkj->bki", cs["K"], dx)
    bound = (2 * nr + 2) * EPS * (np.abs(cs["u"]) + np.einsum("kji,bkj->bki", np.abs(cs["K"]), np.abs(dx)))
    err = np.abs(ua - (cs["u"] + fb))
    print("size %s integ %d: |feedback| / |uff| = %.2f; max |uapp - formula| / bound = %.3f"
          % (size, integ, np.linalg.norm(fb) / np.linalg.norm(cs["u"]), (err / bound).max()))
    assert (err <= bound).all()
    assert np.abs(fb).min(axis=2).max() > 0
    for b in range(B if size in (5, "tree7", "fixed") else 1):
        ref = closed_loop(oracle_lib, size, integ, b)
        for k in range(nsteps):
            assert _rel(qt[b, k], ref["qtraj"][k]) <= 1e-9, (size, integ, b, k, _rel(qt[b, k], ref["qtraj"][k]))
        print("size %s integ %d b %d: |qtraj - proto| / |proto| = %.3e, qdtraj %.3e, uapp %.3e"
              % (size, integ, b, _rel(qt[b], ref["qtraj"]), _rel(qdt[b], ref["qdtraj"]), _rel(ua[b], ref["uapp"])))


# ---------------------------------------------------------------- 3. the tape is the open-loop tape under uapp

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_the_tape_is_the_open_loop_tape_under_uapp(oracle_lib, size, integ):
    from redmax_amd import BatchSim
    sc, cs, nsteps = feedback_case(size, integ)
    sim = BatchSim(sc, batch=B)
    rng = np.random.default_rng(5)
    tu = rng.standard_normal((B, 2, nsteps, sc.nr))

    def reads(qt):
        return (sim.rollout_vjp(nsteps, cs["c"] + qt, cs["d"]) + sim.rollout_linearize(nsteps) + sim.rollout_jvp(nsteps, tu=tu))

    qt, qdt, ua, info = _feedback(sim, sc, cs, integ=integ, stats=True)
    assert (info["status"] & 15 == 0).all()
    closed = reads(qt)
    q2, qd2, ua2, i2 = _feedback(sim, sc, cs, integ=integ, K=None, xref=None, uff=ua, stats=True)
    assert np.array_equal(ua2, ua) and np.array_equal(q2, qt) and np.array_equal(qd2, qdt)
    assert np.array_equal(i2["newton_iters"], info["newton_iters"]) and np.array_equal(i2["status"], info["status"])
    replay = reads(q2)
    sim.close()
    assert len(closed) == 8 and _same(closed, replay)
    du, dq0, dqd0 = closed[:3]
    proto = proto1 if integ == 1 else proto2
    for b in range(B if size in (5, "tree7", "fixed") else 1):
        ref = proto.reference(oracle_lib, sc, cs["q0"][b], cs["qd0"][b], ua[b], sc.h, sc.task["pscale"], cs["c"][b], cs["d"][b])
        errs = (_rel(du[b], ref["du"]), _rel(dq0[b], ref["dq0"]), _rel(dqd0[b], ref["dqd0"]))
        print("size %s integ %d b %d: du %.3e dq0 %.3e dqd0 %.3e (relative to the proto under uapp)" % ((size, integ, b) + errs))
        assert max(errs) <= 1e-7, (size, integ, b, errs)


# ---------------------------------------------------------------- 4. exact structure

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, "fixed", 16, 40])
def test_tables_per_rollout_permutation_device_form_and_null_reference(size, integ):
    from redmax_amd import BatchSim
    sc, cs, nsteps = feedback_case(size, integ)
    ps = sc.task["pscale"]
    sim = BatchSim(sc, batch=B)
    base = _feedback(sim, sc, cs, integ=integ, stats=True)
    assert (base[3]["status"] & 15 == 0).all()
    # one table per rollout, the shared tables repeated: the same bits
    rep = _feedback(sim, sc, cs, integ=integ, K=np.repeat(cs["K"][None], B, axis=0), xref=np.repeat(cs["xref"][None], B, axis=0), stats=True)
    assert _same(rep[:3], base[:3]) and np.array_equal(rep[3]["newton_iters"], base[3]["newton_iters"])
    # truly different tables per rollout, and a permuted batch: permuted results
    rng = np.random.default_rng(9)
    Kb = cs["K"][None] * (1.0 + 0.3 * rng.standard_normal((B, 1, 1, 1)))
    xb = cs["xref"][None] + 0.01 * rng.standard_normal((B,) + cs["xref"].shape)
    own = _feedback(sim, sc, cs, integ=integ, K=Kb, xref=xb)
    assert not np.array_equal(own[0][1], base[0][1])
    perm = np.array([2, 0, 1])
    pcs = {k: cs[k][perm] for k in ("q0", "qd0", "u")}
    sim.set_state(pcs["q0"], pcs["qd0"])
    pout = sim.rollout_feedback(nsteps, sc.h, pcs["u"], K=Kb[perm], xref=xb[perm], pscale=ps, integrator=integ)
    assert all(np.array_equal(p, o[perm]) for p, o in zip(pout, own))
    # rollout b of the batch is a batch-of-one call
    one = BatchSim(sc, batch=1)
    one.set_state(cs["q0"][1:2], cs["qd0"][1:2])
    o1 = one.rollout_feedback(nsteps, sc.h, cs["u"][1:2], K=Kb[1:2], xref=xb[1:2], pscale=ps, integrator=integ)
    one.close()
    assert all(np.array_equal(a[0], o[1]) for a, o in zip(o1, own))
    # a NULL reference is a table of zeros
    z = _feedback(sim, sc, cs, integ=integ, xref=np.zeros_like(cs["xref"]))
    n = _feedback(sim, sc, cs, integ=integ, xref=None)
    assert _same(z, n) and not np.array_equal(z[0], base[0])
    # device pointers: the host form's bits, shared and per rollout; inputs untouched
    nan = np.full(base[0].shape, np.nan)
    for K, xref, per, want in ((cs["K"], cs["xref"], False, base), (Kb, xb, True, own)):
        d = [_DevArray(a) for a in (cs["u"], K, xref, nan, nan, nan)]
        sim.set_state(cs["q0"], cs["qd0"])
        info = sim.rollout_feedback_device(nsteps, sc.h, *(a.ptr.value for a in d), per_rollout=per, pscale=ps, stats=True, integrator=integ)
        assert (info["status"] & 15 == 0).all()
        assert all(np.array_equal(a.get(), w) for a, w in zip(d[3:], want))
        assert np.array_equal(d[0].get(), cs["u"]) and np.array_equal(d[1].get(), K) and np.array_equal(d[2].get(), xref)
        # no record, no uapp: the same rollout
        sim.set_state(cs["q0"], cs["qd0"])
        sim.rollout_feedback_device(nsteps, sc.h, d[0].ptr.value, d[1].ptr.value, d[2].ptr.value, None, None, None, per_rollout=per, pscale=ps,
                                    integrator=integ)
        assert np.array_equal(sim.get_state()[0], want[0][:, -1])
        for a in d:
            a.free()
    sim.close()


# ---------------------------------------------------------------- 5. refusals, stepping on, torch

@pytest.mark.gpu
def test_refusals_leave_the_tape_alone():
    from redmax_amd import BatchSim, _abi
    import ctypes as C
    sc, cs, nsteps = feedback_case(5, 1)
    sim = BatchSim(sc, batch=B)
    qt, qdt, ua = _feedback(sim, sc, cs)
    gq, gqd = cs["c"] + qt, cs["d"]
    du = sim.rollout_vjp(nsteps, gq, gqd)[0]
    count = sim.tape_count
    d = _DevArray(cs["u"])
    with pytest.raises(_abi.RedMaxHipError, match="rmx_rollout_tape_feedback: null argument"):
        sim.rollout_feedback_device(nsteps, sc.h, None, None, None, None, None, None)
    with pytest.raises(_abi.RedMaxHipError, match="rmx_rollout_tape_feedback: null argument"):      # (a null struct)
        _abi.check(sim._L.rmx_rollout_tape_feedback_device(sim._batch, None, nsteps, 1, 1.0, None, None, None, None, None), "rmx_rollout_tape_feedback_device")
    with pytest.raises(_abi.RedMaxHipError, match="rmx_rollout_tape: qtraj and qdtraj must be given together"):
        sim.rollout_feedback_device(nsteps, sc.h, d.ptr.value, None, None, d.ptr.value, None, None)
    with pytest.raises(_abi.RedMaxHipError, match="nsteps < 1"):
        sim.rollout_feedback_device(0, sc.h, d.ptr.value, None, None, None, None, None)
    fb = _abi.Feedback(d.ptr.value, None, None, 2)
    opts = sim._tape_opts(sc.h)
    for integ, per, words in ((3, 0, "integrator must be 1 \\(BDF1\\) or 2 \\(BDF2\\)"), (1, 2, "per_rollout must be 0 or 1")):
        fb.per_rollout = per
        with pytest.raises(_abi.RedMaxHipError, match=words):
            _abi.check(sim._L.rmx_rollout_tape_feedback_device(sim._batch, C.byref(opts), nsteps, integ, 1.0, C.byref(fb), None, None, None,
                                                               None), "rmx_rollout_tape_feedback_device")
    d.free()
    with pytest.raises(ValueError, match="integrator"):
        sim.rollout_feedback(nsteps, sc.h, cs["u"], integrator=3)
    for bad in (dict(uff=np.zeros((B, nsteps + 1, sc.nr))), dict(K=cs["K"][:, :-1]), dict(xref=cs["xref"][:-1]),
                dict(K=np.repeat(cs["K"][None], B, axis=0))):
        with pytest.raises(ValueError, match="shape|both"):
            sim.rollout_feedback(nsteps, sc.h, **dict(dict(uff=cs["u"], K=cs["K"], xref=cs["xref"]), **bad))
    # the refused calls left the tape alone
    assert np.array_equal(sim.rollout_vjp(nsteps, gq, gqd)[0], du)
    assert sim.tape_count > count       # (the Python wrappers count every attempt: diff.rollout's guard errs on the safe side)
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["chart", "point forces", "ground", "big"])
def test_models_outside_the_adjoint_path_are_refused_in_rollout_tapes_words(kind):
    from redmax_amd import BatchSim, _abi
    from redmax_amd.scenes import sceneChain, scenesRedMax
    sc = {"chart": lambda: scenesRedMax(7), "point forces": lambda: scenesRedMax(12), "ground": lambda: scenesRedMax(11),
          "big": lambda: sceneChain(100)}[kind]()
    sc.init()
    words = {"chart": "spherical joints", "point forces": "point forces", "ground": "ground contact", "big": "more than 64 nodes"}[kind]
    nsteps, Bs = 2, 2
    u = np.zeros((Bs, nsteps, sc.nr))
    q0, qd0 = sc.getQ()
    sim = BatchSim(sc, batch=Bs)
    sim.set_state(q0[None, :], qd0[None, :])
    with pytest.raises(_abi.RedMaxHipError, match=words) as tape:
        sim.rollout_tape(nsteps, sc.h, u)
    with pytest.raises(_abi.RedMaxHipError, match=words) as fbk:
        sim.rollout_feedback(nsteps, sc.h, u, K=np.zeros((nsteps, 2 * sc.nr, sc.nr)))
    assert str(fbk.value).split(": ", 1)[1] == str(tape.value).split(": ", 1)[1]        # (behind the name of the entry point)
    out = sim.step_bdf1(2, h=sc.h, stats=True)
    sim.close()
    assert (out["status"] & 15 == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
def test_stepping_continues_from_the_state_the_call_left(integ):
    """step_bdf1 after a BDF1 feedback rollout is a step from its final state; step_bdf2 after a BDF2 one continues its history - as
    after the replay of the rollout under uapp without gains."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = feedback_case(5, integ)
    sim, ref = BatchSim(sc, batch=B), BatchSim(sc, batch=B)
    qt, qdt, ua = _feedback(sim, sc, cs, integ=integ)
    step = (lambda s: s.step_bdf1(2, h=sc.h, stats=True)) if integ == 1 else (lambda s: s.step_bdf2(2, h=sc.h, stats=True))
    out = step(sim)
    if integ == 1:
        ref.set_state(qt[:, -1], qdt[:, -1])
    else:
        _feedback(ref, sc, cs, integ=2, K=None, xref=None, uff=ua)
    oref = step(ref)
    assert (out["status"] & 15 == 0).all() and np.array_equal(out["newton_iters"], oref["newton_iters"])
    a, b = sim.get_state(), ref.get_state()
    print("integ %d: max |q - q_ref| after two more steps = %.3e" % (integ, np.abs(a[0] - b[0]).max()))
    assert _same(a, b) and not np.array_equal(a[0], qt[:, -1])
    sim.close()
    ref.close()


@pytest.mark.gpu
def test_torch_side():
    import torch
    from redmax_amd import BatchSim, diff
    sc, cs, nsteps = feedback_case(5, 1)
    dev = torch.device("cuda", 0)
    t = {k: torch.tensor(cs[k], dtype=torch.float64, device=dev) for k in ("q0", "qd0", "u", "K", "xref")}
    ps = sc.task["pscale"]
    sim = BatchSim(sc, batch=B)
    want = _feedback(sim, sc, cs)
    for integ in (1, 2):
        w = _feedback(sim, sc, cs, integ=integ)
        got = diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"], t["K"], t["xref"], h=sc.h, pscale=ps, integrator=integ)
        assert all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(got, w))
        assert not any(g.requires_grad for g in got)
    # one table per rollout, and no gains at all
    Kb, xb = t["K"].unsqueeze(0).repeat(B, 1, 1, 1), t["xref"].unsqueeze(0).repeat(B, 1, 1)
    got = diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"], Kb, xb, h=sc.h, pscale=ps)
    assert all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(got, want))
    none = diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"], h=sc.h, pscale=ps)
    assert torch.equal(none[2], t["u"])
    # the checks and words of rollout
    with pytest.raises(ValueError, match="rollout: q0 must be float64"):
        diff.rollout_feedback(sim, t["q0"].float(), t["qd0"], t["u"], h=sc.h)
    with pytest.raises(ValueError, match="rollout: u must have shape"):
        diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"][:, :, :-1], h=sc.h)
    with pytest.raises(ValueError, match="rollout: K must have shape"):
        diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"], t["K"].transpose(1, 2), h=sc.h)
    with pytest.raises(ValueError, match="rollout: xref must be on"):
        diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"], t["K"], t["xref"].cpu(), h=sc.h)
    with pytest.raises(ValueError, match="both"):
        diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"], Kb, t["xref"], h=sc.h)
    with pytest.raises(ValueError, match="integrator"):
        diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"], integrator=3)
    # a feedback rollout replaces the tape of a differentiable rollout
    u1 = t["u"].clone().requires_grad_(True)
    qt1, _ = diff.rollout(sim, t["q0"], t["qd0"], u1, h=sc.h, pscale=ps)
    diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"], t["K"], t["xref"], h=sc.h, pscale=ps)
    with pytest.raises(RuntimeError, match="the tape of this rollout has been replaced"):
        qt1.sum().backward()
    u2 = t["u"].clone().requires_grad_(True)
    qt2, _ = diff.rollout(sim, t["q0"], t["qd0"], u2, h=sc.h, pscale=ps)
    _feedback(sim, sc, cs)
    with pytest.raises(RuntimeError, match="the tape of this rollout has been replaced"):
        qt2.sum().backward()
    sim.close()


# ---------------------------------------------------------------- 6. the MEX command

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
def test_mex_command_equals_the_python_call(gw, integ):  # noqa: F811
    """'rollout_feedback' through the gateway (stub), over two shards: MATLAB's nr x 2nr x nsteps [x B] column-major K is the ABI's
    [B][nsteps][2nr*nr] with entry j*nr + i, xref 2nr x nsteps [x B], the trajectories nr x nsteps x B."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = feedback_case(5, integ)
    ps = float(sc.task["pscale"])
    rng = np.random.default_rng(13)
    Kb = cs["K"][None] * (1.0 + 0.3 * rng.standard_normal((B, 1, 1, 1)))
    xb = cs["xref"][None] + 0.01 * rng.standard_normal((B,) + cs["xref"].shape)
    sim = BatchSim(sc, batch=B)
    shared = _feedback(sim, sc, cs, integ=integ, stats=True)
    own = _feedback(sim, sc, cs, integ=integ, K=Kb, xref=xb, stats=True)
    nogain = _feedback(sim, sc, cs, integ=integ, K=None, xref=None, stats=True)
    gq, gqd = cs["c"] + nogain[0], cs["d"]
    du = sim.rollout_vjp(nsteps, gq, gqd)[0]
    sim.close()
    h = gw.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    uffm = cs["u"].transpose(2, 1, 0)
    empty = np.zeros((0, 0))
    for K, xref, want in ((cs["K"].transpose(2, 1, 0), cs["xref"].T, shared), (Kb.transpose(3, 2, 1, 0), xb.transpose(2, 1, 0), own),
                          (empty, empty, nogain)):
        gw.call(0, "set", h, cs["q0"].T, cs["qd0"].T)
        qtm, qdtm, uam, st = gw.call(4, "rollout_feedback", h, sc.h, float(nsteps), ps, uffm, K, xref, float(integ))
        assert qtm.shape == (sc.nr, nsteps, B)
        assert all(np.array_equal(m.transpose(2, 1, 0), w) for m, w in zip((qtm, qdtm, uam), want))
        assert np.array_equal(st[:, 0], want[3]["newton_iters"]) and np.array_equal(st[:, 1], want[3]["status"])
    dum = gw.call(1, "rollout_vjp", h, float(nsteps), gq.transpose(2, 1, 0), gqd.transpose(2, 1, 0))
    dum = dum[0] if isinstance(dum, (tuple, list)) else dum
    assert np.array_equal(dum.transpose(2, 1, 0), du)
    with pytest.raises(MexError, match="K must be a real double array"):
        gw.call(1, "rollout_feedback", h, sc.h, float(nsteps), ps, uffm, cs["K"].transpose(2, 1, 0)[:, :-1], cs["xref"].T)
    with pytest.raises(MexError, match="K and xref alike"):
        gw.call(1, "rollout_feedback", h, sc.h, float(nsteps), ps, uffm, Kb.transpose(3, 2, 1, 0), cs["xref"].T)
    with pytest.raises(MexError, match="integrator must be 1"):
        gw.call(1, "rollout_feedback", h, sc.h, float(nsteps), ps, uffm, empty, empty, 3.0)
    with pytest.raises(MexError, match="nr x nsteps x batch"):
        gw.call(1, "rollout_feedback", h, sc.h, float(nsteps), ps, uffm[:, :-1], empty, empty)
    gw.call(0, "destroy", h)
