"""rmx_rollout_lqr: the Riccati sweep of iLQR on the device, read off the BDF1 tape (redmax_amd/csrc/rmx_lqr.h).

The checks, in the order of the sections below:
  1. against the reference: ilqr.backward_pass (float64, CPU) and the device call are both judged against the longdouble recursion
     of tests/proto_lqr_backward.py on IDENTICAL inputs - A, B assembled from rmx_rollout_linearize on the same tape.  Per rollout
     and per quantity (kff, K, expected), e = max |. - ext| / max |ext|, and e_gpu <= 8 e_ref with e_ref floored at 16 eps: two
     correct float64 evaluations of one recursion with different summation orders and another factorisation differ by small
     constant factors in an error that is eps * conditioning for both; three bits allow that and do not allow a lost term;
  2. closing the loop through rmx_rollout_tape_feedback_device; 3. exact structure, bit for bit; 4. a rollout that is not positive
     definite; 5. refusals; 6. ilqr.solve(backward="device").

Scenes: sceneAdjointChain(5) (nr 5, padded to 8), sceneAdjointTree7, sceneAdjointChain(32) (the LDS limit); B = 3, N = 8 (N = 3
for the 32-link chain); states from test_rollout_vjp_proto.case; the cost of test_gpu_ilqr._problem: Q = diag(1 on q, 0.01 on qdot),
R = 0.1 I, mu = 1e-6.

Measured on an MI355X (the worst rollout of each case; cond(Quu) the largest over steps and rollouts).  Every e_ref is below the
floor of 16 eps = 3.6e-15, so the bound is 8 * 16 eps = 2.84e-14 throughout; per-rollout copies of Q give the figures of the shared Q:
    scene   N   quantity   e_ref      e_gpu      cond(Quu)
    5       8   kff        7.29e-16   6.22e-16   6.3
    5       8   K          1.30e-15   9.06e-16   6.3
    5       8   expected   1.98e-16   1.80e-16   6.3
    tree7   8   kff        5.24e-16   4.66e-16   10.9
    tree7   8   K          7.68e-16   5.41e-16   10.9
    tree7   8   expected   3.04e-16   3.04e-16   10.9
    32      3   kff        9.29e-16   1.59e-15   6.4
    32      3   K          1.88e-15   2.85e-15   6.4
    32      3   expected   1.37e-16   3.54e-16   6.4
    5       1   kff        3.78e-16   2.02e-16   5.9
    5       1   K          6.27e-16   6.55e-16   5.9
    5       1   expected   4.69e-16   2.35e-16   5.9
"""
import ctypes as C

import numpy as np
import pytest

import proto_lqr_backward as P
import proto_rollout_linearize as lin
from test_gpu_adjoint_controls import _DevArray, _scene
from test_rollout_vjp_proto import case

B, MU = 3, 1e-6
STEPS = {5: 8, "tree7": 8, 32: 3}
EPS = np.finfo(np.float64).eps
_CACHE = {}


def _setup(size, nsteps=None):
    nsteps = STEPS[size] if nsteps is None else nsteps
    key = (size, nsteps)
    if key not in _CACHE:
        sc = _scene(size, 1)
        _CACHE[key] = (sc, case(sc, 53, nsteps=nsteps, B=B), nsteps)
    return _CACHE[key]


def _tape(sim, sc, cs, sel=slice(None)):
    sim.set_state(cs["q0"][sel], cs["qd0"][sel])
    qt, qdt, info = sim.rollout_tape(cs["u"].shape[1], sc.h, cs["u"][sel], pscale=sc.task["pscale"], stats=True)
    assert (info["status"] & 15 == 0).all()
    return qt, qdt


def _cost(sc, cs, qt, qdt, sel=slice(None)):
    """(lx, lu, Q, R) of test_gpu_ilqr._problem's cost at the nominal (qt, qdt, u)."""
    nr, N = sc.nr, qt.shape[1]
    q0, _ = sc.getQ()
    goal = np.concatenate([q0 - 0.1, np.zeros(nr)])
    Q = np.tile(np.diag([1.0] * nr + [0.01] * nr), (N, 1, 1))
    R = 0.1 * np.eye(nr)
    x = np.concatenate([qt, qdt], axis=-1)
    return np.einsum("kij,bkj->bki", Q, x - goal), np.einsum("ij,bkj->bki", R, cs["u"][sel]), Q, R


def _nominal(size, nsteps=None):
    """One tape per (size, nsteps), its linearisation assembled on the CPU and the cost at it: computed once, left unchanged."""
    key = ("nom", size, nsteps)
    if key not in _CACHE:
        from redmax_amd import BatchSim
        sc, cs, N = _setup(size, nsteps)
        sim = BatchSim(sc, batch=B)
        qt, qdt = _tape(sim, sc, cs)
        XA, XB, XU = sim.rollout_linearize(N)
        sim.close()
        A, Bm = zip(*(lin.assemble_bdf1(XA[b], XB[b], XU[b], sc.h) for b in range(B)))
        _CACHE[key] = dict(qt=qt, qdt=qdt, A=np.array(A), Bm=np.array(Bm), cost=_cost(sc, cs, qt, qdt))
    return _CACHE[key]


# ---------------------------------------------------------------- 1. against the reference

@pytest.mark.gpu
@pytest.mark.parametrize("size,nsteps,per", [(5, None, False), (5, None, True), ("tree7", None, False), (32, None, False), (32, None, True),
                                             (5, 1, False)])
def test_gains_meet_the_extended_recursion_as_closely_as_backward_pass(size, nsteps, per):
    import torch
    from redmax_amd import BatchSim
    from redmax_amd.ilqr import backward_pass
    sc, cs, N = _setup(size, nsteps)
    nom = _nominal(size, nsteps)
    lx, lu, Q, R = nom["cost"]
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    kff, K, expected, notpd = sim.rollout_lqr(N, lx, lu, np.tile(Q, (B, 1, 1, 1)) if per else Q, R, mu=MU)
    sim.close()
    assert kff.shape == (B, N, sc.nr) and K.shape == (B, N, 2 * sc.nr, sc.nr) and expected.shape == (B,) and not notpd.any()
    t = lambda a: torch.tensor(a, dtype=torch.float64)      # noqa: E731
    rk, rK, re = (a.numpy() for a in backward_pass(t(nom["A"]), t(nom["Bm"]), t(lx), t(lu), t(Q), t(R), MU))
    ok = True
    for b in range(B):
        ek, eK, ee, bad, cond = P.backward_pass_ext(nom["A"][b], nom["Bm"][b], lx[b], lu[b], Q, R, MU)
        assert not bad
        for name, ref, gpu, ext in (("kff", rk[b], kff[b], ek), ("K", rK[b], K[b].transpose(0, 2, 1), eK), ("expected", re[b], expected[b], ee)):
            e_ref, e_gpu = P.rel_err(ref, ext), P.rel_err(gpu, ext)
            bound = 8 * max(e_ref, 16 * EPS)
            print("size %s N %d per %d b %d %-8s: e_ref %.3e e_gpu %.3e bound %.3e cond(Quu) %.3e%s"
                  % (size, N, per, b, name, e_ref, e_gpu, bound, cond, "" if e_gpu <= bound else "   <-- over"))
            ok = ok and e_gpu <= bound
    assert ok


# ---------------------------------------------------------------- 2. closing the loop

def _torch_problem():
    from test_gpu_ilqr import _problem
    return _problem()


@pytest.mark.gpu
def test_gains_close_the_loop_through_the_feedback_kernel():
    """alpha = 0: K around the nominal reproduces it bit for bit; alpha = 1: the cost falls on every rollout, and expected > 0."""
    import torch
    from redmax_amd import BatchSim, diff
    sc, cs, t, cost = _torch_problem()
    N, ps = t["u"].shape[1], sc.task["pscale"]
    sim = BatchSim(sc, batch=B)
    qt, qdt, ubar = diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"], h=sc.h, pscale=ps)
    xbar = torch.cat([qt, qdt], dim=-1)
    J0 = cost.value(xbar, ubar)
    lx, lu = cost.gradients(xbar, ubar)
    kff, K, expected, notpd = diff.lqr_backward(sim, lx, lu, cost.Q, cost.R, MU)
    assert K.shape == (B, N, 2 * sc.nr, sc.nr) and not notpd.any() and (expected > 0).all()
    xref = torch.cat([torch.cat([t["q0"], t["qd0"]], dim=-1).unsqueeze(1), xbar[:, :-1]], dim=1).contiguous()
    q1, qd1, u1 = diff.rollout_feedback(sim, t["q0"], t["qd0"], ubar, K, xref, h=sc.h, pscale=ps)
    assert torch.equal(q1, qt) and torch.equal(qd1, qdt) and torch.equal(u1, ubar)
    q2, qd2, u2 = diff.rollout_feedback(sim, t["q0"], t["qd0"], ubar + kff, K, xref, h=sc.h, pscale=ps)
    J1 = cost.value(torch.cat([q2, qd2], dim=-1), u2)
    print("J before %s\nJ after the full step %s\nexpected decrease %s" % (J0.cpu().numpy(), J1.cpu().numpy(), expected.cpu().numpy()))
    assert (J1 < J0).all()
    sim.close()


# ---------------------------------------------------------------- 3. exact structure

def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, 32])
def test_exact_structure(size):
    from redmax_amd import BatchSim
    sc, cs, N = _setup(size)
    nom = _nominal(size)
    lx, lu, Q, R = nom["cost"]
    rng = np.random.default_rng(7)
    gq, gqd = rng.standard_normal((B, N, sc.nr)), rng.standard_normal((B, N, sc.nr))
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    vjp0, lin0 = sim.rollout_vjp(N, gq, gqd), sim.rollout_linearize(N)
    ref = sim.rollout_lqr(N, lx, lu, Q, R, mu=MU)
    assert _same(ref, sim.rollout_lqr(N, lx, lu, Q, R, mu=MU))                                         # repeat calls
    assert _same(vjp0, sim.rollout_vjp(N, gq, gqd)) and _same(lin0, sim.rollout_linearize(N))        # the tape is left alone
    assert _same(ref, sim.rollout_lqr(N, lx, lu, np.tile(Q, (B, 1, 1, 1)), R, mu=MU))                  # shared Q against copies
    assert _same(ref, sim.rollout_lqr(N, lx, lu, Q, R, mu=123.0, mu_b=np.full(B, MU)))                 # mu against a constant mu_b
    mub = np.array([MU, 1e-3, 0.5])
    mixed = sim.rollout_lqr(N, lx, lu, Q, R, mu_b=mub)                                                 # differing mu_b against separate calls
    for b in range(B):
        one = sim.rollout_lqr(N, lx, lu, Q, R, mu=float(mub[b]))
        assert all(np.array_equal(m[b], o[b]) for m, o in zip(mixed, one)), b
    assert not np.array_equal(mixed[0][1], ref[0][1])
    # expected and status NULL, and the device form against the host form
    d = {k: _DevArray(v) for k, v in (("lx", lx), ("lu", lu), ("Q", Q), ("R", R), ("kff", np.zeros_like(ref[0])), ("K", np.zeros_like(ref[1])),
                                      ("exp", np.zeros(B)), ("kff2", np.zeros_like(ref[0])), ("K2", np.zeros_like(ref[1])))}
    st = _DevArray(np.zeros(B))      # (room for B int32 words)
    sim.rollout_lqr_device(N, d["lx"].ptr.value, d["lu"].ptr.value, d["Q"].ptr.value, d["R"].ptr.value, d["kff"].ptr.value, d["K"].ptr.value,
                           d["exp"].ptr.value, st.ptr.value, mu=MU)
    sim.rollout_lqr_device(N, d["lx"].ptr.value, d["lu"].ptr.value, d["Q"].ptr.value, d["R"].ptr.value, d["kff2"].ptr.value, d["K2"].ptr.value, mu=MU)
    assert np.array_equal(d["kff"].get(), ref[0]) and np.array_equal(d["K"].get(), ref[1]) and np.array_equal(d["exp"].get(), ref[2])
    assert not st.get().view(np.int32)[:B].any()
    assert np.array_equal(d["kff2"].get(), ref[0]) and np.array_equal(d["K2"].get(), ref[1])
    assert np.array_equal(d["lx"].get(), lx) and np.array_equal(d["Q"].get(), Q)
    for a in list(d.values()) + [st]:
        a.free()
    assert _same(vjp0, sim.rollout_vjp(N, gq, gqd))
    sim.close()
    # a permuted batch, and B = 1 against B = 3
    perm = np.array([2, 0, 1])
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs, perm)
    got = sim.rollout_lqr(N, lx[perm], lu[perm], Q, R, mu=MU)
    sim.close()
    assert all(np.array_equal(g, r[perm]) for g, r in zip(got, ref))
    sim = BatchSim(sc, batch=1)
    _tape(sim, sc, cs, slice(1, 2))
    got = sim.rollout_lqr(N, lx[1:2], lu[1:2], Q, R, mu=MU)
    sim.close()
    assert all(np.array_equal(g, r[1:2]) for g, r in zip(got, ref))


@pytest.mark.gpu
def test_a_tape_from_the_feedback_call_is_the_replayed_open_loop_tape():
    from redmax_amd import BatchSim
    sc, cs, N = _setup(5)
    nom = _nominal(5)
    lx, lu, Q, R = nom["cost"]
    rng = np.random.default_rng(9)
    K = 1e-3 * rng.standard_normal((B, N, 2 * sc.nr, sc.nr))
    xref = np.concatenate([nom["qt"], nom["qdt"]], axis=-1) + 0.01 * rng.standard_normal((B, N, 2 * sc.nr))
    sim = BatchSim(sc, batch=B)
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, uapp = sim.rollout_feedback(N, sc.h, cs["u"], K, xref, pscale=sc.task["pscale"])[:3]
    closed = sim.rollout_lqr(N, lx, lu, Q, R, mu=MU)
    sim.set_state(cs["q0"], cs["qd0"])
    qo, qdo, _ = sim.rollout_tape(N, sc.h, uapp, pscale=sc.task["pscale"])
    replay = sim.rollout_lqr(N, lx, lu, Q, R, mu=MU)
    sim.close()
    assert np.array_equal(qt, qo) and np.array_equal(qdt, qdo)
    assert _same(closed, replay) and np.abs(uapp - cs["u"]).max() > 0


# ---------------------------------------------------------------- 4. not positive definite

@pytest.mark.gpu
def test_a_rollout_that_is_not_positive_definite_takes_no_step_and_leaves_the_others_alone():
    from redmax_amd import BatchSim
    sc, cs, N = _setup(5)
    nom = _nominal(5)
    lx, lu, Q, R = nom["cost"]
    BN = nom["Bm"][1, N - 1]
    c = 2 * np.linalg.eigvalsh(R).max() / np.linalg.eigvalsh(BN.T @ BN).min()
    Qb = np.tile(Q, (B, 1, 1, 1))
    Qb[1, N - 1] = -c * np.eye(2 * sc.nr)
    assert np.linalg.eigvalsh(R + BN.T @ Qb[1, N - 1] @ BN).max() < -MU      # negative definite, mu included, for rollout 1 only
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    ref = sim.rollout_lqr(N, lx, lu, Q, R, mu=MU)
    kff, K, expected, notpd = sim.rollout_lqr(N, lx, lu, Qb, R, mu=MU)      # (raises unless the call returns 0)
    sim.close()
    assert notpd.tolist() == [False, True, False]
    assert not kff[1].any() and not K[1].any() and expected[1] == 0
    for b in (0, 2):
        assert all(np.array_equal(g[b], r[b]) for g, r in zip((kff, K, expected), ref)), b


# ---------------------------------------------------------------- 5. refusals

@pytest.mark.gpu
def test_refusals_leave_the_tape_alone():
    from redmax_amd import BatchSim, _abi
    sc, cs, N = _setup(5)
    nom = _nominal(5)
    lx, lu, Q, R = nom["cost"]
    rng = np.random.default_rng(11)
    gq, gqd = rng.standard_normal((B, N, sc.nr)), rng.standard_normal((B, N, sc.nr))
    sim = BatchSim(sc, batch=B)
    with pytest.raises(_abi.RedMaxHipError, match="no tape"):
        sim.rollout_lqr(N, lx, lu, Q, R)
    _tape(sim, sc, cs)
    vjp0 = sim.rollout_vjp(N, gq, gqd)
    L, bt = sim._L, sim._batch
    kff, K = np.empty((B, N, sc.nr)), np.empty((B, N, 2 * sc.nr, sc.nr))

    def call(nsteps=N, batch=bt, cost=True, out=True, per=0, mu=MU, **null):
        p = dict(lx=lx, lu=lu, Q=Q, R=R, kff=kff, K=K)
        p.update(null)
        ptr = {k: (None if v is None else v.ctypes.data) for k, v in p.items()}
        cst = _abi.LqrCost(ptr["lx"], ptr["lu"], ptr["Q"], ptr["R"], per, mu, None)
        gains = _abi.LqrGains(ptr["kff"], ptr["K"], None, None)
        rc = L.rmx_rollout_lqr(batch, nsteps, C.byref(cst) if cost else None, C.byref(gains) if out else None)
        return rc, (L.rmx_last_error() or b"").decode()

    for kw in (dict(batch=None), dict(cost=False), dict(out=False), dict(lx=None), dict(lu=None), dict(Q=None), dict(R=None), dict(kff=None),
               dict(K=None)):
        rc, msg = call(**kw)
        assert rc != 0 and "null argument" in msg, (kw, msg)
    for kw, words in ((dict(nsteps=N - 1), "nsteps differs"), (dict(per=2), "per_rollout"), (dict(mu=-1.0), "mu"), (dict(mu=float("nan")), "mu"),
                      (dict(mu=float("inf")), "mu")):
        rc, msg = call(**kw)
        assert rc != 0 and words in msg, (kw, msg)
    assert _same(vjp0, sim.rollout_vjp(N, gq, gqd))
    # a BDF2 tape
    sim.set_state(cs["q0"], cs["qd0"])
    sim.rollout_tape(N, sc.h, cs["u"], pscale=sc.task["pscale"], integrator=2)
    vjp2 = sim.rollout_vjp(N, gq, gqd)
    with pytest.raises(_abi.RedMaxHipError, match="BDF1 tape"):
        sim.rollout_lqr(N, lx, lu, Q, R)
    assert _same(vjp2, sim.rollout_vjp(N, gq, gqd))
    sim.close()
    # nr > 32
    sc40 = _scene(40, 1)
    c40 = case(sc40, 53, nsteps=2, B=1)
    sim = BatchSim(sc40, batch=1)
    sim.set_state(c40["q0"], c40["qd0"])
    sim.rollout_tape(2, sc40.h, c40["u"], pscale=sc40.task["pscale"])
    g = np.ones((1, 2, 40))
    vjp40 = sim.rollout_vjp(2, g, g)
    with pytest.raises(_abi.RedMaxHipError, match=r"nr > 32.*nr = 40"):
        sim.rollout_lqr(2, np.zeros((1, 2, 80)), np.zeros((1, 2, 40)), np.tile(np.eye(80), (2, 1, 1)), np.eye(40))
    assert _same(vjp40, sim.rollout_vjp(2, g, g))
    sim.close()


# ---------------------------------------------------------------- 6. ilqr.solve(backward="device")

@pytest.mark.gpu
def test_ilqr_solve_with_the_device_backward_pass():
    import torch
    from redmax_amd import BatchSim, ilqr
    from test_gpu_ilqr import ITERS, _grad_norm
    sc, cs, t, cost = _torch_problem()
    N, ps = t["u"].shape[1], sc.task["pscale"]
    sim = BatchSim(sc, batch=B)
    J0, g0 = _grad_norm(sim, sc, t, cost, t["u"])
    res, hist = ilqr.solve(sim, t["q0"], t["qd0"], t["u"], cost, iters=ITERS, h=sc.h, pscale=ps, backward="device")
    h = hist.cpu().numpy()
    assert h.shape == (ITERS + 1, B)
    assert (h[1:] <= h[:-1]).all()                                   # exact: a rollout keeps a trial only where it lowers its own cost
    assert (h[-1] < h[0]).all()
    assert np.array_equal(res.cost.cpu().numpy(), h[-1])
    # the sim is at the end of the returned trajectories, and its tape is theirs
    q, qd = sim.get_state()
    assert np.array_equal(q, res.qtraj[:, -1].cpu().numpy()) and np.array_equal(qd, res.qdtraj[:, -1].cpu().numpy())
    rng = np.random.default_rng(3)
    gq, gqd = rng.standard_normal((B, N, sc.nr)), rng.standard_normal((B, N, sc.nr))
    after_solve = sim.rollout_vjp(N, gq, gqd)
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, _ = sim.rollout_tape(N, sc.h, res.u.cpu().numpy(), pscale=ps)
    explicit = sim.rollout_vjp(N, gq, gqd)
    assert np.array_equal(qt, res.qtraj.cpu().numpy()) and np.array_equal(qdt, res.qdtraj.cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(after_solve, explicit))
    assert np.allclose(h[0], J0.cpu().numpy(), rtol=1e-12)
    J1, g1 = _grad_norm(sim, sc, t, cost, res.u)
    assert np.allclose(J1.cpu().numpy(), h[-1], rtol=1e-12)
    assert (g1 < g0).all()
    rt, ht = ilqr.solve(sim, t["q0"], t["qd0"], t["u"], cost, iters=ITERS, h=sc.h, pscale=ps, backward="torch")
    print("final cost per rollout, backward='device' %s\n                        backward='torch'  %s" % (h[-1], ht[-1].cpu().numpy()))
    with pytest.raises(ValueError, match="backward"):
        ilqr.solve(sim, t["q0"], t["qd0"], t["u"], cost, iters=1, h=sc.h, pscale=ps, backward="numpy")
    sim.close()
