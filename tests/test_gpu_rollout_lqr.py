"""rmx_rollout_lqr: the Riccati sweep of iLQR on the device, read off the BDF1 tape (redmax_amd/csrc/rmx_lqr.h).

The checks, in the order of the sections below:
  1. against the reference: ilqr.backward_pass (float64, CPU) and the device call are both judged against the longdouble recursion
     of tests/proto_lqr_backward.py on IDENTICAL inputs - A, B assembled from rmx_rollout_linearize on the same tape.  Per rollout
     and per quantity (kff, K, expected), e = max |. - ext| / max |ext|, and e_gpu <= 8 e_ref with e_ref floored at 16 eps: two
     correct float64 evaluations of one recursion with different summation orders and another factorisation differ by small
     constant factors in an error that is eps * conditioning for both; three bits allow that and do not allow a lost term;
  2. closing the loop through rmx_rollout_tape_feedback_device; 3. exact structure, bit for bit; 4. a rollout that is not positive
     definite - at the first step processed, and at an interior step behind a good pivot, then rescued by a larger mu of its own;
     5. refusals; 6. ilqr.solve(backward="device").

Scenes: sceneAdjointChain(5) (nr 5, padded to 8), sceneAdjointTree7, sceneAdjointChain(32) (the LDS limit); B = 3, N = 8 (N = 3
for the 32-link chain); states from test_rollout_vjp_proto.case; the cost of test_gpu_ilqr._problem: Q = diag(1 on q, 0.01 on qdot),
R = 0.1 I, mu = 1e-6 ("diag").  With the dense costs of proto_lqr_backward.dense_cost ("dense": every entry of Q and R set, another
Q at every step and, per rollout, for every rollout) also sceneAdjointChain(2) and (3) (NP 4: one tile, and an odd d), "fixed" of
test_rollout_feedback_proto (n 5, nr 3, NP 8: nodes without a DOF inside the tree), sceneAdjointChain(11) (NP 16, part-filled) and
(16) (NP 16, full); N = 6, N = 3 for the 16-link chain.

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
The cases on dense costs, one line each (e_ref e_gpu per quantity, the rollout with the largest e_gpu; "per": one table per rollout).
Where e_ref leaves the floor the bound is 8 e_ref; the largest e_gpu / bound of these lines is 0.33:
    scene   N   cost                      kff                 K                   expected            cond(Quu)
    2       6   dense                     1.06e-14 1.61e-14   8.27e-15 1.31e-14   3.90e-16 4.30e-16   561
    2       6   dense per                 1.18e-14 1.04e-14   8.27e-15 1.31e-14   3.90e-16 4.30e-16   484
    3       6   dense                     8.27e-15 1.09e-14   7.29e-15 1.01e-14   2.05e-16 1.32e-16   660
    3       6   dense per                 1.11e-14 1.51e-14   4.64e-15 1.23e-14   5.69e-16 2.50e-16   640
    fixed   6   dense                     8.35e-16 7.88e-16   6.60e-16 7.14e-16   2.22e-16 2.07e-16   7.7
    fixed   6   dense per                 5.79e-16 9.86e-16   1.25e-15 1.49e-15   3.17e-16 2.66e-16   11.7
    5       8   dense                     2.57e-14 5.73e-14   1.47e-14 3.48e-14   2.09e-16 2.09e-16   1.6e3
    5       8   dense per                 9.56e-15 3.45e-14   2.56e-14 2.94e-14   2.09e-16 2.09e-16   1.6e3
    tree7   8   dense                     7.59e-16 1.52e-15   2.12e-15 3.48e-15   3.64e-16 1.90e-16   2.6e3
    tree7   8   dense per                 7.59e-16 1.52e-15   2.09e-15 2.29e-15   9.91e-17 2.63e-16   3.6e3
    11      6   dense                     2.95e-14 3.41e-14   1.39e-14 3.57e-14   1.66e-15 9.49e-16   2.0e3
    11      6   dense per                 5.07e-14 7.13e-14   1.39e-14 3.57e-14   5.95e-16 5.83e-16   3.4e3
    16      3   dense                     1.75e-14 1.58e-14   2.89e-14 3.80e-14   3.26e-16 3.26e-16   788
    16      3   dense per                 2.98e-14 2.67e-14   4.37e-14 4.75e-14   1.55e-15 2.86e-16   1.6e3
    32      3   dense                     9.76e-15 1.05e-14   2.73e-14 4.59e-14   3.50e-16 6.50e-16   548
    32      3   dense per                 9.76e-15 1.05e-14   3.01e-14 3.09e-14   4.01e-16 4.01e-16   580
    3       6   dense, R not symmetric    1.05e-14 6.34e-15   7.30e-15 1.01e-14   3.07e-16 1.80e-16   660
    5       8   dense, R not symmetric    2.56e-14 4.70e-14   2.56e-14 2.62e-14   2.93e-16 2.93e-16   1.6e3
    5       8   ill-conditioned, mu 0     1.14e-11 8.36e-12   4.63e-11 3.29e-11   1.72e-15 8.76e-15   1.3e6  (Q x 1e-6; bound 8 eps cond = 1.8e-9)
    16      3   ill-conditioned, mu 0     1.15e-10 1.55e-10   1.94e-10 1.70e-10   6.11e-17 6.11e-17   2.6e7  (Q x 1e-9; bound 4.4e-8)
    5       8   rescued, mu 95.1272       4.53e-16 2.84e-16   2.19e-15 1.08e-15   3.56e-16 1.46e-16   2.5    (rollout 1)
    11      6   rescued, mu 112.669       4.82e-16 4.06e-16   4.08e-16 7.81e-16   3.58e-17 2.37e-16   2.1    (rollout 1)
The indefinite cases: scene 5, step row 4 of 8, c = 2, the recursion stops at pivot 1; scene 11, step row 3 of 6, c = 2, pivot 1; one
quadrupling of mu from |lambda_min(Quu0)| makes each positive definite again, and the margin's makes the mu above.  Closing the loop
with the dense cost: J 60.27, 60.99, 54.89 before, 0.989, 1.814, 1.941 after the full step with either path's gains.
"""
import ctypes as C

import numpy as np
import pytest

import proto_lqr_backward as P
import proto_rollout_linearize as lin
from test_gpu_adjoint_controls import _DevArray, _scene
from test_rollout_feedback_proto import scene as _scene_or_fixed
from test_rollout_vjp_proto import case

B, MU = 3, 1e-6
STEPS = {5: 8, "tree7": 8, 32: 3, 2: 6, 3: 6, "fixed": 6, 11: 6, 16: 3}
SEED = {2: 2, 3: 3, "fixed": 4, 5: 5, "tree7": 7, 11: 11, 16: 16, 32: 32}      # of a size's dense cost
EPS = np.finfo(np.float64).eps
_CACHE = {}


def _setup(size, nsteps=None):
    nsteps = STEPS[size] if nsteps is None else nsteps
    key = (size, nsteps)
    if key not in _CACHE:
        sc = _scene_or_fixed(size, 1)
        _CACHE[key] = (sc, case(sc, 53, nsteps=nsteps, B=B), nsteps)
    return _CACHE[key]


def _tape(sim, sc, cs, sel=slice(None)):
    sim.set_state(cs["q0"][sel], cs["qd0"][sel])
    qt, qdt, info = sim.rollout_tape(cs["u"].shape[1], sc.h, cs["u"][sel], pscale=sc.task["pscale"], stats=True)
    assert (info["status"] & 15 == 0).all()
    return qt, qdt


def _cost(sc, cs, qt, qdt, sel=slice(None), QR=None):
    """(lx, lu, Q, R) of test_gpu_ilqr._problem's cost at the nominal (qt, qdt, u); QR = (Q, R): of that cost instead, Q [N][.][.] or
    one table per rollout - lx = Q_k (x_k - goal), lu = R u_k for the same goal."""
    nr, N = sc.nr, qt.shape[1]
    q0, _ = sc.getQ()
    goal = np.concatenate([q0 - 0.1, np.zeros(nr)])
    x = np.concatenate([qt, qdt], axis=-1)
    if QR is not None:
        Q, R = QR
        return np.einsum("kij,bkj->bki" if Q.ndim == 3 else "bkij,bkj->bki", Q, x - goal), np.einsum("ij,bkj->bki", R, cs["u"][sel]), Q, R
    Q = np.tile(np.diag([1.0] * nr + [0.01] * nr), (N, 1, 1))
    R = 0.1 * np.eye(nr)
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

def _dense(size, nsteps=None, per=False, **spectra):
    """(lx, lu, Q, R) of proto_lqr_backward.dense_cost at a size's nominal, shared or one table per rollout: computed once."""
    key = ("dense", size, nsteps, per) + tuple(sorted(spectra.items()))
    if key not in _CACHE:
        sc, cs, N = _setup(size, nsteps)
        nom = _nominal(size, nsteps)
        _CACHE[key] = _cost(sc, cs, nom["qt"], nom["qdt"], QR=P.dense_cost(9000 + SEED[size], sc.nr, N, B if per else None, **spectra))
    return _CACHE[key]


def _table(Q, b):
    return Q[b] if Q.ndim == 4 else Q


def _backward_pass(nom, lx, lu, Q, R, mu, b):
    """ilqr.backward_pass (float64, CPU) of rollout b with its own table and its own mu."""
    import torch
    from redmax_amd.ilqr import backward_pass
    t = lambda a: torch.tensor(a, dtype=torch.float64)      # noqa: E731
    return tuple(a.numpy()[0] for a in backward_pass(t(nom["A"][b:b + 1]), t(nom["Bm"][b:b + 1]), t(lx[b:b + 1]), t(lu[b:b + 1]),
                                                     t(_table(Q, b)), t(R), float(mu)))


def _judge(tag, b, ref, gpu, ext, cond, stability=False):
    """The file's rule for one rollout: ref = backward_pass's (kff, K, expected), gpu = the device's with K as backward_pass orders it,
    ext = the longdouble recursion's.  e_gpu <= 8 max(e_ref, 16 eps) per quantity; stability: eps * cond joins the maximum."""
    ok = True
    for name, r, g, e in zip(("kff", "K", "expected"), ref, gpu, ext):
        e_ref, e_gpu = P.rel_err(r, e), P.rel_err(g, e)
        bound = 8 * max(e_ref, 16 * EPS, EPS * cond if stability else 0.0)
        print("%s b %d %-8s: e_ref %.3e e_gpu %.3e bound %.3e cond(Quu) %.3e%s"
              % (tag, b, name, e_ref, e_gpu, bound, cond, "" if e_gpu <= bound else "   <-- over"))
        ok = ok and e_gpu <= bound
    return ok


DENSE_SIZES = [2, 3, "fixed", 5, "tree7", 11, 16, 32]
_DIAG = [(5, None, False), (5, None, True), ("tree7", None, False), (32, None, False), (32, None, True), (5, 1, False)]
CASES = [pytest.param(s, n, p, "diag", id="%s-%s-%s" % (s, n, p)) for s, n, p in _DIAG] + \
        [pytest.param(s, None, p, "dense", id="%s-dense-%s" % (s, "per-rollout" if p else "shared")) for s in DENSE_SIZES for p in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("size,nsteps,per,cost", CASES)
def test_gains_meet_the_extended_recursion_as_closely_as_backward_pass(size, nsteps, per, cost):
    """cost "diag": test_gpu_ilqr._problem's, per: B copies of its table.  "dense": proto_lqr_backward.dense_cost - every entry of Q
    and R set, another table at every step and, with per, for every rollout; each rollout is judged on its own table."""
    import torch
    from redmax_amd import BatchSim
    from redmax_amd.ilqr import backward_pass
    sc, cs, N = _setup(size, nsteps)
    nom = _nominal(size, nsteps)
    if cost == "dense":
        lx, lu, Q, R = _dense(size, nsteps, per)
        assert Q.ndim == (4 if per else 3) and np.abs(Q).min() > 0 and np.abs(R).min() > 0
        sim = BatchSim(sc, batch=B)
        _tape(sim, sc, cs)
        kff, K, expected, notpd = sim.rollout_lqr(N, lx, lu, Q, R, mu=MU)
        sim.close()
        assert kff.shape == (B, N, sc.nr) and K.shape == (B, N, 2 * sc.nr, sc.nr) and expected.shape == (B,) and not notpd.any()
        ok = True
        for b in range(B):
            ext = P.backward_pass_ext(nom["A"][b], nom["Bm"][b], lx[b], lu[b], _table(Q, b), R, MU)
            assert not ext[3]
            ok = _judge("size %s N %d dense per %d" % (size, N, per), b, _backward_pass(nom, lx, lu, Q, R, MU, b),
                        (kff[b], K[b].transpose(0, 2, 1), expected[b]), ext[:3], ext[4]) and ok
        assert ok
        return
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


@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, 16])
def test_ill_conditioned_quu_within_the_stability_bound_of_an_spd_solve(size):
    """mu = 0, R with the spectrum 1e-9 .. 0.1, and Q scaled down by factors of 1e-3 until cond(Quu) >= 1e6 in every rollout (Quu -> R,
    cond 1e8, as Q -> 0).  The rule gains the term eps * cond: the backward-stability bound of an SPD solve; 8 stays the allowance
    between two correct float64 evaluations."""
    from redmax_amd import BatchSim
    sc, cs, N = _setup(size)
    nom = _nominal(size)
    Q0, R = P.dense_cost(9100 + SEED[size], sc.nr, N, r_spectrum=(1e-9, 0.1))
    for power in range(7):
        lx, lu, Q, R = _cost(sc, cs, nom["qt"], nom["qdt"], QR=(Q0 * 1e-3 ** power, R))
        exts = [P.backward_pass_ext(nom["A"][b], nom["Bm"][b], lx[b], lu[b], Q, R, 0.0) for b in range(B)]
        if min(e[4] for e in exts) >= 1e6:
            break
    print("size %s: Q scaled by 1e-%d, cond(Quu) per rollout %s" % (size, 3 * power, [e[4] for e in exts]))
    assert min(e[4] for e in exts) >= 1e6 and not any(e[3] for e in exts)
    refs = [_backward_pass(nom, lx, lu, Q, R, 0.0, b) for b in range(B)]
    assert all(np.isfinite(a).all() for r in refs for a in r)                       # (float64 on the CPU takes the step too)
    assert all(np.linalg.eigvalsh(R + nom["Bm"][b, N - 1].T @ Q[N - 1] @ nom["Bm"][b, N - 1]).min() > 0 for b in range(B))
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    kff, K, expected, notpd = sim.rollout_lqr(N, lx, lu, Q, R, mu=0.0)
    sim.close()
    assert not notpd.any()
    ok = True
    for b in range(B):
        ok = _judge("size %s N %d ill-conditioned" % (size, N), b, refs[b], (kff[b], K[b].transpose(0, 2, 1), expected[b]), exts[b][:3],
                    exts[b][4], stability=True) and ok
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


@pytest.mark.gpu
def test_gains_close_the_loop_through_the_feedback_kernel_with_a_dense_cost():
    """The same loop with a QuadraticCost built from dense_cost.  alpha = 0 is bit for bit as before.  alpha = 1: a full iLQR step on
    a nonlinear rollout need not lower the cost, so J1 < J0 is asserted where it holds for ilqr.backward_pass's gains (diff.linearize
    on the same nominal) through the same feedback kernel; otherwise the two paths must agree on the sign of J1 - J0 per rollout."""
    import torch
    from redmax_amd import BatchSim, diff
    from redmax_amd.ilqr import QuadraticCost, backward_pass
    sc, cs, t, diag = _torch_problem()
    N, ps = t["u"].shape[1], sc.task["pscale"]
    dev = t["u"].device
    Q, R = P.dense_cost(9200, sc.nr, N)
    cost = QuadraticCost(torch.tensor(Q, device=dev), torch.tensor(R, device=dev), diag.xgoal)
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
    _, _, A, Bm = diff.linearize(sim, t["q0"], t["qd0"], ubar, h=sc.h, pscale=ps)
    rk, rK, rexp = backward_pass(A, Bm, lx, lu, cost.Q, cost.R, MU)
    q3, qd3, u3 = diff.rollout_feedback(sim, t["q0"], t["qd0"], ubar + rk, rK.transpose(-1, -2).contiguous(), xref, h=sc.h, pscale=ps)
    J1r = cost.value(torch.cat([q3, qd3], dim=-1), u3)
    print("J before %s\nJ after the full step %s\n  with backward_pass's gains %s\nexpected decrease %s (backward_pass %s)"
          % (J0.cpu().numpy(), J1.cpu().numpy(), J1r.cpu().numpy(), expected.cpu().numpy(), rexp.cpu().numpy()))
    if (J1r < J0).all():
        assert (J1 < J0).all()
    else:
        assert torch.equal(torch.sign(J1 - J0), torch.sign(J1r - J0))
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


FILL = 1234.5                      # what the output buffers hold before a device call
FILL_WORD = 0x55555555             # and the status words


class _Outputs:
    """Device buffers for kff, K, expected and status, each with a guard row behind [B][N].. (one more row of the last axis; B more
    words behind status), all of it pre-filled: what a call leaves untouched shows."""

    def __init__(self, N, nr):
        self.shapes = dict(kff=(B * N + 1, nr), K=(B * N + 1, 2 * nr * nr), exp=(B + 1,))
        self.dev = {k: _DevArray(np.full(s, FILL)) for k, s in self.shapes.items()}
        self.dev["st"] = _DevArray(np.full(2 * B, FILL_WORD, dtype=np.int32).view(np.float64))
        self.N, self.nr = N, nr

    def ptrs(self):
        return tuple(self.dev[k].ptr.value for k in ("kff", "K", "exp", "st"))

    def get(self):
        """(kff, K, expected, notpd) as rollout_lqr returns them, after checking the guards."""
        N, nr = self.N, self.nr
        kff, K, ex, st = (self.dev[k].get() for k in ("kff", "K", "exp", "st"))
        st = st.view(np.int32)
        assert (kff[-1] == FILL).all() and (K[-1] == FILL).all() and ex[-1] == FILL and (st[B:] == FILL_WORD).all()
        assert set(st[:B].tolist()) <= {0, 1}
        return kff[:-1].reshape(B, N, nr), K[:-1].reshape(B, N, 2 * nr, nr), ex[:B], st[:B] != 0

    def free(self):
        for a in self.dev.values():
            a.free()


def _device_call(sim, N, nr, lx, lu, Q, R, mu=MU, mu_b=None):
    """rollout_lqr_device into pre-filled, guarded output buffers: (kff, K, expected, notpd)."""
    ins = [_DevArray(a) for a in (lx, lu, Q, R)] + ([] if mu_b is None else [_DevArray(mu_b)])
    out = _Outputs(N, nr)
    sim.rollout_lqr_device(N, *([a.ptr.value for a in ins[:4]] + list(out.ptrs())), per_rollout=Q.ndim == 4, mu=mu,
                           mu_b_ptr=None if mu_b is None else ins[4].ptr.value)
    got = out.get()
    for a in ins:
        a.free()
    out.free()
    return got


def _interior(size):
    """Per-rollout dense tables at a size and rollout 1's made indefinite at the interior step N // 2 (proto_lqr_backward.indefinite_at),
    with the mu that rescues it: computed once."""
    key = ("interior", size)
    if key not in _CACHE:
        sc, cs, N = _setup(size)
        nom = _nominal(size)
        lx, lu, Qb, R = _dense(size, None, True)
        s = N // 2
        Q1, c = P.indefinite_at(nom["A"][1], nom["Bm"][1], lx[1], lu[1], Qb[1], R, MU, s)
        Qi = Qb.copy()
        Qi[1] = Q1
        where = P.backward_pass_ext(nom["A"][1], nom["Bm"][1], lx[1], lu[1], Q1, R, MU, flag=True)[5]
        mu, rounds = P.rescue_mu(nom["A"][1], nom["Bm"][1], lx[1], lu[1], Q1, R, MU)
        print("size %s: indefinite at step row %d of %d, c = %g, stopped at (step, pivot) %s; rescued by mu = %.6g after %d quadruplings"
              % (size, s, N, c, where, mu, rounds))
        _CACHE[key] = dict(Qi=Qi, s=s, c=c, where=where, mu=mu)
    return _CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, 11])
def test_indefinite_at_an_interior_step_zeroes_the_rows_already_written(size):
    """Rollout 1 stops at step row N // 2 behind one or more good pivots: the gains of the steps after it are in memory by then and
    must be zeroed with the rest.  Device form, output buffers pre-filled: the zeros are written, not left over."""
    from redmax_amd import BatchSim
    sc, cs, N = _setup(size)
    lx, lu, Qb, R = _dense(size, None, True)
    it = _interior(size)
    assert it["where"][0] == it["s"] == N // 2 and it["where"][1] >= 1 and 0 < it["s"] < N - 1
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    ref = sim.rollout_lqr(N, lx, lu, Qb, R, mu=MU)
    assert not ref[3].any() and all(np.abs(ref[0][1, k]).max() > 0 for k in range(N))      # (every row of rollout 1 is non-zero before)
    kff, K, expected, notpd = _device_call(sim, N, sc.nr, lx, lu, it["Qi"], R)
    sim.close()
    assert notpd.tolist() == [False, True, False]
    assert all(not kff[1, k].any() and not K[1, k].any() for k in range(N)) and expected[1] == 0
    for b in (0, 2):
        assert all(np.array_equal(g[b], r[b]) for g, r in zip((kff, K, expected), ref)), b
        assert (kff[b] != FILL).all() and (K[b] != FILL).all() and expected[b] != FILL


@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, 11])
def test_a_larger_mu_for_that_rollout_alone_rescues_it(size):
    """The regularise-and-retry step of an iLQR: the same tables, mu_b = [MU, rescue_mu, MU] - mu of the size of Quu0 decides rollout
    1's answer, where Quu0 and Quu0 + mu I must each keep their place."""
    from redmax_amd import BatchSim
    sc, cs, N = _setup(size)
    nom = _nominal(size)
    lx, lu, Qb, R = _dense(size, None, True)
    it = _interior(size)
    mub = np.array([MU, it["mu"], MU])
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    ref = sim.rollout_lqr(N, lx, lu, Qb, R, mu=MU)
    kff, K, expected, notpd = sim.rollout_lqr(N, lx, lu, it["Qi"], R, mu=123.0, mu_b=mub)
    dev = _device_call(sim, N, sc.nr, lx, lu, it["Qi"], R, mu=123.0, mu_b=mub)
    sim.close()
    assert not notpd.any() and _same((kff, K, expected, notpd), dev)
    for b in (0, 2):
        assert all(np.array_equal(g[b], r[b]) for g, r in zip((kff, K, expected), ref)), b
    ext = P.backward_pass_ext(nom["A"][1], nom["Bm"][1], lx[1], lu[1], it["Qi"][1], R, it["mu"])
    assert not ext[3] and np.abs(ext[0]).max() > 0
    assert _judge("size %s N %d rescued, mu %.6g" % (size, N, it["mu"]), 1, _backward_pass(nom, lx, lu, it["Qi"], R, it["mu"], 1),
                  (kff[1], K[1].transpose(0, 2, 1), expected[1]), ext[:3], ext[4])


@pytest.mark.gpu
@pytest.mark.parametrize("size", [3, 5])
def test_the_device_form_reads_both_triangles_of_R(size):
    """R as the kernel reads it is 0.5 (R(i, j) + R(j, i)): a table with an antisymmetric part of the size of its entries, which no
    host wrapper would pass on as it is, gives the gains of its symmetric part - judged by the file's rule against the longdouble
    recursion on (R + R')/2."""
    from redmax_amd import BatchSim
    sc, cs, N = _setup(size)
    nom = _nominal(size)
    lx, lu, Q, R = _dense(size, None, False)
    skew = np.triu(np.random.default_rng(13).uniform(0.25, 0.5, R.shape), 1) * np.abs(R).max()
    Rns = R + skew - skew.T
    assert np.abs(Rns - Rns.T).max() > np.abs(R).max() / 4
    Rs = (Rns.astype(P.LD) + Rns.T.astype(P.LD)) / 2
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    kff, K, expected, notpd = _device_call(sim, N, sc.nr, lx, lu, Q, Rns)
    sim.close()
    assert not notpd.any()
    ok = True
    for b in range(B):
        ext = P.backward_pass_ext(nom["A"][b], nom["Bm"][b], lx[b], lu[b], Q, Rs, MU)
        assert not ext[3]
        ok = _judge("size %s N %d R with an antisymmetric part" % (size, N), b, _backward_pass(nom, lx, lu, Q, Rs.astype(np.float64), MU, b),
                    (kff[b], K[b].transpose(0, 2, 1), expected[b]), ext[:3], ext[4]) and ok
    assert ok


@pytest.mark.gpu
def test_lqr_backward_returns_the_bits_of_rollout_lqr_on_dense_per_rollout_tables():
    import torch
    from redmax_amd import BatchSim, diff
    sc, cs, N = _setup(5)
    lx, lu, Qb, R = _dense(5, None, True)
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    ref = sim.rollout_lqr(N, lx, lu, Qb, R, mu=MU)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=torch.device("cuda", sim.device))      # noqa: E731
    for Q, want in ((Qb, ref), (Qb[2], sim.rollout_lqr(N, lx, lu, Qb[2], R, mu=MU))):
        kff, K, expected, notpd = diff.lqr_backward(sim, t(lx), t(lu), t(Q), t(R), MU)
        assert K.shape == (B, N, 2 * sc.nr, sc.nr) and K.is_contiguous()                  # rollout_feedback's layout, as it takes it
        assert _same(want, (kff.cpu().numpy(), K.cpu().numpy(), expected.cpu().numpy(), notpd.cpu().numpy()))
    assert not np.array_equal(want[1], ref[1])
    sim.close()


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
