"""rmx_rollout_lqr_box: the box-constrained Riccati sweep of control-limited DDP on the device (k_rollout_lqr<NP, true>,
redmax_amd/csrc/rmx_lqr.h), against tests/proto_lqr_box.py.

B = 3; sizes 3 (NP 4, an odd d), 5 (NP 8), "fixed" (nodes without a DOF), 11 (NP 16, part-filled), 32 (the LDS limit, N = 3); the
"diag" and "dense" costs of tests/test_gpu_rollout_lqr.py, whose scenes, tapes and helpers this file imports.

Limits of a case ("recipe"): kff of the unconstrained longdouble recursion, r_i = half the median of |kff_{., i}| over rollouts and
steps, ulo_i = min ubar_{., i} - r_i, uhi_i = max ubar_{., i} + r_i (one box for the batch: minimum and maximum over rollouts and
steps) - the nominal is feasible; DOF 0 is unbounded above, DOF 1 has no bound at all.  With the random nominal torques of these
scenes the range of ubar is wide next to kff where the cost is "diag", and few steps clamp there (none for the 3-link chain), so
every case is run a second time with limits of this file's own ("tight"): the quartiles of the unconstrained target ubar + kff per
DOF, the same two DOFs unbounded - the nominal is not feasible at every step there, and a third to a half of the DOF-steps clamp.
Precondition, asserted for every rollout and step of every case: on the longdouble result every clamped multiplier and every free
DOF's distance to its finite bounds exceeds 1e-6 of its scale (proto_lqr_box.margins), so that a float64 evaluation must find the
same clamped sets; an input that fails gets its r_i (its quantile level) redrawn from the next seed, never a skip.  Every case
passed with the limits of attempt 0.

Against the proto: the clamped masks equal the proto's exactly; kff, K, expected are judged by test_gpu_rollout_lqr._judge with the
float64 run of the proto as the reference evaluation and its longdouble run as the truth: e_gpu <= 8 max(e_ref, 16 eps), three bits
for two correct float64 evaluations of one recursion in different summation orders.

Measured on an MI355X (per quantity e_ref e_gpu of the rollout with the largest e_gpu; cond(Quu) the largest over steps and rollouts;
clamped: DOF-steps on a bound of all; the mean number of QP iterations per step, 2 being the unconstrained solve).  The largest
e_gpu / bound of these lines is 0.48:
    scene N  cost  limits   kff                 K                   expected            cond(Quu) clamped  iterations
    3     6  diag  recipe   2.19e-16 2.73e-16   3.00e-16 3.15e-16   1.35e-16 1.41e-16   5.13       0/54    2.00
    3     6  diag  tight    3.32e-16 2.53e-16   4.52e-16 8.14e-16   2.31e-16 2.75e-16   5.13      15/54    2.78
    3     6  dense recipe   3.91e-15 7.16e-15   3.95e-15 1.43e-14   3.84e-16 9.58e-17   633       12/54    2.67
    3     6  dense tight    3.37e-15 1.19e-14   1.04e-14 1.27e-14   1.76e-16 2.89e-16   640       15/54    3.72
    5     8  diag  recipe   4.53e-16 7.44e-16   1.46e-15 7.31e-16   2.85e-16 2.26e-16   6.27      17/120   2.71
    5     8  diag  tight    7.12e-16 5.93e-16   6.95e-16 6.46e-16   1.09e-16 1.09e-16   6.27      39/120   3.04
    5     8  dense recipe   2.21e-15 3.54e-15   1.56e-15 1.85e-15   9.47e-17 9.47e-17   1.6e3     59/120   3.88
    5     8  dense tight    1.11e-14 1.02e-14   8.44e-15 1.10e-14   9.51e-16 5.61e-16   1.6e3     42/120   4.67
    fixed 6  diag  recipe   8.91e-17 2.23e-16   1.45e-16 3.06e-16   9.59e-20 1.96e-16   1.23       8/54    2.44
    fixed 6  diag  tight    2.25e-16 3.00e-16   3.49e-16 4.21e-16   2.16e-17 2.93e-16   1.22      14/54    2.56
    fixed 6  dense recipe   2.95e-16 4.79e-16   1.54e-15 1.21e-15   1.60e-16 2.26e-16   15.6      24/54    2.94
    fixed 6  dense tight    1.35e-15 1.33e-15   7.94e-16 2.20e-15   1.91e-16 3.28e-16   15.2      14/54    2.83
    11    6  diag  recipe   1.16e-15 7.85e-16   2.00e-15 9.09e-16   9.85e-17 1.00e-16   6.69      26/198   2.67
    11    6  diag  tight    4.77e-16 1.37e-15   1.08e-15 1.23e-15   2.05e-16 2.05e-16   6.83      83/198   3.39
    11    6  dense recipe   1.34e-14 1.71e-14   1.07e-14 2.28e-14   9.33e-17 8.21e-16   3.4e3     76/198   7.06
    11    6  dense tight    6.02e-15 2.33e-14   1.44e-14 2.86e-14   4.47e-16 3.05e-16   3.4e3     78/198   7.00
    32    3  diag  recipe   8.02e-16 1.32e-15   1.25e-15 1.58e-15   2.58e-16 5.06e-16   6.45      13/288   2.78
    32    3  diag  tight    7.59e-16 1.17e-15   5.15e-16 1.69e-15   1.08e-16 2.77e-16   6.66     159/288   4.22
    32    3  dense recipe   5.53e-15 3.75e-15   1.50e-14 1.01e-14   5.26e-16 5.26e-16   580      108/288   7.56
    32    3  dense tight    4.40e-15 5.84e-15   7.37e-15 6.23e-15   4.65e-16 1.13e-15   580      159/288   7.78
The cap: the proto needs 9, 9 and 5 QP iterations in the worst step of the three rollouts of the 5-link chain (dense, tight); with
max_iter below that a rollout gets status 2.  Closing the loop (test_gpu_ilqr's problem): J 0.891, 1.295, 0.987 before, 0.402,
0.863, 0.562 after the full constrained step; ilqr.solve under limits at the 0.2 / 0.8 quantiles of the unconstrained result ends at
0.3759, 0.8507, 0.5361 against 0.3727, 0.8427, 0.5343 without limits.
"""
import ctypes as C

import numpy as np
import pytest

import proto_lqr_backward as P
import proto_lqr_box as PB
from test_gpu_adjoint_controls import _DevArray, _scene
from test_gpu_rollout_lqr import B, MU, _dense, _interior, _judge, _nominal, _setup, _table, _tape
from test_rollout_vjp_proto import case

SIZES = [3, 5, "fixed", 11, 32]
MODES = ("recipe", "tight")
CASES = [pytest.param(s, c, m, id="%s-%s-%s" % (s, c, m)) for s in SIZES for c in ("diag", "dense") for m in MODES]
MARGIN = 1e-6
_CACHE = {}


def _inputs(size, cost):
    """(lx, lu, Q, R) of a case: the diag cost at the nominal, or the dense cost with one table per rollout."""
    if cost == "diag":
        return _nominal(size)["cost"]
    return _dense(size, None, True)


def _problem(size, cost, mode="recipe"):
    """The limits of a case and the proto's two runs per rollout, computed once: dict(ulo, uhi, ext[b], f64[b], attempt).  mode
    "recipe": the limits of the docstring; "tight": the quartiles of the unconstrained target ubar + kff per DOF."""
    key = (size, cost, mode)
    if key in _CACHE:
        return _CACHE[key]
    sc, cs, N = _setup(size)
    nom = _nominal(size)
    lx, lu, Q, R = _inputs(size, cost)
    nr, ubar = sc.nr, cs["u"]
    kff = np.array([np.asarray(P.backward_pass_ext(nom["A"][b], nom["Bm"][b], lx[b], lu[b], _table(Q, b), R, MU)[0], dtype=np.float64)
                    for b in range(B)])
    r0 = 0.5 * np.median(np.abs(kff).reshape(-1, nr), axis=0)
    for attempt in range(8):
        if mode == "recipe":
            r = r0 if attempt == 0 else r0 * np.random.default_rng(attempt).uniform(0.8, 1.2, nr)
            ulo = ubar.reshape(-1, nr).min(axis=0) - r
            uhi = ubar.reshape(-1, nr).max(axis=0) + r
        else:
            lev = 0.25 if attempt == 0 else np.random.default_rng(attempt).uniform(0.2, 0.3)
            ulo = np.quantile((ubar + kff).reshape(-1, nr), lev, axis=0)
            uhi = np.quantile((ubar + kff).reshape(-1, nr), 1 - lev, axis=0)
        uhi[0] = np.inf
        ulo[1], uhi[1] = -np.inf, np.inf
        ext = [PB.backward_pass_box(nom["A"][b], nom["Bm"][b], lx[b], lu[b], _table(Q, b), R, ubar[b], ulo, uhi, MU) for b in range(B)]
        marg = [PB.margins(e, ubar[b], ulo, uhi) for b, e in enumerate(ext)]
        print("size %s %s %s attempt %d: status %s, margins (multiplier, distance) %s" % (size, cost, mode, attempt, [e["status"] for e in ext], marg))
        if all(e["status"] == 0 for e in ext) and all(min(m) > MARGIN for m in marg):
            break
    else:
        raise AssertionError("no limits with strict complementarity above %g for size %s %s" % (MARGIN, size, cost))
    f64 = [PB.backward_pass_box(nom["A"][b], nom["Bm"][b], lx[b], lu[b], _table(Q, b), R, ubar[b], ulo, uhi, MU, dtype=np.float64)
           for b in range(B)]
    _CACHE[key] = dict(ulo=ulo, uhi=uhi, ext=ext, f64=f64, attempt=attempt, ubar=ubar)
    return _CACHE[key]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. against the proto

@pytest.mark.gpu
@pytest.mark.parametrize("size,cost,mode", CASES)
def test_gains_and_clamped_sets_meet_the_proto(size, cost, mode):
    from redmax_amd import BatchSim
    sc, cs, N = _setup(size)
    nr = sc.nr
    lx, lu, Q, R = _inputs(size, cost)
    pr = _problem(size, cost, mode)
    ulo, uhi, ubar = pr["ulo"], pr["uhi"], pr["ubar"]
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    kff, K, expected, status, clamped = sim.rollout_lqr_box(N, lx, lu, Q, R, ubar, (ulo, uhi), mu=MU)
    assert sim.last_step_kernel() == "k_rollout_lqr<box>"
    sim.close()
    assert kff.shape == (B, N, nr) and K.shape == (B, N, 2 * nr, nr) and clamped.shape == (B, N) and clamped.dtype == np.uint32
    assert not status.any()
    ok, nclamped = True, 0
    for b in range(B):
        ext, f64 = pr["ext"][b], pr["f64"][b]
        assert f64["status"] == 0 and np.array_equal(f64["clamped"], ext["clamped"])      # (the precondition at work on the CPU)
        assert np.array_equal(clamped[b], ext["clamped"]), (b, clamped[b], ext["clamped"])
        nclamped += int(ext["c"].sum())
        cond = max(float(np.linalg.cond(ext["H"][s].astype(np.float64))) for s in range(N))
        ok = _judge("size %s N %d %s %s" % (size, N, cost, mode), b, (f64["kff"], f64["K"], f64["expected"]),
                    (kff[b], K[b].transpose(0, 2, 1), expected[b]), (ext["kff"], ext["K"], ext["expected"]), cond) and ok
        # exact structure of the rows on a bound
        for s in range(N):
            for i in range(nr):
                if ext["c"][s, i]:
                    assert not K[b, s, :, i].any()
                    assert kff[b, s, i] in (ulo[i] - ubar[b, s, i], uhi[i] - ubar[b, s, i])
                else:
                    assert K[b, s, :, i].any()
    iters = np.mean([pr["ext"][b]["iters"].mean() for b in range(B)])
    print("size %s N %d %s %s: %d of %d DOF-steps on a bound, %.2f QP iterations per step, limits of attempt %d"
          % (size, N, cost, mode, nclamped, B * N * nr, iters, pr["attempt"]))
    u = ubar + kff
    slack = 4 * np.finfo(float).eps * np.abs(ubar).max()      # (ubar + (bound - ubar) rounds twice)
    assert (u >= ulo - slack).all() and (u <= uhi + slack).all()
    if mode == "tight":
        assert 0 < nclamped < B * N * nr
    assert ok


# ---------------------------------------------------------------- 2. exact structure

@pytest.mark.gpu
@pytest.mark.parametrize("size,cost", [pytest.param(s, c, id="%s-%s" % (s, c)) for s in SIZES for c in ("diag", "dense")])
def test_no_finite_bound_gives_the_bits_of_rollout_lqr(size, cost):
    from redmax_amd import BatchSim
    sc, cs, N = _setup(size)
    lx, lu, Q, R = _inputs(size, cost)
    inf = np.full(sc.nr, np.inf)
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    ref = sim.rollout_lqr(N, lx, lu, Q, R, mu=MU)
    for ulim in ((None, None), (-inf, inf), (None, inf), (-inf, None)):
        kff, K, expected, status, clamped = sim.rollout_lqr_box(N, lx, lu, Q, R, cs["u"], ulim, mu=MU)
        assert _same((kff, K, expected, status != 0), ref) and not clamped.any() and not status.any()
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, 32])
def test_exact_structure(size):
    from redmax_amd import BatchSim
    sc, cs, N = _setup(size)
    lx, lu, Q, R = _inputs(size, "diag")
    pr = _problem(size, "diag", "tight")
    ulim, ubar = (pr["ulo"], pr["uhi"]), pr["ubar"]
    rng = np.random.default_rng(7)
    gq, gqd = rng.standard_normal((B, N, sc.nr)), rng.standard_normal((B, N, sc.nr))
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    vjp0, lin0, state = sim.rollout_vjp(N, gq, gqd), sim.rollout_linearize(N), sim.get_state()
    ref = sim.rollout_lqr_box(N, lx, lu, Q, R, ubar, ulim, mu=MU)
    assert ref[4].any() and not ref[3].any()
    assert _same(ref, sim.rollout_lqr_box(N, lx, lu, Q, R, ubar, ulim, mu=MU))                                # repeat calls
    assert _same(vjp0, sim.rollout_vjp(N, gq, gqd)) and _same(lin0, sim.rollout_linearize(N)) and _same(state, sim.get_state())
    assert _same(ref, sim.rollout_lqr_box(N, lx, lu, np.tile(Q, (B, 1, 1, 1)), R, ubar, ulim, mu=MU))         # shared Q against copies
    assert _same(ref, sim.rollout_lqr_box(N, lx, lu, Q, R, ubar, ulim, mu=123.0, mu_b=np.full(B, MU)))        # mu against a constant mu_b
    assert _same(ref, sim.rollout_lqr_box(N, lx, lu, Q, R, ubar, ulim, mu=MU, max_iter=64))                   # 0 is the default of 64
    # NULL optional outputs and the device form against the host form
    d = {k: _DevArray(v) for k, v in (("lx", lx), ("lu", lu), ("Q", Q), ("R", R), ("ubar", ubar), ("ulo", ulim[0]), ("uhi", ulim[1]),
                                      ("kff", np.zeros_like(ref[0])), ("K", np.zeros_like(ref[1])), ("exp", np.zeros(B)),
                                      ("kff2", np.zeros_like(ref[0])), ("K2", np.zeros_like(ref[1])))}
    st = _DevArray(np.full(B, np.nan))                                 # (room for B int32 words)
    cl = _DevArray(np.full(B * N, np.nan))                             # (room for B * N uint32 words)
    p = lambda k: d[k].ptr.value                                       # noqa: E731
    sim.rollout_lqr_box_device(N, p("lx"), p("lu"), p("Q"), p("R"), p("ubar"), p("ulo"), p("uhi"), p("kff"), p("K"), p("exp"), st.ptr.value,
                               cl.ptr.value, mu=MU)
    sim.rollout_lqr_box_device(N, p("lx"), p("lu"), p("Q"), p("R"), p("ubar"), p("ulo"), p("uhi"), p("kff2"), p("K2"), mu=MU)
    assert np.array_equal(d["kff"].get(), ref[0]) and np.array_equal(d["K"].get(), ref[1]) and np.array_equal(d["exp"].get(), ref[2])
    assert not st.get().view(np.int32)[:B].any() and np.array_equal(cl.get().view(np.uint32)[:B * N].reshape(B, N), ref[4])
    assert np.array_equal(d["kff2"].get(), ref[0]) and np.array_equal(d["K2"].get(), ref[1])
    assert np.array_equal(d["lx"].get(), lx) and np.array_equal(d["ubar"].get(), ubar) and np.array_equal(d["ulo"].get(), ulim[0])
    for a in list(d.values()) + [st, cl]:
        a.free()
    assert _same(vjp0, sim.rollout_vjp(N, gq, gqd))
    sim.close()
    # a permuted batch, and B = 1 against B = 3
    perm = np.array([2, 0, 1])
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs, perm)
    got = sim.rollout_lqr_box(N, lx[perm], lu[perm], Q, R, ubar[perm], ulim, mu=MU)
    sim.close()
    assert all(np.array_equal(g, r[perm]) for g, r in zip(got, ref))
    sim = BatchSim(sc, batch=1)
    _tape(sim, sc, cs, slice(1, 2))
    got = sim.rollout_lqr_box(N, lx[1:2], lu[1:2], Q, R, ubar[1:2], ulim, mu=MU)
    sim.close()
    assert all(np.array_equal(g, r[1:2]) for g, r in zip(got, ref))


# ---------------------------------------------------------------- 3. status

@pytest.mark.gpu
def test_indefinite_at_an_interior_step_gives_status_1_for_that_rollout_alone():
    from redmax_amd import BatchSim
    size = 5
    sc, cs, N = _setup(size)
    nom = _nominal(size)
    lx, lu, Qb, R = _dense(size, None, True)
    it = _interior(size)
    pr = _problem(size, "dense", "recipe")      # (0 lies strictly inside every step's box: the first QP iteration factorises all of Hq)
    ulim, ubar = (pr["ulo"], pr["uhi"]), pr["ubar"]
    ext = PB.backward_pass_box(nom["A"][1], nom["Bm"][1], lx[1], lu[1], it["Qi"][1], R, ubar[1], ulim[0], ulim[1], MU)
    assert ext["status"] == 1 and 0 < it["s"] < N - 1
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    ref = sim.rollout_lqr_box(N, lx, lu, Qb, R, ubar, ulim, mu=MU)
    assert not ref[3].any() and all(np.abs(ref[0][1, k]).max() > 0 for k in range(N))
    kff, K, expected, status, clamped = sim.rollout_lqr_box(N, lx, lu, it["Qi"], R, ubar, ulim, mu=MU)
    sim.close()
    assert status.tolist() == [0, 1, 0]
    assert not kff[1].any() and not K[1].any() and expected[1] == 0 and not clamped[1].any()
    for b in (0, 2):
        assert all(np.array_equal(g[b], r[b]) for g, r in zip((kff, K, expected, clamped), (ref[0], ref[1], ref[2], ref[4]))), b


@pytest.mark.gpu
def test_a_cap_below_what_the_qp_needs_gives_status_2():
    from redmax_amd import BatchSim
    size = 5
    sc, cs, N = _setup(size)
    lx, lu, Q, R = _inputs(size, "dense")
    pr = _problem(size, "dense", "tight")
    ulim, ubar = (pr["ulo"], pr["uhi"]), pr["ubar"]
    need = np.array([pr["ext"][b]["iters"].max() for b in range(B)])
    print("QP iterations the proto needs per rollout (the largest over the steps): %s" % need)
    assert (need > 1).all()
    sim = BatchSim(sc, batch=B)
    _tape(sim, sc, cs)
    ref = sim.rollout_lqr_box(N, lx, lu, Q, R, ubar, ulim, mu=MU)
    for cap in sorted({1, int(need.min()), int(need.max()) - 1, int(need.max())}):
        kff, K, expected, status, clamped = sim.rollout_lqr_box(N, lx, lu, Q, R, ubar, ulim, mu=MU, max_iter=cap)
        assert status.tolist() == [0 if need[b] <= cap else 2 for b in range(B)], (cap, status, need)
        for b in range(B):
            if status[b]:
                assert not kff[b].any() and not K[b].any() and expected[b] == 0 and not clamped[b].any()
            else:
                assert all(np.array_equal(g[b], r[b]) for g, r in zip((kff, K, expected, clamped), (ref[0], ref[1], ref[2], ref[4]))), (cap, b)
    sim.close()


# ---------------------------------------------------------------- 4. closing the loop, ilqr.solve

def _torch_problem():
    from test_gpu_ilqr import _problem as problem
    return problem()


@pytest.mark.gpu
def test_constrained_gains_close_the_loop_inside_the_limits():
    import torch
    from redmax_amd import BatchSim, diff
    sc, cs, t, cost = _torch_problem()
    N, ps, nr = t["u"].shape[1], sc.task["pscale"], sc.nr
    sim = BatchSim(sc, batch=B)
    qt, qdt, ubar = diff.rollout_feedback(sim, t["q0"], t["qd0"], t["u"], h=sc.h, pscale=ps)
    xbar = torch.cat([qt, qdt], dim=-1)
    J0 = cost.value(xbar, ubar)
    lx, lu = cost.gradients(xbar, ubar)
    kfree = diff.lqr_backward(sim, lx, lu, cost.Q, cost.R, MU)[0]
    r = 0.5 * kfree.abs().reshape(-1, nr).median(dim=0).values
    ulo, uhi = ubar.reshape(-1, nr).min(dim=0).values - r, ubar.reshape(-1, nr).max(dim=0).values + r
    kff, K, expected, status, clamped = diff.lqr_backward_box(sim, lx, lu, cost.Q, cost.R, ubar, (ulo, uhi), MU)
    assert not status.any() and (expected > 0).all() and clamped.any() and K.shape == (B, N, 2 * nr, nr)
    xref = torch.cat([torch.cat([t["q0"], t["qd0"]], dim=-1).unsqueeze(1), xbar[:, :-1]], dim=1).contiguous()
    q1, qd1, u1 = diff.rollout_feedback(sim, t["q0"], t["qd0"], ubar, K, xref, h=sc.h, pscale=ps, ulim=(ulo, uhi))
    assert torch.equal(q1, qt) and torch.equal(qd1, qdt) and torch.equal(u1, ubar)      # alpha = 0: the nominal, bit for bit
    q2, qd2, u2 = diff.rollout_feedback(sim, t["q0"], t["qd0"], ubar + kff, K, xref, h=sc.h, pscale=ps, ulim=(ulo, uhi))
    assert "feedback,box" in sim.last_step_kernel()
    J1 = cost.value(torch.cat([q2, qd2], dim=-1), u2)
    print("J before %s\nJ after the full constrained step %s\nexpected decrease %s" % (J0.cpu().numpy(), J1.cpu().numpy(), expected.cpu().numpy()))
    assert (u2 >= ulo).all() and (u2 <= uhi).all() and ((u2 == ulo) | (u2 == uhi)).any()
    assert (J1 < J0).all()
    sim.close()


@pytest.mark.gpu
def test_ilqr_solve_with_torque_limits():
    import torch
    from redmax_amd import BatchSim, ilqr
    from test_gpu_ilqr import ITERS
    sc, cs, t, cost = _torch_problem()
    N, ps, nr = t["u"].shape[1], sc.task["pscale"], sc.nr
    sim = BatchSim(sc, batch=B)
    free, _ = ilqr.solve(sim, t["q0"], t["qd0"], t["u"], cost, iters=ITERS, h=sc.h, pscale=ps, backward="device")
    ulo = torch.quantile(free.u.reshape(-1, nr), 0.2, dim=0)
    uhi = torch.quantile(free.u.reshape(-1, nr), 0.8, dim=0)
    assert ((free.u < ulo) | (free.u > uhi)).any(dim=1).all()            # the unconstrained result violates them, in every rollout and DOF
    res, hist = ilqr.solve(sim, t["q0"], t["qd0"], t["u"], cost, iters=ITERS, h=sc.h, pscale=ps, backward="device", ulim=(ulo, uhi))
    h = hist.cpu().numpy()
    print("cost history per rollout under limits:\n%s\nunconstrained final cost %s" % (h, free.cost.cpu().numpy()))
    assert h.shape == (ITERS + 1, B) and (h[1:] <= h[:-1]).all() and (h[-1] < h[0]).any()
    assert (res.u >= ulo).all() and (res.u <= uhi).all() and ((res.u == ulo) | (res.u == uhi)).any()
    assert np.array_equal(res.cost.cpu().numpy(), h[-1])
    # the tape of the result belongs to result.u
    rng = np.random.default_rng(3)
    gq, gqd = rng.standard_normal((B, N, nr)), rng.standard_normal((B, N, nr))
    after_solve = sim.rollout_vjp(N, gq, gqd)
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, _ = sim.rollout_tape(N, sc.h, res.u.cpu().numpy(), pscale=ps)
    assert np.array_equal(qt, res.qtraj.cpu().numpy()) and np.array_equal(qdt, res.qdtraj.cpu().numpy())
    assert _same(after_solve, sim.rollout_vjp(N, gq, gqd))
    with pytest.raises(ValueError, match="backward='device'"):
        ilqr.solve(sim, t["q0"], t["qd0"], t["u"], cost, iters=1, h=sc.h, pscale=ps, backward="torch", ulim=(ulo, uhi))
    sim.close()


# ---------------------------------------------------------------- 5. refusals

@pytest.mark.gpu
def test_refusals_leave_the_tape_alone():
    from redmax_amd import BatchSim, _abi
    sc, cs, N = _setup(5)
    nr = sc.nr
    lx, lu, Q, R = _nominal(5)["cost"]
    ubar = np.ascontiguousarray(cs["u"])
    ulo, uhi = ubar.reshape(-1, nr).min(axis=0) - 0.1, ubar.reshape(-1, nr).max(axis=0) + 0.1
    rng = np.random.default_rng(11)
    gq, gqd = rng.standard_normal((B, N, nr)), rng.standard_normal((B, N, nr))
    sim = BatchSim(sc, batch=B)
    with pytest.raises(_abi.RedMaxHipError, match="rmx_rollout_lqr_box: no tape"):
        sim.rollout_lqr_box(N, lx, lu, Q, R, ubar, (ulo, uhi))
    _tape(sim, sc, cs)
    vjp0 = sim.rollout_vjp(N, gq, gqd)
    L, bt = sim._L, sim._batch
    kff, K = np.empty((B, N, nr)), np.empty((B, N, 2 * nr, nr))

    def call(nsteps=N, batch=bt, cost=True, out=True, box=True, per=0, mu=MU, max_iter=0, **null):
        p = dict(lx=lx, lu=lu, Q=Q, R=R, kff=kff, K=K, ubar=ubar, ulo=ulo, uhi=uhi)
        p.update(null)
        p = {k: (None if v is None else np.ascontiguousarray(v, dtype=np.float64)) for k, v in p.items()}
        p["kff"], p["K"] = (None if null.get("kff", 1) is None else kff), (None if null.get("K", 1) is None else K)
        ptr = {k: (None if v is None else v.ctypes.data) for k, v in p.items()}
        cst = _abi.LqrCost(ptr["lx"], ptr["lu"], ptr["Q"], ptr["R"], per, mu, None)
        gains = _abi.LqrGains(ptr["kff"], ptr["K"], None, None)
        bx = _abi.Box(ptr["ulo"], ptr["uhi"])
        rc = L.rmx_rollout_lqr_box(batch, nsteps, C.byref(cst) if cost else None, C.byref(bx) if box else None, ptr["ubar"], max_iter,
                                   C.byref(gains) if out else None, None)
        return rc, (L.rmx_last_error() or b"").decode()

    assert call()[0] == 0
    for kw in (dict(batch=None), dict(cost=False), dict(out=False), dict(box=False), dict(ubar=None), dict(lx=None), dict(lu=None), dict(Q=None),
               dict(R=None), dict(kff=None), dict(K=None)):
        rc, msg = call(**kw)
        assert rc != 0 and "rmx_rollout_lqr_box: null argument" in msg, (kw, msg)
    bad_lo = ulo.copy()
    bad_lo[3] = uhi[3] + 1
    nan_hi = uhi.copy()
    nan_hi[0] = np.nan
    for kw, words in ((dict(nsteps=N - 1), "nsteps differs"), (dict(per=2), "per_rollout"), (dict(mu=-1.0), "mu"), (dict(mu=float("nan")), "mu"),
                      (dict(mu=float("inf")), "mu"), (dict(max_iter=-1), "max_iter"), (dict(ulo=bad_lo), "ulo > uhi at DOF 3"),
                      (dict(uhi=nan_hi), "DOF 0 is NaN")):
        rc, msg = call(**kw)
        assert rc != 0 and words in msg, (kw, msg)
    d = [_DevArray(a) for a in (lx, lu, Q, R, ubar, bad_lo, uhi, kff, K)]
    with pytest.raises(_abi.RedMaxHipError, match="ulo > uhi at DOF 3"):                  # the device form reads the bounds back
        sim.rollout_lqr_box_device(N, *(a.ptr.value for a in d), mu=MU)
    for a in d:
        a.free()
    assert _same(vjp0, sim.rollout_vjp(N, gq, gqd))
    # a BDF2 tape
    sim.set_state(cs["q0"], cs["qd0"])
    sim.rollout_tape(N, sc.h, cs["u"], pscale=sc.task["pscale"], integrator=2)
    vjp2 = sim.rollout_vjp(N, gq, gqd)
    with pytest.raises(_abi.RedMaxHipError, match="BDF1 tape"):
        sim.rollout_lqr_box(N, lx, lu, Q, R, ubar, (ulo, uhi))
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
        sim.rollout_lqr_box(2, np.zeros((1, 2, 80)), np.zeros((1, 2, 40)), np.tile(np.eye(80), (2, 1, 1)), np.eye(40), c40["u"], (None, None))
    assert _same(vjp40, sim.rollout_vjp(2, g, g))
    sim.close()
