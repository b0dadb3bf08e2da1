"""tests/proto_lqr_box.py pinned on the CPU: the box QP meets the KKT conditions, infinite bounds give proto_lqr_backward's recursion
exactly, clamped DOFs have zero gain rows, ``expected`` is the decrease of the quadratic model along the constrained step, and the
cap on the iterations is reported as status 2."""
import numpy as np
import pytest

import proto_lqr_backward as P
import proto_lqr_box as PB

LD = P.LD
EPS = float(np.finfo(np.float64).eps)


def _problem(rng, d, finite=0.7):
    """A random SPD problem whose unconstrained minimiser leaves the box in most DOFs; bounds mixed finite / infinite."""
    H = P._spd(rng, d, 0.03, 30.0)
    g = rng.standard_normal(d) * 3
    x0 = -np.linalg.solve(H, g)
    w = np.abs(x0) * rng.uniform(0.1, 0.6, d) + 0.01
    lo, hi = -w * rng.uniform(0.2, 1.0, d), w * rng.uniform(0.2, 1.0, d)
    lo[rng.uniform(size=d) > finite] = -np.inf
    hi[rng.uniform(size=d) > finite] = np.inf
    return H, g, lo, hi


@pytest.mark.parametrize("d", [1, 2, 3, 8, 32])
def test_box_qp_meets_the_kkt_conditions(d):
    rng = np.random.default_rng(100 + d)
    clamped = iters = 0
    for _ in range(40 if d < 32 else 12):
        H, g, lo, hi = _problem(rng, d)
        x, c, status, it = PB.box_qp(H, g, lo, hi)
        assert status == 0 and it <= 20
        x64, c64, st64, _ = PB.box_qp(H, g, lo, hi, dtype=np.float64)
        assert st64 == 0 and x64.dtype == np.float64
        grad = g.astype(LD) + H.astype(LD) @ x
        scale = float(np.abs(g).max() + np.abs(H).max() * np.abs(x).max())
        assert (x >= lo).all() and (x <= hi).all()                                 # feasible
        assert np.abs(grad[~c]).max(initial=0) <= 1e3 * float(np.finfo(LD).eps) * scale * d      # the free gradient is zero to rounding
        at_lo, at_hi = c & (x == lo), c & (x == hi)
        assert (at_lo | at_hi)[c].all() and (grad[at_lo] > 0).all() and (grad[at_hi] < 0).all()   # multipliers of the right sign
        assert ((x[~c] > lo[~c]) & (x[~c] < hi[~c])).all() or np.abs(grad[~c]).max(initial=0) <= 1e-12 * scale
        clamped += int(c.sum())
        iters += it
    assert clamped > 0
    print("d %d: %d clamped DOFs, %.2f iterations on average" % (d, clamped, iters / (40 if d < 32 else 12)))


def _linear_problem(seed, nr=3, N=5):
    """A random linear system x_k = A x_{k-1} + B u_k with the structure of the taped rollout and a dense quadratic cost."""
    rng = np.random.default_rng(seed)
    h = 0.05
    S = np.eye(nr) + 0.1 * rng.standard_normal((N, nr, nr))
    X = 0.5 * np.eye(nr) + 0.1 * rng.standard_normal((N, nr, nr))
    U = h * h * (np.eye(nr) + 0.1 * rng.standard_normal((N, nr, nr)))
    A, Bm = zip(*(P.assemble(S[k], X[k], U[k], h) for k in range(N)))
    Q, R = P.dense_cost(seed, nr, N)
    x0 = rng.standard_normal(2 * nr)
    ubar = rng.standard_normal((N, nr))
    xg = rng.standard_normal((N, 2 * nr))
    return np.array(A), np.array(Bm), Q, R, x0, ubar, xg


def _rollout(A, Bm, x0, u):
    x, out = np.asarray(x0, dtype=LD), []
    for k in range(len(u)):
        x = A[k].astype(LD) @ x + Bm[k].astype(LD) @ u[k]
        out.append(x)
    return np.array(out)


def _cost(Q, R, xg, x, u):
    dx = x - xg
    return sum(dx[k] @ Q[k].astype(LD) @ dx[k] / 2 + u[k] @ R.astype(LD) @ u[k] / 2 for k in range(len(u)))


def _gradients(Q, R, xg, x, u):
    return np.einsum("kij,kj->ki", Q.astype(LD), x - xg), np.einsum("ij,kj->ki", R.astype(LD), u)


def test_infinite_bounds_reproduce_the_unconstrained_recursion_exactly():
    A, Bm, Q, R, x0, ubar, xg = _linear_problem(3)
    x = _rollout(A, Bm, x0, ubar.astype(LD))
    lx, lu = _gradients(Q, R, xg, x, ubar.astype(LD))
    ref = P.backward_pass_ext(A, Bm, lx, lu, Q, R, 1e-6)
    for ulo, uhi in ((None, None), (np.full(3, -np.inf), np.full(3, np.inf)), (None, np.full(3, np.inf))):
        got = PB.backward_pass_box(A, Bm, lx, lu, Q, R, ubar, ulo, uhi, 1e-6)
        assert got["status"] == 0 and not got["clamped"].any()
        assert np.array_equal(got["kff"], ref[0]) and np.array_equal(got["K"], ref[1]) and got["expected"] == ref[2]
        assert (got["iters"] == 2).all()      # one Newton step, and the iteration that sees it was a full one


def test_a_clamped_dof_has_a_zero_gain_row_and_sits_on_its_bound():
    A, Bm, Q, R, x0, ubar, xg = _linear_problem(4)
    x = _rollout(A, Bm, x0, ubar.astype(LD))
    lx, lu = _gradients(Q, R, xg, x, ubar.astype(LD))
    free = PB.backward_pass_box(A, Bm, lx, lu, Q, R, ubar, None, None, 1e-6)
    r = 0.5 * np.median(np.abs(free["kff"].astype(np.float64)), axis=0)
    ulo, uhi = ubar.min(axis=0) - r, ubar.max(axis=0) + r
    got = PB.backward_pass_box(A, Bm, lx, lu, Q, R, ubar, ulo, uhi, 1e-6)
    assert got["status"] == 0 and got["c"].any() and not got["c"].all()
    for s in range(len(ubar)):
        for i in range(3):
            if got["c"][s, i]:
                assert not got["K"][s, i].any()
                assert got["kff"][s, i] in (LD(ulo[i]) - LD(ubar[s, i]), LD(uhi[i]) - LD(ubar[s, i]))
                assert got["clamped"][s] >> i & 1
            else:
                assert got["K"][s, i].any() and not got["clamped"][s] >> i & 1
    u = ubar + got["kff"]
    assert (u >= ulo - 1e-15).all() and (u <= uhi + 1e-15).all()


def test_expected_is_the_decrease_of_the_quadratic_model_along_the_constrained_step():
    """On a linear system with a quadratic cost the model is the cost.  The constrained step applied in closed loop,
    u_k = ubar_k + k_k + K_k (x_{k-1} - xbar_{k-1}), lowers J by ``expected`` exactly; and because every step's QP is solved exactly
    and the constrained value function is the true one only where the set does not change with the state, the result is also
    checked against a dense solve of the whole constrained problem over the torques of the LAST step, where it IS exact."""
    A, Bm, Q, R, x0, ubar, xg = _linear_problem(5)
    N = len(ubar)
    xbar = _rollout(A, Bm, x0, ubar.astype(LD))
    lx, lu = _gradients(Q, R, xg, xbar, ubar.astype(LD))
    free = PB.backward_pass_box(A, Bm, lx, lu, Q, R, ubar, None, None, 0.0)
    r = 0.5 * np.median(np.abs(free["kff"].astype(np.float64)), axis=0)
    ulo, uhi = ubar.min(axis=0) - r, ubar.max(axis=0) + r
    got = PB.backward_pass_box(A, Bm, lx, lu, Q, R, ubar, ulo, uhi, 0.0)
    assert got["status"] == 0 and got["c"].any()
    x, xs, us = np.asarray(x0, dtype=LD), [], []
    for k in range(N):
        xprev = np.asarray(x0, dtype=LD) if k == 0 else xbar[k - 1]
        u = ubar[k] + got["kff"][k] + got["K"][k] @ (x - xprev)
        x = A[k].astype(LD) @ x + Bm[k].astype(LD) @ u
        xs.append(x)
        us.append(u)
    J0, J1 = _cost(Q, R, xg, xbar, ubar.astype(LD)), _cost(Q, R, xg, np.array(xs), np.array(us))
    assert abs((J0 - J1) - got["expected"]) <= 1e-15 * abs(J0)
    assert got["expected"] > 0 and got["expected"] < free["expected"]      # the limits cost some of the unconstrained decrease
    # the last step alone, dense: min over u_N in the box of the cost of x_N = A x_{N-1} + B u_N, at x_{N-1} = xbar_{N-1}
    Bn, Qn = Bm[N - 1].astype(LD), Q[N - 1].astype(LD)
    H = R.astype(LD) + Bn.T @ Qn @ Bn
    H = (H + H.T) / 2
    g = lu[N - 1] + Bn.T @ lx[N - 1]
    lo, hi = LD(1) * ulo - ubar[N - 1], LD(1) * uhi - ubar[N - 1]
    best = None
    for pattern in range(3 ** 3):      # every assignment of (free, at lo, at hi) to the three DOFs: the dense constrained solve
        kind = [(pattern // 3 ** i) % 3 for i in range(3)]
        f = np.array([t == 0 for t in kind])
        xk = np.array([0 if t == 0 else (lo[i] if t == 1 else hi[i]) for i, t in enumerate(kind)], dtype=LD)
        if f.any():
            xk[f] = -np.linalg.solve((H[np.ix_(f, f)]).astype(np.float64), (g[f] + H[np.ix_(f, ~f)] @ xk[~f]).astype(np.float64))
        if (xk >= lo - 1e-12).all() and (xk <= hi + 1e-12).all():
            v = g @ xk + xk @ H @ xk / 2
            best = (v, xk) if best is None or v < best[0] else best
    assert np.abs(best[1] - got["kff"][N - 1]).max() <= 1e-9 * max(1.0, float(np.abs(best[1]).max()))


def test_max_iter_one_on_a_problem_that_needs_more_gives_status_2():
    rng = np.random.default_rng(8)
    H, g, lo, hi = _problem(rng, 8, finite=1.0)
    x, c, status, it = PB.box_qp(H, g, lo, hi)
    assert status == 0 and it > 1
    assert PB.box_qp(H, g, lo, hi, max_iter=1)[2] == 2
    A, Bm, Q, R, x0, ubar, xg = _linear_problem(6)
    xbar = _rollout(A, Bm, x0, ubar.astype(LD))
    lx, lu = _gradients(Q, R, xg, xbar, ubar.astype(LD))
    got = PB.backward_pass_box(A, Bm, lx, lu, Q, R, ubar, None, None, 1e-6, max_iter=1)
    assert got["status"] == 2 and not got["kff"].any() and not got["K"].any() and got["expected"] == 0 and not got["clamped"].any()


def test_a_pivot_that_is_not_positive_gives_status_1():
    H = np.array([[1.0, 2.0], [2.0, 1.0]])
    assert PB.box_qp(H, np.array([1.0, 1.0]), np.full(2, -1.0), np.full(2, 1.0))[2] == 1


def test_the_float64_run_agrees_with_the_extended_run_to_rounding():
    A, Bm, Q, R, x0, ubar, xg = _linear_problem(7, nr=5, N=6)
    xbar = _rollout(A, Bm, x0, ubar.astype(LD))
    lx, lu = (a.astype(np.float64) for a in _gradients(Q, R, xg, xbar, ubar.astype(LD)))
    free = PB.backward_pass_box(A, Bm, lx, lu, Q, R, ubar, None, None, 1e-6)
    r = 0.5 * np.median(np.abs(free["kff"].astype(np.float64)), axis=0)
    ulo, uhi = ubar.min(axis=0) - r, ubar.max(axis=0) + r
    ext = PB.backward_pass_box(A, Bm, lx, lu, Q, R, ubar, ulo, uhi, 1e-6)
    f64 = PB.backward_pass_box(A, Bm, lx, lu, Q, R, ubar, ulo, uhi, 1e-6, dtype=np.float64)
    assert f64["kff"].dtype == np.float64 and np.array_equal(ext["clamped"], f64["clamped"]) and ext["clamped"].any()
    assert P.rel_err(f64["kff"], ext["kff"]) < 1e-10 and P.rel_err(f64["K"], ext["K"]) < 1e-10
