"""tests/proto_lqr_backward.py on the CPU: the extended-precision recursion meets redmax_amd.ilqr.backward_pass, the structured
(nr x nr block) identities of the kernel's algebra meet the dense products, the gain table's layout, the zeros of a flagged rollout.

Tolerances.  backward_pass is a float64 evaluation whose error is eps * cond(Quu) times a modest growth factor; the problems are
drawn so that cond(Quu) stays below 1e6 (printed, asserted), eps * 1e6 = 2e-10, and 1e-8 leaves two decades.  The identities are
compared in longdouble (eps 1.1e-19): the largest intermediate is |Vvv|/h^2 = 1e4 |Vvv|, so 1e-13 of the result's largest entry
leaves two decades as well.
"""
import numpy as np
import pytest
import torch

import proto_lqr_backward as P
from test_ilqr_backward import _problem as linear_problem, _roll, N as LN, BATCH as LB

LD = np.longdouble
H = 0.01


def structured_problem(seed, nr=4, N=5):
    """Random S, XB, XU of the sizes a BDF1 step has at h = 0.01 (S - I of order h, XB a contraction, XU of order h^2 pscale) and a
    quadratic cost: (S, X, U [N][nr][nr], lx, lu, Q, R)."""
    rng = np.random.default_rng(seed)
    eye = np.eye(nr)
    S = eye + 0.01 * rng.standard_normal((N, nr, nr))
    X = 0.9 * eye + 0.05 * rng.standard_normal((N, nr, nr))
    U = 1e-3 * (eye + 0.3 * rng.standard_normal((N, nr, nr)))
    Q = np.tile(np.diag([1.0] * nr + [0.01] * nr), (N, 1, 1))
    R = 0.1 * eye
    return S, X, U, rng.standard_normal((N, 2 * nr)), rng.standard_normal((N, nr)), Q, R


def _assemble_all(S, X, U):
    AB = [P.assemble(S[k], X[k], U[k], H) for k in range(S.shape[0])]
    return np.array([a for a, _ in AB]), np.array([b for _, b in AB])


def _compare(A, Bm, lx, lu, Q, R, mu, tag):
    """Q [N][.][.] for the batch, or [B][N][.][.]: then one backward_pass call per rollout, each with its own table."""
    t = lambda a: torch.tensor(a, dtype=torch.float64)      # noqa: E731
    if np.ndim(Q) == 4:
        for b in range(A.shape[0]):
            _compare(A[b:b + 1], Bm[b:b + 1], lx[b:b + 1], lu[b:b + 1], Q[b], R, mu, "%s, table %d" % (tag, b))
        return
    kff, K, expected = (a.numpy() for a in ilqr_backward(t(A), t(Bm), t(lx), t(lu), t(Q), t(R), mu))
    for b in range(A.shape[0]):
        ek, eK, ee, notpd, cond = P.backward_pass_ext(A[b], Bm[b], lx[b], lu[b], Q, R, mu)
        errs = (P.rel_err(kff[b], ek), P.rel_err(K[b], eK), P.rel_err(expected[b], ee))
        print("%s b %d: cond(Quu) %.3e, backward_pass against longdouble: kff %.3e K %.3e expected %.3e" % ((tag, b, cond) + errs))
        assert not notpd and cond < 1e6
        assert max(errs) < 1e-8


def ilqr_backward(*a):
    from redmax_amd.ilqr import backward_pass
    return backward_pass(*a)


@pytest.mark.parametrize("seed", [1, 2])
def test_extended_recursion_meets_backward_pass_on_the_random_linear_problem(seed):
    A, Bm, c, Q, R, xg, x0, ubar = linear_problem(seed)
    xbar = np.array([_roll(A[b], Bm[b], c[b], x0[b], lambda k, x: ubar[b, k])[0] for b in range(LB)])
    lx = np.einsum("kij,bkj->bki", Q, xbar - xg)
    lu = np.einsum("ij,bkj->bki", R, ubar)
    assert A.shape[1] == LN
    _compare(A, Bm, lx, lu, Q, R, 0.0, "linear seed %d" % seed)


@pytest.mark.parametrize("seed", [11, 12])
def test_extended_recursion_meets_backward_pass_on_a_structured_problem(seed):
    S, X, U, lx, lu, Q, R = structured_problem(seed)
    A, Bm = _assemble_all(S, X, U)
    _compare(A[None], Bm[None], lx[None], lu[None], Q, R, 1e-6, "structured seed %d" % seed)


@pytest.mark.parametrize("form", ["z", "w"])
def test_structured_identities_meet_the_dense_products(form):
    S, X, U, lx, lu, Q, R = structured_problem(21, nr=5)
    rng = np.random.default_rng(22)
    nr = 5
    G = rng.standard_normal((2 * nr, 2 * nr))
    Vxx = (G @ G.T).astype(LD)
    Vx = rng.standard_normal(2 * nr).astype(LD)
    A, Bm = P.assemble(S[0], X[0], U[0], H, dtype=LD)
    dense = (A.T @ Vx, Bm.T @ Vx, A.T @ Vxx @ A, Bm.T @ Vxx @ A, Bm.T @ Vxx @ Bm)
    got = (P.structured_step if form == "z" else P.structured_step_w)(S[0], X[0], U[0], H, Vx, Vxx)
    for name, g, d in zip(("Qx", "B'Vx", "Qxx", "Qux", "B'VxxB"), got, dense):
        e = P.rel_err(g, d)
        print("%s form, %s: %.3e" % (form, name, e))
        assert g.shape == d.shape and e < 1e-13


def test_the_w_form_loses_digits_in_float64_where_the_z_form_does_not():
    """Why the kernel forms Z = (S - I)/h: in float64 the W-only Qxx carries an absolute error of eps |Vvv|/h^2."""
    S, X, U, lx, lu, Q, R = structured_problem(31, nr=5)
    rng = np.random.default_rng(32)
    G = rng.standard_normal((10, 10))
    Vxx, Vx = G @ G.T, rng.standard_normal(10)
    A, Bm = P.assemble(S[0], X[0], U[0], H, dtype=LD)
    ref = A.T @ Vxx.astype(LD) @ A
    ez = P.rel_err(P.structured_step(S[0], X[0], U[0], H, Vx, Vxx, dtype=np.float64)[2], ref)
    ew = P.rel_err(P.structured_step_w(S[0], X[0], U[0], H, Vx, Vxx, dtype=np.float64)[2], ref)
    print("float64 Qxx against longdouble: Z form %.3e, W form %.3e" % (ez, ew))
    assert ez < 64 * np.finfo(np.float64).eps      # (a handful of roundings of entries the size of the result)
    assert ew > ez


def test_gain_table_layout_is_the_transpose():
    rng = np.random.default_rng(5)
    nr = 3
    K = rng.standard_normal((2, 4, nr, 2 * nr))
    T = P.to_feedback_layout(K)
    assert T.shape == (2, 4, 2 * nr, nr) and T.flags["C_CONTIGUOUS"]
    flat = T.reshape(2, 4, -1)
    for i in range(nr):
        for j in range(2 * nr):
            assert np.array_equal(flat[:, :, j * nr + i], K[:, :, i, j])
    # the feedback law with the table as rollout_feedback reads it: u_i = sum_j T[j, i] dx_j
    dx = rng.standard_normal(2 * nr)
    assert np.allclose(T[0, 0].T @ dx, K[0, 0] @ dx, rtol=0, atol=1e-15)


def test_flagged_rollout_is_all_zeros():
    S, X, U, lx, lu, Q, R = structured_problem(41)
    A, Bm = _assemble_all(S, X, U)
    ok = P.backward_pass_ext(A, Bm, lx, lu, Q, R, 1e-6)
    assert not ok[3] and np.abs(ok[0]).max() > 0 and ok[2] > 0
    Qbad = Q.copy()
    c = 2 * np.linalg.eigvalsh(R).max() / np.linalg.eigvalsh(Bm[-1].T @ Bm[-1]).min()
    Qbad[-1] = -c * np.eye(Q.shape[1])      # R + B_N'Q_N B_N = R - c B_N'B_N is negative definite
    assert np.linalg.eigvalsh(R + Bm[-1].T @ Qbad[-1] @ Bm[-1]).max() < 0
    kff, K, expected, notpd, _ = P.backward_pass_ext(A, Bm, lx, lu, Qbad, R, 1e-6)
    assert notpd and expected == 0 and not kff.any() and not K.any()
    assert kff.shape == ok[0].shape and K.shape == ok[1].shape


# ---------------------------------------------------------------- the cost families of proto_lqr_backward

def _structured_batch(seed, nr, N, B):
    """B structured problems with differing S, X, U, lx, lu: (A [B][N][2nr][2nr], Bm, lx, lu)."""
    out = []
    for b in range(B):
        S, X, U, lx, lu, _, _ = structured_problem(seed + 100 * b, nr=nr, N=N)
        out.append(_assemble_all(S, X, U) + (lx, lu))
    return tuple(np.array(a) for a in zip(*out))


def test_dense_cost_is_what_it_says():
    Q, R = P.dense_cost(3, 4, 5, B=3)
    assert Q.shape == (3, 5, 8, 8) and R.shape == (4, 4)
    assert np.array_equal(Q, Q.swapaxes(-1, -2)) and np.array_equal(R, R.T)      # exactly symmetric: row-major is column-major
    lam = np.linalg.eigvalsh(Q)
    for k in range(5):
        assert np.allclose(lam[:, k, 0], 1e-2 * (0.5 + k), rtol=1e-10) and np.allclose(lam[:, k, -1], 0.5 + k, rtol=1e-10)
    assert np.allclose(np.linalg.eigvalsh(R)[[0, -1]], (0.03, 0.3), rtol=1e-10)
    assert np.abs(Q[:, :, :4, 4:]).min() > 0 and np.abs(R).min() > 0               # a full q-qdot block, no zero anywhere
    tables = Q.reshape(15, -1)
    assert all(np.abs(tables[i] - tables[j]).min() > 0 for i in range(15) for j in range(i))      # no two tables share an entry
    Q1, R1 = P.dense_cost(3, 4, 5)
    assert Q1.shape == (5, 8, 8) and np.array_equal(R1, R) and np.array_equal(Q1, Q[0])
    assert P.dense_cost(3, 1, 2)[1].shape == (1, 1)


@pytest.mark.parametrize("nr", [1, 2, 3, 5, 11, 16, 32])
def test_extended_recursion_meets_backward_pass_on_dense_costs(nr):
    """Dense SPD Q_k that differ per step (and per rollout) and a dense SPD R on structured_problem's S, X, U: every entry of the
    tables enters, the q-qdot block included."""
    N, nb = 4, 2
    A, Bm, lx, lu = _structured_batch(200 + nr, nr, N, nb)
    Q, R = P.dense_cost(300 + nr, nr, N)
    _compare(A, Bm, lx, lu, Q, R, 1e-6, "dense nr %d" % nr)
    Qb, Rb = P.dense_cost(400 + nr, nr, N, B=nb)
    _compare(A, Bm, lx, lu, Qb, Rb, 1e-6, "dense per rollout nr %d" % nr)


def _indefinite_problem(nr, N=6):
    A, Bm, lx, lu = (a[0] for a in _structured_batch(500 + nr, nr, N, 1))
    Q, R = P.dense_cost(600 + nr, nr, N)
    return A, Bm, lx, lu, Q, R


@pytest.mark.parametrize("nr", [2, 5, 11])
def test_indefinite_at_stops_the_recursion_at_its_step_behind_a_good_pivot(nr):
    A, Bm, lx, lu, Q, R = _indefinite_problem(nr)
    N, mu = Q.shape[0], 1e-6
    s = N // 2
    Q0 = Q.copy()
    base = P.backward_pass_ext(A, Bm, lx, lu, Q, R, mu, flag=True)
    assert not base[3] and base[5] is None
    Qi, c = P.indefinite_at(A, Bm, lx, lu, Q, R, mu, s)
    assert np.array_equal(Q, Q0) and np.array_equal(Qi, Qi.swapaxes(-1, -2))
    assert all(np.array_equal(Qi[k], Q[k]) for k in range(N) if k != s) and not np.array_equal(Qi[s], Q[s])
    kff, K, expected, notpd, cond, where = P.backward_pass_ext(A, Bm, lx, lu, Qi, R, mu, flag=True)
    print("nr %d: c = %g, stopped at (step, pivot) = %s" % (nr, c, where))
    assert notpd and where[0] == s and where[1] >= 1
    assert not kff.any() and not K.any() and expected == 0 and kff.shape == base[0].shape and K.shape == base[1].shape
    # the margin: half of c still stops it there, behind the untouched first pivot
    half = Q.copy()
    half[s] = Q[s] - 0.5 * (Q[s] - Qi[s])
    w_half = P.backward_pass_ext(A, Bm, lx, lu, half, R, mu, flag=True)[5]
    assert w_half is not None and w_half[0] == s and w_half[1] >= 1
    # an untouched rollout next to it is unchanged: per-rollout tables [Q, Q', Q], rollouts 0 and 2 against the call before
    for Qb in (Q, Qi, Q):
        again = P.backward_pass_ext(A, Bm, lx, lu, Qb, R, mu)
        want = base if Qb is Q else (kff, K, expected, True)
        assert all(np.array_equal(g, w) for g, w in zip(again[:4], want[:4]))


@pytest.mark.parametrize("nr", [2, 5, 11])
def test_rescue_mu_makes_the_indefinite_problem_positive_definite_again(nr):
    A, Bm, lx, lu, Q, R = _indefinite_problem(nr)
    Qi, c = P.indefinite_at(A, Bm, lx, lu, Q, R, 1e-6, Q.shape[0] // 2)
    mu, rounds = P.rescue_mu(A, Bm, lx, lu, Qi, R, 1e-6)
    out = P.backward_pass_ext(A, Bm, lx, lu, Qi, R, mu, flag=True)
    print("nr %d: c = %g, mu = %.6g after %d quadruplings, cond(Quu) %.3e" % (nr, c, mu, rounds, out[4]))
    assert not out[3] and out[5] is None and np.abs(out[0]).max() > 0
    assert P.backward_pass_ext(A, Bm, lx, lu, Qi, R, mu / 4)[3] is False      # the margin: a quarter of it passes too
    _compare(A[None], Bm[None], lx[None], lu[None], Qi, R, mu, "rescued nr %d" % nr)


@pytest.mark.parametrize("seed", [1, 2])
def test_quu0_and_quu0_plus_mu_keep_their_places_where_mu_decides(seed):
    """mu of the size of Quu0 on the random linear problem with a dense cost.  The KKT helper of test_ilqr_backward cannot carry mu:
    R + mu I in its place is the minimiser of ANOTHER cost, whose value function is Qxx - Qux'(Quu0 + mu I)^-1 Qux, while the
    recursion's Vx, Vxx and ``expected`` are those of the true cost under the regularised gains (Quu0 there, Quu0 + mu I in the solve
    alone).  So: the longdouble recursion against backward_pass under the file's rule, and against a statement that shares nothing
    with either - on a linear system ``expected`` IS the decrease of J under u = ubar + k + K dx, rolled out here in float64.  Were
    Quu0 + mu I used in ``expected`` or in Vx it would be off by about mu |k|^2 / 2, printed and asserted to be no rounding matter."""
    A, Bm, c, _, _, xg, x0, ubar = linear_problem(seed)
    Q, R = P.dense_cost(700 + seed, Bm.shape[-1], LN)
    xbar = np.array([_roll(A[b], Bm[b], c[b], x0[b], lambda k, x: ubar[b, k])[0] for b in range(LB)])
    lx = np.einsum("kij,bkj->bki", Q, xbar - xg)
    lu = np.einsum("ij,bkj->bki", R, ubar)
    mu = float(np.linalg.eigvalsh(R + Bm[0, -1].T @ Q[-1] @ Bm[0, -1]).max())
    _compare(A, Bm, lx, lu, Q, R, mu, "linear, dense cost, mu %.3g, seed %d" % (mu, seed))
    from test_ilqr_backward import _cost
    for b in range(LB):
        ek, eK, ee, notpd, cond = P.backward_pass_ext(A[b], Bm[b], lx[b], lu[b], Q, R, mu)
        k64, K64 = ek.astype(np.float64), eK.astype(np.float64)
        xstart = np.concatenate([x0[b][None], xbar[b, :-1]])
        x, u = _roll(A[b], Bm[b], c[b], x0[b], lambda k, xp: ubar[b, k] + k64[k] + K64[k] @ (xp - xstart[k]))
        dJ = _cost(Q, R, xg[b], xbar[b], ubar[b]) - _cost(Q, R, xg[b], x, u)
        slip = 0.5 * mu * float((k64 * k64).sum())
        print("seed %d b %d: mu %.3g, decrease %.6e, expected %.6e, mu |k|^2 / 2 = %.3e" % (seed, b, mu, dJ, float(ee), slip))
        assert dJ > 0 and abs(dJ - float(ee)) <= 1e-8 * dJ
        assert slip > 1e-3 * dJ
