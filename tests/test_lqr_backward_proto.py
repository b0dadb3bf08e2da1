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
    t = lambda a: torch.tensor(a, dtype=torch.float64)      # noqa: E731
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
