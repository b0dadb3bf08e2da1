"""rmx_rollout_linearize (include/redmax_hip.h) in numpy: the forward sensitivities of one taped solve, the BDF1 assembly of A_k, B_k
from them, and both backward recursions of rmx_rollout_vjp rewritten on them - a reference for the GPU tests that shares no code with
the library.

One taped solve x(qA, qB, u) solves g = M(x)(x - qB) - eta^2 (f(x, (x - qA)/eta) + pscale u) = 0, with H = dg/dx, dg/dqA = eta D,
dg/dqB = -M, dg/du = -eta^2 pscale I:
    XA = dx/dqA = -eta H^-1 D        XB = dx/dqB = H^-1 M        XU = dx/du = eta^2 pscale H^-1
BDF1 (qA = q_{k-1}, qB = q_{k-1} + h qdot_{k-1}, eta = h, qdot_k = (q_k - q_{k-1})/h), state order (q, qdot):
    A_k = [[XA + XB, h XB], [(XA + XB - I)/h, XB]]        B_k = [[XU], [XU/h]]
Backwards through one solve, with w = xbar + vbar/eta:  A = -vbar/eta + XA' w,  Bq = XB' w,  ubar = XU' w.
tests/test_rollout_linearize_proto.py checks all this against central differences of the oracle's step and against the two
recursions of tests/proto_rollout_vjp.py and tests/proto_rollout_vjp_bdf2.py.
"""
import numpy as np

AL = (2.0 - np.sqrt(2.0)) / 2.0


def sens(H, M, D, eta, pscale):
    """(XA, XB, XU) of one solve, [nr][nr] each with [i, j] = dx_i/d(.)_j; H, M, D may carry leading slot axes (eta then a scalar or
    an array over them)."""
    H, M, D = (np.asarray(a, dtype=np.float64) for a in (H, M, D))
    eta = np.asarray(eta, dtype=np.float64)[..., None, None]
    Hi = np.linalg.inv(H)
    return -eta * np.linalg.solve(H, D), np.linalg.solve(H, M), eta * eta * pscale * Hi


def etas(nsteps, h, integrator):
    """eta of every slot of a tape: [nsteps] under BDF1, [nsteps + 1] under BDF2 (slots 0 and nsteps: the SDIRK2 solves)."""
    if integrator == 1:
        return np.full(nsteps, h)
    e = np.full(nsteps + 1, 2.0 * h / 3.0)
    e[0] = e[nsteps] = AL * h
    return e


def assemble_bdf1(XA, XB, XU, h):
    """(A, Bm): [..][2nr][2nr] and [..][2nr][nr] from [..][nr][nr] sensitivities of BDF1 slots."""
    XA, XB, XU = (np.asarray(a, dtype=np.float64) for a in (XA, XB, XU))
    S = XA + XB
    eye = np.eye(XA.shape[-1])
    A = np.concatenate([np.concatenate([S, h * XB], axis=-1), np.concatenate([(S - eye) / h, XB], axis=-1)], axis=-2)
    return A, np.concatenate([XU, XU / h], axis=-2)


def chain_bdf1(A, Bm, gq, gqd):
    """The backward chain lam_k = (gq_k, gqd_k) + A_{k+1}' lam_{k+1}, du_k = B_k' lam_k, (dq0, dqd0) = A_1' lam_1 of one rollout:
    A [N][2nr][2nr], Bm [N][2nr][nr], gq, gqd [N][nr] -> (du[N][nr], dq0[nr], dqd0[nr])."""
    N, nr = gq.shape
    du = np.empty((N, nr))
    lam = np.zeros(2 * nr)
    for k in range(N, 0, -1):
        lam = np.concatenate([gq[k - 1], gqd[k - 1]]) + lam
        du[k - 1] = Bm[k - 1].T @ lam
        lam = A[k - 1].T @ lam
    return du, lam[:nr], lam[nr:]


def _solve_bwd_x(XA, XB, XU, eta, xbar, vbar):
    w = xbar + vbar / eta
    return -vbar / eta + XA.T @ w, XB.T @ w, XU.T @ w


def vjp_bdf2(XA, XB, XU, gq, gqd, h):
    """proto_rollout_vjp_bdf2.vjp on the sensitivities of its N + 1 slots (pscale is inside XU): (du[N][nr], dq0[nr], dqd0[nr])."""
    N, nr = gq.shape
    qbar = np.vstack([np.zeros((1, nr)), gq])
    vbar = np.vstack([np.zeros((1, nr)), gqd])
    du = np.empty((N, nr))
    eta = 2.0 * h / 3.0
    for k in range(N - 1, 0, -1):
        A, Bq, ub = _solve_bwd_x(XA[k], XB[k], XU[k], eta, qbar[k + 1], vbar[k + 1])
        du[k] = ub
        s = A + Bq
        qbar[k] += 4.0 / 3.0 * s
        vbar[k] += 8.0 / 9.0 * h * Bq
        qbar[k - 1] -= 1.0 / 3.0 * s
        vbar[k - 1] -= 2.0 / 9.0 * h * Bq
    eta = AL * h
    A, Bq, ubb = _solve_bwd_x(XA[0], XB[0], XU[0], eta, qbar[1], vbar[1])
    qbar[0] += A + Bq
    vbar[0] += (2.0 * AL - 1.0) * h * Bq
    qdabar = (1.0 - AL) * h * A + 2.0 * (1.0 - AL) * h * Bq
    A2, B2, uba = _solve_bwd_x(XA[N], XB[N], XU[N], eta, np.zeros(nr), qdabar)
    qbar[0] += A2 + B2
    vbar[0] += AL * h * B2
    du[0] = uba + ubb
    return du, qbar[0], vbar[0]


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))
