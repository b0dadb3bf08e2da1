"""The forward recursions of rmx_rollout_jvp (include/redmax_hip.h) in numpy, on the oracle's tape: a reference for the GPU tests that
shares no code with the library.

Every taped solve is x(qA, qB, u) with dg/dx = H, dg/dqA = eta D, dg/dqB = -M, dg/du = -eta^2 pscale I, so tangents go through it as
    solve_fwd(H, M, D, eta; dqA, dqB, du):   H dx = -eta D dqA + M dqB + eta^2 pscale du ;   dv = (dx - dqA)/eta
BDF1 (eta = h, slot k-1 is step k), from (dq_0, dqd_0) = (tq0, tqd0):
    (dq_k, dqd_k) = solve_fwd(slot k-1; dq_{k-1}, dq_{k-1} + h dqd_{k-1}, tu_k)
BDF2 (al = (2 - sqrt 2)/2; slots 0 and N: eta = al h, the others 2h/3; tu_1 holds for both start solves):
    SDIRK2a (slot N): (dqa, dqda)   = solve_fwd(dq0, dq0 + al h dqd0, tu_1)
    SDIRK2b (slot 0): (dq_1, dqd_1) = solve_fwd(dq0 + (1-al) h dqda, dq0 + (2al-1) h dqd0 + 2(1-al) h dqda, tu_1)
    BDF2    (slot k): dqA = 4/3 dq_k - 1/3 dq_{k-1} ; dqB = dqA + 8/9 h dqd_k - 2/9 h dqd_{k-1} ; -> (dq_{k+1}, dqd_{k+1})
The tapes are those of tests/proto_rollout_vjp.py (tape) and tests/proto_rollout_vjp_bdf2.py (forward).
tests/test_rollout_jvp_proto.py checks all this against central differences of the oracle's rollout and against the two backward
recursions.
"""
import numpy as np

AL = (2.0 - np.sqrt(2.0)) / 2.0


def solve_fwd(H, M, D, eta, pscale, dqA, dqB, du):
    dx = np.linalg.solve(H, -eta * (D @ dqA) + M @ dqB + eta * eta * pscale * du)
    return dx, (dx - dqA) / eta


def _zeros(a, shape):
    return np.zeros(shape) if a is None else np.asarray(a, dtype=np.float64)


def jvp_bdf1(H, M, D, h, pscale, tu=None, tq0=None, tqd0=None):
    """One direction on a BDF1 tape of N slots: (tq[N][nr], tqd[N][nr]); a None input is zero."""
    N, nr = H.shape[0], H.shape[1]
    tu, dq, dqd = _zeros(tu, (N, nr)), _zeros(tq0, nr), _zeros(tqd0, nr)
    tq, tqd = np.empty((N, nr)), np.empty((N, nr))
    for k in range(1, N + 1):
        dq, dqd = solve_fwd(H[k - 1], M[k - 1], D[k - 1], h, pscale, dq, dq + h * dqd, tu[k - 1])
        tq[k - 1], tqd[k - 1] = dq, dqd
    return tq, tqd


def jvp_bdf2(H, M, D, h, pscale, tu=None, tq0=None, tqd0=None):
    """One direction on a BDF2 tape of N + 1 slots (slot N: the SDIRK2a solve): (tq[N][nr], tqd[N][nr]); a None input is zero."""
    N, nr = H.shape[0] - 1, H.shape[1]
    tu, dq0, dqd0 = _zeros(tu, (N, nr)), _zeros(tq0, nr), _zeros(tqd0, nr)
    tq, tqd = np.empty((N, nr)), np.empty((N, nr))
    eta = AL * h
    _, dqda = solve_fwd(H[N], M[N], D[N], eta, pscale, dq0, dq0 + AL * h * dqd0, tu[0])
    tq[0], tqd[0] = solve_fwd(H[0], M[0], D[0], eta, pscale, dq0 + (1.0 - AL) * h * dqda,
                              dq0 + (2.0 * AL - 1.0) * h * dqd0 + 2.0 * (1.0 - AL) * h * dqda, tu[0])
    eta = 2.0 * h / 3.0
    pq, pqd = dq0, dqd0
    for k in range(1, N):                      # slot k: step k+1 (row k) from steps k (row k-1) and k-1
        dqA = 4.0 / 3.0 * tq[k - 1] - 1.0 / 3.0 * pq
        dqB = dqA + 8.0 / 9.0 * h * tqd[k - 1] - 2.0 / 9.0 * h * pqd
        tq[k], tqd[k] = solve_fwd(H[k], M[k], D[k], eta, pscale, dqA, dqB, tu[k])
        pq, pqd = tq[k - 1], tqd[k - 1]
    return tq, tqd


def jvp(integrator, H, M, D, h, pscale, tu=None, tq0=None, tqd0=None):
    return (jvp_bdf1 if integrator == 1 else jvp_bdf2)(H, M, D, h, pscale, tu, tq0, tqd0)


def chain_bdf1(A, Bm, tu, tq0, tqd0):
    """The forward chain x_k = A_k x_{k-1} + B_k tu_k of one rollout, x = (dq, dqd): A [N][2nr][2nr], Bm [N][2nr][nr] ->
    (tq[N][nr], tqd[N][nr])."""
    N, nr = tu.shape
    x = np.concatenate([tq0, tqd0])
    tq, tqd = np.empty((N, nr)), np.empty((N, nr))
    for k in range(N):
        x = A[k] @ x + Bm[k] @ tu[k]
        tq[k], tqd[k] = x[:nr], x[nr:]
    return tq, tqd


def jvp_on_sensitivities(integrator, XA, XB, XU, h, tu, tq0, tqd0):
    """The two recursions on XA, XB, XU of every slot (dx = XA dqA + XB dqB + XU du; pscale and eta^2 are inside XU), with eta per
    slot as the tape has it: what rmx_rollout_linearize's outputs give for one direction."""
    def fwd(s, eta, dqA, dqB, du):
        dx = XA[s] @ dqA + XB[s] @ dqB + XU[s] @ du
        return dx, (dx - dqA) / eta
    N, nr = tu.shape
    tq, tqd = np.empty((N, nr)), np.empty((N, nr))
    if integrator == 1:
        dq, dqd = tq0, tqd0
        for k in range(N):
            dq, dqd = fwd(k, h, dq, dq + h * dqd, tu[k])
            tq[k], tqd[k] = dq, dqd
        return tq, tqd
    eta = AL * h
    _, dqda = fwd(N, eta, tq0, tq0 + AL * h * tqd0, tu[0])
    tq[0], tqd[0] = fwd(0, eta, tq0 + (1.0 - AL) * h * dqda, tq0 + (2.0 * AL - 1.0) * h * tqd0 + 2.0 * (1.0 - AL) * h * dqda, tu[0])
    eta = 2.0 * h / 3.0
    pq, pqd = tq0, tqd0
    for k in range(1, N):
        dqA = 4.0 / 3.0 * tq[k - 1] - 1.0 / 3.0 * pq
        dqB = dqA + 8.0 / 9.0 * h * tqd[k - 1] - 2.0 / 9.0 * h * pqd
        tq[k], tqd[k] = fwd(k, eta, dqA, dqB, tu[k])
        pq, pqd = tq[k - 1], tqd[k - 1]
    return tq, tqd


def tangents(seed, B, ntan, nsteps, nr):
    """Fixed-seed standard-normal tangents: dict(tu [B][ntan][nsteps][nr], tq0 [B][ntan][nr], tqd0 [B][ntan][nr])."""
    rng = np.random.default_rng(seed)
    return dict(tu=rng.standard_normal((B, ntan, nsteps, nr)), tq0=rng.standard_normal((B, ntan, nr)),
                tqd0=rng.standard_normal((B, ntan, nr)))


def pairing(g, t, grads, tans):
    """The identity <gq, tq> + <gqd, tqd> = <du, tu> + <dq0, tq0> + <dqd0, tqd0>: |lhs - rhs| relative to the sum of the magnitudes of
    the three terms on the right.  g = (gq, gqd), t = (tq, tqd), grads = (du, dq0, dqd0), tans = (tu, tq0, tqd0), None: zero."""
    lhs = float((g[0] * t[0]).sum() + (g[1] * t[1]).sum())
    terms = [float((a * b).sum()) if b is not None else 0.0 for a, b in zip(grads, tans)]
    return abs(lhs - sum(terms)) / max(sum(abs(x) for x in terms), 1e-300)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))
