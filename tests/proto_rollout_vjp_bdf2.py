"""The BDF2 rollout of rmx_rollout_tape_bdf2 and the backward recursion of its rmx_rollout_vjp (include/redmax_hip.h) in numpy, on top
of the CPU oracle: a reference for the GPU tests that shares no code with the library.  The Newton iteration is this file's own, on
Oracle.eval_residual; M and D come from Oracle.compute_values at each solve's solution.

Every solve is x(qA, qB, eta, u):  g = eval_residual(x, qA, qB, eta) - eta^2 pscale u = 0,  v = (x - qA)/eta.  With al = (2 - sqrt 2)/2
    SDIRK2a: eta = al h, qA = q0, qB = q0 + al h qd0                                        -> qa, qda
    SDIRK2b: eta = al h, qA = q0 + (1-al) h qda, qB = q0 + (2al-1) h qd0 + 2(1-al) h qda    -> q1, qd1
    BDF2   : eta = 2h/3, qA = 4/3 q_k - 1/3 q_{k-1}, qB = qA + 8/9 h qd_k - 2/9 h qd_{k-1}  -> q_{k+1}, qd_{k+1}
Backwards through one solve (H = dg/dx, dg/dqB = -M, dg/dqA = eta D, dg/du = -eta^2 pscale):
    H' z = xbar + vbar/eta ;  A = -vbar/eta - eta D' z ;  Bq = M' z ;  ubar = eta^2 pscale z
The tape has N + 1 slots: step s in slot s-1 (slot 0 the SDIRK2b solve), the SDIRK2a solve in slot N.
tests/test_rollout_vjp_bdf2_proto.py checks all this against central differences of rollout().
"""
import numpy as np

AL = (2.0 - np.sqrt(2.0)) / 2.0


def _newton(o, qA, qB, eta, tau, x0):
    """x with eval_residual(x, qA, qB, eta) = eta^2 tau, iterated until the update is at rounding level; (x, v, H, M, D) there."""
    x, prev = np.array(x0, dtype=np.float64), np.inf
    for _ in range(40):
        g, H = o.eval_residual(x, qA, qB, eta)
        dx = -np.linalg.solve(H, g - eta * eta * tau)
        x = x + dx
        step = np.linalg.norm(dx)
        if step <= 1e-9 * max(1.0, np.linalg.norm(x)) and (step >= prev or step <= 1e-15 * np.linalg.norm(x)):
            break                               # (quadratic convergence has ended: the updates no longer shrink)
        prev = step
    else:
        raise RuntimeError("proto Newton did not settle")
    v = (x - qA) / eta
    _, H = o.eval_residual(x, qA, qB, eta)
    o.set_state(x, v)
    M, _, _, _, D = o.compute_values()
    return x, v, H, M, D


def forward(orc, sc, q0, qd0, u, h, pscale):
    """The BDF2 rollout from (q0, qd0), self-started with SDIRK2, under tau + pscale*u[k-1] at step k: (qtraj, qdtraj, H, M, D) with
    qtraj, qdtraj [nsteps][nr] (row k-1 the state after step k) and H, M, D [nsteps + 1][nr][nr] in the slots of the module docstring."""
    o = orc.Oracle(sc.desc())
    u = np.asarray(u, dtype=np.float64)
    N, nr = u.shape
    q0, qd0 = np.array(q0, dtype=np.float64), np.array(qd0, dtype=np.float64)
    qtraj, qdtraj = np.empty((N, nr)), np.empty((N, nr))
    H, M, D = (np.empty((N + 1, nr, nr)) for _ in range(3))
    eta = AL * h
    qa, qda, H[N], M[N], D[N] = _newton(o, q0, q0 + AL * h * qd0, eta, pscale * u[0], q0 + AL * h * qd0)
    qA = q0 + (1.0 - AL) * h * qda
    qB = q0 + (2.0 * AL - 1.0) * h * qd0 + 2.0 * (1.0 - AL) * h * qda
    qtraj[0], qdtraj[0], H[0], M[0], D[0] = _newton(o, qA, qB, eta, pscale * u[0], qa + (1.0 - AL) * h * qda)
    qm, qdm = q0, qd0
    eta = 2.0 * h / 3.0
    for k in range(1, N):                      # produces step k+1 (row k) from steps k (row k-1) and k-1
        qk, qdk = qtraj[k - 1], qdtraj[k - 1]
        qA = 4.0 / 3.0 * qk - 1.0 / 3.0 * qm
        qB = qA + 8.0 / 9.0 * h * qdk - 2.0 / 9.0 * h * qdm
        qtraj[k], qdtraj[k], H[k], M[k], D[k] = _newton(o, qA, qB, eta, pscale * u[k], qk + h * qdk)
        qm, qdm = qk, qdk
    return qtraj, qdtraj, H, M, D


def rollout(orc, sc, q0, qd0, u, h, pscale):
    return forward(orc, sc, q0, qd0, u, h, pscale)[:2]


def _solve_bwd(H, M, D, eta, xbar, vbar):
    z = np.linalg.solve(H.T, xbar + vbar / eta)
    return -vbar / eta - eta * (D.T @ z), M.T @ z, z


def vjp(H, M, D, gq, gqd, h, pscale):
    """The recursion of include/redmax_hip.h on a tape of N + 1 slots: (du[N][nr], dq0[nr], dqd0[nr])."""
    N, nr = gq.shape
    qbar = np.vstack([np.zeros((1, nr)), gq])         # qbar[k], vbar[k] for k = 0 .. N
    vbar = np.vstack([np.zeros((1, nr)), gqd])
    du = np.empty((N, nr))
    eta = 2.0 * h / 3.0
    for k in range(N - 1, 0, -1):
        A, Bq, z = _solve_bwd(H[k], M[k], D[k], eta, qbar[k + 1], vbar[k + 1])
        du[k] = eta * eta * pscale * z
        s = A + Bq
        qbar[k] += 4.0 / 3.0 * s
        vbar[k] += 8.0 / 9.0 * h * Bq
        qbar[k - 1] -= 1.0 / 3.0 * s
        vbar[k - 1] -= 2.0 / 9.0 * h * Bq
    eta = AL * h
    A, Bq, zb = _solve_bwd(H[0], M[0], D[0], eta, qbar[1], vbar[1])
    qbar[0] += A + Bq
    vbar[0] += (2.0 * AL - 1.0) * h * Bq
    qdabar = (1.0 - AL) * h * A + 2.0 * (1.0 - AL) * h * Bq
    A2, B2, za = _solve_bwd(H[N], M[N], D[N], eta, np.zeros(nr), qdabar)
    qbar[0] += A2 + B2
    vbar[0] += AL * h * B2
    du[0] = eta * eta * pscale * (za + zb)
    return du, qbar[0], vbar[0]


def loss_and_cotangents(qtraj, qdtraj, c, d):
    """L = sum_k c_k.q_k + d_k.qdot_k + |q_k|^2 / 2 and (dL/dq_k, dL/dqdot_k)."""
    L = float((c * qtraj).sum() + (d * qdtraj).sum() + 0.5 * (qtraj ** 2).sum())
    return L, c + qtraj, np.array(d, dtype=np.float64)


def reference(orc, sc, q0, qd0, u, h, pscale, c, d):
    """Everything the GPU tests compare against, for one rollout: dict(qtraj, qdtraj, L, du, dq0, dqd0)."""
    qtraj, qdtraj, H, M, D = forward(orc, sc, q0, qd0, u, h, pscale)
    L, gq, gqd = loss_and_cotangents(qtraj, qdtraj, c, d)
    du, dq0, dqd0 = vjp(H, M, D, gq, gqd, h, pscale)
    return dict(qtraj=qtraj, qdtraj=qdtraj, L=L, du=du, dq0=dq0, dqd0=dqd0)
