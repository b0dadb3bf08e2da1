"""The backward recursion of rmx_rollout_vjp (include/redmax_hip.h) in numpy, on top of the CPU oracle: a reference for the GPU
tests that shares no code with the library.

The forward rollout is the oracle's, one step per call (oracle_rollout_per_step of tests/test_gpu_adjoint_controls.py); H comes from
the oracle's evalBDF1 and M, D from its computeValues at each step's final state.  With z_{N+1} = z_{N+2} = 0, gqd_{N+1} = 0, for
k = N .. 1:
    y_k  = gq_k + (gqd_k - gqd_{k+1})/h - (-2 M_{k+1} + h D_{k+1})' z_{k+1} - M_{k+2}' z_{k+2}
    H_k' z_k = y_k
    du_k = h^2 pscale z_k
    dq0  = -gqd_1/h - (-M_1 + h D_1)' z_1 - M_2' z_2
    dqd0 = h M_1' z_1
tests/test_rollout_vjp_proto.py checks this against central differences of the oracle rollout.
"""
import numpy as np

from test_gpu_adjoint_controls import oracle_rollout_per_step


class _StartedFrom:
    """A scene as oracle_rollout_per_step reads it (desc, getQ), started from another state."""

    def __init__(self, sc, q, qd):
        self._sc, self._q, self._qd = sc, np.array(q, dtype=np.float64), np.array(qd, dtype=np.float64)

    def desc(self):
        return self._sc.desc()

    def getQ(self):
        return self._q.copy(), self._qd.copy()


def rollout(orc, sc, q0, qd0, u, h, pscale):
    """The oracle's controlled BDF1 rollout from (q0, qd0) under the torques tau + pscale*u[k-1]: (qtraj, qdtraj), both [nsteps][nr],
    row k-1 the state after step k."""
    u = np.asarray(u, dtype=np.float64)
    task = dict(sc.task, pscale=float(pscale), t=2 * h)       # (measured nowhere that matters: only the states are kept)
    q, qd = np.array(q0, dtype=np.float64), np.array(qd0, dtype=np.float64)
    qtraj, qdtraj = np.empty_like(u), np.empty_like(u)
    for k in range(u.shape[0]):
        q, qd, _, _ = oracle_rollout_per_step(orc, _StartedFrom(sc, q, qd), h, 1, task, u[k:k + 1])
        qtraj[k], qdtraj[k] = q, qd
    return qtraj, qdtraj


def tape(orc, sc, q0, qd0, qtraj, qdtraj, h):
    """H (evalBDF1), M, D (computeValues) of every step at its final state: three [nsteps][nr][nr] arrays."""
    o = orc.Oracle(sc.desc())
    H, M, D = (np.empty((len(qtraj), o.nr, o.nr)) for _ in range(3))
    qp, qdp = np.asarray(q0, dtype=np.float64), np.asarray(qd0, dtype=np.float64)
    for k in range(len(qtraj)):
        o.set_state(qtraj[k], qdtraj[k])
        M[k], _, _, _, D[k] = o.compute_values()
        _, H[k] = o.eval_bdf1(qtraj[k], qp, qdp, h)
        qp, qdp = qtraj[k], qdtraj[k]
    return H, M, D


def vjp(H, M, D, gq, gqd, h, pscale):
    """The recursion of the module docstring: (du[nsteps][nr], dq0[nr], dqd0[nr])."""
    N, nr = gq.shape
    z = np.zeros((N + 3, nr))                 # z[k] for k = 1 .. N; z[N+1] = z[N+2] = 0
    gd = np.vstack([np.zeros((1, nr)), gqd, np.zeros((1, nr))])      # gd[k] = gqd_k, gd[N+1] = 0
    du = np.empty((N, nr))
    for k in range(N, 0, -1):
        y = gq[k - 1] + (gd[k] - gd[k + 1]) / h
        if k + 1 <= N:
            y = y - (-2.0 * M[k] + h * D[k]).T @ z[k + 1]
        if k + 2 <= N:
            y = y - M[k + 1].T @ z[k + 2]
        z[k] = np.linalg.solve(H[k - 1].T, y)
        du[k - 1] = h * h * pscale * z[k]
    dq0 = -gd[1] / h - (-M[0] + h * D[0]).T @ z[1]
    if N >= 2:
        dq0 = dq0 - M[1].T @ z[2]
    dqd0 = h * M[0].T @ z[1]
    return du, dq0, dqd0


def loss_and_cotangents(qtraj, qdtraj, c, d):
    """L = sum_k c_k.q_k + d_k.qdot_k + |q_k|^2 / 2 and (dL/dq_k, dL/dqdot_k)."""
    L = float((c * qtraj).sum() + (d * qdtraj).sum() + 0.5 * (qtraj ** 2).sum())
    return L, c + qtraj, np.array(d, dtype=np.float64)


def reference(orc, sc, q0, qd0, u, h, pscale, c, d):
    """Everything the GPU tests compare against, for one rollout: dict(qtraj, qdtraj, L, du, dq0, dqd0)."""
    qtraj, qdtraj = rollout(orc, sc, q0, qd0, u, h, pscale)
    H, M, D = tape(orc, sc, q0, qd0, qtraj, qdtraj, h)
    L, gq, gqd = loss_and_cotangents(qtraj, qdtraj, c, d)
    du, dq0, dqd0 = vjp(H, M, D, gq, gqd, h, pscale)
    return dict(qtraj=qtraj, qdtraj=qdtraj, L=L, du=du, dq0=dq0, dqd0=dqd0)
