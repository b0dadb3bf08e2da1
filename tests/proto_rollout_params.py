"""The model-parameter gradients of rmx_rollout_vjp_params (include/redmax_hip.h) in numpy, on top of the CPU oracle: a reference for
the GPU tests that shares no code with the library.

Every taped solve is g(x; qA, qB, u, theta) = 0 with adjoint vector z (H' z = xbar + vbar/eta), so
    dL/dtheta = - sum over the slots s of the tape   z_s' dg_s/dtheta
with dg_s/dtheta at the slot's solution x_s and its qA, qB, eta.  g is exactly linear in joint stiffness, damping and rest position,
in the body inertia (the diagonal I_i) and in gravity, so dg/dtheta . delta = g(theta + delta) - g(theta): Oracle.eval_residual on
a description with one array perturbed, and no closed form of the library's enters.

The tape and z come from tests/proto_rollout_vjp.py (BDF1: z_k = du_k / (h^2 pscale)) and from the recursion of
tests/proto_rollout_vjp_bdf2.py (BDF2, restated here so that za and zb of step 1 stay apart: N + 1 slots, step s in slot s-1, the
SDIRK2a solve in slot N).  Joints of at most one DOF (revolute, prismatic, fixed): the per-DOF arrays are the per-joint ones through
the oracle's idxR.  tests/test_rollout_params_proto.py pins all this against central differences of the oracle's rollouts.
"""
import numpy as np

import proto_rollout_vjp as proto1
import proto_rollout_vjp_bdf2 as proto2

AL = proto2.AL
GROUPS = ("stiffness", "damping", "qrest", "inertia", "grav")
DESC_KEY = {"stiffness": "stiffness", "damping": "damping", "qrest": "qRest", "inertia": "I_i", "grav": "grav"}


class Perturbed:
    """A scene as the protos read it (desc, task, getQ, h, nr) whose description has some arrays replaced."""

    def __init__(self, sc, **arrays):
        self._sc = sc
        self._d = dict(sc.desc())
        for k, v in arrays.items():
            self._d[k] = np.array(v, dtype=np.float64)
        self.task, self.h, self.nr = sc.task, sc.h, sc.nr

    def desc(self):
        return self._d

    def getQ(self):
        return self._sc.getQ()


def values(orc, sc):
    """The model's parameters in the layout of the gradients: stiffness, damping, qrest [nr] (reduced order), inertia [njoints][6],
    grav [3]."""
    d = sc.desc()
    idx = orc.Oracle(d).idxR()
    assert all(int(t) <= 2 for t in d["type"]), "joints of at most one DOF"
    out = {g: np.zeros(sc.nr) for g in GROUPS[:3]}
    for j, r in enumerate(idx):
        if r >= 0:
            for g in GROUPS[:3]:
                out[g][r] = d[DESC_KEY[g]][j]
    out["inertia"] = np.array(d["I_i"], dtype=np.float64).reshape(-1, 6)
    out["grav"] = np.array(d["grav"], dtype=np.float64).reshape(3)
    return out


def perturbed(orc, sc, group, delta, idx=None):
    """The scene with `delta` (in the layout of values()) added to one group of parameters.  idx: the oracle's idxR, if at hand."""
    d = sc.desc()
    key = DESC_KEY[group]
    arr = np.array(d[key], dtype=np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    extra = {}
    if group in GROUPS[:3]:
        for j, r in enumerate(orc.Oracle(d).idxR() if idx is None else idx):
            if r >= 0:
                arr[j] += delta[r]
        if group == "qrest" and d.get("qRestR") is not None and len(d["qRestR"]) == len(delta):
            extra["qRestR"] = np.asarray(d["qRestR"], dtype=np.float64) + delta      # (the per-DOF copy the library reads)
    else:
        arr = arr + delta.reshape(arr.shape)
    return Perturbed(sc, **{key: arr}, **extra)


def slots_bdf1(q0, qd0, qtraj, qdtraj, h):
    """(x, qA, qB, eta) of every slot of a BDF1 tape: slot k-1 is step k."""
    out, qp, qdp = [], np.asarray(q0, dtype=np.float64), np.asarray(qd0, dtype=np.float64)
    for k in range(len(qtraj)):
        out.append((qtraj[k], qp, qp + h * qdp, h))
        qp, qdp = qtraj[k], qdtraj[k]
    return out


def slots_bdf2(q0, qd0, qtraj, qdtraj, qa, qda, h):
    """(x, qA, qB, eta) of every slot of a BDF2 tape: slot 0 SDIRK2b, slots 1 .. N-1 the BDF2 steps, slot N SDIRK2a."""
    N = len(qtraj)
    out = [(qtraj[0], q0 + (1.0 - AL) * h * qda, q0 + (2.0 * AL - 1.0) * h * qd0 + 2.0 * (1.0 - AL) * h * qda, AL * h)]
    qm, qdm = q0, qd0
    for k in range(1, N):
        qk, qdk = qtraj[k - 1], qdtraj[k - 1]
        qA = 4.0 / 3.0 * qk - 1.0 / 3.0 * qm
        out.append((qtraj[k], qA, qA + 8.0 / 9.0 * h * qdk - 2.0 / 9.0 * h * qdm, 2.0 * h / 3.0))
        qm, qdm = qk, qdk
    out.append((qa, q0, q0 + AL * h * qd0, AL * h))
    return out


def vjp_bdf2_z(H, M, D, gq, gqd, h, pscale):
    """proto_rollout_vjp_bdf2.vjp keeping z of all N + 1 slots: (du, dq0, dqd0, z[N + 1][nr])."""
    N, nr = gq.shape
    qbar = np.vstack([np.zeros((1, nr)), gq])
    vbar = np.vstack([np.zeros((1, nr)), gqd])
    du, z = np.empty((N, nr)), np.empty((N + 1, nr))
    eta = 2.0 * h / 3.0
    for k in range(N - 1, 0, -1):
        A, Bq, z[k] = proto2._solve_bwd(H[k], M[k], D[k], eta, qbar[k + 1], vbar[k + 1])
        du[k] = eta * eta * pscale * z[k]
        s = A + Bq
        qbar[k] += 4.0 / 3.0 * s
        vbar[k] += 8.0 / 9.0 * h * Bq
        qbar[k - 1] -= 1.0 / 3.0 * s
        vbar[k - 1] -= 2.0 / 9.0 * h * Bq
    eta = AL * h
    A, Bq, z[0] = proto2._solve_bwd(H[0], M[0], D[0], eta, qbar[1], vbar[1])
    qbar[0] += A + Bq
    vbar[0] += (2.0 * AL - 1.0) * h * Bq
    qdabar = (1.0 - AL) * h * A + 2.0 * (1.0 - AL) * h * Bq
    A2, B2, z[N] = proto2._solve_bwd(H[N], M[N], D[N], eta, np.zeros(nr), qdabar)
    qbar[0] += A2 + B2
    vbar[0] += AL * h * B2
    du[0] = eta * eta * pscale * (z[N] + z[0])
    return du, qbar[0], vbar[0], z


def residuals(orc, sc, slots):
    """g of every slot on a scene's model, [nslots][nr] (the torque term does not depend on the parameters and is left out)."""
    o = orc.Oracle(sc.desc())
    return np.array([o.eval_residual(x, qA, qB, eta, want_H=False) for x, qA, qB, eta in slots])


def dg(orc, sc, slots, group, delta, g0=None, idx=None):
    """dg/dtheta . delta of every slot, by linearity: g(theta + delta) - g(theta)."""
    g0 = residuals(orc, sc, slots) if g0 is None else g0
    return residuals(orc, perturbed(orc, sc, group, delta, idx), slots) - g0


def grads(orc, sc, slots, z):
    """The five gradient arrays, one unit perturbation per entry (scaled to the group's magnitude, which linearity takes out again)."""
    vals = values(orc, sc)
    g0 = residuals(orc, sc, slots)
    idx = orc.Oracle(sc.desc()).idxR()
    out = {}
    for group in GROUPS:
        scale = max(1.0, float(np.abs(vals[group]).max()))
        grad = np.zeros(vals[group].shape)
        for i in np.ndindex(grad.shape):
            delta = np.zeros(grad.shape)
            delta[i] = scale
            grad[i] = -(z * dg(orc, sc, slots, group, delta, g0, idx)).sum() / scale
        out[group] = grad
    return out


def loss(orc, sc, q0, qd0, u, h, pscale, c, d, integ):
    """The loss of the proto tests on a scene's own model."""
    mod = proto1 if integ == 1 else proto2
    qt, qdt = mod.rollout(orc, sc, q0, qd0, u, h, pscale)
    return mod.loss_and_cotangents(qt, qdt, c, d)[0]


def reference(orc, sc, q0, qd0, u, h, pscale, c, d, integ=1):
    """Everything the GPU tests compare against, for one rollout: dict(qtraj, qdtraj, L, du, dq0, dqd0, z, slots, grads)."""
    q0, qd0 = np.array(q0, dtype=np.float64), np.array(qd0, dtype=np.float64)
    if integ == 1:
        qtraj, qdtraj = proto1.rollout(orc, sc, q0, qd0, u, h, pscale)
        H, M, D = proto1.tape(orc, sc, q0, qd0, qtraj, qdtraj, h)
        L, gq, gqd = proto1.loss_and_cotangents(qtraj, qdtraj, c, d)
        du, dq0, dqd0 = proto1.vjp(H, M, D, gq, gqd, h, pscale)
        z = du / (h * h * pscale)
        slots = slots_bdf1(q0, qd0, qtraj, qdtraj, h)
    else:
        qtraj, qdtraj, H, M, D = proto2.forward(orc, sc, q0, qd0, u, h, pscale)
        o = orc.Oracle(sc.desc())      # the SDIRK2a solve once more: forward() does not return its result
        qa, qda = proto2._newton(o, q0, q0 + AL * h * qd0, AL * h, pscale * np.asarray(u, dtype=np.float64)[0], q0 + AL * h * qd0)[:2]
        L, gq, gqd = proto2.loss_and_cotangents(qtraj, qdtraj, c, d)
        du, dq0, dqd0, z = vjp_bdf2_z(H, M, D, gq, gqd, h, pscale)
        slots = slots_bdf2(q0, qd0, qtraj, qdtraj, qa, qda, h)
    return dict(qtraj=qtraj, qdtraj=qdtraj, L=L, du=du, dq0=dq0, dqd0=dqd0, z=z, slots=slots, grads=grads(orc, sc, slots, z))
