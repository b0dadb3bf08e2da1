"""The forward recursion of rmx_rollout_jvp_params (include/redmax_hip.h) in numpy, on the oracle's tape: a reference for the GPU
tests that shares no code with the library.

Every taped solve is g(x; qA, qB, u, theta) = 0, so a direction ttheta in the model's parameters goes through it as
    solve_fwd(H, M, D, eta; dqA, dqB, du) with one more term on the right:   H dx = -eta D dqA + M dqB + eta^2 pscale du - r
    r = (dg/dtheta) ttheta  at the slot's recorded x, qA, qB, eta
and the slots follow each other as in tests/proto_rollout_jvp.py (BDF1; BDF2 with its SDIRK2 start, slot N the SDIRK2a solve).
g is exactly linear in joint stiffness, damping and rest position, in the body inertia and in gravity, so
r = g(theta + ttheta) - g(theta): tests/proto_rollout_params.py's dg on a perturbed description at its slots_bdf1 / slots_bdf2 - no
closed form of the library's enters.  tests/test_rollout_jvp_params_proto.py pins all this against central differences of the
oracle's rollouts on perturbed models and against the gradients of tests/proto_rollout_params.py.
"""
import numpy as np

import proto_rollout_jvp as pj
import proto_rollout_params as pp
import proto_rollout_vjp as proto1
import proto_rollout_vjp_bdf2 as proto2

AL = pj.AL
GROUPS = pp.GROUPS


def tape(orc, sc, q0, qd0, u, h, pscale, integ):
    """The oracle's tape of one rollout and the slots the parameter term is taken at: dict(qtraj, qdtraj, H, M, D, slots)."""
    q0, qd0 = np.array(q0, dtype=np.float64), np.array(qd0, dtype=np.float64)
    if integ == 1:
        qtraj, qdtraj = proto1.rollout(orc, sc, q0, qd0, u, h, pscale)
        H, M, D = proto1.tape(orc, sc, q0, qd0, qtraj, qdtraj, h)
        slots = pp.slots_bdf1(q0, qd0, qtraj, qdtraj, h)
    else:
        qtraj, qdtraj, H, M, D = proto2.forward(orc, sc, q0, qd0, u, h, pscale)
        o = orc.Oracle(sc.desc())      # the SDIRK2a solve once more: forward() does not return its result
        qa, qda = proto2._newton(o, q0, q0 + AL * h * qd0, AL * h, pscale * np.asarray(u, dtype=np.float64)[0], q0 + AL * h * qd0)[:2]
        slots = pp.slots_bdf2(q0, qd0, qtraj, qdtraj, qa, qda, h)
    return dict(qtraj=qtraj, qdtraj=qdtraj, H=H, M=M, D=D, slots=slots)


def param_rhs(orc, sc, slots, tparams, g0=None, idx=None):
    """r = (dg/dtheta) ttheta of every slot, [nslots][nr], for a direction given as a dict group -> array (a missing group: zero)."""
    g0 = pp.residuals(orc, sc, slots) if g0 is None else g0
    r = np.zeros_like(g0)
    for group in GROUPS:
        if tparams.get(group) is not None:
            r += pp.dg(orc, sc, slots, group, tparams[group], g0, idx)
    return r


def _solve(H, M, D, eta, pscale, dqA, dqB, du, r):
    dx = np.linalg.solve(H, -eta * (D @ dqA) + M @ dqB + eta * eta * pscale * du - r)
    return dx, (dx - dqA) / eta


def jvp_with_rhs(integ, H, M, D, h, pscale, r, tu=None, tq0=None, tqd0=None):
    """tests/proto_rollout_jvp.py's two recursions with r[slot] taken off the right-hand side of every solve: (tq[N][nr], tqd[N][nr])."""
    nr = H.shape[1]
    N = H.shape[0] - (1 if integ == 2 else 0)
    tu, dq0, dqd0 = pj._zeros(tu, (N, nr)), pj._zeros(tq0, nr), pj._zeros(tqd0, nr)
    tq, tqd = np.empty((N, nr)), np.empty((N, nr))
    if integ == 1:
        dq, dqd = dq0, dqd0
        for k in range(N):
            dq, dqd = _solve(H[k], M[k], D[k], h, pscale, dq, dq + h * dqd, tu[k], r[k])
            tq[k], tqd[k] = dq, dqd
        return tq, tqd
    eta = AL * h
    _, dqda = _solve(H[N], M[N], D[N], eta, pscale, dq0, dq0 + AL * h * dqd0, tu[0], r[N])
    tq[0], tqd[0] = _solve(H[0], M[0], D[0], eta, pscale, dq0 + (1.0 - AL) * h * dqda,
                           dq0 + (2.0 * AL - 1.0) * h * dqd0 + 2.0 * (1.0 - AL) * h * dqda, tu[0], r[0])
    eta = 2.0 * h / 3.0
    pq, pqd = dq0, dqd0
    for k in range(1, N):
        dqA = 4.0 / 3.0 * tq[k - 1] - 1.0 / 3.0 * pq
        dqB = dqA + 8.0 / 9.0 * h * tqd[k - 1] - 2.0 / 9.0 * h * pqd
        tq[k], tqd[k] = _solve(H[k], M[k], D[k], eta, pscale, dqA, dqB, tu[k], r[k])
        pq, pqd = tq[k - 1], tqd[k - 1]
    return tq, tqd


def jvp_params(orc, sc, integ, tp, h, pscale, tparams, tu=None, tq0=None, tqd0=None, g0=None, idx=None):
    """One direction on the tape `tp` of tape(): (tq, tqd)."""
    r = param_rhs(orc, sc, tp["slots"], tparams, g0, idx)
    return jvp_with_rhs(integ, tp["H"], tp["M"], tp["D"], h, pscale, r, tu, tq0, tqd0)


def directions(vals, seed, shape=()):
    """Random directions per group, scaled to the group's magnitude (tests/test_rollout_params_proto.py directions): group ->
    shape + the group's shape."""
    rng = np.random.default_rng(seed)
    return {g: max(1.0, float(np.abs(vals[g]).max())) * rng.standard_normal(tuple(shape) + vals[g].shape) for g in GROUPS}


def pairing(g, t, grads, tans, pgrads, tparams):
    """<gq, tq> + <gqd, tqd> = <du, tu> + <dq0, tq0> + <dqd0, tqd0> + sum over the groups of <grad_group, ttheta_group>: |lhs - rhs|
    relative to the sum of the magnitudes of the terms on the right.  None / a missing group: zero."""
    lhs = float((g[0] * t[0]).sum() + (g[1] * t[1]).sum())
    terms = [float((a * b).sum()) for a, b in zip(grads, tans) if b is not None]
    terms += [float((pgrads[k] * tparams[k]).sum()) for k in GROUPS if tparams.get(k) is not None]
    return abs(lhs - sum(terms)) / max(sum(abs(x) for x in terms), 1e-300)
