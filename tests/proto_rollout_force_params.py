"""The force-constant gradients of rmx_rollout_vjp_forces (include/redmax_hip.h) in numpy, on proto_rollout_pf.World: a reference
for the GPU tests that shares no code with the library (development aid + executable derivation; NOT the oracle, NOT the product).

Every taped solve is g(x; qA, qB, u, theta) = 0 with adjoint vector z_s, so
    dL/dtheta = - sum over the slots s of the tape   z_s' dg_s/dtheta
with dg_s/dtheta at the slot's solution x_s and its qA, qB, eta (proto_rollout_pf.solves: under BDF2 the rebuilt SDIRK2a state in
slot N).  theta: stiffness ks, damping kd and rest length L of every row of the force table.  No closed form of the library's enters:
the share of ONE force in g (proto_point_forces.world_terms on a table of that force alone) is
    linear in (ks, kd)   so   dg/dks = share(ks = 1, kd = 0)   and   dg/dkd = share(ks = 0, kd = 1)   exactly, and
    affine in 1/L for a spring or a taut cable (tension = (ks l + kd ldot)/L - ks), so with L' = L/2 - which keeps a taut cable
        taut -  share(L') - share(L) = (1/L) d share/d(1/L)  and  dg/dL = -(1/L^2) d share/d(1/L) = -(share(L/2) - share(L))/L;
    a point-point force has no L, and a cable with !(strain > 0) at the slot's x contributes nothing to any of the three.
z: BDF1 z_k = du_k/(h^2 pscale) from proto_rollout_pf.vjp; BDF2 from proto_rollout_params.vjp_bdf2_z (the proto recursion that keeps z of
all N + 1 slots).  Besides the gradient G every entry gets its scale S = sum_s |z_s' dg_s/dtheta|, the sum of the magnitudes of the
terms G is the sum of: the yardstick of the GPU tests, proof against cancellation between the slots.
tests/test_rollout_force_params_proto.py pins all this against central differences of whole rollouts.
"""
import copy

import numpy as np

import proto_point_forces as ppf
import proto_rollout_pf as P

NAMES = ("force_stiffness", "force_damping", "force_L")


def constants(ev):
    """[nforces][3]: ks, kd, L of the evaluator's force table."""
    return np.array([[f[2], f[3], f[4]] for f in ev.forces], dtype=np.float64).reshape(len(ev.forces), 3)


def with_constants(ev, theta):
    """The evaluator with the constants of its force table replaced (theta: [nforces][3])."""
    out = copy.copy(ev)
    out.forces = [(f[0], f[1], float(t[0]), float(t[1]), float(t[2])) for f, t in zip(ev.forces, np.asarray(theta, float))]
    return out


def _share(m, force, x, v, eta):
    """One force's share of g in reduced coordinates."""
    idx = m["idx"]
    dg = ppf.world_terms(m, [force], x, v, eta, False)[0]
    g = np.zeros(m["nr"])
    for j in range(m["n"]):
        if idx[j] >= 0:
            g[idx[j]] += dg[j]
    return g


def taut(m, force, x, v):
    """False for a cable with !(strain > 0) at the state, True for everything else."""
    kind, _, _, _, L = force
    if kind != ppf.CABLE:
        return True
    xs = ppf.point_state(m, [force], x, v)[0][0][0]
    l = sum(np.linalg.norm(xs[j + 1] - xs[j]) for j in range(len(xs) - 1))
    return bool((l - L) / L > 0)


def dg_dtheta(m, force, x, v, eta):
    """[3][nr]: dg/dks, dg/dkd, dg/dL of one force at one state, by the linearity rules of the module docstring."""
    kind, pts, ks, kd, L = force
    out = np.zeros((3, m["nr"]))
    if not taut(m, force, x, v):
        return out
    out[0] = _share(m, (kind, pts, 1.0, 0.0, L), x, v, eta)
    out[1] = _share(m, (kind, pts, 0.0, 1.0, L), x, v, eta)
    if kind != ppf.PP:
        out[2] = -(_share(m, (kind, pts, ks, kd, 0.5 * L), x, v, eta) - _share(m, force, x, v, eta)) / L
    return out


def adjoint_vectors(ev, q0, qd0, qtraj, qdtraj, gq, gqd, h, pscale, integ=1):
    """z of every slot of the tape at a record, [nslots][nr] in the tape's slot order, and (du, dq0, dqd0) of the same sweep."""
    H, M, D = P.tape(ev, q0, qd0, qtraj, qdtraj, h, integ)
    if integ == 1:
        du, dq0, dqd0 = P.vjp(H, M, D, gq, gqd, h, pscale, 1)
        return du / (h * h * pscale), (du, dq0, dqd0)
    import proto_rollout_params as prm
    du, dq0, dqd0, z = prm.vjp_bdf2_z(H, M, D, np.asarray(gq, float), np.asarray(gqd, float), h, pscale)
    return z, (du, dq0, dqd0)


def contract(ev, q0, qd0, qtraj, qdtraj, z, h, integ=1):
    """(G, S), [nforces][3] each (columns: ks, kd, L): G = - sum_s z_s' dg_s/dtheta and S = sum_s |z_s' dg_s/dtheta|."""
    nf = len(ev.forces)
    G, S = np.zeros((nf, 3)), np.zeros((nf, 3))
    sv = P.solves(np.asarray(q0, float), np.asarray(qd0, float), np.asarray(qtraj, float), np.asarray(qdtraj, float), h, integ)
    for slot, eta, qA, _, x, _, _ in sv:
        v = (x - qA) / eta
        for f, force in enumerate(ev.forces):
            t = dg_dtheta(ev.m, force, x, v, eta) @ z[slot]
            G[f] -= t
            S[f] += np.abs(t)
    return G, S


def on_record(ev, q0, qd0, qtraj, qdtraj, gq, gqd, h, pscale, integ=1):
    """dict(G, S, z, du, dq0, dqd0) at a given record (the GPU's own, or the proto's)."""
    z, (du, dq0, dqd0) = adjoint_vectors(ev, q0, qd0, qtraj, qdtraj, gq, gqd, h, pscale, integ)
    G, S = contract(ev, q0, qd0, qtraj, qdtraj, z, h, integ)
    return dict(G=G, S=S, z=z, du=du, dq0=dq0, dqd0=dqd0)


def loss(ev, q0, qd0, u, h, pscale, c, d, integ=1, info=None):
    """The loss of proto_rollout_pf on the evaluator's model (for the central differences)."""
    qt, qdt = P.rollout(ev, q0, qd0, u, h, pscale, integ, info)
    return P.loss_and_cotangents(qt, qdt, c, d)[0]


def reference(ev, q0, qd0, u, h, pscale, c, d, integ=1):
    """The proto's own rollout and on_record at it, plus qtraj, qdtraj, L and whether every Newton solve converged."""
    info = {}
    qt, qdt = P.rollout(ev, q0, qd0, u, h, pscale, integ, info)
    L, gq, gqd = P.loss_and_cotangents(qt, qdt, c, d)
    out = on_record(ev, q0, qd0, qt, qdt, gq, gqd, h, pscale, integ)
    out.update(qtraj=qt, qdtraj=qdt, L=L, converged=info["converged"])
    return out


def case(n, nsteps=None):
    """proto_rollout_pf.case(n): the inputs of the GPU tests, on which tests/test_rollout_force_params_proto.py asserts the
    conditions those tests rest on (every entry but the point-point L carries |G| >= 1e-3 S)."""
    return P.case(n, nsteps)
