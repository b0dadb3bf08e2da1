"""The taped rollout of a model with body-to-body forces in numpy (development aid + executable derivation beside
proto_point_forces.py; NOT the oracle and NOT the product): the controlled, line-search-free rollout of rmx_rollout_tape /
rmx_rollout_tape_bdf2 on such a model, the tape it leaves, and the gradients the tape's readers form from it.  It shares no code
with the library.

The residual is an `Evaluator`: World (proto_point_forces.eval_world_pf, the world-frame algebra the kernels use) or Lit
(proto_point_forces.Literal: the oracle's force-free residual plus the reference's literal J'(fm, Km, Dm)J).  A solve is
    g(x; qA, qB, eta) - eta^2 pscale u = 0,   v = (x - qA)/eta
iterated as the device's taped sweep iterates it: evaluate g, H at x; dx = -H^-1 (g - eta^2 pscale u); x += dx; stop where the
EVALUATED iterate had |g - eta^2 pscale u| < tol.  The integrator stages are those of proto_rollout_vjp_bdf2's docstring.

The tape at given states: H (with the forces), M, and D = D0 + D_pf, D0 = df/dqdot of the force-free model (eval_MD_world), and
the forces' share of D = df/dqdot twice:
  D_pf_world     the world-frame formula, in the notation of proto_point_forces' docstring, per force
                     point-point            D(a,i) -= kd  dA(a) . dA(i)
                     spring / taut cable    D(a,i) -= (kd/L) lam(a) lam(i),   lam(a) = sum_j u_j . dA_j(a)
                     slack cable            nothing
                 (the coefficient of 1/eta in C, divided by eta: what remains of dB = dA/eta + ... when q is held and qdot moves)
  D_pf_literal   J' Dm J with Dm of literal_fKD - what the reference's computeValues adds to D.
The recursions that read the tape are the existing ones, fed with it: proto_rollout_vjp.vjp (BDF1), proto_rollout_vjp_bdf2.vjp,
proto_rollout_linearize.sens, proto_rollout_vjp_feedback.vjp.  tests/test_rollout_pf_proto.py pins all of it on the CPU.
"""
import numpy as np

import proto_point_forces as ppf
import proto_rollout_linearize as plin
import proto_worldframe as pw

AL = (2.0 - np.sqrt(2.0)) / 2.0
TOL = 1e-9


# ----------------------------------------------------------------------------- the forces' share of D
def D_pf_world(m, forces, q, qdot):
    """The block of the module docstring in reduced coordinates, [nr][nr]."""
    n, idx = m["n"], m["idx"]
    st, _ = ppf.point_state(m, forces, q, qdot)
    Dn = np.zeros((n, n))
    for (kind, pts, ks, kd, L), (xs, vs, As, Bs) in zip(forces, st):
        nseg = len(pts) - 1
        dA = [As[j + 1] - As[j] for j in range(nseg)]
        dx = [xs[j + 1] - xs[j] for j in range(nseg)]
        if kind == ppf.PP:
            Dn -= kd * dA[0].T @ dA[0]
            continue
        ln = [np.linalg.norm(d) for d in dx]
        l = sum(ln)
        if kind == ppf.CABLE and not (l - L) / L > 0:
            continue
        lam = sum((dx[j] / ln[j]) @ dA[j] for j in range(nseg))
        Dn -= (kd / L) * np.outer(lam, lam)
    dof = [j for j in range(n) if idx[j] >= 0]
    r = [idx[j] for j in dof]
    D = np.zeros((m["nr"], m["nr"]))
    D[np.ix_(r, r)] = Dn[np.ix_(dof, dof)]
    return D


def D_pf_literal(lit, q, qdot):
    """J' Dm J of the reference's literal blocks (lit: proto_point_forces.Literal)."""
    q, qdot = np.asarray(q, float), np.asarray(qdot, float)
    _, _, Dm, _ = ppf.literal_fKD(lit.m, lit.forces, lit.idxM, lit.nm, q, qdot)
    lit.o.set_state(q, qdot)
    J, _ = lit.o.jacobian()
    return J.T @ Dm @ J


# ----------------------------------------------------------------------------- the two evaluators
class World:
    """The world-frame residual and tape blocks of a scene whose joints have one DOF each (sceneTree, sceneChain)."""

    def __init__(self, sc):
        d = sc.desc()
        self.m = pw.build_model(d)
        self.forces = ppf.forces_of(d)
        self.nr = self.m["nr"]

    def eval(self, x, qA, qB, eta, want_H=True):
        return ppf.eval_world_pf(self.m, self.forces, x, qA, qB, eta, want_H)

    def MD(self, q, qd, with_pf=True):
        M, D = pw.eval_MD_world(self.m, np.asarray(q, float), np.asarray(qd, float))
        return M, (D + D_pf_world(self.m, self.forces, q, qd)) if with_pf else D

    def cable_lengths(self, q, qd):
        """(l, L) of every cable of the table at a state."""
        st, _ = ppf.point_state(self.m, self.forces, np.asarray(q, float), np.asarray(qd, float))
        return [(sum(np.linalg.norm(xs[j + 1] - xs[j]) for j in range(len(xs) - 1)), f[4])
                for f, (xs, _, _, _) in zip(self.forces, st) if f[0] == ppf.CABLE]


class Lit:
    """The same on proto_point_forces.Literal: Literal.eval, the oracle's computeValues for M, D0 and the literal J' Dm J."""

    def __init__(self, lit):
        self.lit, self.m, self.forces, self.nr = lit, lit.m, lit.forces, lit.nr

    def eval(self, x, qA, qB, eta, want_H=True):
        return self.lit.eval(x, qA, qB, eta, want_H)

    def MD(self, q, qd, with_pf=True):
        q, qd = np.asarray(q, float), np.asarray(qd, float)
        self.lit.o.set_state(q, qd)
        M, _, _, _, D = self.lit.o.compute_values()
        return M, (D + D_pf_literal(self.lit, q, qd)) if with_pf else D


# ----------------------------------------------------------------------------- the rollout
def newton(ev, qA, qB, eta, tau, x0, tol=TOL, info=None):
    """The taped sweep's Newton loop: returns x; info (a dict) takes 'iters' and 'converged'."""
    x = np.array(x0, float)
    itmax = 10 * len(x)
    for it in range(1, itmax + 1):
        g, H = ev.eval(x, qA, qB, eta)
        r = g - eta * eta * tau
        x = x - np.linalg.solve(H, r)
        if np.linalg.norm(r) < tol:
            break
    if info is not None:
        info["iters"] = info.get("iters", 0) + it
        info["converged"] = info.get("converged", True) and bool(np.linalg.norm(r) < tol)
    return x


def solves(q0, qd0, qtraj, qdtraj, h, integ):
    """(slot, eta, qA, qB, x, guess, step) of every taped solve of a trajectory, from its states alone: BDF1 one per step in slot
    k-1; BDF2 the slots of proto_rollout_vjp_bdf2 (slot N the SDIRK2a solve, whose result is rebuilt from q0, q1, qd1)."""
    N = len(qtraj)
    out = []
    if integ == 1:
        qp, qdp = q0, qd0
        for k in range(N):
            out.append((k, h, qp, qp + h * qdp, qtraj[k], qp + h * qdp, k))
            qp, qdp = qtraj[k], qdtraj[k]
        return out
    eta = AL * h
    qda = (qtraj[0] - AL * h * qdtraj[0] - q0) / ((1.0 - AL) * h)
    qa = q0 + AL * h * qda
    out.append((N, eta, q0, q0 + AL * h * qd0, qa, q0 + AL * h * qd0, 0))
    out.append((0, eta, q0 + (1.0 - AL) * h * qda, q0 + (2.0 * AL - 1.0) * h * qd0 + 2.0 * (1.0 - AL) * h * qda, qtraj[0],
                qa + (1.0 - AL) * h * qda, 0))
    qm, qdm = q0, qd0
    eta = 2.0 * h / 3.0
    for k in range(1, N):
        qk, qdk = qtraj[k - 1], qdtraj[k - 1]
        qA = 4.0 / 3.0 * qk - 1.0 / 3.0 * qm
        out.append((k, eta, qA, qA + 8.0 / 9.0 * h * qdk - 2.0 / 9.0 * h * qdm, qtraj[k], qk + h * qdk, k))
        qm, qdm = qk, qdk
    return out


def rollout(ev, q0, qd0, u, h, pscale, integ=1, info=None):
    """The controlled rollout from (q0, qd0) under tau + pscale*u[k-1] at step k: (qtraj, qdtraj), row k-1 the state after step k."""
    u = np.asarray(u, float)
    N, nr = u.shape
    q0, qd0 = np.array(q0, float), np.array(qd0, float)
    qtraj, qdtraj = np.empty((N, nr)), np.empty((N, nr))
    if integ == 1:
        q, qd = q0, qd0
        for k in range(N):
            xB = q + h * qd
            x = newton(ev, q, xB, h, pscale * u[k], xB, info=info)
            q, qd = x, (x - q) / h
            qtraj[k], qdtraj[k] = q, qd
        return qtraj, qdtraj
    eta = AL * h
    tau = pscale * u[0]
    qa = newton(ev, q0, q0 + AL * h * qd0, eta, tau, q0 + AL * h * qd0, info=info)
    qda = (qa - q0) / eta
    qA = q0 + (1.0 - AL) * h * qda
    qB = q0 + (2.0 * AL - 1.0) * h * qd0 + 2.0 * (1.0 - AL) * h * qda
    q1 = newton(ev, qA, qB, eta, tau, qa + (1.0 - AL) * h * qda, info=info)
    qtraj[0], qdtraj[0] = q1, (q1 - q0 - (1.0 - AL) * h * qda) / eta
    qm, qdm = q0, qd0
    eta = 2.0 * h / 3.0
    for k in range(1, N):
        qk, qdk = qtraj[k - 1], qdtraj[k - 1]
        qA = 4.0 / 3.0 * qk - 1.0 / 3.0 * qm
        qB = qA + 8.0 / 9.0 * h * qdk - 2.0 / 9.0 * h * qdm
        x = newton(ev, qA, qB, eta, pscale * u[k], qk + h * qdk, info=info)
        qtraj[k], qdtraj[k] = x, (3.0 / (2.0 * h)) * (x - 4.0 / 3.0 * qk + 1.0 / 3.0 * qm)
        qm, qdm = qk, qdk
    return qtraj, qdtraj


# ----------------------------------------------------------------------------- the tape and its readers
def tape(ev, q0, qd0, qtraj, qdtraj, h, integ=1, with_pf=True):
    """H, M, D of every taped solve at the solve's solution: [nslots][nr][nr] each, nslots = N (BDF1) or N + 1 (BDF2).
    with_pf False leaves D_pf out of D (the negative control of the tests): H keeps the forces."""
    q0, qd0 = np.asarray(q0, float), np.asarray(qd0, float)
    sv = solves(q0, qd0, np.asarray(qtraj, float), np.asarray(qdtraj, float), h, integ)
    nslots = len(sv)
    H, M, D = (np.empty((nslots, ev.nr, ev.nr)) for _ in range(3))
    for slot, eta, qA, qB, x, _, _ in sv:
        _, H[slot] = ev.eval(x, qA, qB, eta)
        M[slot], D[slot] = ev.MD(x, (x - qA) / eta, with_pf)
    return H, M, D


def vjp(H, M, D, gq, gqd, h, pscale, integ=1):
    import proto_rollout_vjp as p1          # (imports the oracle's test helpers: only where a recursion is asked for)
    import proto_rollout_vjp_bdf2 as p2
    return (p1.vjp if integ == 1 else p2.vjp)(H, M, D, gq, gqd, h, pscale)


def linearize(H, M, D, h, pscale, integ=1):
    """XA, XB, XU of every slot (proto_rollout_linearize.sens with the slot's eta)."""
    nslots = len(H)
    N = nslots if integ == 1 else nslots - 1
    eta = plin.etas(N, h, integ)
    out = [plin.sens(H[s], M[s], D[s], eta[s], pscale) for s in range(nslots)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def loss_and_cotangents(qtraj, qdtraj, c, d):
    """L = sum_k c_k.q_k + d_k.qdot_k + |q_k|^2 / 2 and (dL/dq_k, dL/dqdot_k): proto_rollout_vjp's loss."""
    L = float((c * qtraj).sum() + (d * qdtraj).sum() + 0.5 * (qtraj ** 2).sum())
    return L, c + qtraj, np.array(d, dtype=np.float64)


def reference(ev, q0, qd0, u, h, pscale, c, d, integ=1, with_pf=True):
    """dict(qtraj, qdtraj, L, du, dq0, dqd0) of one rollout."""
    qtraj, qdtraj = rollout(ev, q0, qd0, u, h, pscale, integ)
    H, M, D = tape(ev, q0, qd0, qtraj, qdtraj, h, integ, with_pf)
    L, gq, gqd = loss_and_cotangents(qtraj, qdtraj, c, d)
    du, dq0, dqd0 = vjp(H, M, D, gq, gqd, h, pscale, integ)
    return dict(qtraj=qtraj, qdtraj=qdtraj, L=L, du=du, dq0=dq0, dqd0=dqd0, H=H, M=M, D=D)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


# ----------------------------------------------------------------------------- the inputs the tests share
SIZES = (4, 5, 8, 16, 32, 33, 64)      # each fills its padded size but 5 (of 8) and 33 (of 64)
PSCALE = 1e3


def nsteps_of(n):
    return 3 if n > 32 else 4


def case(n, nsteps=None):
    """sizedSceneWithForces(n) with the two states of sizedStates and, per rollout, torques u and the loss weights c, d:
    dict(sc, q0, qd0 [2][nr], u, c, d [2][N][nr], h, pscale, nsteps).  Chosen on the CPU: the line-search-free Newton converges on
    every solve of both integrators from them (tests/test_rollout_pf_proto.py asserts it)."""
    sc = ppf.sizedSceneWithForces(n)
    q0, qd0 = ppf.sizedStates(sc, n)[:2]
    N = nsteps_of(n) if nsteps is None else nsteps
    rng = np.random.default_rng(4000 + n)
    u, c, d = 0.1 * rng.standard_normal((2, N, sc.nr)), rng.standard_normal((2, N, sc.nr)), rng.standard_normal((2, N, sc.nr))
    return dict(sc=sc, q0=q0, qd0=qd0, u=u, c=c, d=d, h=sc.h, pscale=PSCALE, nsteps=N)


SWITCH_STEPS = 20


def switching_case():
    """proto_point_forces.switchingScene() - two cables that go slack and taut again within twenty steps - from switchingStates,
    with small torques: the dict of case().  Included in the GPU tests because (tests/test_rollout_pf_proto.py) the Newton above
    converges on it for both integrators and no recorded step has a cable within 1e-6 relative of its rest length."""
    sc = ppf.switchingScene()
    q0, qd0 = ppf.switchingStates(sc)
    N = SWITCH_STEPS
    rng = np.random.default_rng(4100)
    u, c, d = 0.1 * rng.standard_normal((2, N, sc.nr)), rng.standard_normal((2, N, sc.nr)), rng.standard_normal((2, N, sc.nr))
    return dict(sc=sc, q0=q0, qd0=qd0, u=u, c=c, d=d, h=sc.h, pscale=PSCALE, nsteps=N)


def cable_strains(ev, qtraj, qdtraj):
    """(l - L)/L of every cable at every recorded step: [nsteps][ncables]."""
    return np.array([[(l - L) / L for l, L in ev.cable_lengths(q, qd)] for q, qd in zip(qtraj, qdtraj)])
