"""numpy definition of rmx_rollout_frames / rmx_rollout_cost_frames (development aid + executable derivation; NOT the oracle and NOT
the product): position, velocity and orientation of body frames along a state record, their Jacobians at the given state, and the
value, gradient and Gauss-Newton table of "joint-space quadratic + frame targets".  On top of proto_point_cost.kinematics; every
function takes a dtype (float64: the reference the device is compared with; longdouble: what both are judged against).

A frame term is a point xlocal of body n read at step k with weights wpos, wvel, wrot >= 0.  At the state (q_k, qdot_k), with the
world frames Rw, pw and world joint screws sw_j, sv_j of the kinematics and path = n and its strict ancestors:
    p  = Rw[n] xlocal + pw[n]               Jp_j = sv_j + sw_j x p                     (exact zeros off the path)
    R  = Rw[n]                              Jw_j = sw_j
    om_i = sum_{j in anc*(i)} sw_j qdot_j   V_i = sum_{j in anc*(i)} sv_j qdot_j       (node twists, i included)
    v  = V_n + om_n x p  ( = Jp qdot )      dv/dqdot_j = Jp_j
    dv/dq_i = G_i = sw_i x (v - (V_i + om_i x p)) + om_i x Jp_i                        (i on the path)
    r = p - xtarget, rv = v - vtarget, e_w = 1/2 a(R Rtarget'), a(M) = (M32 - M23, M13 - M31, M21 - M12)
    cost = wpos/2 |r|^2 + wvel/2 |rv|^2 + wrot/4 |R - Rtarget|_F^2                     (the last: wrot (1 - cos theta))
    gradient: q rows wpos Jp'r + wvel G'rv + wrot Jw'e_w, qdot rows wvel Jp'rv
    Gauss-Newton: qq wpos Jp'Jp + wvel G'G + wrot Jw'Jw; q,qdot wvel G'Jp; qdot,q its transpose; qdot,qdot wvel Jp'Jp
    pull-back: gq = Jp'gx + G'gv + Jw'a(gR R'), gqd = Jp'gv
G is formed twice: by the closed form above (G_closed, what the kernel does) and by summing d(Jp_j)/dq_i qdot_j over the path
(G_summed), with d sw_j/dq_i = sw_i x sw_j and d sv_j/dq_i = sw_i x sv_j + sv_i x sw_j for i in anc*(j) (zero otherwise: a joint
does not move its own screw nor those above it) and dp/dq_i = Jp_i.
"""
import numpy as np

import proto_point_cost as P

_cross = P._cross


def avec(M):
    return np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]], dtype=M.dtype)


def term_weights(t):
    return tuple(float(t.get(k, 0.0)) for k in ("wpos", "wvel", "wrot"))


def twists(m, kin, qd):
    """(om [n][3], V [n][3]): the sums of sw_j qd_j, sv_j qd_j over anc*(i), in ascending j."""
    sw, sv = kin[2], kin[3]
    n, idx = m["n"], m["idx"]
    om, V = np.zeros_like(sw), np.zeros_like(sv)
    for i in range(n):
        for j in range(n):
            if m["anc"][j, i] and idx[j] >= 0:
                om[i] = om[i] + sw[j] * qd[idx[j]]
                V[i] = V[i] + sv[j] * qd[idx[j]]
    return om, V


def _path(m, body):
    return [j for j in range(m["n"]) if m["anc"][j, body] and m["idx"][j] >= 0]


def G_closed(m, kin, tw, body, pt, v):
    sw, (om, V) = kin[2], tw
    G = np.zeros((3, m["nr"]), dtype=pt.dtype)
    for i in _path(m, body):
        Jp = kin[3][i] + _cross(sw[i], pt)
        G[:, m["idx"][i]] = _cross(sw[i], v - (V[i] + _cross(om[i], pt))) + _cross(om[i], Jp)
    return G


def G_summed(m, kin, qd, body, pt):
    sw, sv = kin[2], kin[3]
    G = np.zeros((3, m["nr"]), dtype=pt.dtype)
    path = _path(m, body)
    for i in path:
        Jpi = sv[i] + _cross(sw[i], pt)
        acc = np.zeros(3, dtype=pt.dtype)
        for j in path:
            d = _cross(sw[j], Jpi)                                    # sw_j x dp/dq_i
            if m["anc"][i, j]:                                        # i in anc*(j): the screw of j moves with q_i
                d = d + _cross(sw[i], sv[j]) + _cross(sv[i], sw[j]) + _cross(_cross(sw[i], sw[j]), pt)
            acc = acc + d * qd[m["idx"][j]]
        G[:, m["idx"][i]] = acc
    return G


def frame(m, kin, tw, body, xl):
    """dict(p, v, R, Jp, G, Jw) of one frame at one state; kin = kinematics(q), tw = twists(kin, qd)."""
    pt = P.point(kin, body, xl)
    om, V = tw
    v = V[body] + _cross(om[body], pt)
    Jp = P.jac_screw(m, kin, body, pt)
    Jw = np.zeros_like(Jp)
    for j in _path(m, body):
        Jw[:, m["idx"][j]] = kin[2][j]
    return dict(p=pt, v=v, R=kin[0][body], Jp=Jp, G=G_closed(m, kin, tw, body, pt, v), Jw=Jw)


def frames(m, q, qd, terms, dtype=np.float64):
    """(x [T][3], v [T][3], R [T][3][3]) along the record q, qd [N][nr] of ONE rollout."""
    q, qd = np.asarray(q, dtype=dtype), np.asarray(qd, dtype=dtype)
    T = len(terms)
    x, v, R = np.zeros((T, 3), dtype=dtype), np.zeros((T, 3), dtype=dtype), np.zeros((T, 3, 3), dtype=dtype)
    for k, own in enumerate(P.by_step(terms, q.shape[0])):
        if own:
            kin = P.kinematics(m, q[k], dtype)
            tw = twists(m, kin, qd[k])
            for i in own:
                f = frame(m, kin, tw, terms[i]["body"], terms[i]["xlocal"])
                x[i], v[i], R[i] = f["p"], f["v"], f["R"]
    return x, v, R


def pullback(m, q, qd, terms, gx=None, gv=None, gR=None, dtype=np.float64):
    """(gq, gqd) [N][nr]: gq = sum_t Jp'gx + G'gv + Jw'a(gR R'), gqd = sum_t Jp'gv; a cotangent that is None adds nothing."""
    q, qd = np.asarray(q, dtype=dtype), np.asarray(qd, dtype=dtype)
    gq, gqd = np.zeros(q.shape, dtype=dtype), np.zeros(q.shape, dtype=dtype)
    for k, own in enumerate(P.by_step(terms, q.shape[0])):
        if own:
            kin = P.kinematics(m, q[k], dtype)
            tw = twists(m, kin, qd[k])
            for i in own:
                f = frame(m, kin, tw, terms[i]["body"], terms[i]["xlocal"])
                if gx is not None:
                    gq[k] += f["Jp"].T @ np.asarray(gx[i], dtype=dtype)
                if gv is not None:
                    g = np.asarray(gv[i], dtype=dtype)
                    gq[k] += f["G"].T @ g
                    gqd[k] += f["Jp"].T @ g
                if gR is not None:
                    gq[k] += f["Jw"].T @ avec(np.asarray(gR[i], dtype=dtype) @ f["R"].T)
    return gq, gqd


def cost(m, q, qd, Q=None, xgoal=None, terms=(), xtarget=None, vtarget=None, Rtarget=None, dtype=np.float64):
    """dict(Jk [N], lx [N][2nr], Q [N][2nr][2nr], x, v [T][3], R [T][3][3], r, rv, ew [T][3]) of ONE rollout.  The joint-space part
    first, then the terms in the caller's order; inside a term position, velocity, rotation; a zero weight adds nothing."""
    q, qd = np.asarray(q, dtype=dtype), np.asarray(qd, dtype=dtype)
    N, nr = q.shape
    T = len(terms)
    Qin = np.zeros((N, 2 * nr, 2 * nr), dtype=dtype) if Q is None else np.asarray(Q, dtype=dtype)
    xg = np.zeros((N, 2 * nr), dtype=dtype) if xgoal is None else np.asarray(xgoal, dtype=dtype)
    out = dict(Jk=np.zeros(N, dtype=dtype), lx=np.zeros((N, 2 * nr), dtype=dtype), Q=Qin.copy())
    for k in ("x", "v", "r", "rv", "ew"):
        out[k] = np.zeros((T, 3), dtype=dtype)
    out["R"] = np.zeros((T, 3, 3), dtype=dtype)
    for k, own in enumerate(P.by_step(terms, N)):
        dx = np.concatenate([q[k], qd[k]]) - xg[k]
        out["lx"][k] = Qin[k] @ dx
        out["Jk"][k] = dx @ out["lx"][k] / 2
        if not own:
            continue
        kin = P.kinematics(m, q[k], dtype)
        tw = twists(m, kin, qd[k])
        for i in own:
            t = terms[i]
            wp, wv, wr = (dtype(w) for w in term_weights(t))
            f = frame(m, kin, tw, t["body"], t["xlocal"])
            out["x"][i], out["v"][i], out["R"][i] = f["p"], f["v"], f["R"]
            Jp, G, Jw = f["Jp"], f["G"], f["Jw"]
            if wp > 0 or xtarget is not None:
                r = f["p"] - np.asarray(xtarget[i], dtype=dtype)
                out["r"][i] = r
                out["Jk"][k] += wp * (r @ r) / 2
                out["lx"][k, :nr] += wp * (Jp.T @ r)
                out["Q"][k, :nr, :nr] += wp * (Jp.T @ Jp)
            if wv > 0:
                rv = f["v"] - np.asarray(vtarget[i], dtype=dtype)
                out["rv"][i] = rv
                out["Jk"][k] += wv * (rv @ rv) / 2
                out["lx"][k, :nr] += wv * (G.T @ rv)
                out["lx"][k, nr:] += wv * (Jp.T @ rv)
                out["Q"][k, :nr, :nr] += wv * (G.T @ G)
                out["Q"][k, :nr, nr:] += wv * (G.T @ Jp)
                out["Q"][k, nr:, :nr] += wv * (Jp.T @ G)
                out["Q"][k, nr:, nr:] += wv * (Jp.T @ Jp)
            if wr > 0:
                Rt = np.asarray(Rtarget[i], dtype=dtype)
                ew = avec(f["R"] @ Rt.T) / 2
                out["ew"][i] = ew
                D = f["R"] - Rt
                out["Jk"][k] += wr * np.sum(D * D) / 4
                out["lx"][k, :nr] += wr * (Jw.T @ ew)
                out["Q"][k, :nr, :nr] += wr * (Jw.T @ Jw)
    return out


def rot(axis, theta, dtype=np.float64):
    """exp(theta [axis]x) by Rodrigues' formula."""
    ax = np.asarray(axis, dtype=dtype)
    ax = ax / np.sqrt(ax @ ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], dtype=dtype)
    return np.eye(3, dtype=dtype) + np.sin(dtype(theta)) * K + (1 - np.cos(dtype(theta))) * (K @ K)


rel_err = P.rel_err
