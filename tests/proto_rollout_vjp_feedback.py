"""The closed-loop backward recursion of rmx_rollout_vjp_feedback (include/redmax_hip.h) in numpy, on the oracle's tape of the proto's
closed loop (tests/proto_rollout_feedback.py): a reference for the GPU tests that shares no code with the library.

The rollout ran under uapp_k = uff_k + K_k' (x_{k-1} - xref_{k-1}), x = (q, qdot), K_k[j][i] = du_i/dx_j; its tape is the open-loop
tape under uapp (proto_rollout_vjp.tape for BDF1, proto_rollout_vjp_bdf2.forward for BDF2).  With solve_bwd of proto_rollout_vjp_bdf2,
gu the cotangent of uapp and qbar[k], vbar[k] starting as gq_k, gqd_k (zero for k = 0):
    BDF1, k = N .. 1:   (A, Bq, z) = solve_bwd(slot k-1, h; qbar[k], vbar[k]) ;  ubar_k = h^2 pscale z + gu_k
                        qbar[k-1] += A + Bq + Kq_k' ubar_k ;  vbar[k-1] += h Bq + Kv_k' ubar_k
    BDF2: the recursion of proto_rollout_vjp_bdf2.vjp, with ubar_{k+1} = (2h/3)^2 pscale z + gu_{k+1} going into qbar[k], vbar[k]
          through K_{k+1} behind the solve of step k+1, and ubar_1 = (al h)^2 pscale (za + zb) + gu_1 into qbar[0], vbar[0].
    duff_k = ubar_k ;  dxref_{k-1} = -K_k ubar_k ;  dK_k[j][i] = (x_{k-1} - xref_{k-1})_j ubar_{k,i} ;  dq0 = qbar[0], dqd0 = vbar[0]
(K_k ubar with K_k as the [2nr][nr] C array is the header's K' ubar.)  tests/test_rollout_vjp_feedback_proto.py checks this against
central differences of the closed loop.
"""
import numpy as np

import proto_rollout_feedback as protofb
import proto_rollout_vjp as proto1
import proto_rollout_vjp_bdf2 as proto2
from proto_rollout_vjp_bdf2 import AL, _solve_bwd


def start_states(q0, qd0, qtraj, qdtraj):
    """x_{k-1} = (q, qdot) at the start of step k, k = 1 .. N: [N][2nr]."""
    return np.concatenate([np.concatenate([q0, qd0])[None], np.concatenate([qtraj, qdtraj], axis=1)[:-1]])


def _through_gains(K_k, dx_k, ubar, out, k):
    """What step k+1 (row k) does with its ubar: the rows of duff, dxref, dK, and the K term (into qbar, vbar of the state it started from)."""
    nr = len(ubar)
    out["duff"][k] = ubar
    if K_k is None:
        return np.zeros(nr), np.zeros(nr)
    kb = K_k @ ubar
    out["dxref"][k] = -kb
    out["dK"][k] = np.outer(dx_k, ubar)
    return kb[:nr], kb[nr:]


def vjp(integ, H, M, D, K, dx, gq, gqd, gu, h, pscale):
    """The recursion of the module docstring on a tape H, M, D (N slots under BDF1, N + 1 under BDF2): dict(duff [N][nr], dK
    [N][2nr][nr], dxref [N][2nr], dq0, dqd0 [nr]).  K [N][2nr][nr] or None (dK, dxref zero then), dx [N][2nr] = x_{k-1} - xref_{k-1},
    gu [N][nr] or None."""
    N, nr = gq.shape
    gu = np.zeros((N, nr)) if gu is None else gu
    qbar = np.vstack([np.zeros((1, nr)), gq])
    vbar = np.vstack([np.zeros((1, nr)), gqd])
    out = dict(duff=np.zeros((N, nr)), dK=np.zeros((N, 2 * nr, nr)), dxref=np.zeros((N, 2 * nr)))
    Kof = (lambda k: None) if K is None else (lambda k: K[k])
    if integ == 1:
        for k in range(N, 0, -1):
            A, Bq, z = _solve_bwd(H[k - 1], M[k - 1], D[k - 1], h, qbar[k], vbar[k])
            kq, kv = _through_gains(Kof(k - 1), dx[k - 1], h * h * pscale * z + gu[k - 1], out, k - 1)
            qbar[k - 1] += A + Bq + kq
            vbar[k - 1] += h * Bq + kv
    else:
        eta = 2.0 * h / 3.0
        for k in range(N - 1, 0, -1):
            A, Bq, z = _solve_bwd(H[k], M[k], D[k], eta, qbar[k + 1], vbar[k + 1])
            kq, kv = _through_gains(Kof(k), dx[k], eta * eta * pscale * z + gu[k], out, k)
            s = A + Bq
            qbar[k] += 4.0 / 3.0 * s + kq
            vbar[k] += 8.0 / 9.0 * h * Bq + kv
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
        kq, kv = _through_gains(Kof(0), dx[0], eta * eta * pscale * (za + zb) + gu[0], out, 0)
        qbar[0] += kq
        vbar[0] += kv
    out["dq0"], out["dqd0"] = qbar[0], vbar[0]
    return out


def closed_loop(orc, sc, integ, q0, qd0, uff, K, xref, h, pscale):
    """The proto's closed loop: (qtraj, qdtraj, uapp)."""
    fn = protofb.rollout if integ == 1 else protofb.rollout_bdf2
    return fn(orc, sc, q0, qd0, uff, K, xref, h, pscale)


def loss_and_cotangents(qtraj, qdtraj, uapp, c, d, e):
    """proto_rollout_vjp.loss_and_cotangents plus sum_k e_k . uapp_k: (L, dL/dq_k, dL/dqdot_k, dL/duapp_k)."""
    L, gq, gqd = proto1.loss_and_cotangents(qtraj, qdtraj, c, d)
    return L + float((e * uapp).sum()), gq, gqd, np.array(e, dtype=np.float64)


def tape(orc, sc, integ, q0, qd0, qtraj, qdtraj, uapp, h, pscale):
    """H, M, D of the closed loop's solves: the open-loop tape under uapp."""
    if integ == 1:
        return proto1.tape(orc, sc, q0, qd0, qtraj, qdtraj, h)
    qt, qdt, H, M, D = proto2.forward(orc, sc, q0, qd0, uapp, h, pscale)
    assert np.array_equal(qt, qtraj) and np.array_equal(qdt, qdtraj)      # (the same solves from the same starting points)
    return H, M, D


def reference(orc, sc, integ, q0, qd0, uff, K, xref, h, pscale, c, d, e):
    """Everything the GPU tests compare against, for one rollout: dict(qtraj, qdtraj, uapp, L, gq, gqd, gu, duff, dK, dxref, dq0, dqd0)."""
    qtraj, qdtraj, uapp = closed_loop(orc, sc, integ, q0, qd0, uff, K, xref, h, pscale)
    H, M, D = tape(orc, sc, integ, q0, qd0, qtraj, qdtraj, uapp, h, pscale)
    L, gq, gqd, gu = loss_and_cotangents(qtraj, qdtraj, uapp, c, d, e)
    x = start_states(q0, qd0, qtraj, qdtraj)
    out = vjp(integ, H, M, D, K, x if xref is None else x - xref, gq, gqd, gu, h, pscale)
    return dict(out, qtraj=qtraj, qdtraj=qdtraj, uapp=uapp, L=L, gq=gq, gqd=gqd, gu=gu)
