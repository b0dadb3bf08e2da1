"""numpy definition of the cost rmx_rollout_search evaluates inside its launch (development aid + executable derivation; NOT the
oracle and NOT the product), on a GIVEN record of one rollout:

    J = sum_{k=1..N} [ 1/2 dx_k' Q_k dx_k  +  1/2 u_k' R u_k  +  sum_{t: step_t = k} wpos/2 |r|^2 + wvel/2 |rv|^2 + wrot/4 |R - Rtarget|_F^2 ]

with x_k = (q_k, qdot_k) the state after step k (row k-1 of the record), u_k the APPLIED torque of step k and the state and term
parts those of proto_frame_cost.cost - its Jk, which this module does not restate.  The sum runs over the steps in ascending order;
within a step the state part and the terms (proto_frame_cost's Jk[k]) and the control part are added.  The kernel adds the control
part between the state part and the terms: one value, another order of three additions per step - the GPU test judges both against
the longdouble evaluation of this module by the project's rule.  Every function takes a dtype (float64: the reference; longdouble:
what the reference and the device are judged against).
"""
import numpy as np

import proto_frame_cost as F


def control_part(u, R, dtype=np.float64):
    """Ju [N] = 1/2 u_k' R u_k; R None: zeros."""
    u = np.asarray(u, dtype=dtype)
    if R is None:
        return np.zeros(u.shape[0], dtype=dtype)
    R = np.asarray(R, dtype=dtype)
    return np.array([u[k] @ (R @ u[k]) / 2 for k in range(u.shape[0])], dtype=dtype)


def cost(m, q, qd, u, Q=None, xgoal=None, R=None, terms=None, xtarget=None, vtarget=None, Rtarget=None, dtype=np.float64):
    """dict(J, Jk [N], Ju [N]) of ONE rollout: the record q, qd [N][nr] and the applied torques u [N][nr].  Q, xgoal None: no state
    part; terms None: no terms; R None: no control part."""
    q, qd = np.asarray(q, dtype=dtype), np.asarray(qd, dtype=dtype)
    N = q.shape[0]
    if Q is None and xgoal is None and not terms:
        Jk = np.zeros(N, dtype=dtype)
    else:
        Jk = F.cost(m, q, qd, Q, xgoal, terms or (), xtarget, vtarget, Rtarget, dtype)["Jk"]
    Ju = control_part(u, R, dtype)
    J = dtype(0)
    for k in range(N):
        J = J + (Jk[k] + Ju[k])
    return dict(J=J, Jk=Jk, Ju=Ju)


def rel_err(a, b):
    """|a - b| / |b| of two values, b in the wider type."""
    return float(abs(np.longdouble(a) - np.longdouble(b)) / abs(np.longdouble(b)))
