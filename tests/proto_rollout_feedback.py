"""The closed loop of rmx_rollout_tape_feedback (include/redmax_hip.h) in numpy, on top of the CPU oracle: a reference for the GPU
tests that shares no code with the library.

BDF1: one oracle step at a time (oracle_rollout_per_step of tests/test_gpu_adjoint_controls.py, through proto_rollout_vjp.rollout with
a one-row torque array), the torque of step k recomputed from the state the loop has reached:
    uapp_k = uff_k + K_k' (x_{k-1} - xref_{k-1}),     x = (q, qdot),     K_k[j][i] = du_i/dx_j   (the ABI's table as a C array)
BDF2: the solves of proto_rollout_vjp_bdf2 (its own Newton iteration on the oracle's residual), the torque of step 1 holding for both
SDIRK2 solves.  oracle_rollout_per_step asserts that the oracle's Newton iteration converged in every step, and the BDF2 proto's
raises where it does not settle: a rollout these functions return is one every solve of which converged.
"""
import numpy as np

import proto_rollout_vjp as proto1
import proto_rollout_vjp_bdf2 as proto2


def torque(uff_k, K_k, xref_k, q, qd):
    """uff_k [nr] + K_k' (x - xref_k): K_k [2nr][nr] or None (no feedback), xref_k [2nr] or None (zero)."""
    if K_k is None:
        return np.array(uff_k, dtype=np.float64)
    x = np.concatenate([q, qd])
    return uff_k + K_k.T @ (x if xref_k is None else x - xref_k)


def rollout(orc, sc, q0, qd0, uff, K, xref, h, pscale):
    """The closed loop under BDF1 for ONE rollout: (qtraj, qdtraj, uapp), each [nsteps][nr].  uff [nsteps][nr], K [nsteps][2nr][nr] or
    None, xref [nsteps][2nr] or None."""
    uff = np.asarray(uff, dtype=np.float64)
    q, qd = np.array(q0, dtype=np.float64), np.array(qd0, dtype=np.float64)
    qtraj, qdtraj, uapp = (np.empty_like(uff) for _ in range(3))
    for k in range(uff.shape[0]):
        uapp[k] = torque(uff[k], None if K is None else K[k], None if xref is None else xref[k], q, qd)
        qt, qdt = proto1.rollout(orc, sc, q, qd, uapp[k:k + 1], h, pscale)
        q, qd = qt[0], qdt[0]
        qtraj[k], qdtraj[k] = q, qd
    return qtraj, qdtraj, uapp


def rollout_bdf2(orc, sc, q0, qd0, uff, K, xref, h, pscale):
    """The closed loop under BDF2, self-started with SDIRK2 (the torque of step 1 holds for both solves): (qtraj, qdtraj, uapp)."""
    AL, newton = proto2.AL, proto2._newton
    o = orc.Oracle(sc.desc())
    uff = np.asarray(uff, dtype=np.float64)
    N = uff.shape[0]
    q0, qd0 = np.array(q0, dtype=np.float64), np.array(qd0, dtype=np.float64)
    qtraj, qdtraj, uapp = (np.empty_like(uff) for _ in range(3))

    def tq(k, q, qd):
        return torque(uff[k], None if K is None else K[k], None if xref is None else xref[k], q, qd)

    uapp[0] = tq(0, q0, qd0)
    eta = AL * h
    qa, qda = newton(o, q0, q0 + AL * h * qd0, eta, pscale * uapp[0], q0 + AL * h * qd0)[:2]
    qA = q0 + (1.0 - AL) * h * qda
    qB = q0 + (2.0 * AL - 1.0) * h * qd0 + 2.0 * (1.0 - AL) * h * qda
    qtraj[0], qdtraj[0] = newton(o, qA, qB, eta, pscale * uapp[0], qa + (1.0 - AL) * h * qda)[:2]
    qm, qdm = q0, qd0
    eta = 2.0 * h / 3.0
    for k in range(1, N):
        qk, qdk = qtraj[k - 1], qdtraj[k - 1]
        uapp[k] = tq(k, qk, qdk)
        qA = 4.0 / 3.0 * qk - 1.0 / 3.0 * qm
        qB = qA + 8.0 / 9.0 * h * qdk - 2.0 / 9.0 * h * qdm
        qtraj[k], qdtraj[k] = newton(o, qA, qB, eta, pscale * uapp[k], qk + h * qdk)[:2]
        qm, qdm = qk, qdk
    return qtraj, qdtraj, uapp
