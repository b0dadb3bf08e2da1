"""The formulas of rmx_rollout_linearize, pinned on the CPU before any GPU run (tests/proto_rollout_linearize.py, on the oracle's tape):

  - A_1, B_1 of the BDF1 assembly against central differences (eps 1e-6) of one oracle step, elementwise to 2e-5 |A| + 1e-6 max|A|,
    the project's testGrad bound.  Measured: max abs error 9.9e-9 on the 5-link chain, 2.1e-9 on the 7-joint tree.
  - The backward chain with A_k', B_k' equals the recursion of tests/proto_rollout_vjp.py (5, tree7, 16, 32) to 1e-10 relative;
    measured <= 2.0e-12.
  - The BDF2 recursion on XA, XB, XU equals tests/proto_rollout_vjp_bdf2.py on its N + 1-slot tape (5, tree7), same bound.
  - The two entry points are declared, bound and exported.

Inputs: case(sc, 17) of tests/test_rollout_vjp_proto.py and the step counts of tests/test_gpu_rollout_vjp.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import proto_rollout_linearize as lin
import proto_rollout_vjp as proto1
import proto_rollout_vjp_bdf2 as proto2
from test_gpu_adjoint_controls import _scene
from test_rollout_vjp_proto import case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {5: 6, "tree7": 6, 16: 5, 32: 4}      # (tests/test_gpu_rollout_vjp.py STEPS)
NAMES = ("rmx_rollout_linearize", "rmx_rollout_linearize_device")


def _case0(sc, nsteps):
    return {k: v[0] for k, v in case(sc, 17, nsteps=nsteps).items()}


@pytest.mark.parametrize("size", [5, "tree7"])
def test_first_step_meets_central_differences(oracle_lib, size):
    sc = _scene(size, 1)
    h, pscale, nr = sc.h, sc.task["pscale"], sc.nr
    cs = _case0(sc, STEPS[size])
    u1 = cs["u"][:1]
    qt, qdt = proto1.rollout(oracle_lib, sc, cs["q0"], cs["qd0"], u1, h, pscale)
    H, M, D = proto1.tape(oracle_lib, sc, cs["q0"], cs["qd0"], qt, qdt, h)
    A, Bm = lin.assemble_bdf1(*lin.sens(H[0], M[0], D[0], h, pscale), h)

    def step(x, u):
        a, b = proto1.rollout(oracle_lib, sc, x[:nr], x[nr:], u[None], h, pscale)
        return np.concatenate([a[0], b[0]])

    eps = 1e-6
    x0 = np.concatenate([cs["q0"], cs["qd0"]])
    An, Bn = np.empty_like(A), np.empty_like(Bm)
    for j in range(2 * nr):
        e = np.zeros(2 * nr)
        e[j] = eps
        An[:, j] = (step(x0 + e, u1[0]) - step(x0 - e, u1[0])) / (2 * eps)
    for j in range(nr):
        e = np.zeros(nr)
        e[j] = eps
        Bn[:, j] = (step(x0, u1[0] + e) - step(x0, u1[0] - e)) / (2 * eps)
    for name, ana, num in (("A", A, An), ("B", Bm, Bn)):
        err = np.abs(num - ana)
        print("linearize proto %s, %s_1: max |num - ana| = %.3e, max|ana| = %.3e, relative Frobenius %.3e"
              % (size, name, err.max(), np.abs(ana).max(), lin.rel(num, ana)))
        assert np.abs(ana).max() > 0
        assert (err <= 2e-5 * np.abs(ana) + 1e-6 * np.abs(ana).max()).all(), (name, err.max())


@pytest.mark.parametrize("size", [5, "tree7", 16, 32])
def test_bdf1_chain_is_the_vjp_recursion(oracle_lib, size):
    sc = _scene(size, 1)
    h, pscale = sc.h, sc.task["pscale"]
    cs = _case0(sc, STEPS[size])
    qt, qdt = proto1.rollout(oracle_lib, sc, cs["q0"], cs["qd0"], cs["u"], h, pscale)
    H, M, D = proto1.tape(oracle_lib, sc, cs["q0"], cs["qd0"], qt, qdt, h)
    _, gq, gqd = proto1.loss_and_cotangents(qt, qdt, cs["c"], cs["d"])
    ref = proto1.vjp(H, M, D, gq, gqd, h, pscale)
    A, Bm = lin.assemble_bdf1(*lin.sens(H, M, D, lin.etas(len(qt), h, 1), pscale), h)
    got = lin.chain_bdf1(A, Bm, gq, gqd)
    errs = tuple(lin.rel(a, b) for a, b in zip(got, ref))
    print("linearize proto %s: chain against vjp du %.3e dq0 %.3e dqd0 %.3e; max|A| %.3g max|B| %.3g, max cond(H) %.3g"
          % ((size,) + errs + (np.abs(A).max(), np.abs(Bm).max(), max(np.linalg.cond(x) for x in H))))
    assert max(errs) <= 1e-10, (size, errs)


@pytest.mark.parametrize("size", [5, "tree7"])
def test_bdf2_recursion_on_the_sensitivities_is_the_vjp_recursion(oracle_lib, size):
    sc = _scene(size, 2)
    h, pscale = sc.h, sc.task["pscale"]
    cs = _case0(sc, STEPS[size])
    qt, qdt, H, M, D = proto2.forward(oracle_lib, sc, cs["q0"], cs["qd0"], cs["u"], h, pscale)
    assert H.shape[0] == len(qt) + 1
    _, gq, gqd = proto2.loss_and_cotangents(qt, qdt, cs["c"], cs["d"])
    ref = proto2.vjp(H, M, D, gq, gqd, h, pscale)
    XA, XB, XU = lin.sens(H, M, D, lin.etas(len(qt), h, 2), pscale)
    got = lin.vjp_bdf2(XA, XB, XU, gq, gqd, h)
    errs = tuple(lin.rel(a, b) for a, b in zip(got, ref))
    print("linearize proto bdf2 %s: X-form against vjp du %.3e dq0 %.3e dqd0 %.3e" % ((size,) + errs))
    assert max(errs) <= 1e-10, (size, errs)


def test_entry_points_are_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from redmax_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "redmax_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_abi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _abi.SYMBOLS
        assert hasattr(L, name), name
    assert _abi.lib().rmx_version() == 111
