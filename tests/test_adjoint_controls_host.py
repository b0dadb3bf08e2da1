"""rmx_adjoint_controls, the checks that need no GPU: the step-by-step oracle driver the GPU tests rely on, and the MEX command's
place in the gateway."""
import numpy as np
import pytest

from test_gpu_adjoint_controls import _rel, _scene, oracle_rollout_per_step
from test_mex_gateway import MexError, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)


def test_per_step_oracle_helper_reproduces_one_call(oracle_lib):
    """(CPU arithmetic only.)  Under constant controls the step-by-step helper is the oracle's single adjoint call to roundoff."""
    sc = _scene(5, 1)
    nsteps = 10
    p = 0.1 * np.random.default_rng(2).standard_normal(sc.nr)
    task = dict(sc.task, t=6 * sc.h)
    o = oracle_lib.Oracle(sc.desc())
    Po, _, st = o.adjoint_bdf1(sc.h, nsteps, dict(task, wreg=0.0), p)
    qo, qdo = o.get_state()
    q, qd, P, iters = oracle_rollout_per_step(oracle_lib, sc, sc.h, nsteps, task, np.repeat(p[None, :], nsteps, axis=0))
    assert _rel(q, qo) <= 1e-13 and _rel(qd, qdo) <= 1e-10, (_rel(q, qo), _rel(qd, qdo))
    assert abs(P - Po) <= 1e-13 * abs(Po) and iters == st.newton_iters


def test_mex_command_checks_its_handle(gw):  # noqa: F811
    """'adjoint_controls' is a command of the gateway and, like every command that names a handle, refuses a made-up one."""
    with pytest.raises(MexError, match="handle"):
        gw.call(1, "adjoint_controls", np.array([[12345]], dtype=np.uint64), 1e-2, 4.0, {}, np.zeros((2, 4, 1)))
    with pytest.raises(MexError, match="handle"):
        gw.call(1, "adjoint_controls")
