"""'rollout_vjp_forces' through the MEX gateway (stub): the command is in the gateway's table and asks for a handle; on a device it
checks its arguments in the gateway's words and reaches rmx_rollout_vjp_forces on every shard.

A gateway handle is a group, and a group takes no force table (rmx_group_create; GroupSim refuses such a scene), so no tape behind a
handle carries point forces yet: what a device can show today is that the command arrives in the library with the caller's arrays and
that the library's refusal of a tape without point forces - the words the ctypes call gets on the same model - comes back through it,
leaving the tape usable.  The bit-for-bit comparison with the ctypes call needs force tables in groups first."""
import numpy as np
import pytest

from test_mex_cost import _Gateway, _cm
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)


def test_the_command_is_in_the_table_and_asks_for_a_handle(gw):  # noqa: F811
    with pytest.raises(MexError, match="handle"):
        gw.call(6, "rollout_vjp_forces", np.array([[12345]], dtype=np.uint64), 2.0, np.zeros((1, 2)), np.zeros((1, 2)), 4.0)
    with pytest.raises(MexError, match="handle"):
        gw.call(6, "rollout_vjp_forces")


def test_hipsim_has_the_method():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "matlab", "+redmax", "HipSim.m")).read()
    assert "function [du, dq0, dqd0, fgrads, grads] = rolloutVjpForces(this, nsteps, gq, gqd, nforces)" in src
    assert src.count("redmax_hip_mex('rollout_vjp_forces', this.h, nsteps, gq, gqd, nforces)") == 2


@pytest.mark.gpu
def test_the_command_reaches_the_library_on_every_shard(gw):  # noqa: F811
    from redmax_amd import BatchSim, _abi, scenesRedMax
    g = _Gateway(gw.L)
    sc = scenesRedMax(2)
    sc.init()
    B, N = 3, 3
    h = g.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    q0, qd0 = sc.getQ()
    rng = np.random.default_rng(5)
    q = q0[None] + 0.05 * rng.standard_normal((B, sc.nr))
    qd = qd0[None] + 0.2 * rng.standard_normal((B, sc.nr))
    u = 0.1 * rng.standard_normal((B, N, sc.nr))
    gq = rng.standard_normal((B, N, sc.nr))
    g.call(0, "set", h, _cm(q), _cm(qd))
    g.call(2, "rollout_tape", h, float(sc.h), float(N), 1.0, _cm(u))
    before = g.call(3, "rollout_vjp", h, float(N), _cm(gq), _cm(gq))
    words = "rmx_rollout_vjp_forces: the tape carries no point forces"
    for nlhs in (6, 11):
        with pytest.raises(MexError, match=words):
            g.call(nlhs, "rollout_vjp_forces", h, float(N), _cm(gq), _cm(gq), 4.0)
    # the gateway's own checks
    with pytest.raises(MexError, match="usage"):
        g.call(6, "rollout_vjp_forces", h, float(N), _cm(gq), _cm(gq))
    with pytest.raises(MexError, match="nforces must be an integer"):
        g.call(6, "rollout_vjp_forces", h, float(N), _cm(gq), _cm(gq), 33.0)
    with pytest.raises(MexError, match="nforces must be an integer"):
        g.call(6, "rollout_vjp_forces", h, float(N), _cm(gq), _cm(gq), 1.5)
    with pytest.raises(MexError, match="nsteps must be at least 1"):
        g.call(6, "rollout_vjp_forces", h, 0.0, _cm(gq), _cm(gq), 4.0)
    after = g.call(3, "rollout_vjp", h, float(N), _cm(gq), _cm(gq))
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    g.call(0, "destroy", h)
    # the ctypes call on the same model and tape: the same words
    sim = BatchSim(sc, batch=B)
    sim.set_state(q, qd)
    sim.rollout_tape(N, sc.h, u)
    with pytest.raises(_abi.RedMaxHipError, match=words):
        sim.rollout_vjp_forces(N, gq, gq)
    sim.close()
