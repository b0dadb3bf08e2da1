"""'rollout_jvp_params' through the MEX gateway (stub): the command is in the gateway's table, asks for a handle and is documented in
the command list; HipSim has the method; on a device the gateway's own usage errors come in its words
(tests/test_gpu_rollout_jvp_params.py compares the command with the ctypes call bit for bit)."""
import os

import numpy as np
import pytest

from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE = r"usage: \[tq,tqd\] = redmax_hip_mex\('rollout_jvp_params', h, nsteps, tk, td, tqrest, tI, tgrav, tu, tq0, tqd0\)"


def test_the_command_is_in_the_table_and_asks_for_a_handle(gw):  # noqa: F811
    e = np.zeros((0, 0))
    with pytest.raises(MexError, match="handle"):
        gw.call(2, "rollout_jvp_params", np.array([[12345]], dtype=np.uint64), 2.0, np.zeros((2, 1)), e, e, e, e, e, e, e)
    with pytest.raises(MexError, match="handle"):
        gw.call(2, "rollout_jvp_params")


def test_the_command_list_and_hipsim_have_it():
    src = open(os.path.join(ROOT, "mex", "redmax_hip_mex.c")).read()
    assert "[tq,tqd] = redmax_hip_mex('rollout_jvp_params', h, nsteps, tk, td, tqrest, tI, tgrav, tu, tq0, tqd0)" in src.split("*/")[0]
    m = open(os.path.join(ROOT, "matlab", "+redmax", "HipSim.m")).read()
    assert "function [tq, tqd] = rolloutJvpParams(this, nsteps, tp, tu, tq0, tqd0)" in m
    assert "redmax_hip_mex('rollout_jvp_params', this.h, nsteps, args{:}, tu, tq0, tqd0)" in m
    assert "rolloutJvpParams" in open(os.path.join(ROOT, "matlab", "README.md")).read()


@pytest.mark.gpu
def test_usage_errors_in_the_gateways_words(gw):  # noqa: F811
    from redmax_amd import scenesRedMax
    sc = scenesRedMax(2)
    sc.init()
    B = 3
    e = np.zeros((0, 0))
    h = gw.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    tk = np.zeros((sc.nr, 2, B))
    with pytest.raises(MexError, match=USAGE):
        gw.call(2, "rollout_jvp_params", h, 3.0, tk, e, e, e, e, e, e)
    with pytest.raises(MexError, match="rollout_jvp_params: nsteps must be at least 1"):
        gw.call(2, "rollout_jvp_params", h, 0.0, tk, e, e, e, e, e, e, e)
    with pytest.raises(MexError, match="rollout_jvp_params: tI must be a real double array of %d x ntan x %d elements, the same ntan" % (6 * len(sc.joints), B)):
        gw.call(2, "rollout_jvp_params", h, 3.0, tk, e, e, np.zeros((6, len(sc.joints), 3, B)), e, e, e, e)
    with pytest.raises(MexError, match="rollout_jvp_params: tgrav must be a real double array of 3 x ntan x %d" % B):
        gw.call(2, "rollout_jvp_params", h, 3.0, e, e, e, e, np.zeros((2, 2, B)), e, e, e)
    with pytest.raises(MexError, match="rmx_rollout_jvp_params: no tape"):
        gw.call(2, "rollout_jvp_params", h, 3.0, tk, e, e, e, e, e, e, e)
    gw.call(0, "destroy", h)
