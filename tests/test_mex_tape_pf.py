"""'tape_point_forces' through the MEX gateway (stub): the command is in the gateway's table and asks for a handle; on a device it
sets the switch on the model of every shard, reads it back, refuses an enable that is not 0 or 1, and leaves the rollout of a model
without a force table alone, bit for bit."""
import numpy as np
import pytest

from test_mex_cost import _Gateway, _cm
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)


def test_the_command_is_in_the_table_and_asks_for_a_handle(gw):  # noqa: F811
    with pytest.raises(MexError, match="handle"):
        gw.call(1, "tape_point_forces", np.array([[12345]], dtype=np.uint64), 1.0)
    with pytest.raises(MexError, match="handle"):
        gw.call(1, "tape_point_forces")


@pytest.mark.gpu
def test_the_switch_over_two_shards(gw):  # noqa: F811
    from redmax_amd import scenesRedMax
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

    def tape():
        g.call(0, "set", h, _cm(q), _cm(qd))
        return g.call(2, "rollout_tape", h, float(sc.h), float(N), 1.0, _cm(u))

    off = tape()
    assert g.call(1, "tape_point_forces", h, 1.0) == 1.0
    on = tape()
    assert g.call(1, "tape_point_forces", h, 0.0) == 0.0
    assert np.array_equal(off[0], on[0]) and np.array_equal(off[1], on[1])
    with pytest.raises(MexError, match="0 or 1"):
        g.call(0, "tape_point_forces", h, 2.0)
    with pytest.raises(MexError, match="enable"):
        g.call(0, "tape_point_forces", h)
    g.call(0, "destroy", h)
