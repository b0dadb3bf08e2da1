"""'rollout_lqr' through the MEX gateway (stub), over two shards: MATLAB's column-major arrays are the ABI's - lx 2nr x nsteps x B,
lu and kff nr x nsteps x B, Q 2nr x 2nr x nsteps [x B], K nr x 2nr x nsteps x B with K(i,j,k,b) = du_i/dx_j - and the command returns
the bits of the ctypes call.  Two costs: the diagonal one of test_gpu_ilqr._problem (per rollout: copies, the third doubled) and
proto_lqr_backward.dense_cost, shared and per rollout - tables that differ in every entry, so that the offset of a shard's first
table in Q matters in all of them."""
import numpy as np
import pytest

import proto_lqr_backward as P
from test_gpu_rollout_lqr import B, MU, _cost, _setup, _tape
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)


@pytest.mark.gpu
def test_mex_command_equals_the_ctypes_call(gw):  # noqa: F811
    from redmax_amd import BatchSim
    sc, cs, N = _setup(5)
    nr = sc.nr
    sim = BatchSim(sc, batch=B)
    qt, qdt = _tape(sim, sc, cs)
    lx, lu, Q, R = _cost(sc, cs, qt, qdt)
    Qb = np.tile(Q, (B, 1, 1, 1))
    Qb[2] *= 2.0
    dQ, dR = P.dense_cost(9300, nr, N)
    dQb, _ = P.dense_cost(9300, nr, N, B=B)
    assert all(np.abs(dQb[i] - dQb[j]).min() > 0 for i in range(B) for j in range(i))      # no two rollouts share an entry
    costs = [(lx, lu, Q, R), (lx, lu, Qb, R), _cost(sc, cs, qt, qdt, QR=(dQ, dR)), _cost(sc, cs, qt, qdt, QR=(dQb, dR))]
    refs = [sim.rollout_lqr(N, *c, mu=MU) for c in costs]
    sim.close()
    assert not np.array_equal(refs[2][1], refs[3][1]) and not np.array_equal(refs[3][1][2], refs[3][1][1])
    h = gw.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    args = (lx.transpose(2, 1, 0), lu.transpose(2, 1, 0), Q.transpose(2, 1, 0), R.T)
    with pytest.raises(MexError, match="no tape"):
        gw.call(4, "rollout_lqr", h, float(N), *args, MU)
    gw.call(0, "set", h, cs["q0"].T, cs["qd0"].T)
    gw.call(3, "rollout_tape", h, sc.h, float(N), float(sc.task["pscale"]), cs["u"].transpose(2, 1, 0))
    for (clx, clu, cQ, cR), want in zip(costs, refs):
        Qm = cQ.transpose(2, 1, 0) if cQ.ndim == 3 else cQ.transpose(3, 2, 1, 0)
        kff, K, expected, notpd = gw.call(4, "rollout_lqr", h, float(N), clx.transpose(2, 1, 0), clu.transpose(2, 1, 0), Qm, cR.T, MU)
        assert kff.shape == (nr, N, B) and K.shape == (nr, 2 * nr, N, B)
        assert np.array_equal(kff.transpose(2, 1, 0), want[0])
        assert np.array_equal(K.transpose(3, 2, 1, 0), want[1])            # [B][N][2nr][nr]: K(i,j,k,b) at [b][k][j][i]
        assert np.array_equal(np.asarray(expected).reshape(-1), want[2]) and not np.asarray(notpd).any()
    (kff,) = (gw.call(1, "rollout_lqr", h, float(N), *args),)              # one output, the default mu = 0
    assert np.asarray(kff).shape == (nr, N, B)
    with pytest.raises(MexError, match="nsteps differs"):
        gw.call(4, "rollout_lqr", h, float(N - 1), args[0][:, :-1], args[1][:, :-1], args[2][:, :, :-1], args[3], MU)
    with pytest.raises(MexError, match="lx must be"):
        gw.call(4, "rollout_lqr", h, float(N), args[0][:, :-1], args[1], args[2], args[3], MU)
    gw.call(0, "destroy", h)
