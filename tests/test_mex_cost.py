"""'rollout_points' and 'rollout_cost' through the MEX gateway (stub), over two shards: MATLAB's column-major arrays are the ABI's -
q, qdot, gq nr x nsteps x B, x, gx, xtarget 3 x nterms [x B], Qin, Q 2nr x 2nr x nsteps [x B], xgoal, lx 2nr x nsteps [x B], Jk
nsteps x B, terms a struct array with 1-based bodies - and the commands return the bits of the ctypes calls.  The tables differ in
every entry from rollout to rollout, so that the offset of a shard's first table matters in all of them."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_rollout_cost import B, N, _case, _gpu
from test_mex_gateway import Gateway, MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)


class _Gateway(Gateway):
    """Gateway with MATLAB struct ARRAYS: a list of dicts with the same keys becomes a 1 x n struct."""

    def to_mx(self, v):
        if isinstance(v, list) and v and isinstance(v[0], dict):
            L, names = self.L, list(v[0])
            s = L.mxCreateStructMatrix(1, len(v), len(names), (C.c_char_p * len(names))(*[k.encode() for k in names]))
            for i, d in enumerate(v):
                for k in names:
                    L.mxSetField(s, i, k.encode(), Gateway.to_mx(self, d[k]))
            return s
        return Gateway.to_mx(self, v)


def _cm(a):
    """[B][..] row-major -> MATLAB's .. x B column-major view of the same memory order."""
    return a.transpose(*range(a.ndim - 1, -1, -1))


@pytest.mark.gpu
def test_mex_commands_equal_the_ctypes_calls(gw):  # noqa: F811
    from redmax_amd import BatchSim
    g = _Gateway(gw.L)
    c = _case("tree7")
    nr, T = c["sc"].nr, len(c["terms"])
    sim = BatchSim(c["sc"], batch=B)
    want = {k: _gpu(sim, c, c[k]) for k in ("per", "shared")}
    bare = sim.rollout_cost(N, c["q"], c["qd"], Q=c["per"]["Q"], xgoal=c["per"]["xgoal"])
    only = sim.rollout_cost(N, c["q"], c["qd"], terms=c["terms"], xtarget=c["shared"]["xtarget"])
    x, gq = sim.rollout_points(N, c["q"], c["terms"], gx=c["gx"])
    sim.close()
    terms = [dict(body=float(t["body"] + 1), xlocal=np.array(t["xlocal"]), step=float(t["step"]), wpos=float(t["wpos"])) for t in c["terms"]]
    h = g.call(1, "create", flatten(c["sc"]), float(B), np.array([0.0, 0.0]))
    none = np.zeros((0, 0))
    for k in ("per", "shared"):
        tab = c[k]
        Jk, lx, Q = g.call(3, "rollout_cost", h, float(N), _cm(c["q"]), _cm(c["qd"]), _cm(tab["Q"]), _cm(tab["xgoal"]), terms, _cm(tab["xtarget"]))
        assert Jk.shape == (N, B) and lx.shape == (2 * nr, N, B) and Q.shape == (2 * nr, 2 * nr, N, B)
        assert np.array_equal(_cm(Jk), want[k]["Jk"]) and np.array_equal(_cm(lx), want[k]["lx"]) and np.array_equal(_cm(Q), want[k]["Q"])
    Jk, lx, Q = g.call(3, "rollout_cost", h, float(N), _cm(c["q"]), _cm(c["qd"]), _cm(c["per"]["Q"]), _cm(c["per"]["xgoal"]), none, none)
    assert all(np.array_equal(_cm(a), bare[n]) for a, n in ((Jk, "Jk"), (lx, "lx"), (Q, "Q")))
    Jk, lx = g.call(2, "rollout_cost", h, float(N), _cm(c["q"]), _cm(c["qd"]), none, none, terms, _cm(c["shared"]["xtarget"]))
    assert np.array_equal(_cm(Jk), only["Jk"]) and np.array_equal(_cm(lx), only["lx"])
    xm, gm = g.call(2, "rollout_points", h, float(N), _cm(c["q"]), terms, _cm(c["gx"]))
    assert xm.shape == (3, T, B) and gm.shape == (nr, N, B)
    assert np.array_equal(_cm(xm), x) and np.array_equal(_cm(gm), gq)
    assert np.array_equal(_cm(g.call(1, "rollout_points", h, float(N), _cm(c["q"]), terms)), x)
    with pytest.raises(MexError, match="q must be"):
        g.call(1, "rollout_points", h, float(N), _cm(c["q"])[:, :-1], terms)
    with pytest.raises(MexError, match="gq needs gx"):
        g.call(2, "rollout_points", h, float(N), _cm(c["q"]), terms)
    with pytest.raises(MexError, match="xtarget must be"):
        g.call(1, "rollout_cost", h, float(N), _cm(c["q"]), _cm(c["qd"]), none, none, terms, _cm(c["shared"]["xtarget"])[:, :-1])
    with pytest.raises(MexError, match="null argument"):
        g.call(1, "rollout_cost", h, float(N), _cm(c["q"]), _cm(c["qd"]), none, none, none, none)
    bad = [dict(t, step=float(N + 1)) if i == 1 else t for i, t in enumerate(terms)]
    with pytest.raises(MexError, match=r"term 1: step %d is outside \[1, %d\]" % (N + 1, N)):
        g.call(1, "rollout_points", h, float(N), _cm(c["q"]), bad)
    g.call(0, "destroy", h)
