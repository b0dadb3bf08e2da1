"""'rollout_frames' and 'rollout_cost_frames' through the MEX gateway (stub), over two shards: MATLAB's column-major arrays are the
ABI's - q, qdot, gq, gqd nr x nsteps x B; x, v, gx, gv, xtarget, vtarget 3 x nterms [x B]; R, gR, Rtarget 3 x 3 x nterms [x B] (the
library's column-major 3x3 as it stands); terms a struct array with 1-based bodies and optional weights - and the commands return the
bits of the ctypes calls.  On a CPU: the commands are in the gateway's table and refuse a handle that does not exist."""
import numpy as np
import pytest

from test_gpu_rollout_frames import B, N, _case, _frames, _gpu
from test_mex_cost import _Gateway, _cm
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)


def test_the_commands_are_in_the_table_and_ask_for_a_handle(gw):  # noqa: F811
    for cmd in ("rollout_frames", "rollout_cost_frames"):
        with pytest.raises(MexError, match="handle"):
            gw.call(1, cmd, np.array([[12345]], dtype=np.uint64))
        with pytest.raises(MexError, match="handle"):
            gw.call(1, cmd)


def _r(a):
    """[B][T][3][3] with R[..., r, c] -> MATLAB's 3 x 3 x T x B: _cm of the column-major copy."""
    return _cm(np.ascontiguousarray(np.swapaxes(a, -1, -2)))


@pytest.mark.gpu
def test_mex_commands_equal_the_ctypes_calls(gw):  # noqa: F811
    from redmax_amd import BatchSim
    g = _Gateway(gw.L)
    c = _case("tree7")
    nr, T, cot = c["sc"].nr, len(c["terms"]), c["cot"]
    sim = BatchSim(c["sc"], batch=B)
    want = {k: _gpu(sim, c, c[k]) for k in ("per", "shared")}
    fr = _frames(sim, c)
    _, gq_v, gqd_v = sim.rollout_frames(N, c["q"], c["qd"], c["terms"], gv=cot["gv"], want=())
    novel = [dict(t, wvel=0.0) for t in c["terms"]]
    only = sim.rollout_cost_frames(N, c["q"], c["qd"], terms=novel, xtarget=c["shared"]["xtarget"], Rtarget=c["shared"]["Rtarget"])
    sim.close()
    terms = [dict(body=float(t["body"] + 1), xlocal=np.array(t["xlocal"]), step=float(t["step"]), wpos=float(t["wpos"]), wvel=float(t["wvel"]),
                  wrot=float(t["wrot"])) for t in c["terms"]]
    bare = [dict(body=t["body"], xlocal=t["xlocal"], step=t["step"]) for t in terms]      # (no weights: a missing one is 0)
    h = g.call(1, "create", flatten(c["sc"]), float(B), np.array([0.0, 0.0]))
    none = np.zeros((0, 0))
    q, qd = _cm(c["q"]), _cm(c["qd"])
    for k in ("per", "shared"):
        tab = c[k]
        Jk, lx, Q = g.call(3, "rollout_cost_frames", h, float(N), q, qd, _cm(tab["Q"]), _cm(tab["xgoal"]), terms, _cm(tab["xtarget"]),
                           _cm(tab["vtarget"]), _r(tab["Rtarget"]))
        assert Jk.shape == (N, B) and lx.shape == (2 * nr, N, B) and Q.shape == (2 * nr, 2 * nr, N, B)
        assert np.array_equal(_cm(Jk), want[k]["Jk"]) and np.array_equal(_cm(lx), want[k]["lx"]) and np.array_equal(_cm(Q), want[k]["Q"])
    nv = [dict(t, wvel=0.0) for t in terms]
    Jk, lx = g.call(2, "rollout_cost_frames", h, float(N), q, qd, none, none, nv, _cm(c["shared"]["xtarget"]), none, _r(c["shared"]["Rtarget"]))
    assert np.array_equal(_cm(Jk), only["Jk"]) and np.array_equal(_cm(lx), only["lx"])
    x, v, R, gq, gqd = g.call(5, "rollout_frames", h, float(N), q, qd, bare, _cm(cot["gx"]), _cm(cot["gv"]), _r(cot["gR"]))
    assert x.shape == (3, T, B) and v.shape == (3, T, B) and R.shape == (3, 3, T, B) and gq.shape == (nr, N, B) and gqd.shape == (nr, N, B)
    assert all(np.array_equal(_cm(a), fr[n]) for a, n in ((x, "x"), (v, "v"), (gq, "gq"), (gqd, "gqd")))
    assert np.array_equal(np.swapaxes(_cm(R), -1, -2), fr["R"])
    x, v, R = g.call(3, "rollout_frames", h, float(N), q, qd, bare)
    assert np.array_equal(_cm(x), fr["x"]) and np.array_equal(_cm(v), fr["v"]) and np.array_equal(np.swapaxes(_cm(R), -1, -2), fr["R"])
    _, _, _, gq, gqd = g.call(5, "rollout_frames", h, float(N), q, qd, bare, none, _cm(cot["gv"]), none)
    assert np.array_equal(_cm(gq), gq_v) and np.array_equal(_cm(gqd), gqd_v)
    with pytest.raises(MexError, match="qdot must be"):
        g.call(1, "rollout_frames", h, float(N), q, qd[:, :-1], bare)
    with pytest.raises(MexError, match="gq needs gx, gv or gR"):
        g.call(4, "rollout_frames", h, float(N), q, qd, bare)
    with pytest.raises(MexError, match="Rtarget must be"):
        g.call(1, "rollout_cost_frames", h, float(N), q, qd, none, none, terms, _cm(c["shared"]["xtarget"]), _cm(c["shared"]["vtarget"]),
               _r(c["shared"]["Rtarget"])[:, :, :-1])
    with pytest.raises(MexError, match="must all be shared by the batch or all hold one table per rollout"):
        g.call(1, "rollout_cost_frames", h, float(N), q, qd, none, none, terms, _cm(c["per"]["xtarget"]), _cm(c["shared"]["vtarget"]),
               _r(c["shared"]["Rtarget"]))
    with pytest.raises(MexError, match="term 0: wvel > 0 needs vtarget, which is null"):
        g.call(1, "rollout_cost_frames", h, float(N), q, qd, none, none, terms, _cm(c["shared"]["xtarget"]), none, _r(c["shared"]["Rtarget"]))
    with pytest.raises(MexError, match="null argument"):
        g.call(1, "rollout_cost_frames", h, float(N), q, qd, none, none, none, none, none, none)
    g.call(0, "destroy", h)
