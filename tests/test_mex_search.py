"""'rollout_search' through the MEX gateway (stub), over two shards: MATLAB's column-major arrays are the ABI's - ubar, kff, qtraj,
qdtraj, uapp nr x nsteps x B; K nr x 2nr x nsteps x B and xref 2nr x nsteps x B; Jbar, J, alpha 1 x B; the cost a struct whose fields
are shaped as 'rollout_cost_frames' takes them, with R nr x nr - and the command returns the bits of the ctypes call.  On a CPU: the
command is in the gateway's table and refuses a handle that does not exist."""
import numpy as np
import pytest

from test_mex_cost import _Gateway, _cm
from test_mex_frames import _r
from test_mex_gateway import MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)


def test_the_command_is_in_the_table_and_asks_for_a_handle(gw):  # noqa: F811
    with pytest.raises(MexError, match="handle"):
        gw.call(1, "rollout_search", np.array([[12345]], dtype=np.uint64))
    with pytest.raises(MexError, match="handle"):
        gw.call(1, "rollout_search")


@pytest.mark.gpu
def test_mex_command_equals_the_ctypes_call(gw):  # noqa: F811
    from test_gpu_rollout_search import ALPHAS, B, N, _case, _flow
    g = _Gateway(gw.L)
    f, c = _flow(5), _case(5)
    sc, tab, nr = c["sc"], c["per"], c["sc"].nr
    terms = [dict(body=float(t["body"] + 1), xlocal=np.array(t["xlocal"]), step=float(t["step"]), wpos=float(t["wpos"]), wvel=float(t["wvel"]),
                  wrot=float(t["wrot"])) for t in c["terms"]]
    cost = dict(Q=_cm(tab["Q"]), xgoal=_cm(tab["xgoal"]), R=_cm(c["R"]), terms=terms, xtarget=_cm(tab["xtarget"]), vtarget=_cm(tab["vtarget"]),
                Rtarget=_r(tab["Rtarget"]))
    h = g.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))
    none = np.zeros((0, 0))
    ps = float(sc.task["pscale"])

    def set_state():
        g.call(0, "set", h, _cm(c["q0"]), _cm(c["qd0"]))

    set_state()
    qt, qdt, ua, J, alpha, st = g.call(6, "rollout_search", h, float(sc.h), float(N), ps, _cm(f["nom"][2]), _cm(f["direction"]), _cm(f["K"]),
                                       _cm(f["xref"]), np.array(ALPHAS), _cm(f["Jbar"]), cost)
    assert qt.shape == (nr, N, B) and J.shape == (1, B) and alpha.shape == (1, B) and st.shape == (B, 2)
    want = f["srch"]
    assert np.array_equal(_cm(qt), want[0]) and np.array_equal(_cm(qdt), want[1]) and np.array_equal(_cm(ua), want[2])
    assert np.array_equal(J[0], want[3]["J"]) and np.array_equal(alpha[0], want[3]["alpha"]) and np.array_equal(st[:, 1], want[3]["status"])
    # the nominal pass alone: no alphas, kff and Jbar empty
    set_state()
    qt, qdt, ua, J, alpha = g.call(5, "rollout_search", h, float(sc.h), float(N), ps, _cm(c["u"]), none, none, none, none, none, cost)
    nom = f["nom"]
    assert np.array_equal(_cm(qt), nom[0]) and np.array_equal(_cm(ua), nom[2]) and np.array_equal(J[0], nom[3]["J"]) and not alpha.any()
    with pytest.raises(MexError, match="cost must be a struct"):
        g.call(1, "rollout_search", h, float(sc.h), float(N), ps, _cm(c["u"]), none, none, none, none, none, none)
    with pytest.raises(MexError, match="sc, ft and R are all null"):
        g.call(1, "rollout_search", h, float(sc.h), float(N), ps, _cm(c["u"]), none, none, none, none, none, dict(R=none))
    with pytest.raises(MexError, match="alpha 1 must be finite and > 0"):
        g.call(1, "rollout_search", h, float(sc.h), float(N), ps, _cm(c["u"]), _cm(f["direction"]), none, none, np.array([1.0, -1.0]), _cm(f["Jbar"]), cost)
    g.call(0, "destroy", h)
