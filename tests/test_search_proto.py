"""tests/proto_search.py against proto_frame_cost.py, on the CPU: J of rmx_rollout_search's definition on a given record, in float64
and in longdouble, is proto_frame_cost's Jk summed over the steps plus the control part 1/2 u'R u.

Scenes, records and dense tables: test_point_cost_proto's; terms and targets: test_frame_cost_proto's (point and frame terms, one
step without a term).  Tolerances: two evaluations of one sum in different orders, or in the two types: 64 eps of the sum of the
absolute values of its terms.
"""
import numpy as np
import pytest

import proto_frame_cost as F
import proto_search as S
from test_frame_cost_proto import _targets, frame_terms_of
from test_point_cost_proto import SIZES, _dense, _record, _scene

EPS = np.finfo(np.float64).eps
LD = np.longdouble
N = 5


def _problem(size):
    sc, m = _scene(size)
    nr = sc.nr
    q, qd, rng = _record(sc, 11, N)
    u = rng.standard_normal((N, nr))
    Q, xg = _dense(rng, N, nr)
    Q = np.einsum("kij,klj->kil", Q, Q)      # symmetric positive semi-definite
    A = rng.standard_normal((nr, nr))
    R = A @ A.T + nr * np.eye(nr)            # symmetric positive definite
    terms = frame_terms_of(m, N)
    xt, vt, Rt = _targets(rng, len(terms))
    return m, q, qd, u, Q, xg, R, terms, xt, vt, Rt


@pytest.mark.parametrize("size", SIZES)
def test_J_is_the_frame_cost_summed_plus_the_control_part(size):
    m, q, qd, u, Q, xg, R, terms, xt, vt, Rt = _problem(size)
    for dtype in (np.float64, LD):
        out = S.cost(m, q, qd, u, Q, xg, R, terms, xt, vt, Rt, dtype)
        assert out["J"].dtype == dtype and out["Jk"].dtype == dtype and out["Ju"].dtype == dtype
        Jk = F.cost(m, q, qd, Q, xg, terms, xt, vt, Rt, dtype)["Jk"]
        assert (out["Jk"] == Jk).all()      # (proto_frame_cost's, not restated)
        Ju = 0.5 * np.einsum("ki,ij,kj->k", u.astype(dtype), R.astype(dtype), u.astype(dtype))
        scale = float(np.sum(np.abs(Jk)) + np.sum(np.abs(Ju)))
        assert np.max(np.abs(out["Ju"] - Ju)) <= 64 * EPS * float(np.max(np.abs(Ju)))
        assert abs(out["J"] - (Jk.sum() + Ju.sum())) <= 64 * EPS * scale
        assert (out["Ju"] > 0).all()        # R is positive definite
    a, b = S.cost(m, q, qd, u, Q, xg, R, terms, xt, vt, Rt)["J"], S.cost(m, q, qd, u, Q, xg, R, terms, xt, vt, Rt, LD)["J"]
    print("%s: J %.17g, float64 against longdouble %.3e" % (size, a, S.rel_err(a, b)))
    assert S.rel_err(a, b) <= 64 * EPS


@pytest.mark.parametrize("size", SIZES)
def test_the_parts_can_be_absent(size):
    m, q, qd, u, Q, xg, R, terms, xt, vt, Rt = _problem(size)
    full = S.cost(m, q, qd, u, Q, xg, R, terms, xt, vt, Rt)
    no_R = S.cost(m, q, qd, u, Q, xg, None, terms, xt, vt, Rt)
    assert (no_R["Ju"] == 0.0).all() and (no_R["Jk"] == full["Jk"]).all()
    assert abs(no_R["J"] - full["Jk"].sum()) <= 64 * EPS * float(np.sum(np.abs(full["Jk"])))
    only_R = S.cost(m, q, qd, u, None, None, R, None)
    assert (only_R["Jk"] == 0.0).all() and (only_R["Ju"] == full["Ju"]).all()
    no_terms = S.cost(m, q, qd, u, Q, xg, R, None)
    state = F.cost(m, q, qd, Q, xg)["Jk"]
    assert (no_terms["Jk"] == state).all()
    # the terms add to the steps that own them alone: step 2 owns none
    assert full["Jk"][1] == state[1] and (full["Jk"][[0, 2, N - 1]] > state[[0, 2, N - 1]]).all()
    no_state = S.cost(m, q, qd, u, None, None, R, terms, xt, vt, Rt)
    assert no_state["Jk"][1] == 0.0
    scale = float(np.sum(np.abs(full["Jk"])) + np.sum(np.abs(state)))
    assert np.max(np.abs((full["Jk"] - state) - no_state["Jk"])) <= 64 * EPS * scale

