"""The formulas of rmx_rollout_vjp_feedback, pinned on the CPU before any GPU run: the numpy recursion of
tests/proto_rollout_vjp_feedback.py
  1. against central differences of the oracle's own closed loop, in uff, K, xref, q0 and qdot0;
  2. with K = 0 and no gu, against the open-loop recursions of proto_rollout_vjp / proto_rollout_vjp_bdf2;
  3. and the two new names in the binding's symbol table and in the built library.

Loss: that of proto_rollout_vjp.loss_and_cotangents plus sum_k e_k.uapp_k with random e (so that the cotangent gu of the applied
torque is exercised); eps = 1e-5, 3 random directions per argument; tolerance rtol 2e-5, atol 1e-6 max|ana| - the bound
tests/test_rollout_vjp_proto.py holds the open-loop proto to.  Scenes and inputs: feedback_case of
tests/test_rollout_feedback_proto.py, which tests/test_gpu_rollout_vjp_feedback.py uses too (through `reference` below).
"""
import ctypes

import numpy as np
import pytest

import proto_rollout_vjp as proto1
import proto_rollout_vjp_bdf2 as proto2
import proto_rollout_vjp_feedback as protob
from test_rollout_feedback_proto import B, feedback_case

EPS, NDIR = 1e-5, 3
_CACHE = {}


def gu_case(size, integ):
    """e of the loss term sum_k e_k.uapp_k, [B][nsteps][nr]: the cotangent gu of the applied torques."""
    sc, cs, nsteps = feedback_case(size, integ)
    return np.random.default_rng(53).standard_normal((B, nsteps, sc.nr))


def reference(orc, size, integ, b):
    """protob.reference for rollout b of a size, computed once and left unchanged."""
    key = (size, integ, b)
    if key not in _CACHE:
        sc, cs, _ = feedback_case(size, integ)
        _CACHE[key] = protob.reference(orc, sc, integ, cs["q0"][b], cs["qd0"][b], cs["u"][b], cs["K"], cs["xref"], sc.h, sc.task["pscale"],
                                       cs["c"][b], cs["d"][b], gu_case(size, integ)[b])
    return _CACHE[key]


@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, "tree7", "fixed"])
def test_proto_meets_central_differences(oracle_lib, size, integ):
    sc, cs, nsteps = feedback_case(size, integ)
    h, pscale = sc.h, sc.task["pscale"]
    e = gu_case(size, integ)[0]
    ref = reference(oracle_lib, size, integ, 0)
    for name in ("duff", "dK", "dxref", "dq0", "dqd0"):
        assert np.isfinite(ref[name]).all() and np.abs(ref[name]).max() > 0
    base = dict(q0=cs["q0"][0], qd0=cs["qd0"][0], uff=cs["u"][0], K=cs["K"], xref=cs["xref"])

    def L(**args):
        qt, qdt, ua = protob.closed_loop(oracle_lib, sc, integ, args["q0"], args["qd0"], args["uff"], args["K"], args["xref"], h, pscale)
        return protob.loss_and_cotangents(qt, qdt, ua, cs["c"][0], cs["d"][0], e)[0]

    assert L(**base) == ref["L"]
    rng = np.random.default_rng(11)
    for name, grad in (("uff", ref["duff"]), ("K", ref["dK"]), ("xref", ref["dxref"]), ("q0", ref["dq0"]), ("qd0", ref["dqd0"])):
        dirs = rng.standard_normal((NDIR,) + grad.shape)
        num = np.empty(NDIR)
        for i, dv in enumerate(dirs):
            num[i] = (L(**dict(base, **{name: base[name] + EPS * dv})) - L(**dict(base, **{name: base[name] - EPS * dv}))) / (2 * EPS)
        ana = (dirs.reshape(NDIR, -1) * grad.reshape(1, -1)).sum(axis=1)
        err = np.abs(num - ana)
        print("proto %s integ %d, d/d%s: max |num - ana| / max|ana| = %.3e" % (size, integ, name, err.max() / np.abs(ana).max()))
        assert (err <= 2e-5 * np.abs(ana) + 1e-6 * np.abs(ana).max()).all(), (name, num, ana)


@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, "fixed"])
def test_without_gains_it_is_the_open_loop_recursion(oracle_lib, size, integ):
    """K = 0 (and K None) with no gu: duff, dq0, dqd0 are proto_rollout_vjp.vjp / proto_rollout_vjp_bdf2.vjp on the same tape - another
    arrangement of the same sums under BDF1, the same statements under BDF2 -, and dK's rows are the outer products the formula gives
    while dxref is zero."""
    sc, cs, nsteps = feedback_case(size, integ)
    h, ps = sc.h, sc.task["pscale"]
    q0, qd0, u = cs["q0"][0], cs["qd0"][0], cs["u"][0]
    if integ == 1:
        qt, qdt = proto1.rollout(oracle_lib, sc, q0, qd0, u, h, ps)
        H, M, D = proto1.tape(oracle_lib, sc, q0, qd0, qt, qdt, h)
        gq, gqd = proto1.loss_and_cotangents(qt, qdt, cs["c"][0], cs["d"][0])[1:]
        du, dq0, dqd0 = proto1.vjp(H, M, D, gq, gqd, h, ps)
    else:
        qt, qdt, H, M, D = proto2.forward(oracle_lib, sc, q0, qd0, u, h, ps)
        gq, gqd = proto2.loss_and_cotangents(qt, qdt, cs["c"][0], cs["d"][0])[1:]
        du, dq0, dqd0 = proto2.vjp(H, M, D, gq, gqd, h, ps)
    dx = protob.start_states(q0, qd0, qt, qdt) - cs["xref"]
    for K in (np.zeros_like(cs["K"]), None):
        out = protob.vjp(integ, H, M, D, K, dx, gq, gqd, None, h, ps)
        for name, a, r in (("duff", out["duff"], du), ("dq0", out["dq0"], dq0), ("dqd0", out["dqd0"], dqd0)):
            rel = np.linalg.norm(a - r) / np.linalg.norm(r)
            print("proto %s integ %d, K %s: |%s - open loop| / |open loop| = %.3e" % (size, integ, "None" if K is None else "0", name, rel))
            assert rel <= (1e-9 if integ == 1 else 0.0), (name, rel)      # (BDF1: H'^-1 amplifies the rounding of the other arrangement)
        assert not out["dxref"].any()
        if K is None:
            assert not out["dK"].any()
        else:
            assert np.array_equal(out["dK"], np.einsum("kj,ki->kji", dx, out["duff"]))


def test_binding_and_library_hold_the_two_entries():
    """The CPU test that fails without the feature: both names in _abi.SYMBOLS, exported by the built library and bound with their
    argument lists; rmx_feedback_grads has the header's five members in the header's order."""
    import __graft_entry__ as g
    g.build()
    from redmax_amd import _abi
    names = ("rmx_rollout_vjp_feedback", "rmx_rollout_vjp_feedback_device")
    L = ctypes.CDLL(_abi.LIB_PATH)
    for n in names:
        assert n in _abi.SYMBOLS and hasattr(L, n), n
        assert len(getattr(_abi.lib(), n).argtypes) == 7
    assert _abi.FEEDBACK_GRAD_NAMES == ("duff", "dK", "dxref", "dq0", "dqd0")
    assert tuple(f[0] for f in _abi.FeedbackGrads._fields_) == _abi.FEEDBACK_GRAD_NAMES
    assert _abi.lib().rmx_version() == 111
