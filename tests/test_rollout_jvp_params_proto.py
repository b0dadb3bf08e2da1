"""The recursion of rmx_rollout_jvp_params, pinned on the CPU before any GPU run (tests/proto_rollout_jvp_params.py, on the oracle's
tape):

  (a) the parameter JVP against central differences of the oracle's own rollout on perturbed models (tests/proto_rollout_params.py
      perturbed), 5 and tree7, BDF1 and BDF2: one direction per group, scaled to the group's magnitude as
      tests/test_rollout_params_proto.py scales, eps 1e-5, elementwise rtol 2e-5, atol 1e-6 max|ana| (the project's testGrad bound);
  (b) the pairing <gq, tq> + <gqd, tqd> = <du, tu> + <dq0, tq0> + <dqd0, tqd0> + sum over the groups of <grad_group, ttheta_group>
      against tests/proto_rollout_params.py reference's gradients, each group alone and all together with tu, tq0, tqd0, relative to
      the sum of the magnitudes of the terms on the right, to 1e-10 (the bound the suite holds this kind of CPU identity to).

Inputs: case(sc, 17) of tests/test_rollout_vjp_proto.py with the step counts and B = 3 of tests/test_gpu_rollout_vjp.py, rollout 0;
the tangents of tests/test_rollout_jvp_proto.py for tu, tq0, tqd0 and fixed-seed parameter directions (tangents() below), direction 0 -
the rollout and direction tests/test_gpu_rollout_jvp_params.py checks its pairing on, with a bound taken from the figure printed here
(PAIRING_CPU).  Measured: the largest pairing error is 6.624e-12 (the 32-link chain, BDF1, stiffness alone; 1.207e-12 under BDF2,
the 16-link chain, stiffness alone); the central-difference errors are at most 0.24 of the testGrad bound (stiffness, the 5-link
chain under BDF2) and stand per group in CD_CPU of tests/test_gpu_rollout_jvp_params.py with the cases they came from.
"""
import numpy as np
import pytest

import proto_rollout_jvp as pj
import proto_rollout_jvp_params as pjp
import proto_rollout_params as pp
from test_gpu_adjoint_controls import _scene
from test_rollout_jvp_proto import STEPS, TSEED
from test_rollout_vjp_proto import case

PSEED = 71
KEYS = ("tu", "tq0", "tqd0")
PAIR_CASES = [(5, 1), ("tree7", 1), (16, 1), (32, 1), (5, 2), ("tree7", 2), (16, 2)]
_CASES, _REFS = {}, {}


def tangents(orc, sc, nsteps, ntan, nb=3):
    """The directions of the tests: tu, tq0, tqd0 of tests/proto_rollout_jvp.py (seed TSEED) and one array per parameter group,
    [nb][ntan] + the group's shape, scaled to the group's magnitude (seed PSEED)."""
    t = pj.tangents(TSEED, nb, ntan, nsteps, sc.nr)
    t.update(pjp.directions(pp.values(orc, sc), PSEED, (nb, ntan)))
    return t


def oracle_case(orc, size, integ, b=0, B=3):
    """(scene, case of rollout b of B, the oracle's tape and slots) computed once and left unchanged; the GPU tests share it."""
    key = (size, integ, b, B)
    if key not in _CASES:
        sc = _scene(size, integ)
        cs = {k: v[b] for k, v in case(sc, 17, nsteps=STEPS[size], B=B).items()}
        _CASES[key] = (sc, cs, pjp.tape(orc, sc, cs["q0"], cs["qd0"], cs["u"], sc.h, sc.task["pscale"], integ))
    return _CASES[key]


def oracle_reference(orc, size, integ):
    """tests/proto_rollout_params.py reference of rollout 0 (cotangents, du, dq0, dqd0 and the five gradients), once."""
    key = (size, integ)
    if key not in _REFS:
        sc, cs, _ = oracle_case(orc, size, integ)
        _REFS[key] = pp.reference(orc, sc, cs["q0"], cs["qd0"], cs["u"], sc.h, sc.task["pscale"], cs["c"], cs["d"], integ)
    return _REFS[key]


def pairing_figures(orc, size, integ):
    """The pairing error on rollout 0, direction 0: each group alone, and all five together with tu, tq0, tqd0."""
    sc, cs, tp = oracle_case(orc, size, integ)
    ref = oracle_reference(orc, size, integ)
    h, pscale = sc.h, sc.task["pscale"]
    proto = pp.proto1 if integ == 1 else pp.proto2
    _, gq, gqd = proto.loss_and_cotangents(tp["qtraj"], tp["qdtraj"], cs["c"], cs["d"])
    t = {k: v[0, 0] for k, v in tangents(orc, sc, len(tp["qtraj"]), 3).items()}
    g0 = pp.residuals(orc, sc, tp["slots"])
    out = {}
    for name in pjp.GROUPS + ("all",):
        tpar = {g: t[g] for g in pjp.GROUPS if name in (g, "all")}
        tans = tuple(t[k] if name == "all" else None for k in KEYS)
        tq, tqd = pjp.jvp_params(orc, sc, integ, tp, h, pscale, tpar, *tans, g0=g0)
        out[name] = pjp.pairing((gq, gqd), (tq, tqd), (ref["du"], ref["dq0"], ref["dqd0"]), tans, ref["grads"], tpar)
    return out


def central_differences(orc, sc, cs, integ, group, dv, eps=1e-5):
    """(tq, tqd) of a parameter direction by central differences of the oracle's rollout on the two perturbed models."""
    proto = pp.proto1 if integ == 1 else pp.proto2
    p, m = (proto.rollout(orc, pp.perturbed(orc, sc, group, s * eps * dv), cs["q0"], cs["qd0"], cs["u"], sc.h, sc.task["pscale"])
            for s in (1.0, -1.0))
    return (p[0] - m[0]) / (2 * eps), (p[1] - m[1]) / (2 * eps)


def cd_error(num, ana):
    """The largest elementwise |num - ana| in units of the testGrad bound 2e-5 |ana| + 1e-6 max|ana|: <= 1 passes."""
    return max(float((np.abs(n - a) / (2e-5 * np.abs(a) + 1e-6 * np.abs(a).max())).max()) for n, a in zip(num, ana))


@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, "tree7"])
def test_parameter_jvp_meets_central_differences(oracle_lib, size, integ):
    sc, cs, tp = oracle_case(oracle_lib, size, integ)
    t = {k: v[0, 0] for k, v in tangents(oracle_lib, sc, len(tp["qtraj"]), 3).items()}
    for group in pjp.GROUPS:
        ana = pjp.jvp_params(oracle_lib, sc, integ, tp, sc.h, sc.task["pscale"], {group: t[group]})
        num = central_differences(oracle_lib, sc, cs, integ, group, t[group])
        assert all(np.abs(a).max() > 0 for a in ana), group
        err = cd_error(num, ana)
        print("jvp_params proto %s bdf%d, %s: central-difference error %.3e of the testGrad bound (tq %.3e, tqd %.3e relative Frobenius)"
              % (size, integ, group, err, pj.rel(num[0], ana[0]), pj.rel(num[1], ana[1])))
        assert err <= 1.0, (group, err)


@pytest.mark.parametrize("size,integ", PAIR_CASES)
def test_pairing_with_the_parameter_gradients(oracle_lib, size, integ):
    figs = pairing_figures(oracle_lib, size, integ)
    print("jvp_params proto %s bdf%d: PAIRING_CPU %.3e  (%s)" % (size, integ, max(figs.values()), "  ".join("%s %.3e" % kv for kv in figs.items())))
    assert max(figs.values()) <= 1e-10, (size, integ, figs)


@pytest.mark.parametrize("integ", [1, 2])
def test_zero_parameter_directions_give_the_plain_jvp(oracle_lib, integ):
    sc, cs, tp = oracle_case(oracle_lib, 5, integ)
    t = {k: v[0, 0] for k, v in tangents(oracle_lib, sc, len(tp["qtraj"]), 3).items()}
    zero = {g: np.zeros_like(t[g]) for g in pjp.GROUPS}
    got = pjp.jvp_params(oracle_lib, sc, integ, tp, sc.h, sc.task["pscale"], zero, t["tu"], t["tq0"], t["tqd0"])
    want = pj.jvp(integ, tp["H"], tp["M"], tp["D"], sc.h, sc.task["pscale"], t["tu"], t["tq0"], t["tqd0"])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
