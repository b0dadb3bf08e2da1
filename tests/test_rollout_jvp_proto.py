"""The recursions of rmx_rollout_jvp, pinned on the CPU before any GPU run (tests/proto_rollout_jvp.py, on the oracle's tape):

  - the full-rollout JVP against central differences (eps 1e-6) of the oracle's rollout in tu, tq0 and tqd0 together (5, tree7; BDF1
    and BDF2), elementwise to 2e-5 |ana| + 1e-6 max|ana|, the project's testGrad bound;
  - the pairing <gq, tq> + <gqd, tqd> = <du, tu> + <dq0, tq0> + <dqd0, tqd0> with tests/proto_rollout_vjp.py (5, tree7, 16, 32) and
    tests/proto_rollout_vjp_bdf2.py (5, tree7, 16), all three groups of tangents together and each alone, relative to
    |<du, tu>| + |<dq0, tq0>| + |<dqd0, tqd0>|, to 1e-10 (the bound the suite holds this kind of CPU identity to).  Measured: at most
    7.32e-11 (BDF2, the 16-link chain, tq0 alone; 5.4e-12 under BDF1).  The figure is relative to single inner products that may
    nearly cancel, so it belongs to its rollout and direction: rollout 0 of the B = 3 case, direction tangent0, the ones
    tests/test_gpu_rollout_jvp.py checks on the device with a bound taken from this figure;
  - the BDF1 JVP against the forward chain x_k = A_k x_{k-1} + B_k tu_k of tests/proto_rollout_linearize.py's assembly, to 1e-10;
  - the two entry points are declared, bound and exported.

Inputs: case(sc, 17) of tests/test_rollout_vjp_proto.py, the step counts of tests/test_gpu_rollout_vjp.py, standard-normal tangents
of a fixed seed.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import proto_rollout_jvp as pj
import proto_rollout_linearize as lin
import proto_rollout_vjp as proto1
import proto_rollout_vjp_bdf2 as proto2
from test_gpu_adjoint_controls import _scene
from test_rollout_vjp_proto import case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {3: 5, 5: 6, 11: 5, 16: 5, 32: 4, 40: 4, "tree7": 6}      # (tests/test_gpu_rollout_vjp.py STEPS)
NAMES = ("rmx_rollout_jvp", "rmx_rollout_jvp_device")
TSEED = 53


def tangent0(nsteps, nr):
    """Direction 0 of rollout 0 of the 3 x 3 directions tests/test_gpu_rollout_jvp.py draws for its pairing test: dict(tu, tq0, tqd0)."""
    return {k: v[0, 0] for k, v in pj.tangents(TSEED, 3, 3, nsteps, nr).items()}
GROUPS = (("all", (1, 1, 1)), ("tu", (1, 0, 0)), ("tq0", (0, 1, 0)), ("tqd0", (0, 0, 1)))
_TAPES = {}


def oracle_tape(orc, size, integ, b=0, B=3):
    """(scene, case of rollout b of B, qtraj, qdtraj, H, M, D) on the oracle, computed once per (size, integrator, rollout) and left
    unchanged; tests/test_gpu_rollout_jvp.py shares it (B = 3 is its batch: rollout 0 here is rollout 0 there)."""
    key = (size, integ, b, B)
    if key not in _TAPES:
        sc = _scene(size, integ)
        cs = {k: v[b] for k, v in case(sc, 17, nsteps=STEPS[size], B=B).items()}
        h, pscale = sc.h, sc.task["pscale"]
        if integ == 1:
            qt, qdt = proto1.rollout(orc, sc, cs["q0"], cs["qd0"], cs["u"], h, pscale)
            H, M, D = proto1.tape(orc, sc, cs["q0"], cs["qd0"], qt, qdt, h)
        else:
            qt, qdt, H, M, D = proto2.forward(orc, sc, cs["q0"], cs["qd0"], cs["u"], h, pscale)
        _TAPES[key] = (sc, cs, qt, qdt, H, M, D)
    return _TAPES[key]


def pairing_figures(orc, size, integ):
    """The pairing error of every group of GROUPS on the oracle's tape of rollout 0, direction tangent0: dict(name -> relative error).
    The figure is relative to a sum of three inner products, each of which may nearly cancel: it belongs to its rollout and direction."""
    sc, cs, qt, qdt, H, M, D = oracle_tape(orc, size, integ)
    h, pscale = sc.h, sc.task["pscale"]
    proto = proto1 if integ == 1 else proto2
    _, gq, gqd = proto.loss_and_cotangents(qt, qdt, cs["c"], cs["d"])
    grads = proto.vjp(H, M, D, gq, gqd, h, pscale)
    t = tangent0(len(qt), sc.nr)
    out = {}
    for name, (wu, wq, wv) in GROUPS:
        tans = (t["tu"] if wu else None, t["tq0"] if wq else None, t["tqd0"] if wv else None)
        tq, tqd = pj.jvp(integ, H, M, D, h, pscale, *tans)
        out[name] = pj.pairing((gq, gqd), (tq, tqd), grads, tans)
    return out


@pytest.mark.parametrize("size,integ", [(5, 1), ("tree7", 1), (5, 2), ("tree7", 2)])
def test_jvp_meets_central_differences(oracle_lib, size, integ):
    sc, cs, qt, qdt, H, M, D = oracle_tape(oracle_lib, size, integ)
    h, pscale = sc.h, sc.task["pscale"]
    t = tangent0(len(qt), sc.nr)
    ana = pj.jvp(integ, H, M, D, h, pscale, t["tu"], t["tq0"], t["tqd0"])
    proto = proto1 if integ == 1 else proto2
    eps = 1e-6
    p = proto.rollout(oracle_lib, sc, cs["q0"] + eps * t["tq0"], cs["qd0"] + eps * t["tqd0"], cs["u"] + eps * t["tu"], h, pscale)
    m = proto.rollout(oracle_lib, sc, cs["q0"] - eps * t["tq0"], cs["qd0"] - eps * t["tqd0"], cs["u"] - eps * t["tu"], h, pscale)
    for name, a, hi, lo in (("tq", ana[0], p[0], m[0]), ("tqd", ana[1], p[1], m[1])):
        num = (hi - lo) / (2 * eps)
        err = np.abs(num - a)
        print("jvp proto %s bdf%d %s: max |num - ana| = %.3e, max|ana| = %.3e, relative Frobenius %.3e"
              % (size, integ, name, err.max(), np.abs(a).max(), pj.rel(num, a)))
        assert np.abs(a).max() > 0
        assert (err <= 2e-5 * np.abs(a) + 1e-6 * np.abs(a).max()).all(), (name, err.max())


@pytest.mark.parametrize("size,integ", [(5, 1), ("tree7", 1), (16, 1), (32, 1), (5, 2), ("tree7", 2), (16, 2)])
def test_pairing_with_the_backward_recursion(oracle_lib, size, integ):
    figs = pairing_figures(oracle_lib, size, integ)
    print("jvp proto %s bdf%d: pairing error %s" % (size, integ, "  ".join("%s %.3e" % kv for kv in figs.items())))
    assert max(figs.values()) <= 1e-10, (size, integ, figs)


@pytest.mark.parametrize("size", [5, "tree7", 16, 32])
def test_bdf1_jvp_is_the_forward_chain(oracle_lib, size):
    sc, cs, qt, qdt, H, M, D = oracle_tape(oracle_lib, size, 1)
    h, pscale = sc.h, sc.task["pscale"]
    t = tangent0(len(qt), sc.nr)
    ref = pj.jvp_bdf1(H, M, D, h, pscale, t["tu"], t["tq0"], t["tqd0"])
    A, Bm = lin.assemble_bdf1(*lin.sens(H, M, D, lin.etas(len(qt), h, 1), pscale), h)
    got = pj.chain_bdf1(A, Bm, t["tu"], t["tq0"], t["tqd0"])
    errs = tuple(pj.rel(a, b) for a, b in zip(got, ref))
    print("jvp proto %s: forward chain against the recursion tq %.3e tqd %.3e" % ((size,) + errs))
    assert max(errs) <= 1e-10, (size, errs)


def test_entry_points_are_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from redmax_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "redmax_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_abi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _abi.SYMBOLS
        assert hasattr(L, name), name
    assert _abi.lib().rmx_version() == 111
