"""The rule behind rmx_rollout_vjp_forces, pinned on the CPU before any GPU run: the numpy proto of
tests/proto_rollout_force_params.py (dL/dtheta = - sum over the slots of z' dg/dtheta for the stiffness, damping and rest length of
every force of the table) against

  1. central differences of the proto rollout's loss (proto_rollout_pf.rollout on the table with one constant moved), per entry at
     n = 4 and 8 with relative step 1e-6, and along 3 random directions over all constants at once at n = 16 with relative step 1e-5,
     BDF1 and BDF2.  The tolerances are what the difference quotient delivers here (the rollouts' Newton stops at |g| < 1e-9, and a
     relative step of 1e-6 on a constant moves the loss by 1e-6 of its sensitivity).  Measured, worst over the entries, the two
     rollouts and both integrators:
         per entry    |fd - ana| <= 1.4e-6 S  (n = 8, BDF1, the body-body spring's damping; 1.3e-5 of |ana| at worst)
         directions   |fd - ana| <= 2.2e-9 |ana| (n = 16, BDF2)
     with S = sum_s |z_s' dg_s/dtheta|, the scale the GPU tests use; asserted with one decade of margin: 1.5e-5 S and 2.2e-8 |ana|.
     On case(8) the cable goes slack within the rollout, so the branch rule is part of what the differences see;
  2. a spring's analytic closed form: one prismatic joint on the line of a world-anchored spring-damper, where a BDF1 step is a scalar
     linear equation;
  3. a cable that is slack throughout: exact zeros;
and the conditions the GPU tests rest on, on proto_rollout_pf.case(n) at every n of SIZES and both integrators: the proto's Newton
converges, and every entry that is not the point-point force's L has |G| >= 1e-3 S (measured minimum 1.5e-3: n = 8, BDF2) - so the
GPU tests' bound of 1e-7 S is at most 1e-4 of any entry, and no entry is a cancellation of large terms.
Also here: the two symbols are declared and exported, RMX_VERSION is 111, the struct has three pointers
(tests/test_mex_force_params.py has the MEX command).
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import proto_point_forces as ppf
import proto_rollout_force_params as F
import proto_rollout_pf as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _case(n):
    cs = P.case(n)
    return cs, P.World(cs["sc"])


@functools.lru_cache(maxsize=None)
def _reference(n, integ, b):
    cs, ev = _case(n)
    return F.reference(ev, cs["q0"][b], cs["qd0"][b], cs["u"][b], cs["h"], cs["pscale"], cs["c"][b], cs["d"][b], integ)


def _loss(cs, ev, theta, integ, b):
    info = {}
    L = F.loss(F.with_constants(ev, theta), cs["q0"][b], cs["qd0"][b], cs["u"][b], cs["h"], cs["pscale"], cs["c"][b], cs["d"][b], integ, info)
    assert info["converged"]
    return L


def _free(ev):
    """[nforces][3] of 0/1: the constants the model reads (a point-point force has no L)."""
    mask = np.ones((len(ev.forces), 3))
    mask[[f[0] == ppf.PP for f in ev.forces], 2] = 0.0
    return mask


# ---------------------------------------------------------------- 1. central differences of whole rollouts

@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", [4, 8])
def test_every_entry_meets_central_differences(n, integ):
    cs, ev = _case(n)
    theta, mask = F.constants(ev), _free(ev)
    assert mask.sum() == 11
    worst = 0.0
    for b in range(2):
        ref = _reference(n, integ, b)
        for f, c in zip(*np.nonzero(mask)):
            e = 1e-6 * theta[f, c]
            tp, tm = theta.copy(), theta.copy()
            tp[f, c] += e
            tm[f, c] -= e
            fd = (_loss(cs, ev, tp, integ, b) - _loss(cs, ev, tm, integ, b)) / (2 * e)
            err = abs(fd - ref["G"][f, c]) / ref["S"][f, c]
            worst = max(worst, err)
            assert err <= 1.5e-5, (n, integ, b, f, c, fd, ref["G"][f, c], ref["S"][f, c])
    print("n=%d BDF%d: worst |fd - ana| / S = %.2e" % (n, integ, worst))
    if n == 8 and integ == 1:      # the cable goes slack within rollout 0: the branch rule is under test
        strains = P.cable_strains(ev, _reference(8, 1, 0)["qtraj"], _reference(8, 1, 0)["qdtraj"])
        assert (strains > 0).any() and not (strains > 0).all()


@pytest.mark.parametrize("integ", [1, 2])
def test_random_directions_meet_central_differences(integ):
    n = 16
    cs, ev = _case(n)
    theta, mask = F.constants(ev), _free(ev)
    rng = np.random.default_rng(16)
    worst = 0.0
    for b in range(2):
        ref = _reference(n, integ, b)
        for _ in range(3):
            dth = rng.standard_normal(theta.shape) * mask * theta
            eps = 1e-5
            fd = (_loss(cs, ev, theta + eps * dth, integ, b) - _loss(cs, ev, theta - eps * dth, integ, b)) / (2 * eps)
            ana = float((dth * ref["G"]).sum())
            worst = max(worst, abs(fd - ana) / abs(ana))
            assert abs(fd - ana) <= 2.2e-8 * abs(ana), (integ, b, fd, ana)
    print("n=16 BDF%d: worst |fd - ana| / |ana| along directions = %.2e" % (integ, worst))


# ---------------------------------------------------------------- 2. a spring's closed form

def test_a_spring_on_a_slider_has_the_closed_form():
    """A body of mass m on a prismatic joint along x, its origin on the line of a spring-damper from a world anchor on that line, no
    gravity along the axis: l = a + x, ldot = (x - q0)/h, and the BDF1 step solves the linear equation
        Hs x = m (q0 + h qd0) - h^2 ks (a - L)/L + h kd q0/L,    Hs = m + h^2 ks/L + h kd/L,
    so dx/dks = -h^2 (l - L)/(L Hs), dx/dkd = -h^2 ldot/(L Hs), dx/dL = h^2 (ks l + kd ldot)/(L^2 Hs), and with the loss
    c x + d (x - q0)/h + x^2/2 the gradient is (c + x + d/h) dx/dtheta."""
    from redmax_amd.redmax import BodyCuboid, ForceSpringDamper, JointPrismatic, Scene
    sc = Scene()
    body = BodyCuboid(1.0, [10, 1, 1])
    joint = JointPrismatic(None, body, [1, 0, 0])
    joint.setJointTransform(np.eye(4))
    T = np.eye(4)
    T[0, 3] = 5.0
    body.setBodyTransform(T)
    sc.bodies.append(body)
    sc.joints.append(joint)
    f = ForceSpringDamper(None, [-3.0, 0.0, 0.0], body, [0.0, 0.0, 0.0])
    f.setStiffness(4e3)
    f.setDamping(30.0)
    sc.forces = [f]
    sc.h = 5e-3
    sc.init()
    f.setRetLength(0.9 * f.L)
    sc.init()
    assert abs(np.asarray(sc.desc()["grav"], float)[0]) == 0.0
    ev = P.World(sc)
    (_, _, ks, kd, L), = ev.forces
    h, m, a = sc.h, 10.0, 8.0
    q0, qd0, c, d = 0.07, -0.4, 0.6, -0.02
    ref = F.reference(ev, np.array([q0]), np.array([qd0]), np.zeros((1, 1)), h, 1.0, np.array([[c]]), np.array([[d]]), 1)
    assert ref["converged"]
    Hs = m + h * h * ks / L + h * kd / L
    x = (m * (q0 + h * qd0) - h * h * ks * (a - L) / L + h * kd * q0 / L) / Hs
    assert abs(ref["qtraj"][0, 0] - x) <= 1e-12 * max(1.0, abs(x))
    l, ldot = a + x, (x - q0) / h
    dx = np.array([-h * h * (l - L) / (L * Hs), -h * h * ldot / (L * Hs), h * h * (ks * l + kd * ldot) / (L * L * Hs)])
    want = (c + x + d / h) * dx
    assert np.abs(want).min() > 0
    assert np.allclose(ref["G"][0], want, rtol=1e-10, atol=0.0), (ref["G"][0], want)
    assert np.allclose(ref["S"][0], np.abs(want), rtol=1e-10, atol=0.0)      # (one slot: S = |G|)


# ---------------------------------------------------------------- 3. a cable that is slack throughout

@pytest.mark.parametrize("integ", [1, 2])
def test_a_cable_that_is_slack_throughout_has_exact_zeros(integ):
    cs, _ = _case(8)
    sc = ppf.sizedSceneWithForces(8)
    cable = sc.forces[3]
    cable.setRetLength(1.5 * cable.L / 0.97)
    sc.init()
    ev = P.World(sc)
    for b in range(2):
        ref = F.reference(ev, cs["q0"][b], cs["qd0"][b], cs["u"][b], cs["h"], cs["pscale"], cs["c"][b], cs["d"][b], integ)
        assert ref["converged"] and (P.cable_strains(ev, ref["qtraj"], ref["qdtraj"]) < 0).all()
        assert (ref["G"][3] == 0.0).all() and (ref["S"][3] == 0.0).all()
        assert (np.abs(ref["G"][:3]) > 0).sum() == 8


# ---------------------------------------------------------------- what the GPU tests rest on

@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", P.SIZES)
def test_the_gpu_tests_inputs_carry_every_entry(n, integ):
    _, ev = _case(n)
    mask = _free(ev) > 0
    low = np.inf
    for b in range(2):
        ref = _reference(n, integ, b)
        assert ref["converged"], (n, integ, b)
        G, S = ref["G"], ref["S"]
        assert (G[~mask] == 0.0).all() and (S[~mask] == 0.0).all()
        assert (np.abs(G[mask]) > 0).all()
        assert (np.abs(G[mask]) >= 1e-3 * S[mask]).all(), (n, integ, b, np.abs(G) / np.where(S > 0, S, 1.0))
        low = min(low, float((np.abs(G[mask]) / S[mask]).min()))
    print("n=%d BDF%d: min |G| / S = %.3g" % (n, integ, low))


# ---------------------------------------------------------------- the symbols and the MEX command

def test_symbols_struct_and_version():
    import __graft_entry__ as g
    g.build()
    from redmax_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "redmax_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_abi.LIB_PATH)
    for name in ("rmx_rollout_vjp_forces", "rmx_rollout_vjp_forces_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _abi.SYMBOLS and hasattr(L, name), name
    assert re.search(r"#define\s+RMX_VERSION\s+111\b", src) and _abi.lib().rmx_version() == 111
    body = re.search(r"typedef\s+struct\s+rmx_force_grads\s*\{(.*?)\}\s*rmx_force_grads\s*;", src, flags=re.S).group(1)
    assert re.findall(r"double\s*\*\s*(\w+)\s*;", body) == ["stiffness", "damping", "L"]
    assert ctypes.sizeof(_abi.ForceGrads) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert _abi.FORCE_PARAM_NAMES == ("force_stiffness", "force_damping", "force_L")
    assert _abi.PARAM_NAMES == ("stiffness", "damping", "qrest", "inertia", "grav")
