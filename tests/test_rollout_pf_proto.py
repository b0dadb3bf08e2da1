"""The taped rollout with body-to-body forces, pinned on the CPU before any GPU run (tests/proto_rollout_pf.py):
  - the forces' share of D = df/dqdot in its two forms - the world-frame formula the kernel uses and the reference's literal
    J' Dm J - agree to 1e-11 relative (the suite's bound for the forces' H against the literal form), and the formula meets central
    differences of the forces' generalised force in qdot;
  - the unchanged recursions of rmx_rollout_vjp, fed with the tape that carries the forces, meet central differences of the proto's
    own rollout in u, q0 and qdot0, for both integrators: eps = 1e-5, 3 random directions per argument, the floor of
    tests/test_rollout_vjp_proto.py (rtol 2e-5, atol 1e-6 max|ana|);
  - a negative control: with D_pf left out of the tape the same comparison misses that floor by a factor of 100 or more;
  - the line-search-free Newton of the taped sweep converges on every input the GPU tests use.
"""
import functools

import numpy as np
import pytest

import proto_point_forces as ppf
import proto_rollout_pf as P

EPS, NDIR = 1e-5, 3


@functools.lru_cache(maxsize=None)
def _case(n):
    cs = P.case(n)
    return cs, P.World(cs["sc"])


@pytest.mark.parametrize("n", P.SIZES)
def test_the_two_forms_of_D_pf_agree(oracle_lib, n):
    cs, ev = _case(n)
    lit = ppf.Literal(oracle_lib, cs["sc"])
    for b in range(2):
        q, qd = cs["q0"][b], cs["qd0"][b]
        Dw, Dl = P.D_pf_world(ev.m, ev.forces, q, qd), P.D_pf_literal(lit, q, qd)
        M, D0 = P.pw.eval_MD_world(ev.m, q, qd)
        print("n=%d b=%d: |Dw - Dl|/|Dl| = %.2e, |D_pf|/|D0| = %.0f, h|D_pf|/|M| = %.2f" % (
            n, b, P.rel(Dw, Dl), np.linalg.norm(Dw) / np.linalg.norm(D0), cs["h"] * np.linalg.norm(Dw) / np.linalg.norm(M)))
        assert P.rel(Dw, Dl) <= 1e-11
        # a missing block cannot hide on these scenes
        assert np.linalg.norm(Dw) >= 100 * np.linalg.norm(D0) and cs["h"] * np.linalg.norm(Dw) >= 0.1 * np.linalg.norm(M)
        # the whole of D against the oracle's force-free D plus the literal block
        assert P.rel(ev.MD(q, qd)[1], P.Lit(lit).MD(q, qd)[1]) <= 1e-11


@pytest.mark.parametrize("n", [4, 8, 16])
def test_D_pf_meets_central_differences_in_qdot(n):
    """dg = -eta^2 J'fm is the forces' share of the residual (world_terms, eta = 1): D_pf = -d(dg)/dqdot."""
    cs, ev = _case(n)
    q, qd = cs["q0"][0], cs["qd0"][0]
    idx = ev.m["idx"]
    dof = [j for j in range(ev.m["n"]) if idx[j] >= 0]
    r = [idx[j] for j in dof]

    def f(v):
        out = np.zeros(ev.nr)
        out[r] = -ppf.world_terms(ev.m, ev.forces, q, v, 1.0, False)[0][dof]
        return out

    num = np.empty((ev.nr, ev.nr))
    for i in range(ev.nr):
        e = np.zeros(ev.nr)
        e[i] = 1e-4
        num[:, i] = (f(qd + e) - f(qd - e)) / 2e-4
    assert P.rel(num, P.D_pf_world(ev.m, ev.forces, q, qd)) <= 1e-8


def _fd_errors(cs, ev, b, integ, with_pf):
    """Per argument: (|num - ana| per direction, ana per direction) of the loss's directional derivatives."""
    h, ps = cs["h"], cs["pscale"]
    args = dict(q0=cs["q0"][b], qd0=cs["qd0"][b], u=cs["u"][b])
    ref = P.reference(ev, args["q0"], args["qd0"], args["u"], h, ps, cs["c"][b], cs["d"][b], integ, with_pf)
    assert np.isfinite(ref["du"]).all() and np.abs(ref["du"]).max() > 0

    def L(q0, qd0, u):
        qt, qdt = P.rollout(ev, q0, qd0, u, h, ps, integ)
        return P.loss_and_cotangents(qt, qdt, cs["c"][b], cs["d"][b])[0]

    rng = np.random.default_rng(11)
    out = {}
    for name, grad in (("u", ref["du"]), ("q0", ref["dq0"]), ("qd0", ref["dqd0"])):
        dirs = rng.standard_normal((NDIR,) + grad.shape)
        num = np.array([(L(**dict(args, **{name: args[name] + EPS * dv})) - L(**dict(args, **{name: args[name] - EPS * dv}))) / (2 * EPS)
                        for dv in dirs])
        ana = (dirs.reshape(NDIR, -1) * grad.reshape(1, -1)).sum(axis=1)
        out[name] = (np.abs(num - ana), ana)
    return out


@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", [4, 8, 16])
def test_recursion_meets_central_differences(n, integ):
    cs, ev = _case(n)
    for name, (err, ana) in _fd_errors(cs, ev, 0, integ, True).items():
        print("n=%d BDF%d d/d%s: max |num - ana| / max|ana| = %.3e" % (n, integ, name, err.max() / np.abs(ana).max()))
        assert (err <= 2e-5 * np.abs(ana) + 1e-6 * np.abs(ana).max()).all(), (name, err, ana)


@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n", [4, 8, 16])
def test_without_D_pf_the_comparison_fails_by_a_hundred_floors(n, integ):
    """The negative control: H keeps the forces, D loses them."""
    cs, ev = _case(n)
    worst = 0.0
    for name, (err, ana) in _fd_errors(cs, ev, 0, integ, False).items():
        worst = max(worst, float((err / (2e-5 * np.abs(ana) + 1e-6 * np.abs(ana).max())).max()))
    print("n=%d BDF%d without D_pf: worst error = %.1f floors" % (n, integ, worst))
    assert worst >= 100.0


@pytest.mark.parametrize("n", P.SIZES)
def test_the_rollout_converges_on_every_input_of_the_gpu_tests(n):
    cs, ev = _case(n)
    for integ in (1, 2):
        for b in range(2):
            info = {}
            qt, qdt = P.rollout(ev, cs["q0"][b], cs["qd0"][b], cs["u"][b], cs["h"], cs["pscale"], integ, info)
            nsolves = cs["nsteps"] + (1 if integ == 2 else 0)
            print("n=%d BDF%d b=%d: %d iterations over %d solves" % (n, integ, b, info["iters"], nsolves))
            assert info["converged"] and np.isfinite(qt).all() and info["iters"] <= 10 * nsolves


def test_the_switching_scene_qualifies_for_the_gpu_tests():
    """Both conditions of its inclusion: the line-search-free Newton converges on it, and no recorded step of the proto has a cable
    with |l - L|/L < 1e-6 (where the cable is not differentiable); and the cables do switch."""
    cs = P.switching_case()
    ev = P.World(cs["sc"])
    for integ in (1, 2):
        for b in range(2):
            info = {}
            qt, qdt = P.rollout(ev, cs["q0"][b], cs["qd0"][b], cs["u"][b], cs["h"], cs["pscale"], integ, info)
            strain = P.cable_strains(ev, qt, qdt)
            print("switching BDF%d b=%d: %d iterations, min |l - L|/L = %.2e" % (integ, b, info["iters"], np.abs(strain).min()))
            assert info["converged"] and np.abs(strain).min() >= 1e-6
            taut = strain > 0
            assert taut.any(axis=0).all() and (~taut).any(axis=0).all()          # every cable is taut at some step and slack at another
