"""tests/proto_frame_cost.py against itself, on the CPU: the two forms of G = dv/dq agree; lx (in q and in qdot) meets central
differences of the proto's own longdouble value; the pull-back meets central differences of x, v and R; the Gauss-Newton addition is
the explicit sum, symmetric and positive semi-definite; a position-only call is proto_point_cost's.

Scenes: the 5-chain, the 7-joint tree, "fixed" of test_rollout_feedback_proto (nodes without a DOF) and sceneTree(15) (a branching
tree with prismatic and fixed joints).  Tolerances and step size: test_point_cost_proto's (central differences with e = 1e-6: rtol
1e-7 on the largest entry of the gradient; two evaluations of one Jacobian: 64 eps of its largest entry).
"""
import numpy as np
import pytest

import proto_frame_cost as F
import proto_point_cost as P
from test_point_cost_proto import SIZES, _dense, _record, _scene, terms_of

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def frame_terms_of(m, N):
    """terms_of with mixed weights, for a record of N >= 4 steps: step 1 owns a term with all three weights (tip) and a position-only
    one (inner body); step 2 owns none; step 3 owns position-only terms alone; step N owns a term with wrot alone on the root body and
    one with wvel alone on an inner body."""
    t = [dict(x, wvel=0.0, wrot=0.0) for x in terms_of(m, N)]
    t[0].update(wvel=0.8, wrot=1.2)
    t[4].update(wpos=0.0, wrot=3.0)
    t.append(dict(body=max(1, m["n"] // 2), xlocal=[-0.3, 0.25, 0.4], step=N, wpos=0.0, wvel=1.5, wrot=0.0))
    return t


def _targets(rng, T):
    Rt = np.array([F.rot(rng.standard_normal(3), rng.uniform(0.5, 2.0)) for _ in range(T)])
    return rng.standard_normal((T, 3)), rng.standard_normal((T, 3)), Rt


@pytest.mark.parametrize("size", SIZES)
def test_the_two_forms_of_G_agree(size):
    sc, m = _scene(size)
    q, qd, _ = _record(sc, 3, 1)
    kin = P.kinematics(m, q[0])
    tw = F.twists(m, kin, qd[0])
    for t in frame_terms_of(m, 4):
        f = F.frame(m, kin, tw, t["body"], t["xlocal"])
        Gs = F.G_summed(m, kin, qd[0], t["body"], f["p"])
        scale = max(np.max(np.abs(Gs)), np.max(np.abs(f["Jp"])))
        assert np.max(np.abs(f["G"] - Gs)) <= 64 * EPS * scale
        assert np.max(np.abs(f["v"] - f["Jp"] @ qd[0])) <= 64 * EPS * max(np.max(np.abs(f["v"])), 1.0)
        off = [m["idx"][j] for j in range(m["n"]) if m["idx"][j] >= 0 and not m["anc"][j, t["body"]]]
        assert (f["G"][:, off] == 0.0).all() and (f["Jw"][:, off] == 0.0).all()


@pytest.mark.parametrize("size", SIZES)
def test_the_longdouble_frames_are_the_float64_frames(size):
    sc, m = _scene(size)
    q, qd, _ = _record(sc, 5, 4)
    terms = frame_terms_of(m, 4)
    for a, b in zip(F.frames(m, q, qd, terms), F.frames(m, q, qd, terms, LD)):
        assert b.dtype == LD
        assert np.max(np.abs(a - b)) <= 64 * EPS * max(1.0, float(np.max(np.abs(b))))


@pytest.mark.parametrize("size", SIZES)
def test_lx_and_the_pullback_meet_central_differences(size):
    sc, m = _scene(size)
    N, nr = 4, sc.nr
    q, qd, rng = _record(sc, 7, N)
    terms = frame_terms_of(m, N)
    T = len(terms)
    Q, xg = _dense(rng, N, nr)
    xt, vt, Rt = _targets(rng, T)
    gx, gv, gR = rng.standard_normal((T, 3)), rng.standard_normal((T, 3)), rng.standard_normal((T, 3, 3))

    def val(q_, qd_):
        return F.cost(m, q_, qd_, Q, xg, terms, xt, vt, Rt, LD)["Jk"].sum()

    out = F.cost(m, q, qd, Q, xg, terms, xt, vt, Rt, LD)
    gq, gqd = F.pullback(m, q, qd, terms, gx, gv, gR, LD)
    e = LD(1e-6)
    qL, qdL = q.astype(LD), qd.astype(LD)
    for _ in range(3):
        dq, dqd = rng.standard_normal(q.shape).astype(LD), rng.standard_normal(q.shape).astype(LD)
        # lx, in q alone, in qdot alone, and in both
        for sq, sv in ((1, 0), (0, 1), (1, 1)):
            num = (val(qL + e * sq * dq, qdL + e * sv * dqd) - val(qL - e * sq * dq, qdL - e * sv * dqd)) / (2 * e)
            ana = sq * np.sum(out["lx"][:, :nr] * dq) + sv * np.sum(out["lx"][:, nr:] * dqd)
            print("%s lx (%d, %d): numeric %.12e analytic %.12e" % (size, sq, sv, num, ana))
            assert abs(num - ana) <= 1e-7 * max(abs(ana), np.max(np.abs(out["lx"])))
            fp = F.frames(m, qL + e * sq * dq, qdL + e * sv * dqd, terms, LD)
            fm = F.frames(m, qL - e * sq * dq, qdL - e * sv * dqd, terms, LD)
            for name, cot in (("x", (gx, None, None)), ("v", (None, gv, None)), ("R", (None, None, gR)), ("all", (gx, gv, gR))):
                num = sum(np.sum(c * (a - b)) for c, a, b in zip(cot, fp, fm) if c is not None) / (2 * e)
                g1, g2 = F.pullback(m, q, qd, terms, *cot, dtype=LD)
                ana = sq * np.sum(g1 * dq) + sv * np.sum(g2 * dqd)
                assert abs(num - ana) <= 1e-7 * max(abs(ana), np.max(np.abs(g1)), np.max(np.abs(g2))), (name, sq, sv, num, ana)
    assert (gq[1] == 0.0).all() and (gqd[1] == 0.0).all()      # step 2 owns no term


@pytest.mark.parametrize("size", SIZES)
def test_the_gauss_newton_table(size):
    sc, m = _scene(size)
    N, nr = 4, sc.nr
    q, qd, rng = _record(sc, 9, N)
    terms = frame_terms_of(m, N)
    Q, xg = _dense(rng, N, nr)
    xt, vt, Rt = _targets(rng, len(terms))
    out = F.cost(m, q, qd, Q, xg, terms, xt, vt, Rt)
    D = out["Q"] - Q
    assert (D[1] == 0.0).all()                                              # step 2: no term
    assert (D[2][nr:, :] == 0.0).all() and (D[2][:, nr:] == 0.0).all()      # step 3: position-only terms
    for k, own in enumerate(P.by_step(terms, N)):
        A = np.zeros((2 * nr, 2 * nr))
        kin = P.kinematics(m, q[k])
        tw = F.twists(m, kin, qd[k])
        for i in own:
            f = F.frame(m, kin, tw, terms[i]["body"], terms[i]["xlocal"])
            wp, wv, wr = F.term_weights(terms[i])
            Z = np.zeros((3, nr))
            for w, row in ((wp, np.hstack([f["Jp"], Z])), (wv, np.hstack([f["G"], f["Jp"]])), (wr, np.hstack([f["Jw"], Z]))):
                A += w * row.T @ row
        scale = max(np.max(np.abs(out["Q"][k])), 1.0)
        assert np.max(np.abs(D[k] - A)) <= 64 * EPS * scale
        assert np.max(np.abs(D[k] - D[k].T)) <= 64 * EPS * scale
        assert np.linalg.eigvalsh(0.5 * (A + A.T)).min() >= -64 * EPS * scale


@pytest.mark.parametrize("size", SIZES)
def test_position_only_terms_are_the_point_cost(size):
    sc, m = _scene(size)
    N, nr = 4, sc.nr
    q, qd, rng = _record(sc, 11, N)
    terms = terms_of(m, N)
    Q, xg = _dense(rng, N, nr)
    xt = rng.standard_normal((len(terms), 3))
    a, b = F.cost(m, q, qd, Q, xg, terms, xt), P.cost(m, q, qd, Q, xg, terms, xt)
    for k in ("Jk", "lx", "Q", "x"):
        assert np.array_equal(a[k], b[k]), k
    gx = rng.standard_normal((len(terms), 3))
    assert np.array_equal(F.pullback(m, q, qd, terms, gx)[0], P.pullback(m, q, terms, gx))


def test_the_chordal_cost_is_one_minus_cos_theta():
    rng = np.random.default_rng(13)
    for th in (0.0, 0.3, 1.7, np.pi):
        R0, ax = F.rot(rng.standard_normal(3), 0.9), rng.standard_normal(3)
        Rt = R0 @ F.rot(ax, th)
        assert abs(np.sum((R0 - Rt) ** 2) / 4 - (1 - np.cos(th))) <= 64 * EPS
        ew = F.avec(R0 @ Rt.T) / 2
        assert abs(np.linalg.norm(ew) - abs(np.sin(th))) <= 64 * EPS      # the gradient vanishes at theta = pi
