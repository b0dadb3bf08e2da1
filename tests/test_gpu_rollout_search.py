"""rmx_rollout_search: the backtracking line search of the device iLQR in one launch (redmax_amd/csrc/rmx_search.h), on the GPU.

B = 4, N = 5.  Scenes: sceneAdjointChain(3) (NP 4), (5) (NP 8), (11) (NP 16), (32) (NP 32, M and D on the matrix cores).  Initial
states: test_rollout_vjp_proto.case.  Terms: test_frame_cost_proto.frame_terms_of - point and frame terms, step 2 without a term.
Q dense symmetric positive semi-definite, another table at every step (and, per rollout, for every rollout); R dense symmetric positive
definite.

The nominal comes from a nalpha = 0 call; kff, K from rmx_rollout_lqr on its tape with the model of rmx_rollout_cost_frames.  Rollout
0 searches along kff, rollout 1 along 6 kff (the full step overshoots: on a quadratic the cost falls for a step below 2, so 6 a is
refused for a = 1 and 0.5 and taken for 0.25; 1.5 kff on the 32-chain: see OVERSHOOT), rollout 2 along -kff (an ascent direction), rollout 3 along kff with a NaN in one row
(Newton status bits in every trial pass).

The checks, in the order of the sections below:
  1. decisions, exact: alpha, trials and every output of the searched call against single-pass (nalpha = 0) calls under
     uff = ubar + a kff formed in numpy, the outputs of a following rmx_rollout_vjp included; the four rollouts cover the three outcomes;
  2. nominal back, exact: rollouts 2 and 3 return the nominal call's bits, and a nalpha = 0 call from the accepted trajectories
     reproduces them;
  3. the value: J against the longdouble evaluation of tests/proto_search.py on the returned record, e_gpu <= 8 max(e_ref, 16 eps)
     with e_ref the float64 proto's error (the rule of test_gpu_rollout_lqr._judge), at every size, for shared and per-rollout tables,
     with and without R, sc and ft;
  4. the pass itself: a nalpha = 0 call against rmx_rollout_tape_feedback_box on the same inputs and against the closed loop of
     tests/proto_rollout_feedback.py, 1e-9 relative per step - the tolerance tests/test_gpu_rollout_feedback.py holds that kernel to
     against that proto, for qtraj, qdtraj and (against the proto) uapp; uapp against the feedback kernel's within what the
     difference of the two kernels' states and the rounding of the feedback sum allow; with limits every uapp lies inside them and J's
     control part is that of the clamped torque; 4b. the same on a branching tree and on a chain with nodes that have no DOF;
  5. invariance (permuted batch, B = 1 against B = 4, optional outputs NULL, device against host form: bits equal) and refusals:
     the entry's own, rmx_rollout_tape_feedback_box's (the four kinds of model outside the adjoint path included),
     rmx_rollout_cost_frames' and both of rmx_rollout_lqr's (nr > 32; more than 32 nodes with fewer reduced DOFs).

Measured on an MI355X (pytest -s): profiles/ilqr_search.txt holds the tables these tests print.  Decisions: alpha = (1, 0.25, 0, 0)
and trials = (1, 3, 5, 5) at every size.  J: every e_ref and e_gpu below 1.5e-15, under the floor of the bound (8 * 16 eps =
2.84e-14).  The largest difference of a nalpha = 0 pass to rmx_rollout_tape_feedback_box: 2.89e-13 (32-chain, with limits), zero
on the 5-chain without limits - the docstring of test_a_single_pass_is_the_feedback_kernels has every figure.
"""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (ahead of the library: torch finds its HIP runtime by file name, and a process must hold one runtime only)

import proto_search as S
import proto_worldframe as pw
from test_frame_cost_proto import frame_terms_of
from test_gpu_adjoint_controls import _rel, _scene
from test_rollout_feedback_proto import closed_loop, feedback_case
from test_rollout_vjp_proto import case

B, N = 4, 5
SIZES = [3, 5, 11, 32]
ALPHAS = (1.0, 0.5, 0.25, 0.125)
MULT = (1.0, 6.0, -1.0, 1.0)      # the search direction of rollout b is MULT[b] * kff[b]; rollout 3 also has a NaN row
# ... but for the 32-chain, whose problem is stiff (max |kff| = 50 against max |ubar| = 0.3): measured on single passes along m kff,
# the cost falls up to m = 0.5 in every rollout, and from m = 0.75 (rollout 1) or m = 1 (rollouts 2, 3) on the Newton solves run into
# their iteration limit (status 2) with costs 1e7 .. 1e13 above Jbar.  Rollout 1 therefore searches along 1.5 kff there: a = 1 and
# a = 0.5 (m = 1.5, 0.75) are refused, a = 0.25 (m = 0.375) is taken.  Rollout 0 takes the full step with a clean status.
OVERSHOOT = {32: 1.5}
EPS = np.finfo(np.float64).eps
LD = np.longdouble
_CACHE = {}
_FLOW = {}


def _case(size):
    """Scene, proto model, terms, initial states, nominal torques and the cost's tables, shared and per rollout: made once."""
    if size not in _CACHE:
        sc = _scene(size, 1)
        m = pw.build_model(sc.desc())
        nr = sc.nr
        cs = case(sc, 61, nsteps=N, B=B)
        rng = np.random.default_rng(97)
        terms = frame_terms_of(m, N)
        T = len(terms)
        A = rng.standard_normal((B, N, 2 * nr, 2 * nr)) / np.sqrt(2 * nr)
        Q = np.einsum("bkij,bklj->bkil", A, A)
        q0, qd0 = sc.getQ()
        xg = np.concatenate([np.broadcast_to(q0, (B, N, nr)), np.broadcast_to(qd0, (B, N, nr))], axis=-1) + 0.3 * rng.standard_normal((B, N, 2 * nr))
        Ar = rng.standard_normal((nr, nr)) / np.sqrt(nr)
        R = Ar @ Ar.T + np.eye(nr)
        import proto_frame_cost as F
        Rt = np.array([[F.rot(rng.standard_normal(3), rng.uniform(0.5, 2.0)) for _ in range(T)] for _ in range(B)])
        xt, vt = 5.0 * rng.standard_normal((B, T, 3)), rng.standard_normal((B, T, 3))
        per = dict(Q=Q, xgoal=xg, xtarget=xt, vtarget=vt, Rtarget=Rt)
        _CACHE[size] = dict(sc=sc, m=m, terms=terms, q0=cs["q0"], qd0=cs["qd0"], u=cs["u"], c=cs["c"], d=cs["d"], R=R, per=per,
                            shared={k: v[0].copy() for k, v in per.items()})
    return _CACHE[size]


def _search(sim, c, tab, ubar, sel=slice(None), parts=("sc", "ft", "R"), **kw):
    """One call from the case's initial state: (qtraj, qdtraj, uapp, out)."""
    sim.set_state(c["q0"][sel], c["qd0"][sel])
    cost = {}
    if "sc" in parts:
        cost.update(Q=tab["Q"], xgoal=tab["xgoal"])
    if "ft" in parts:
        cost.update(terms=c["terms"], xtarget=tab["xtarget"], vtarget=tab["vtarget"], Rtarget=tab["Rtarget"])
    if "R" in parts:
        cost.update(R=c["R"])
    cost.update(kw)
    return sim.rollout_search(N, c["sc"].h, ubar, pscale=c["sc"].task["pscale"], **cost)


def _row(r, b, decision=False):
    """Rollout b of a result of rollout_search: [qtraj, qdtraj, uapp, J, status], with decision also alpha and trials."""
    return [x[b] for x in r[:3]] + [r[3][k][b] for k in ("J", "status") + (("alpha", "trials") if decision else ())]


def _flow(size):
    """The nominal, the directions and every single-pass reference of a size (per-rollout tables), on the GPU, once."""
    if size in _FLOW:
        return _FLOW[size]
    from redmax_amd import BatchSim
    c = _case(size)
    tab, sc, nr = c["per"], c["sc"], c["sc"].nr
    sim = BatchSim(sc, batch=B)
    nom = _search(sim, c, tab, c["u"], stats=True)
    assert sim.last_step_kernel() == "k_rollout_search<bdf1,tape,feedback>"
    assert (nom[3]["status"] & 7 == 0).all() and (nom[3]["alpha"] == 0).all() and (nom[3]["trials"] == 1).all()
    assert np.array_equal(nom[3]["status"], nom[3]["info"]["status"])
    qt, qdt, ubar = nom[:3]
    assert np.array_equal(ubar, c["u"])      # (no gains, no limits: the applied torque is the nominal's)
    model = sim.rollout_cost_frames(N, qt, qdt, Q=tab["Q"], xgoal=tab["xgoal"], terms=c["terms"], xtarget=tab["xtarget"], vtarget=tab["vtarget"],
                                    Rtarget=tab["Rtarget"], want=("lx", "Q"))
    lu = np.einsum("ij,bkj->bki", c["R"], ubar)
    kff, K, _, notpd = sim.rollout_lqr(N, model["lx"], lu, model["Q"], c["R"], mu=1e-6)
    assert not notpd.any()
    direction = kff * np.array(MULT)[:, None, None]
    direction[1] = kff[1] * OVERSHOOT.get(size, MULT[1])
    direction[3, 2] = np.nan
    xref = np.concatenate([np.concatenate([c["q0"], c["qd0"]], axis=1)[:, None], np.concatenate([qt, qdt], axis=2)[:, :-1]], axis=1)
    Jbar = nom[3]["J"]
    gq, gqd = c["c"], c["d"]
    single = {}      # alpha (0: the nominal) -> (result of the nalpha = 0 call under ubar + a * direction, its rmx_rollout_vjp)
    for a in (0.0,) + ALPHAS:
        uff = ubar if a == 0.0 else ubar + a * direction      # (two roundings per entry: numpy does not fuse)
        r = _search(sim, c, tab, uff, K=K, xref=xref)
        single[a] = (r, sim.rollout_vjp(N, gq, gqd))
    srch = _search(sim, c, tab, ubar, kff=direction, K=K, xref=xref, alphas=ALPHAS, Jbar=Jbar)
    vjp = sim.rollout_vjp(N, gq, gqd)
    sim.close()
    _FLOW[size] = dict(nom=nom, direction=direction, K=K, xref=xref, Jbar=Jbar, single=single, srch=srch, vjp=vjp)
    return _FLOW[size]


def _expected(f):
    """(alpha [B], trials [B]) the definition gives on the single-pass references."""
    alpha, trials = np.zeros(B), np.full(B, len(ALPHAS) + 1, dtype=np.int32)
    for b in range(B):
        for i, a in enumerate(ALPHAS):
            out = f["single"][a][0][3]
            if (out["status"][b] & 7) == 0 and out["J"][b] < f["Jbar"][b]:
                alpha[b], trials[b] = a, i + 1
                break
    return alpha, trials


# ---------------------------------------------------------------- 1. decisions, exact

@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_decisions_are_those_of_the_single_pass_calls(size):
    f = _flow(size)
    alpha, trials = _expected(f)
    out = f["srch"][3]
    for a in ALPHAS:
        o = f["single"][a][0][3]
        print("size %s alpha %-6g J_a - Jbar %s status %s" % (size, a, " ".join("%+.3e" % x for x in o["J"] - f["Jbar"]), o["status"]))
    print("size %s: Jbar %s alpha %s trials %s" % (size, f["Jbar"], out["alpha"], out["trials"]))
    assert np.array_equal(out["alpha"], alpha) and np.array_equal(out["trials"], trials)
    for b in range(B):
        ended, ended_vjp = f["single"][alpha[b]]
        assert all(np.array_equal(x, y) for x, y in zip(_row(f["srch"], b), _row(ended, b))), (size, b)
        assert all(np.array_equal(x[b], y[b]) for x, y in zip(f["vjp"], ended_vjp)), (size, b)
        assert np.isfinite(f["srch"][0][b]).all() and np.isfinite(f["vjp"][0][b]).all()
    # the three outcomes: the first alpha, a later one, none
    assert alpha[0] == ALPHAS[0] and alpha[1] in ALPHAS[1:] and alpha[2] == 0 and alpha[3] == 0, alpha
    assert (out["J"][:2] < f["Jbar"][:2]).all()
    # the NaN row gave status bits in every trial pass, not a fault; the rollout ended clean
    assert all(f["single"][a][0][3]["status"][3] & 4 for a in ALPHAS) and out["status"][3] & 7 == 0


# ---------------------------------------------------------------- 2. nominal back, exact

@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_the_nominal_comes_back_and_accepted_trajectories_reproduce(size):
    from redmax_amd import BatchSim
    f = _flow(size)
    c = _case(size)
    for b in (2, 3):
        got, nom = _row(f["srch"], b), _row(f["nom"], b)
        assert f["srch"][3]["alpha"][b] == 0
        # (record, uapp and J; trials differ: the searched call ran its trial passes first)
        assert all(np.array_equal(got[i], nom[i]) for i in (0, 1, 2, 3)), (size, b)
    qt, qdt, ua, out = f["srch"]
    xref = np.concatenate([np.concatenate([c["q0"], c["qd0"]], axis=1)[:, None], np.concatenate([qt, qdt], axis=2)[:, :-1]], axis=1)
    sim = BatchSim(c["sc"], batch=B)
    again = _search(sim, c, c["per"], ua, K=f["K"], xref=xref)
    sim.close()
    assert all(np.array_equal(x, y) for x, y in zip(again[:3], (qt, qdt, ua)))
    assert np.array_equal(again[3]["J"], out["J"]) and (again[3]["alpha"] == 0).all() and (again[3]["trials"] == 1).all()


# ---------------------------------------------------------------- 3. the value

def _proto_J(c, tab, per, parts, qt, qdt, ua, dtype):
    row = lambda a, b: a[b] if per else a      # noqa: E731
    J = []
    for b in range(qt.shape[0]):
        kw = {}
        if "sc" in parts:
            kw.update(Q=row(tab["Q"], b), xgoal=row(tab["xgoal"], b))
        if "ft" in parts:
            kw.update(terms=c["terms"], xtarget=row(tab["xtarget"], b), vtarget=row(tab["vtarget"], b), Rtarget=row(tab["Rtarget"], b))
        if "R" in parts:
            kw.update(R=c["R"])
        J.append(S.cost(c["m"], qt[b], qdt[b], ua[b], dtype=dtype, **kw)["J"])
    return np.array(J, dtype=dtype)


PARTS = [("sc", "ft", "R"), ("sc", "ft"), ("ft", "R"), ("sc", "R"), ("R",)]


@pytest.mark.gpu
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per"])
@pytest.mark.parametrize("size", SIZES)
def test_J_meets_the_extended_proto(size, per):
    """Measured on an MI355X: every e_gpu is below the floor of the bound, 8 * 16 eps = 2.84e-14 (profiles/ilqr_search.txt)."""
    from redmax_amd import BatchSim
    c = _case(size)
    tab = c["per" if per else "shared"]
    sim = BatchSim(c["sc"], batch=B)
    ok, record = True, None
    for parts in PARTS:
        qt, qdt, ua, out = _search(sim, c, tab, c["u"], parts=parts)
        if record is None:
            record = (qt, qdt, ua)
        assert all(np.array_equal(x, y) for x, y in zip(record, (qt, qdt, ua)))      # (the cost does not steer a nalpha = 0 pass)
        ref, ext = _proto_J(c, tab, per, parts, qt, qdt, ua, np.float64), _proto_J(c, tab, per, parts, qt, qdt, ua, LD)
        for b in range(B):
            e_ref, e_gpu = S.rel_err(ref[b], ext[b]), S.rel_err(out["J"][b], ext[b])
            bound = 8 * max(e_ref, 16 * EPS)
            print("size %s %-6s %-8s b %d: J %.6e e_ref %.2e e_gpu %.2e bound %.2e%s"
                  % (size, "per" if per else "shared", "+".join(parts), b, out["J"][b], e_ref, e_gpu, bound, "" if e_gpu <= bound else "   <-- over"))
            ok = ok and e_gpu <= bound
    sim.close()
    assert ok


# ---------------------------------------------------------------- 4. the pass itself

@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_a_single_pass_is_the_feedback_kernels(size):
    """A nalpha = 0 call against rmx_rollout_tape_feedback_box on the same inputs (the gains and reference of the flow), without and
    with limits: the record per step to 1e-9 relative, the Newton status equal.  The kernel is a text of its own (rmx_search.h), not
    an instantiation of k_adjoint_fwd, so bits are not promised.  Measured on an MI355X, the largest |difference| over q, qdot and
    uapp, without / with limits that bind: 3-chain 3.55e-15 / 2.55e-15; 5-chain 0 (ZERO: the same bits) / 2.67e-15; 11-chain
    4.19e-14 / 6.77e-15; 32-chain 6.75e-14 / 2.89e-13 (the largest: in qdot, a difference of q over h).  uapp against the feedback
    kernel's: at most 0.93 of its bound (3-chain without limits), 0 on the 5-chain without limits."""
    from redmax_amd import BatchSim
    f, c = _flow(size), _case(size)
    sc = c["sc"]
    sim = BatchSim(sc, batch=B)
    spread = np.abs(c["u"]).max()
    for ulim in (None, (np.full(sc.nr, -0.3 * spread), np.full(sc.nr, 0.4 * spread))):
        got = _search(sim, c, c["per"], c["u"], K=f["K"], xref=f["xref"], ulim=ulim, stats=True)
        sim.set_state(c["q0"], c["qd0"])
        qt, qdt, ua, info = sim.rollout_feedback(N, sc.h, c["u"], K=f["K"], xref=f["xref"], pscale=sc.task["pscale"], stats=True,
                                                 ulim=ulim if ulim is not None else (None, None))
        assert "feedback,box" in sim.last_step_kernel()
        diff = max(np.abs(got[0] - qt).max(), np.abs(got[1] - qdt).max(), np.abs(got[2] - ua).max())
        print("size %s limits %s: max |search - feedback kernel| over q, qdot, uapp = %.3e%s"
              % (size, ulim is not None, diff, " (zero: the same bits)" if diff == 0 else ""))
        for b in range(B):
            for k in range(N):
                assert _rel(got[0][b, k], qt[b, k]) <= 1e-9 and _rel(got[1][b, k], qdt[b, k]) <= 1e-9, (size, b, k)
        # uapp is one formula, clamp(uff + K'(x - xref)), on the two kernels' nearly equal start states: it may differ by K' applied to
        # the difference of those states and by the rounding of the sum - (2nr + 2) eps (|uff| + |K|'|x - xref|), the bound
        # tests/test_gpu_rollout_feedback.py holds the feedback kernel's uapp to, once for either kernel; the clamp is 1-Lipschitz
        x0 = np.concatenate([c["q0"], c["qd0"]], axis=1)[:, None]
        xs = np.concatenate([x0, np.concatenate([got[0], got[1]], axis=2)[:, :-1]], axis=1)
        xf = np.concatenate([x0, np.concatenate([qt, qdt], axis=2)[:, :-1]], axis=1)
        absK = np.abs(f["K"])
        bound = np.einsum("bkji,bkj->bki", absK, np.abs(xs - xf)) + 2 * (2 * sc.nr + 2) * EPS * (
            np.abs(c["u"]) + np.einsum("bkji,bkj->bki", absK, np.abs(xf - f["xref"])))
        err = np.abs(got[2] - ua)
        print("size %s limits %s: max |uapp - feedback kernel's| / bound = %.3f" % (size, ulim is not None, (err / bound).max()))
        assert (err <= bound).all(), (size, (err / bound).max())
        assert np.array_equal(got[3]["info"]["status"] & 7, info["status"] & 7)
        if ulim is not None:
            assert (got[2] >= ulim[0]).all() and (got[2] <= ulim[1]).all()
            assert (got[2] == ulim[0]).any() and (got[2] == ulim[1]).any()      # (the limits bite)
            only_R = _search(sim, c, c["per"], c["u"], K=f["K"], xref=f["xref"], ulim=ulim, parts=("R",))
            assert np.array_equal(only_R[2], got[2])
            for b in range(B):      # the control part is that of the CLAMPED torque
                ref, ext = S.control_part(got[2][b], c["R"]).sum(), S.control_part(got[2][b], c["R"], LD).sum()
                assert S.rel_err(only_R[3]["J"][b], ext) <= 8 * max(S.rel_err(ref, ext), 16 * EPS), (size, b)
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, 32])
def test_a_single_pass_meets_the_closed_loop_proto(oracle_lib, size):
    """The inputs of tests/test_gpu_rollout_feedback.py (feedback_case) through a nalpha = 0 call, against the oracle's closed loop:
    qtraj, qdtraj and uapp 1e-9 relative per step - that file's bound for the feedback kernel's record.  The 5-chain in full, the
    32-chain rollout 0."""
    from redmax_amd import BatchSim
    sc, cs, nsteps = feedback_case(size, 1)
    Bf = cs["q0"].shape[0]
    sim = BatchSim(sc, batch=Bf)
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, ua, out = sim.rollout_search(nsteps, sc.h, cs["u"], K=cs["K"], xref=cs["xref"], R=np.eye(sc.nr), pscale=sc.task["pscale"])
    sim.close()
    assert (out["status"] & 15 == 0).all()
    for b in range(Bf if size == 5 else 1):
        ref = closed_loop(oracle_lib, size, 1, b)
        for k in range(nsteps):
            assert _rel(qt[b, k], ref["qtraj"][k]) <= 1e-9, (size, b, k, _rel(qt[b, k], ref["qtraj"][k]))
            # (qdot and the applied torque at the same bound: measured 1.2e-13 and 7.9e-14 at the most)
            assert _rel(qdt[b, k], ref["qdtraj"][k]) <= 1e-9 and _rel(ua[b, k], ref["uapp"][k]) <= 1e-9, (size, b, k)
        print("size %s b %d: |qtraj - proto| / |proto| = %.3e, qdtraj %.3e, uapp %.3e"
              % (size, b, _rel(qt[b], ref["qtraj"]), _rel(qdt[b], ref["qdtraj"]), _rel(ua[b], ref["uapp"])))


# ---------------------------------------------------------------- 4b. a branching tree, and nodes without a DOF

@pytest.mark.gpu
@pytest.mark.parametrize("size", ["tree7", "fixed"])
def test_trees_and_nodes_without_a_dof(size):
    """The scenes above are serial chains with a DOF on every node: reduced index == lane.  "tree7" (a branching tree: the pointer
    jumping of cost_front) and "fixed" (two nodes without a DOF: the map from reduced DOF to node, the dof masks) of
    test_rollout_feedback_proto.feedback_case, B = 3, 6 steps, its gains and reference: the pass against the feedback kernel, J by the
    rule of section 3, and a searched call against the single-pass call of the alpha each rollout took, bit for bit."""
    from redmax_amd import BatchSim
    sc, cs, n = feedback_case(size, 1)
    Bf, nr, ps = cs["q0"].shape[0], sc.nr, sc.task["pscale"]
    m = pw.build_model(sc.desc())
    rng = np.random.default_rng(101)
    terms = frame_terms_of(m, n)
    T = len(terms)
    A = rng.standard_normal((Bf, n, 2 * nr, 2 * nr)) / np.sqrt(2 * nr)
    Q = np.einsum("bkij,bklj->bkil", A, A)
    q0, qd0 = sc.getQ()
    xg = np.concatenate([np.broadcast_to(q0, (Bf, n, nr)), np.broadcast_to(qd0, (Bf, n, nr))], axis=-1) + 0.3 * rng.standard_normal((Bf, n, 2 * nr))
    Ar = rng.standard_normal((nr, nr)) / np.sqrt(nr)
    R = Ar @ Ar.T + np.eye(nr)
    import proto_frame_cost as F
    Rt = np.array([F.rot(rng.standard_normal(3), rng.uniform(0.5, 2.0)) for _ in range(T)])
    xt, vt = 5.0 * rng.standard_normal((T, 3)), rng.standard_normal((T, 3))
    cost = dict(Q=Q, xgoal=xg, terms=terms, xtarget=xt, vtarget=vt, Rtarget=Rt, R=R)
    sim = BatchSim(sc, batch=Bf)

    def run(uff, K, xref, **kw):
        sim.set_state(cs["q0"], cs["qd0"])
        return sim.rollout_search(n, sc.h, uff, K=K, xref=xref, pscale=ps, **cost, **kw)

    qt, qdt, ua, out = run(cs["u"], cs["K"], cs["xref"])
    assert (out["status"] & 7 == 0).all()
    sim.set_state(cs["q0"], cs["qd0"])
    fq, fqd, fua = sim.rollout_feedback(n, sc.h, cs["u"], K=cs["K"], xref=cs["xref"], pscale=ps)
    print("%s: max |search - feedback kernel| over q, qdot, uapp = %.3e" % (size, max(np.abs(qt - fq).max(), np.abs(qdt - fqd).max(), np.abs(ua - fua).max())))
    for b in range(Bf):
        for k in range(n):
            assert _rel(qt[b, k], fq[b, k]) <= 1e-9 and _rel(qdt[b, k], fqd[b, k]) <= 1e-9 and _rel(ua[b, k], fua[b, k]) <= 1e-9, (size, b, k)
        kw = dict(Q=Q[b], xgoal=xg[b], R=R, terms=terms, xtarget=xt, vtarget=vt, Rtarget=Rt)
        ref, ext = S.cost(m, qt[b], qdt[b], ua[b], **kw)["J"], S.cost(m, qt[b], qdt[b], ua[b], dtype=LD, **kw)["J"]
        e_ref, e_gpu = S.rel_err(ref, ext), S.rel_err(out["J"][b], ext)
        print("%s b %d: J %.6e e_ref %.2e e_gpu %.2e" % (size, b, out["J"][b], e_ref, e_gpu))
        assert e_gpu <= 8 * max(e_ref, 16 * EPS), (size, b, e_ref, e_gpu)
    # a search from this nominal along the sweep's direction, against single passes
    model = sim.rollout_cost_frames(n, qt, qdt, Q=Q, xgoal=xg, terms=terms, xtarget=xt, vtarget=vt, Rtarget=Rt, want=("lx", "Q"))
    kff, K, _, notpd = sim.rollout_lqr(n, model["lx"], np.einsum("ij,bkj->bki", R, ua), model["Q"], R, mu=1e-6)
    assert not notpd.any()
    xref = np.concatenate([np.concatenate([cs["q0"], cs["qd0"]], axis=1)[:, None], np.concatenate([qt, qdt], axis=2)[:, :-1]], axis=1)
    srch = run(ua, K, xref, kff=kff, alphas=ALPHAS, Jbar=out["J"])
    alpha = srch[3]["alpha"]
    print("%s: alpha %s trials %s J - Jbar %s" % (size, alpha, srch[3]["trials"], srch[3]["J"] - out["J"]))
    assert (alpha > 0).any() and (srch[3]["J"] <= out["J"]).all()      # (alpha 0: ubar + 0 kff is ubar, the nominal pass again)
    single = run(ua + alpha[:, None, None] * kff, K, xref)
    assert all(np.array_equal(x, y) for x, y in zip(single[:3], srch[:3]))
    assert np.array_equal(single[3]["J"], srch[3]["J"]) and np.array_equal(single[3]["status"], srch[3]["status"])
    sim.close()


# ---------------------------------------------------------------- 5. invariance and refusals

@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_permutation_batch_size_null_outputs_and_shared_tables(size):
    from redmax_amd import BatchSim
    f, c = _flow(size), _case(size)
    tab = c["per"]
    kw = dict(kff=f["direction"], K=f["K"], xref=f["xref"], alphas=ALPHAS, Jbar=f["Jbar"])
    perm = np.array([2, 0, 3, 1])
    sim = BatchSim(c["sc"], batch=B)
    ptab = {k: v[perm] for k, v in tab.items()}
    pkw = dict(kff=kw["kff"][perm], K=kw["K"][perm], xref=kw["xref"][perm], alphas=ALPHAS, Jbar=kw["Jbar"][perm])
    sim.set_state(c["q0"][perm], c["qd0"][perm])
    cost = dict(Q=ptab["Q"], xgoal=ptab["xgoal"], terms=c["terms"], xtarget=ptab["xtarget"], vtarget=ptab["vtarget"], Rtarget=ptab["Rtarget"], R=c["R"])
    p = sim.rollout_search(N, c["sc"].h, c["u"][perm], pscale=c["sc"].task["pscale"], **cost, **pkw)
    for i, b in enumerate(perm):
        assert all(np.array_equal(x, y) for x, y in zip(_row(p, i, True), _row(f["srch"], b, True))), (size, b)
    # optional outputs NULL
    bare = _search(sim, c, tab, f["nom"][2], want=(), **kw)
    assert sorted(bare[3]) == ["J"] and all(np.array_equal(x, y) for x, y in zip(bare[:3], f["srch"][:3]))
    assert np.array_equal(bare[3]["J"], f["srch"][3]["J"])
    sim.close()
    # B = 1 against B = 4, and shared tables (rollout b's own) against per-rollout ones
    for b in (0, 1, 3):
        one = BatchSim(c["sc"], batch=1)
        sel = slice(b, b + 1)
        one.set_state(c["q0"][sel], c["qd0"][sel])
        cost1 = dict(Q=tab["Q"][b], xgoal=tab["xgoal"][b], terms=c["terms"], xtarget=tab["xtarget"][b], vtarget=tab["vtarget"][b],
                     Rtarget=tab["Rtarget"][b], R=c["R"])
        r = one.rollout_search(N, c["sc"].h, f["nom"][2][sel], kff=kw["kff"][sel], K=kw["K"][b], xref=kw["xref"][b], alphas=ALPHAS,
                               Jbar=kw["Jbar"][sel], pscale=c["sc"].task["pscale"], **cost1)
        one.close()
        assert all(np.array_equal(x, y) for x, y in zip(_row(r, 0, True), _row(f["srch"], b, True))), (size, b)


@pytest.mark.gpu
def test_the_device_form_returns_the_host_forms_bits():
    from redmax_amd import BatchSim, diff, ilqr
    size = 5
    f, c = _flow(size), _case(size)
    tab, sc = c["per"], c["sc"]
    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)      # noqa: E731
    sim = BatchSim(sc, batch=B)
    cost = ilqr.TrackingCost(sim, t(tab["Q"]), t(c["R"]), t(tab["xgoal"]), c["terms"], t(tab["xtarget"]), t(tab["vtarget"]), t(tab["Rtarget"]))
    qt, qdt, ua, J, alpha, status = diff.rollout_search(sim, t(c["q0"]), t(c["qd0"]), t(f["nom"][2]), t(f["direction"]), t(f["K"]), t(f["xref"]), ALPHAS,
                                                        t(f["Jbar"]), cost=cost, pscale=sc.task["pscale"], h=sc.h)
    assert not qt.requires_grad
    vjp = sim.rollout_vjp(N, c["c"], c["d"])
    sim.close()
    h = f["srch"]
    for got, want in ((qt, h[0]), (qdt, h[1]), (ua, h[2]), (J, h[3]["J"]), (alpha, h[3]["alpha"]), (status, h[3]["status"])):
        assert np.array_equal(got.cpu().numpy(), want)
    assert all(np.array_equal(x, y) for x, y in zip(vjp, f["vjp"]))


def _raw_call(sim, c, f, **over):
    """rmx_rollout_search through ctypes alone, from valid host arguments with single members replaced: (rc, message)."""
    from redmax_amd import _abi
    L = _abi.lib()
    tab, nr = c["per"], c["sc"].nr
    keep = dict(u=np.ascontiguousarray(f["nom"][2]), kff=np.ascontiguousarray(np.nan_to_num(f["direction"])), K=np.ascontiguousarray(f["K"]),
                xref=np.ascontiguousarray(f["xref"]), Jbar=np.ascontiguousarray(f["Jbar"]), al=np.array(over.get("alphas", ALPHAS), dtype=np.float64),
                Q=np.ascontiguousarray(tab["Q"]), xg=np.ascontiguousarray(tab["xgoal"]), R=np.ascontiguousarray(c["R"]),
                xt=np.ascontiguousarray(tab["xtarget"]), vt=np.ascontiguousarray(tab["vtarget"]),
                Rt=np.ascontiguousarray(np.swapaxes(tab["Rtarget"], -1, -2)), lo=np.full(nr, -1.0), hi=np.full(nr, 1.0))
    arr, nterms = sim._frame_terms(over.get("terms", c["terms"]), "test", c["sc"].h)
    ad = lambda k: keep[k].ctypes.data      # noqa: E731
    fb = _abi.Feedback(ad("u"), ad("K"), ad("xref"), over.get("fb_per", 1))
    sc_ = _abi.StateCost(ad("Q"), ad("xg"), over.get("Q_per", 1), 1)
    ft = _abi.FrameTerms(over.get("nterms", nterms), arr, ad("xt"), None if over.get("no_vt") else ad("vt"), ad("Rt"), over.get("t_per", 1))
    cost = _abi.SearchCost(C.pointer(sc_), C.pointer(ft), ad("R"))
    if over.get("no_cost"):
        cost = _abi.SearchCost(None, None, None)
    nalpha = over.get("nalpha", len(keep["al"]))
    srch = _abi.Search(None if over.get("no_kff") else ad("kff"), _abi.dptr(keep["al"]), nalpha, None if over.get("no_Jbar") else ad("Jbar"))
    out = [np.empty((B, N, nr)) for _ in range(3)] + [np.empty(B)]
    so = _abi.SearchOut(None if over.get("no_J") else out[3].ctypes.data, None, None, None)
    box = _abi.Box(ad("lo"), ad("hi"))
    if "lo" in over:
        keep["lo"][:] = over["lo"]
    opts = sim._tape_opts(c["sc"].h)
    null = over.get("null", ())
    args = [sim._batch, C.byref(opts), over.get("nsteps", N), float(c["sc"].task["pscale"]), C.byref(fb), C.byref(box), C.byref(srch), C.byref(cost),
            out[0].ctypes.data, None if over.get("no_qd") else out[1].ctypes.data, out[2].ctypes.data, C.byref(so), None]
    names = ["b", "opts", "nsteps", "pscale", "fb", "box", "s", "cost", "qtraj", "qdtraj", "uapp", "out", "stats"]
    for n in null:
        args[names.index(n)] = None
    rc = L.rmx_rollout_search(*args)
    return rc, (L.rmx_last_error() or b"").decode()


@pytest.mark.gpu
def test_refusals_leave_the_tape_and_the_batch_alone():
    from redmax_amd import BatchSim, _abi
    size = 5
    f, c = _flow(size), _case(size)
    sim = BatchSim(c["sc"], batch=B)
    sim.set_state(c["q0"], c["qd0"])
    rc, msg = _raw_call(sim, c, f)      # (the helper's arguments are valid)
    assert rc == 0, msg
    _search(sim, c, c["per"], c["u"])
    gq, gqd = c["c"], c["d"]
    vjp0, state0 = sim.rollout_vjp(N, gq, gqd), sim.get_state()
    bad_w = [dict(t) for t in c["terms"]]
    bad_w[0]["wvel"] = -1.0
    bad_step = [dict(t) for t in c["terms"]]
    bad_step[1]["step"] = N + 1
    refusals = [
        (dict(null=("fb",)), "rmx_rollout_search: null argument"), (dict(null=("s",)), "rmx_rollout_search: null argument"),
        (dict(null=("cost",)), "rmx_rollout_search: null argument"), (dict(null=("out",)), "rmx_rollout_search: null argument"),
        (dict(no_J=True), "rmx_rollout_search: null argument"),
        (dict(no_cost=True), "sc, ft and R are all null"),
        (dict(nalpha=17), "nalpha must be 0 .. 16"), (dict(nalpha=-1), "nalpha must be 0 .. 16"),
        (dict(alphas=(1.0, 0.0, 0.25, 0.125)), "alpha 1 must be finite and > 0"), (dict(alphas=(1.0, 0.5, float("nan"), 0.1)), "alpha 2 must be finite"),
        (dict(alphas=(float("inf"), 0.5, 0.2, 0.1)), "alpha 0 must be finite"), (dict(alphas=(1.0, 0.5, 0.2, -0.1)), "alpha 3 must be finite and > 0"),
        (dict(no_kff=True), "nalpha > 0 needs alphas, kff and Jbar"), (dict(no_Jbar=True), "nalpha > 0 needs alphas, kff and Jbar"),
        # rmx_rollout_tape_feedback_box's
        (dict(fb_per=2), "per_rollout must be 0 or 1"), (dict(nsteps=0), "nsteps < 1"), (dict(no_qd=True), "qtraj and qdtraj must be given together"),
        (dict(lo=2.0), "ulo > uhi at DOF 0"), (dict(lo=float("nan")), "a bound of DOF 0 is NaN"),
        # rmx_rollout_cost_frames'
        (dict(t_per=3), "per_rollout must be 0 or 1"), (dict(Q_per=2), "Q_per_rollout and goal_per_rollout must be 0 or 1"),
        (dict(nterms=0), "nterms < 1"), (dict(terms=bad_w), "term 0: wvel must be finite and >= 0"),
        (dict(no_vt=True), "wvel > 0 needs vtarget, which is null"), (dict(terms=bad_step), "step"),
    ]
    for over, words in refusals:
        rc, msg = _raw_call(sim, c, f, **over)
        assert rc == -1 and words in msg, (over, rc, msg)      # RMX_E_INVALID
        assert all(np.array_equal(x, y) for x, y in zip(sim.get_state(), state0)), over
    assert all(np.array_equal(x, y) for x, y in zip(vjp0, sim.rollout_vjp(N, gq, gqd)))
    with pytest.raises(ValueError, match="at most 16 alphas"):
        _search(sim, c, c["per"], c["u"], kff=np.zeros_like(c["u"]), Jbar=np.zeros(B), alphas=np.ones(17))
    sim.close()
    # nr > 32, in rmx_rollout_lqr's words
    sc40 = _scene(40, 1)
    c40 = case(sc40, 53, nsteps=2, B=1)
    sim = BatchSim(sc40, batch=1)
    sim.set_state(c40["q0"], c40["qd0"])
    sim.rollout_tape(2, sc40.h, c40["u"], pscale=sc40.task["pscale"])
    g = np.ones((1, 2, 40))
    vjp40 = sim.rollout_vjp(2, g, g)
    with pytest.raises(_abi.RedMaxHipError, match=r"rmx_rollout_search: nr > 32.*nr = 40"):
        sim.rollout_search(2, sc40.h, c40["u"], R=np.eye(40), pscale=sc40.task["pscale"])
    assert all(np.array_equal(x, y) for x, y in zip(vjp40, sim.rollout_vjp(2, g, g)))
    sim.close()


def _fixed_links_chain(n):
    """A serial chain of n links in which every second joint is fixed: n nodes, n / 2 reduced DOFs (sceneChain's bodies and offsets)."""
    from redmax_amd.redmax import BodyCuboid, JointFixed, JointRevolute, Scene
    from redmax_amd.scenes import _T
    scene = Scene()
    scene.name = "%d-link chain, every second joint fixed" % n
    for i in range(n):
        scene.bodies.append(BodyCuboid(1.0, [10, 1, 1]))
        parent = scene.joints[i - 1] if i else None
        scene.joints.append(JointFixed(parent, scene.bodies[-1]) if i % 2 else JointRevolute(parent, scene.bodies[-1], [0, 1, 0]))
        scene.joints[-1].setJointTransform(np.eye(4) if i == 0 else _T([10, 0, 0]))
        scene.bodies[-1].setBodyTransform(_T([5, 0, 0]))
    return scene


@pytest.mark.gpu
def test_a_tree_of_more_than_32_nodes_is_refused_in_the_sweeps_words():
    """40 nodes, nr = 20: the reduced DOFs would fit, the padded size of the nodes does not - rmx_rollout_lqr's second refusal, by
    its words, from the search and from the sweep alike; the standing tape's rmx_rollout_vjp bits and the state are unchanged."""
    from redmax_amd import BatchSim, _abi
    sc = _fixed_links_chain(40)
    sc.init()
    nr, n = sc.nr, 2
    assert nr == 20
    q0, qd0 = sc.getQ()
    rng = np.random.default_rng(7)
    u = 0.1 * rng.standard_normal((1, n, nr))
    sim = BatchSim(sc, batch=1)
    sim.set_state(q0[None], qd0[None])
    sim.rollout_tape(n, sc.h, u)
    g = rng.standard_normal((1, n, nr))
    vjp, state = sim.rollout_vjp(n, g, g), sim.get_state()
    with pytest.raises(_abi.RedMaxHipError, match=r"rmx_rollout_search: more than 32 nodes \(the model has 40 for nr = 20") as srch:
        sim.rollout_search(n, sc.h, u, R=np.eye(nr))
    with pytest.raises(_abi.RedMaxHipError, match=r"rmx_rollout_lqr: more than 32 nodes \(the model has 40 for nr = 20") as lqr:
        sim.rollout_lqr(n, np.zeros((1, n, 2 * nr)), np.zeros((1, n, nr)), np.tile(np.eye(2 * nr), (n, 1, 1)), np.eye(nr))
    assert str(srch.value).split("rmx_rollout_search: ", 1)[1] == str(lqr.value).split("rmx_rollout_lqr: ", 1)[1]
    assert all(np.array_equal(x, y) for x, y in zip(vjp, sim.rollout_vjp(n, g, g)))
    assert all(np.array_equal(x, y) for x, y in zip(state, sim.get_state()))
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["chart", "point forces", "ground", "big"])
def test_models_outside_the_adjoint_path_are_refused_in_rollout_tapes_words(kind):
    """What rmx_rollout_tape_feedback_box refuses about the model - spherical joints, point forces, ground contact, more than 64
    nodes (the scenes of tests/test_gpu_rollout_feedback.py) - the search refuses in the same words; the state is left alone and the
    batch steps on."""
    from redmax_amd import BatchSim, _abi
    from redmax_amd.scenes import sceneChain, scenesRedMax
    sc = {"chart": lambda: scenesRedMax(7), "point forces": lambda: scenesRedMax(12), "ground": lambda: scenesRedMax(11),
          "big": lambda: sceneChain(100)}[kind]()
    sc.init()
    words = {"chart": "spherical joints", "point forces": "point forces", "ground": "ground contact", "big": "more than 64 nodes"}[kind]
    nsteps, Bs = 2, 2
    u = np.zeros((Bs, nsteps, sc.nr))
    q0, qd0 = sc.getQ()
    sim = BatchSim(sc, batch=Bs)
    sim.set_state(q0[None, :], qd0[None, :])
    state = sim.get_state()
    with pytest.raises(_abi.RedMaxHipError, match=words) as fbk:
        sim.rollout_feedback(nsteps, sc.h, u, K=np.zeros((nsteps, 2 * sc.nr, sc.nr)), ulim=(None, None))
    for kw in (dict(R=np.eye(sc.nr)), dict(R=np.eye(sc.nr), kff=np.zeros_like(u), alphas=(1.0, 0.5), Jbar=np.zeros(Bs), ulim=(None, None))):
        with pytest.raises(_abi.RedMaxHipError, match=words) as srch:
            sim.rollout_search(nsteps, sc.h, u, K=np.zeros((nsteps, 2 * sc.nr, sc.nr)), **kw)
        assert str(srch.value).split(": ", 1)[1] == str(fbk.value).split(": ", 1)[1]        # (behind the name of the entry point)
        assert all(np.array_equal(x, y) for x, y in zip(state, sim.get_state()))
    out = sim.step_bdf1(2, h=sc.h, stats=True)
    sim.close()
    assert (out["status"] & 15 == 0).all()
