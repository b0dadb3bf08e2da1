"""rmx_adjoint_track: the adjoint with per-step controls and a tracking objective - point targets on several bodies at several steps,
optionally one target table per rollout - in one forward and one backward sweep.

The reference for everything but the oracle anchor is rmx_adjoint_controls, which its own tests pin to the oracle: the forward sweep
does not see the task and the backward sweep is linear in its sources, so a K-term objective is the sum of K single-term calls.
Sections, in the order of the checks below:
  1. one term is rmx_adjoint_controls;
  2. many terms equal the sum of single-term calls (and the regulariser enters as wreg * u);
  3. the oracle anchor: constant controls, the sum over the steps against the sum of the oracle's single-term gradients;
  4. the reference's testGrad identity with the whole term set;
  5. structure: rows behind the last measured step, the order of the terms;
  6. one target table per rollout;
  7. plumbing: helper wave, device pointers, forward only, refusals, the MEX command.

The base term set of a scene with nb bodies over a horizon of K steps, as (body, step): (nb-1, K), (nb-1, K//2), (nb//2, K//2), (0, 1),
(nb//2, K) and a second term on (nb-1, K) with another target: two bodies on one step, one body on two steps, a step-1 term and a
same-body same-step pair.  xlocal = [5, 0.5, 0.25] (a point on the root's own axis has no gradient); the targets are the scene's
target plus a seeded N(0,1) offset per term, the weights the scene's wpos times {1, 0.5, 2, 1.5, 0.75, 1.25}.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_adjoint_controls import STEPS, _DevArray, _fd_errors, _rel, _run, _scene
from test_mex_gateway import Gateway, MexError, flatten, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)

B = 3
XLOCAL = [5.0, 0.5, 0.25]
WEIGHTS = (1.0, 0.5, 2.0, 1.5, 0.75, 1.25)
SIZES = [5, 11, 16, "16-one-wave", 32, 40, "tree7"]


def _size(size, monkeypatch):
    if size == "16-one-wave":          # the full 16-link chain without its helper wave: FullChain16
        monkeypatch.setenv("RMX_ADJ_HELP", "0")
        return 16
    return size


def _controls(sc, nsteps, seed=17):
    return 0.1 * np.random.default_rng(seed).standard_normal((B, nsteps, sc.nr))


def _base_terms(sc, K, seed=23):
    """The base term set over a horizon of K steps: (terms, xtarget[6][3])."""
    nb = int(sc.desc()["njoints"])
    where = [(nb - 1, K), (nb - 1, K // 2), (nb // 2, K // 2), (0, 1), (nb // 2, K), (nb - 1, K)]
    terms = [dict(body=b, xlocal=XLOCAL, step=s, wpos=sc.task["wpos"] * w) for (b, s), w in zip(where, WEIGHTS)]
    xt = np.asarray(sc.task["xtarget"], dtype=np.float64)[None, :] + np.random.default_rng(seed).standard_normal((len(where), 3))
    return terms, xt


def _track(sc, terms, xt, wreg=None):
    return dict(terms=terms, xtarget=xt, pscale=sc.task["pscale"], wreg=sc.task["wreg"] if wreg is None else wreg)


def _single(sc, term, xt, wreg=0.0):
    """The rmx_task_pointpos of one term."""
    return dict(body=term["body"], xlocal=term["xlocal"], xtarget=xt, step=term["step"], pscale=sc.task["pscale"], wreg=wreg, wpos=term["wpos"])


def _same_rollout(a, b):
    """State and counters of two results of _run(..., stats=True), bit for bit."""
    return (np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(a[2]["newton_iters"], b[2]["newton_iters"])
            and np.array_equal(a[2]["status"], b[2]["status"]))


# ---------------------------------------------------------------- 1. one term is the existing call

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_one_term_is_the_controls_call(size, integ, monkeypatch):
    from redmax_amd import BatchSim
    size = _size(size, monkeypatch)
    sc = _scene(size, integ)
    nsteps = STEPS[size]
    u = _controls(sc, nsteps)
    task = dict(sc.task, step=nsteps)
    term = dict(body=task["body"], xlocal=task["xlocal"], step=nsteps, wpos=task["wpos"])
    sim = BatchSim(sc, batch=B)
    ref = _run(sim, sc, sim.adjoint_controls, nsteps, sc.h, task, u, integrator=integ, stats=True)
    got = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, _track(sc, [term], np.asarray(task["xtarget"], dtype=np.float64)[None, :]), u,
               integrator=integ, stats=True)
    sim.close()
    assert (ref[2]["status"] == 0).all() and (got[2]["status"] == 0).all()
    assert _same_rollout(got, ref)
    assert np.array_equal(got[0], ref[0])                         # P: the same expression
    for b in range(B):
        print("size %s integ %d b %d: |dPdu_track - dPdu_controls| / |dPdu_controls| = %.3e" % (size, integ, b, _rel(got[1][b], ref[1][b])))
        assert np.linalg.norm(ref[1][b]) > 0
        assert _rel(got[1][b], ref[1][b]) <= 1e-12, (size, integ, b)


# ---------------------------------------------------------------- 2. many terms = the sum of single-term calls

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_many_terms_equal_the_sum_of_single_term_calls(size, integ, monkeypatch):
    """||dPdu_track - sum_i dPdu_i|| <= 1e-7 sum_i ||dPdu_i|| per rollout: the project's bound for one gradient evaluated by two
    arithmetics (the smallest term is between 0.1 % - tree7 under BDF2 - and 4.6 % of the total: a dropped or mis-stepped term misses
    it by four orders).

    Measured on an MI355X (||dPdu_track - sum_i dPdu_i|| / sum_i ||dPdu_i||, printed per rollout), the largest of the 42 rollouts:
    3.5e-14 (40-link chain, BDF1); per size the maxima are 7.4e-15 / 1.6e-14 (5, BDF1 / BDF2), 1.4e-14 / 2.4e-14 (11), 2.8e-14 /
    2.7e-14 (16, with and without the helper wave), 2.9e-14 / 3.1e-14 (32), 3.5e-14 / 3.2e-14 (40), 1.8e-15 / 3.7e-15 (tree7)."""
    from redmax_amd import BatchSim
    size = _size(size, monkeypatch)
    sc = _scene(size, integ)
    nsteps = STEPS[size]
    u = _controls(sc, nsteps)
    terms, xt = _base_terms(sc, nsteps)
    sim = BatchSim(sc, batch=B)
    singles = [_run(sim, sc, sim.adjoint_controls, nsteps, sc.h, _single(sc, t, xt[i]), u, integrator=integ, stats=True)
               for i, t in enumerate(terms)]
    got0 = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, _track(sc, terms, xt, wreg=0.0), u, integrator=integ, stats=True)
    got = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, _track(sc, terms, xt), u, integrator=integ, stats=True)
    sim.close()
    assert (got0[2]["status"] == 0).all() and all((s[2]["status"] == 0).all() for s in singles)
    for s in singles:
        assert _same_rollout(got0, s)
    assert _same_rollout(got, got0)
    Psum = sum(s[0] for s in singles)
    dsum = sum(s[1] for s in singles)
    wreg = sc.task["wreg"]
    for b in range(B):
        scale = sum(np.linalg.norm(s[1][b]) for s in singles)
        smallest = min(np.linalg.norm(s[1][b]) for s in singles)
        err = np.linalg.norm(got0[1][b] - dsum[b])
        print("size %s integ %d b %d: |dPdu_track - sum dPdu_i| / sum |dPdu_i| = %.3e (smallest term %.3e of the total)"
              % (size, integ, b, err / scale, smallest / scale))
        assert scale > 0 and err <= 1e-7 * scale, (size, integ, b, err / scale)
        assert abs(got0[0][b] - Psum[b]) <= 1e-12 * abs(Psum[b]), (size, integ, b, got0[0][b], Psum[b])
        # the regulariser: dPdu moves by wreg * u and P by wreg/2 |u|^2
        assert np.linalg.norm(got[1][b] - (got0[1][b] + wreg * u[b])) <= 1e-12 * np.linalg.norm(got[1][b])
        Preg = got0[0][b] + 0.5 * wreg * float((u[b] ** 2).sum())
        assert abs(got[0][b] - Preg) <= 1e-12 * abs(Preg)


# ---------------------------------------------------------------- 3. the oracle anchor

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, "tree7", 16])
def test_constant_controls_meet_the_sum_of_the_oracles_gradients(oracle_lib, size, integ):
    from redmax_amd import BatchSim
    sc = _scene(size, integ)
    nsteps = STEPS[size]
    p = 0.1 * np.random.default_rng(31).standard_normal((B, sc.nr))
    u = np.repeat(p[:, None, :], nsteps, axis=1)
    terms, xt = _base_terms(sc, nsteps)
    sim = BatchSim(sc, batch=B)
    P, dPdu, info, _, _ = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, _track(sc, terms, xt, wreg=0.0), u, integrator=integ, stats=True)
    sim.close()
    assert (info["status"] == 0).all()
    for b in range(B):
        Po, dPo, scale = 0.0, 0.0, 0.0
        for i, t in enumerate(terms):
            o = oracle_lib.Oracle(sc.desc())
            task = dict(_single(sc, t, xt[i]), t=t["step"] * sc.h)
            Pi, dPi, st = (o.adjoint_bdf1 if integ == 1 else o.adjoint_bdf2)(sc.h, nsteps, task, p[b])
            assert st.not_converged == 0 and st.diverged == 0
            Po, dPo, scale = Po + Pi, dPo + np.asarray(dPi), scale + np.linalg.norm(dPi)
            assert info["newton_iters"][b] == st.newton_iters
        err = np.linalg.norm(dPdu[b].sum(axis=0) - dPo)
        print("size %s integ %d b %d: |sum_k dPdu - sum_i dPo_i| / sum_i |dPo_i| = %.3e, |P - Po| / Po = %.3e"
              % (size, integ, b, err / scale, abs(P[b] - Po) / abs(Po)))
        assert err <= 1e-7 * scale, (size, integ, b, err / scale)
        assert abs(P[b] - Po) <= 1e-9 * abs(Po), (size, integ, b, P[b], Po)


# ---------------------------------------------------------------- 4. the gradient by the reference's testGrad identity

def _fd_errors_track(sc, nsteps, integ):
    """_fd_errors of tests/test_gpu_adjoint_controls.py for the tracking call with the base term set: central differences of P along 3
    random directions of the [nsteps][nr] space (eps = 1e-5; zero in the k = 1 rows under BDF2) against direction . gradient."""
    from redmax_amd import BatchSim
    nd, eps = 3, 1e-5
    rng = np.random.default_rng(53)
    terms, xt = _base_terms(sc, nsteps)
    task = _track(sc, terms, xt)
    base = 0.1 * rng.standard_normal((nsteps, sc.nr))
    d = rng.standard_normal((nd,) + base.shape)
    if integ == 2:
        d[:, 0, :] = 0.0
    one, fd = BatchSim(sc, batch=1), BatchSim(sc, batch=2 * nd)
    pp = np.repeat(base[None], 2 * nd, axis=0)
    pp[0::2] += eps * d
    pp[1::2] -= eps * d
    _, grad, info, _, _ = _run(one, sc, one.adjoint_track, nsteps, sc.h, task, base[None], integrator=integ, stats=True)
    Pf, none, _, _, _ = _run(fd, sc, fd.adjoint_track, nsteps, sc.h, task, pp, integrator=integ, gradient=False)
    one.close()
    fd.close()
    assert none is None and (info["status"] == 0).all()
    num = (Pf[0::2] - Pf[1::2]) / (2 * eps)
    ana = (d.reshape(nd, -1) * grad.reshape(1, -1)).sum(axis=1)
    return num, ana


@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("n,nsteps,kt", [(5, 10, 5), (16, 6, 3)])
def test_gradient_meets_the_testgrad_identity(n, nsteps, kt, integ):
    """Tolerance as test_gpu_adjoint_controls.py::test_gradient_meets_the_testgrad_identity: the floor rtol 2e-5, atol 1e-6 max|ana|;
    under BDF1 twice the error the single-term rmx_adjoint_controls shows in the same identity in the same run (same scene, horizon,
    eps; its task at step kt), if that is larger.  The measured errors, max over the 3 directions of |num - ana| / max|ana|, are
    printed.  Measured on an MI355X (single-term controls call / tracking call): n = 5 BDF1 5.0e-10 / 6.9e-10, BDF2 7.5e-9 / 6.9e-9;
    n = 16 BDF1 1.8e-9 / 3.3e-9, BDF2 1.6e-9 / 2.1e-8 - the floor of 1e-6 decides in all four."""
    sc = _scene(n, integ)
    num_c, ana_c = _fd_errors(sc, nsteps, kt, integ, controls=True)
    err_c = np.abs(num_c - ana_c)
    num, ana = _fd_errors_track(sc, nsteps, integ)
    err = np.abs(num - ana)
    print("testgrad n %d integ %d: single-term controls call %.3e, tracking call %.3e (of max|ana|)"
          % (n, integ, err_c.max() / np.abs(ana_c).max(), err.max() / np.abs(ana).max()))
    assert np.abs(ana).max() > 0
    measured = float(err_c.max() / np.abs(ana_c).max())
    floor = 2e-5 * np.abs(ana) + 1e-6 * np.abs(ana).max()
    tol = np.maximum(2.0 * measured * np.abs(ana).max(), floor) if integ == 1 else floor
    assert (err <= tol).all(), (num, ana, err, tol)


# ---------------------------------------------------------------- 5. exact structure

@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
@pytest.mark.parametrize("size", [5, 16, 40])
def test_rows_behind_the_last_term_and_the_order_of_the_terms(size, integ):
    from redmax_amd import BatchSim
    sc = _scene(size, integ)
    nsteps = STEPS[size]
    last = nsteps - 2                                              # the base term set over a shorter horizon: two rows lie behind it
    u = _controls(sc, nsteps)
    terms, xt = _base_terms(sc, last)
    sim = BatchSim(sc, batch=B)
    got = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, _track(sc, terms, xt), u, integrator=integ, stats=True)
    got0 = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, _track(sc, terms, xt, wreg=0.0), u, integrator=integ, stats=True)
    # a permutation that keeps the relative order of the terms of one step (stable sort by descending step), targets with the terms
    perm = sorted(range(len(terms)), key=lambda i: -terms[i]["step"])
    assert perm != list(range(len(terms)))
    gotp = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, _track(sc, [terms[i] for i in perm], xt[perm]), u, integrator=integ, stats=True)
    sim.close()
    assert (got[2]["status"] == 0).all()
    assert np.array_equal(got[1][:, last:, :], sc.task["wreg"] * u[:, last:, :])
    assert not got0[1][:, last:, :].any()
    assert np.abs(got0[1][:, :last, :]).max(axis=2).min() > 0
    assert np.array_equal(gotp[0], got[0]) and np.array_equal(gotp[1], got[1]) and _same_rollout(gotp, got)


# ---------------------------------------------------------------- 6. one target table per rollout

@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", [(5, 1), (16, 2), (40, 1), ("tree7", 2)])
def test_per_rollout_targets_are_the_shared_call_row_by_row(size, integ):
    from redmax_amd import BatchSim
    sc = _scene(size, integ)
    nsteps = STEPS[size]
    u = _controls(sc, nsteps)
    terms, xt0 = _base_terms(sc, nsteps)
    xt = xt0[None] + np.random.default_rng(67).standard_normal((B,) + xt0.shape)
    sim = BatchSim(sc, batch=B)
    per = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, _track(sc, terms, xt), u, integrator=integ, stats=True)
    assert (per[2]["status"] == 0).all() and len(set(per[0].tolist())) == B
    for b in range(B):
        sh = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, _track(sc, terms, xt[b]), u, integrator=integ, stats=True)
        assert sh[0][b] == per[0][b] and np.array_equal(sh[1][b], per[1][b]) and np.abs(sh[1][b]).sum() > 0
        assert _same_rollout(sh, per)
    sim.close()


# ---------------------------------------------------------------- 7. plumbing

@pytest.mark.gpu
@pytest.mark.parametrize("n,integ", [(16, 1), (16, 2), (11, 1)])
def test_helper_wave_on_and_off_agree(n, integ, monkeypatch):
    from redmax_amd import BatchSim
    sc = _scene(n, integ)
    nsteps = STEPS[n]
    u = _controls(sc, nsteps)
    terms, xt = _base_terms(sc, nsteps)
    res = []
    for helper in ("0", "1"):
        monkeypatch.setenv("RMX_ADJ_HELP", helper)
        sim = BatchSim(sc, batch=B)
        P, dPdu, info, q, qd = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, _track(sc, terms, xt), u, integrator=integ, stats=True)
        res.append((P, dPdu, info["newton_iters"], info["status"], q, qd))
        sim.close()
    assert np.isfinite(res[0][0]).all() and np.abs(res[0][1]).sum() > 0
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("integ", [1, 2])
def test_device_form_and_forward_only(integ):
    """The _device form equals the host form bit for bit, with a shared and with a per-rollout target table, and leaves d_u and
    d_xtarget untouched; gradient=False (host) and a null d_dPdu (device) give the same P, state and counters."""
    from redmax_amd import BatchSim
    sc = _scene(16, integ)
    nsteps = 6
    u = _controls(sc, nsteps)
    terms, xt0 = _base_terms(sc, nsteps)
    q0, qd0 = sc.getQ()
    sim = BatchSim(sc, batch=B)
    for xt in (xt0, xt0[None] + np.random.default_rng(83).standard_normal((B,) + xt0.shape)):
        task = _track(sc, terms, xt)
        P, dPdu, info, q, qd = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, task, u, integrator=integ, stats=True)
        fwd = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, task, u, integrator=integ, stats=True, gradient=False)
        assert fwd[1] is None and np.array_equal(fwd[0], P) and _same_rollout(fwd, (P, dPdu, info, q, qd))
        dtask = dict(task, xtarget=None, per_rollout=xt.ndim == 3)
        u_d, x_d = _DevArray(u), _DevArray(xt)
        for with_grad in (True, False):
            P_d, dP_d = _DevArray(np.full(B, np.nan)), _DevArray(np.full(u.shape, np.nan))      # both passes start from NaN
            sim.set_state(q0[None, :], qd0[None, :])
            info_d = sim.adjoint_track_device(nsteps, sc.h, dtask, x_d.ptr.value, u_d.ptr.value, P_d.ptr.value,
                                              dP_d.ptr.value if with_grad else None, integrator=integ, stats=True)
            qb, qdb = sim.get_state()
            assert np.array_equal(P_d.get(), P)
            if with_grad:
                assert np.array_equal(dP_d.get(), dPdu)
            else:
                assert np.isnan(dP_d.get()).all()                     # a null d_dPdu: the gradient array is left alone
            assert np.array_equal(qb, q) and np.array_equal(qdb, qd)
            assert np.array_equal(info_d["newton_iters"], info["newton_iters"]) and np.array_equal(info_d["status"], info["status"])
            assert np.array_equal(u_d.get(), u) and np.array_equal(x_d.get(), xt)
            P_d.free()
            dP_d.free()
        u_d.free()
        x_d.free()
    sim.close()


@pytest.mark.gpu
def test_bad_arguments_raise_cleanly():
    from redmax_amd import BatchSim, _abi
    from redmax_amd.scenes import scenesRedMax
    sc = _scene(5, 1)
    Bt, nsteps = 2, 4
    terms, xt = _base_terms(sc, nsteps)
    task = _track(sc, terms, xt)
    u = np.zeros((Bt, nsteps, sc.nr))
    sim = BatchSim(sc, batch=Bt)
    for bad in (np.zeros((Bt, nsteps + 1, sc.nr)), np.zeros((Bt, sc.nr)), np.zeros((Bt + 1, nsteps, sc.nr)), np.zeros((nsteps, sc.nr + 1))):
        with pytest.raises(ValueError, match="shape"):
            sim.adjoint_track(nsteps, sc.h, task, bad)
    for bad in (xt[:-1], xt[None], np.zeros((Bt + 1,) + xt.shape), xt[:, :2], None):
        with pytest.raises(ValueError, match="xtarget"):
            sim.adjoint_track(nsteps, sc.h, dict(task, xtarget=bad), u)
    with pytest.raises(ValueError):
        sim.adjoint_track(nsteps, sc.h, task, None)
    with pytest.raises(_abi.RedMaxHipError, match="null xtarget"):
        sim.adjoint_track_device(nsteps, sc.h, task, None, None, None, None)
    with pytest.raises(_abi.RedMaxHipError, match="null"):
        sim.adjoint_track_device(nsteps, sc.h, task, 1 << 20, None, None, None)          # (refused before any pointer is read)
    with pytest.raises(_abi.RedMaxHipError, match="nterms < 1"):
        sim.adjoint_track(nsteps, sc.h, dict(task, terms=[], xtarget=np.zeros((0, 3))), u)
    with pytest.raises(_abi.RedMaxHipError, match="integrator"):
        sim.adjoint_track(nsteps, sc.h, task, u, integrator=3)
    nb = int(sc.desc()["njoints"])
    for body in (-1, nb):
        with pytest.raises(_abi.RedMaxHipError, match=r"term 2: body"):
            sim.adjoint_track(nsteps, sc.h, dict(task, terms=terms[:2] + [dict(terms[2], body=body)] + terms[3:]), u)
    for step in (0, nsteps + 1):
        with pytest.raises(_abi.RedMaxHipError, match=r"term 1: step"):
            sim.adjoint_track(nsteps, sc.h, dict(task, terms=terms[:1] + [dict(terms[1], step=step)] + terms[2:]), u)
    # the C entry itself: a null task, null terms, a null target table
    tk, opts, keep = sim._track_task(task, sc.h, nsteps)
    P = np.empty(Bt)
    L = _abi.lib()
    assert L.rmx_adjoint_track(sim._batch, C.byref(opts), nsteps, 1, None, _abi.dptr(u), _abi.dptr(P), None, None) == -1
    assert b"null task" in L.rmx_last_error()
    tk.xtarget = None
    assert L.rmx_adjoint_track(sim._batch, C.byref(opts), nsteps, 1, C.byref(tk), _abi.dptr(u), _abi.dptr(P), None, None) == -1
    assert b"null xtarget" in L.rmx_last_error()
    tk.xtarget, tk.terms = _abi.dptr(keep[1]), None
    assert L.rmx_adjoint_track(sim._batch, C.byref(opts), nsteps, 1, C.byref(tk), _abi.dptr(u), _abi.dptr(P), None, None) == -1
    assert b"null terms" in L.rmx_last_error()
    P, dPdu, _ = sim.adjoint_track(nsteps, sc.h, task, u)          # ... and the batch is still usable
    assert np.isfinite(P).all() and np.isfinite(dPdu).all() and np.abs(dPdu).sum() > 0
    sim.close()
    ground = scenesRedMax(11)
    ground.init()
    gsim = BatchSim(ground, batch=1)
    with pytest.raises(_abi.RedMaxHipError, match="ground contact"):
        gsim.adjoint_track(2, ground.h, _track(sc, [dict(body=0, xlocal=XLOCAL, step=2, wpos=1.0)], np.zeros((1, 3))),
                           np.zeros((1, 2, ground.nr)))
    gsim.close()


def _refused_scene(kind):
    from redmax_amd.scenes import sceneChain, scenesRedMax
    sc = {"chart": lambda: scenesRedMax(7), "big": lambda: sceneChain(100), "point forces": lambda: scenesRedMax(12)}[kind]()
    sc.init()
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("kind,message", [("chart", "spherical joints"), ("big", "more than 64 nodes"), ("point forces", "point forces")])
def test_models_outside_the_adjoint_path_are_refused(kind, message):
    """What rmx_adjoint_controls refuses, rmx_adjoint_track refuses with the same words, in the host and in the device form, before the
    term table is looked at (the one term is valid) - Euler-chart joints (scene 7), a tree of more than 64 nodes (a 100-link chain),
    point forces (scene 12) - and the batch still steps afterwards exactly as a batch that was never asked."""
    from redmax_amd import BatchSim, _abi
    sc = _refused_scene(kind)
    nsteps = 2
    task = dict(terms=[dict(body=0, xlocal=XLOCAL, step=nsteps, wpos=1.0)], xtarget=np.zeros((1, 3)), pscale=1.0, wreg=0.0)
    u = np.zeros((B, nsteps, sc.nr))
    q0, qd0 = sc.getQ()
    fresh, sim = BatchSim(sc, batch=B), BatchSim(sc, batch=B)
    for s in (fresh, sim):
        s.set_state(q0[None, :], qd0[None, :])
    with pytest.raises(_abi.RedMaxHipError, match=message):
        sim.adjoint_track(nsteps, sc.h, task, u)
    with pytest.raises(_abi.RedMaxHipError, match=message):
        sim.adjoint_track(nsteps, sc.h, task, u, integrator=2, gradient=False)
    u_d, x_d, P_d = _DevArray(u), _DevArray(np.zeros((1, 3))), _DevArray(np.full(B, np.nan))
    with pytest.raises(_abi.RedMaxHipError, match=message):
        sim.adjoint_track_device(nsteps, sc.h, dict(task, xtarget=None, per_rollout=False), x_d.ptr.value, u_d.ptr.value, P_d.ptr.value, None)
    assert np.isnan(P_d.get()).all()                               # nothing ran
    for d in (u_d, x_d, P_d):
        d.free()
    qa, qda = sim.get_state()
    assert np.array_equal(qa, np.repeat(q0[None, :], B, axis=0)) and np.array_equal(qda, np.repeat(qd0[None, :], B, axis=0))
    out, ref = sim.step_bdf1(3, h=sc.h, stats=True), fresh.step_bdf1(3, h=sc.h, stats=True)
    qa, qda = sim.get_state()
    qb, qdb = fresh.get_state()
    sim.close()
    fresh.close()
    assert (out["status"] & 15 == 0).all() and np.isfinite(qa).all()
    assert np.array_equal(qa, qb) and np.array_equal(qda, qdb) and np.array_equal(out["newton_iters"], ref["newton_iters"])


class _TrackGateway(Gateway):
    """The gateway of tests/test_mex_gateway.py with MATLAB struct arrays: a list of dicts is a 1 x N struct array."""

    def to_mx(self, v):
        if isinstance(v, list) and v and isinstance(v[0], dict):
            L = self.L
            names = (C.c_char_p * len(v[0]))(*[k.encode() for k in v[0]])
            s = L.mxCreateStructMatrix(1, len(v), len(v[0]), names)
            for i, d in enumerate(v):
                for k, x in d.items():
                    L.mxSetField(s, i, k.encode(), self.to_mx(x))
            return s
        return super().to_mx(v)


@pytest.mark.gpu
def test_mex_command_equals_the_ctypes_call(gw):  # noqa: F811
    """'adjoint_track' through the gateway (stub) on two shards, with a shared and with a per-rollout target table: MATLAB's
    nr x nsteps x B and 3 x nterms x B column-major arrays are the ABI's [B][nsteps][nr] and [B][nterms][3]."""
    from redmax_amd import BatchSim
    g = _TrackGateway(gw.L)
    sc = _scene(5, 1)
    nsteps = 6
    u = _controls(sc, nsteps)
    terms, xt0 = _base_terms(sc, nsteps)
    q0, qd0 = sc.getQ()
    mterms = [{"body": float(t["body"] + 1), "xlocal": np.array(t["xlocal"]), "step": float(t["step"]), "wpos": t["wpos"]} for t in terms]
    um = u.transpose(2, 1, 0)                                  # nr x nsteps x B
    for integ, xt in ((1, xt0), (2, xt0[None] + np.random.default_rng(97).standard_normal((B,) + xt0.shape))):
        task = _track(sc, terms, xt)
        sim = BatchSim(sc, batch=B)
        P, dPdu, info, q, qd = _run(sim, sc, sim.adjoint_track, nsteps, sc.h, task, u, integrator=integ, stats=True)
        sim.close()
        mtask = {"terms": mterms, "xtarget": xt.T if xt.ndim == 2 else xt.transpose(2, 1, 0), "pscale": task["pscale"], "wreg": task["wreg"]}
        h = g.call(1, "create", flatten(sc), float(B), np.array([0.0, 0.0]))          # two shards: the arrays advance per shard
        g.call(0, "set", h, np.repeat(q0[:, None], B, axis=1), np.repeat(qd0[:, None], B, axis=1))
        Pm, dPm, st = g.call(3, "adjoint_track", h, sc.h, float(nsteps), mtask, um, float(integ))
        qm, qdm = g.call(2, "get", h)
        assert dPm.shape == (sc.nr, nsteps, B) and np.array_equal(dPm.transpose(2, 1, 0), dPdu)
        assert np.array_equal(Pm[0], P) and np.array_equal(qm.T, q) and np.array_equal(qdm.T, qd)
        assert np.array_equal(st[:, 0], info["newton_iters"]) and np.array_equal(st[:, 1], info["status"])
        g.call(0, "set", h, np.repeat(q0[:, None], B, axis=1), np.repeat(qd0[:, None], B, axis=1))
        Pf = g.call(1, "adjoint_track", h, sc.h, float(nsteps), mtask, um, float(integ))      # one output: forward only
        assert np.array_equal(Pf[0], P)
        with pytest.raises(MexError, match="nr x nsteps x batch"):
            g.call(1, "adjoint_track", h, sc.h, float(nsteps), mtask, um[:, :-1, :])
        with pytest.raises(MexError, match="xtarget"):
            g.call(1, "adjoint_track", h, sc.h, float(nsteps), dict(mtask, xtarget=xt0.T[:, :-1]), um)
        with pytest.raises(MexError, match="integrator"):
            g.call(1, "adjoint_track", h, sc.h, float(nsteps), mtask, um, 3.0)
        g.call(0, "destroy", h)
