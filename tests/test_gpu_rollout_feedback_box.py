"""rmx_rollout_tape_feedback_box: the taped closed-loop rollout with the applied torque clamped into ulo <= u <= uhi on the device,
behind the feedback sum (the ADJ_FB branch of k_adjoint_fwd, redmax_amd/csrc/rmx_kernels.h).

B = 3; the 5-link chain with N = 8 and "fixed" (nodes without a DOF) with N = 6; both integrators.  The checks:
  1. K NULL: uapp == clip(uff, ulo, uhi) bit for bit, and the record and the tape are rmx_rollout_tape's / _bdf2's under that torque;
  2. with gains: w = uff + K'(x - xref) recomputed from the returned rows; wherever w is farther from both bounds than 1e-9 of the
     range, uapp is the bound w exceeds, or w to the rounding of the dot product.  The limits come from an unclamped run (its 1/3 and
     2/3 quantiles per DOF), so that about a third of the entries saturate on either side; every class occurs for every DOF;
  3. replaying uapp through rmx_rollout_tape leaves the same record and the same rmx_rollout_vjp bits;
  4. bounds NULL or infinite: rmx_rollout_tape_feedback's bits; one-sided bounds, per-rollout tables, a permuted batch, the device form;
  5. refusals leave the tape alone.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_adjoint_controls import _DevArray
from test_rollout_feedback_proto import B, scene
from test_rollout_vjp_proto import case

STEPS = {5: 8, "fixed": 6}
EPS = np.finfo(float).eps
_CACHE = {}


def _case(size, integ):
    """test_rollout_feedback_proto.feedback_case's recipe at this file's step counts: (scene, case with K, xref, nsteps)."""
    key = (size, integ)
    if key not in _CACHE:
        sc = scene(size, integ)
        nsteps, nr = STEPS[size], sc.nr
        cs = case(sc, 17, nsteps=nsteps, B=B)
        rng = np.random.default_rng(41)
        kp, kd = 0.25, 0.06
        K = np.zeros((nsteps, 2 * nr, nr))
        for k in range(nsteps):
            K[k, :nr] = -kp * np.eye(nr) + 0.2 * kp * rng.standard_normal((nr, nr)) / np.sqrt(nr)
            K[k, nr:] = -kd * np.eye(nr) + 0.2 * kd * rng.standard_normal((nr, nr)) / np.sqrt(nr)
        q0, qd0 = sc.getQ()
        xref = np.concatenate([q0[None] + 0.05 * rng.standard_normal((nsteps, nr)), qd0[None] + 0.2 * rng.standard_normal((nsteps, nr))], axis=1)
        _CACHE[key] = (sc, dict(cs, K=K, xref=xref), nsteps)
    return _CACHE[key]


def _run(sim, sc, cs, integ, ulim, K="case", xref="case", uff=None, sel=slice(None), **kw):
    sim.set_state(cs["q0"][sel], cs["qd0"][sel])
    K = cs["K"] if isinstance(K, str) else K
    xref = cs["xref"] if isinstance(xref, str) else xref
    uff = cs["u"][sel] if uff is None else uff
    return sim.rollout_feedback(uff.shape[1], sc.h, uff, K=K, xref=xref, pscale=sc.task["pscale"], integrator=integ, ulim=ulim, **kw)


def _limits(u):
    """Per DOF the 1/3 and 2/3 quantiles of a [B][N][nr] table: a third of its entries below, a third above."""
    flat = u.reshape(-1, u.shape[-1])
    return np.quantile(flat, 1 / 3, axis=0), np.quantile(flat, 2 / 3, axis=0)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


CASES = [pytest.param(s, i, id="%s-bdf%d" % (s, i)) for s in (5, "fixed") for i in (1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", CASES)
def test_without_gains_the_torque_is_the_clipped_feed_forward_and_the_tape_is_the_open_loop_tape(size, integ):
    from redmax_amd import BatchSim
    sc, cs, N = _case(size, integ)
    ulo, uhi = _limits(cs["u"])
    clip = np.clip(cs["u"], ulo, uhi)
    assert (clip == ulo).any(axis=(0, 1)).all() and (clip == uhi).any(axis=(0, 1)).all() and (clip == cs["u"]).any(axis=(0, 1)).all()
    rng = np.random.default_rng(3)
    gq, gqd = rng.standard_normal((B, N, sc.nr)), rng.standard_normal((B, N, sc.nr))
    sim = BatchSim(sc, batch=B)
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, info = sim.rollout_tape(N, sc.h, clip, pscale=sc.task["pscale"], stats=True, integrator=integ)
    assert (info["status"] & 15 == 0).all()
    state, vjp = sim.get_state(), sim.rollout_vjp(N, gq, gqd)
    lin = sim.rollout_linearize(N)
    for xref in (None, cs["xref"]):
        q1, qd1, ua, i1 = _run(sim, sc, cs, integ, (ulo, uhi), K=None, xref=xref, stats=True)
        assert "feedback,box" in sim.last_step_kernel()
        assert np.array_equal(ua, clip)
        assert np.array_equal(q1, qt) and np.array_equal(qd1, qdt) and _same(sim.get_state(), state)
        assert np.array_equal(i1["newton_iters"], info["newton_iters"]) and np.array_equal(i1["status"], info["status"])
        assert _same(vjp, sim.rollout_vjp(N, gq, gqd)) and _same(lin, sim.rollout_linearize(N))
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", CASES)
def test_with_gains_the_clamp_follows_the_feedback_sum_and_the_tape_replays(size, integ):
    from redmax_amd import BatchSim
    sc, cs, N = _case(size, integ)
    nr = sc.nr
    sim = BatchSim(sc, batch=B)
    free = _run(sim, sc, cs, integ, None)
    ulo, uhi = _limits(free[2])                              # from the unclamped run: about a third saturates on either side
    rng_ = uhi - ulo
    assert (rng_ > 0).all()
    qt, qdt, ua, info = _run(sim, sc, cs, integ, (ulo, uhi), stats=True)
    assert (info["status"] & 15 == 0).all() and (ua >= ulo).all() and (ua <= uhi).all()
    x = np.concatenate([np.concatenate([cs["q0"], cs["qd0"]], axis=1)[:, None], np.concatenate([qt, qdt], axis=2)[:, :-1]], axis=1)
    dx = x - cs["xref"][None]
    w = cs["u"] + np.einsum("kji,bkj->bki", cs["K"], dx)
    bound = (2 * nr + 2) * EPS * (np.abs(cs["u"]) + np.einsum("kji,bkj->bki", np.abs(cs["K"]), np.abs(dx)))      # the dot product's rounding
    clear = (np.abs(w - ulo) > 1e-9 * rng_) & (np.abs(w - uhi) > 1e-9 * rng_)
    low, high = clear & (w < ulo), clear & (w > uhi)
    inside = clear & ~low & ~high
    print("size %s integ %d: %d low, %d high, %d inside, %d within 1e-9 of a bound; max |uapp - w| / bound inside = %.3f"
          % (size, integ, low.sum(), high.sum(), inside.sum(), (~clear).sum(), (np.abs(ua - w)[inside] / bound[inside]).max()))
    assert (ua[low] == np.broadcast_to(ulo, ua.shape)[low]).all() and (ua[high] == np.broadcast_to(uhi, ua.shape)[high]).all()
    assert (np.abs(ua - w)[inside] <= bound[inside]).all()
    for cls in (low, high, inside):                          # every class occurs for every DOF
        assert cls.any(axis=(0, 1)).all()
    assert not np.array_equal(qt, free[0])
    # the tape is the open-loop tape under uapp
    rng = np.random.default_rng(4)
    gq, gqd = rng.standard_normal((B, N, nr)), rng.standard_normal((B, N, nr))
    closed = sim.rollout_vjp(N, gq, gqd) + sim.rollout_linearize(N)
    sim.set_state(cs["q0"], cs["qd0"])
    qo, qdo, _ = sim.rollout_tape(N, sc.h, ua, pscale=sc.task["pscale"], integrator=integ)
    assert np.array_equal(qo, qt) and np.array_equal(qdo, qdt)
    assert _same(closed, sim.rollout_vjp(N, gq, gqd) + sim.rollout_linearize(N))
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size,integ", CASES)
def test_exact_structure(size, integ):
    from redmax_amd import BatchSim
    sc, cs, N = _case(size, integ)
    nr, ps = sc.nr, sc.task["pscale"]
    inf = np.full(nr, np.inf)
    sim = BatchSim(sc, batch=B)
    free = _run(sim, sc, cs, integ, None, stats=True)
    assert "box" not in sim.last_step_kernel()
    # no finite bound: rmx_rollout_tape_feedback's bits
    for ulim in ((None, None), (-inf, inf), (None, inf), (-inf, None)):
        got = _run(sim, sc, cs, integ, ulim, stats=True)
        assert _same(got[:3], free[:3]) and np.array_equal(got[3]["newton_iters"], free[3]["newton_iters"])
    ulo, uhi = _limits(free[2])
    both = _run(sim, sc, cs, integ, (ulo, uhi))
    # one-sided: a NULL side is an infinite side, and differs from the two-sided run
    for a, b in (((ulo, None), (ulo, inf)), ((None, uhi), (-inf, uhi))):
        one = _run(sim, sc, cs, integ, a)
        assert _same(one, _run(sim, sc, cs, integ, b)) and not np.array_equal(one[2], both[2]) and not np.array_equal(one[2], free[2])
    lo_only = _run(sim, sc, cs, integ, (ulo, None))
    assert (lo_only[2] >= ulo).all() and (lo_only[2] > uhi).any()
    # per-rollout tables: the shared ones repeated give the same bits; own tables, a permuted batch and a batch of one
    rep = _run(sim, sc, cs, integ, (ulo, uhi), K=np.repeat(cs["K"][None], B, axis=0), xref=np.repeat(cs["xref"][None], B, axis=0))
    assert _same(rep, both)
    rng = np.random.default_rng(9)
    Kb = cs["K"][None] * (1.0 + 0.3 * rng.standard_normal((B, 1, 1, 1)))
    xb = cs["xref"][None] + 0.01 * rng.standard_normal((B,) + cs["xref"].shape)
    own = _run(sim, sc, cs, integ, (ulo, uhi), K=Kb, xref=xb)
    assert not np.array_equal(own[0], both[0])
    perm = np.array([2, 0, 1])
    pout = _run(sim, sc, cs, integ, (ulo, uhi), K=Kb[perm], xref=xb[perm], sel=perm)
    assert all(np.array_equal(p, o[perm]) for p, o in zip(pout, own))
    one = BatchSim(sc, batch=1)
    o1 = _run(one, sc, cs, integ, (ulo, uhi), K=Kb[1:2], xref=xb[1:2], sel=slice(1, 2))
    one.close()
    assert all(np.array_equal(a[0], o[1]) for a, o in zip(o1, own))
    # the device form: the host form's bits, the inputs untouched; a NULL side there too
    nan = np.full(both[0].shape, np.nan)
    for K, xref, per, lim, want in ((cs["K"], cs["xref"], False, (ulo, uhi), both), (Kb, xb, True, (ulo, uhi), own),
                                    (cs["K"], cs["xref"], False, (ulo, None), lo_only)):
        d = [_DevArray(a) for a in (cs["u"], K, xref, nan, nan, nan)]
        dl = [None if a is None else _DevArray(a) for a in lim]
        sim.set_state(cs["q0"], cs["qd0"])
        info = sim.rollout_feedback_device(N, sc.h, *(a.ptr.value for a in d), per_rollout=per, pscale=ps, stats=True, integrator=integ,
                                           ulim=tuple(0 if a is None else a.ptr.value for a in dl))
        assert (info["status"] & 15 == 0).all() and "feedback,box" in sim.last_step_kernel()
        assert _same([a.get() for a in d[3:]], want)
        assert np.array_equal(d[0].get(), cs["u"]) and np.array_equal(d[1].get(), K)
        assert all(a is None or np.array_equal(a.get(), l) for a, l in zip(dl, lim))
        for a in d + [a for a in dl if a is not None]:
            a.free()
    sim.close()


@pytest.mark.gpu
def test_refusals_leave_the_tape_alone():
    from redmax_amd import BatchSim, _abi
    sc, cs, N = _case(5, 1)
    nr = sc.nr
    rng = np.random.default_rng(11)
    gq, gqd = rng.standard_normal((B, N, nr)), rng.standard_normal((B, N, nr))
    sim = BatchSim(sc, batch=B)
    free = _run(sim, sc, cs, 1, None)
    vjp0, state = sim.rollout_vjp(N, gq, gqd), sim.get_state()
    ulo, uhi = _limits(free[2])
    L, bt = sim._L, sim._batch
    out = [np.empty((B, N, nr)) for _ in range(3)]
    uff = np.ascontiguousarray(cs["u"])
    opts = sim._tape_opts(sc.h)

    def call(lo=ulo, hi=uhi, box=True, fb=True, batch=bt, integ=1):
        lo, hi = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (lo, hi))
        bx = _abi.Box(None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data)
        f = _abi.Feedback(uff.ctypes.data, None, None, 0)
        rc = L.rmx_rollout_tape_feedback_box(batch, C.byref(opts), N, integ, float(sc.task["pscale"]), C.byref(f) if fb else None,
                                             C.byref(bx) if box else None, _abi.dptr(out[0]), _abi.dptr(out[1]), _abi.dptr(out[2]), None)
        return rc, (L.rmx_last_error() or b"").decode()

    for kw in (dict(box=False), dict(fb=False), dict(batch=None)):
        rc, msg = call(**kw)
        assert rc != 0 and "rmx_rollout_tape_feedback_box: null argument" in msg, (kw, msg)
    swapped_lo = ulo.copy()
    swapped_lo[2] = uhi[2] + 1.0
    nan_hi = uhi.copy()
    nan_hi[1] = np.nan
    nan_lo = ulo.copy()
    nan_lo[nr - 1] = np.nan
    for kw, words in ((dict(lo=swapped_lo), "ulo > uhi at DOF 2"), (dict(hi=nan_hi), "DOF 1 is NaN"), (dict(lo=nan_lo, hi=None), "DOF %d is NaN" % (nr - 1)),
                      (dict(integ=3), "integrator")):
        rc, msg = call(**kw)
        assert rc != 0 and words in msg, (kw, msg)
    with pytest.raises(_abi.RedMaxHipError, match="ulo > uhi at DOF 2"):
        _run(sim, sc, cs, 1, (swapped_lo, uhi))
    d = [_DevArray(a) for a in (cs["u"], swapped_lo, uhi)]
    with pytest.raises(_abi.RedMaxHipError, match="ulo > uhi at DOF 2"):                  # the device form reads the bounds back
        sim.rollout_feedback_device(N, sc.h, d[0].ptr.value, 0, 0, 0, 0, 0, ulim=(d[1].ptr.value, d[2].ptr.value))
    for a in d:
        a.free()
    with pytest.raises(ValueError, match="ulim"):
        _run(sim, sc, cs, 1, (ulo,))
    with pytest.raises(ValueError, match="ulo"):
        _run(sim, sc, cs, 1, (ulo[:-1], uhi))
    # ... and all of it left the tape and the state alone (_run sets the state before the call: put it back)
    sim.set_state(*state)
    assert _same(vjp0, sim.rollout_vjp(N, gq, gqd)) and _same(state, sim.get_state())
    rc, msg = call(lo=ulo, hi=ulo)                                                         # ulo == uhi is a box: every torque pinned
    assert rc == 0 and (out[2] == ulo).all()
    sim.close()
