"""rmx_rollout_points / rmx_rollout_cost: point kinematics along a state record and the cost model of the device iLQR
(redmax_amd/csrc/rmx_cost.h, the point instantiation), on the GPU.

The checks, in the order of the sections below:
  1. against tests/proto_point_cost.py at every padded size: with ext the longdouble proto and ref the float64 proto on IDENTICAL
     inputs, per quantity (x, Jk, lx, Qout, gq) e = max |. - ext| / max |ext| over the batch and e_gpu <= 8 max(e_ref, 16 eps) - the
     rule of test_gpu_rollout_lqr._judge: two correct float64 evaluations of one formula in different summation orders differ by
     small constant factors; three bits allow that and do not allow a lost term.  The targets are placed so that |r_t| >= 0.1 |p_t|
     for every term (asserted on the proto): the comparison is not a test of cancellation;
  2. exact structure, bit for bit; 3. against the library itself (rmx_rollout_tape, rmx_adjoint_track); 4. the testGrad identity
     on the GPU's own value; 5. refusals, and the models that are taken.

Scenes: sceneAdjointChain(2), (3) (NP 4), "fixed" of test_rollout_feedback_proto (nodes without a DOF), (5), sceneAdjointTree7
(NP 8), (11), (16) (NP 16), (32) (NP 32) and sceneTree(64) (NP 64, revolute and prismatic joints on a branching tree).  B = 3,
N = 4; states: test_rollout_vjp_proto.case's q0, qd0 plus noise per step; terms: test_point_cost_proto.terms_of (two on step 1, two
sharing body and step 3, one on the root body at step 4, one on an inner body, off-axis local points; step 2 owns none); Q dense
symmetric, another at every step; every table shared by the batch ("shared") or one per rollout ("per").

Measured on an MI355X (test_outputs_meet_the_extended_proto, pytest -s; e_ref e_gpu per quantity over the batch; every e_ref but
three is below the floor of 16 eps = 3.55e-15, where the bound is 2.84e-14; the largest e_gpu / bound is 0.18; the whole table with
the rows of the shared tables is profiles/point_cost.txt):
    scene   tables   x                   Jk                  lx                  Q                   gq
    2       per      1.77e-16 1.79e-16   2.93e-16 4.89e-16   2.46e-16 3.35e-16   1.83e-16 2.76e-16   1.44e-16 1.44e-16
    3       per      1.71e-16 1.50e-16   5.09e-16 4.29e-16   3.56e-16 4.83e-16   2.49e-16 3.83e-16   2.25e-16 3.11e-16
    fixed   per      1.99e-16 2.80e-16   6.78e-16 5.15e-16   8.56e-16 6.47e-16   3.69e-16 3.66e-16   2.06e-16 9.86e-17
    5       per      2.22e-16 2.59e-16   7.11e-16 1.13e-15   9.92e-16 7.36e-16   5.03e-16 4.73e-16   1.73e-16 1.16e-16
    tree7   per      1.73e-16 1.51e-16   3.25e-16 1.70e-16   2.31e-16 2.31e-16   4.22e-16 4.22e-16   1.92e-16 1.78e-16
    11      per      3.35e-16 3.06e-16   5.22e-16 1.33e-15   2.16e-15 1.68e-15   6.73e-16 6.59e-16   5.13e-16 3.09e-16
    16      per      1.79e-15 7.19e-16   1.28e-15 8.68e-16   5.12e-15 1.91e-15   9.41e-16 6.85e-16   2.97e-16 4.04e-16
    32      shared   1.38e-15 2.20e-15   4.80e-16 1.26e-15   7.30e-16 9.71e-16   7.57e-16 1.40e-15   4.79e-16 7.75e-16
    32      per      1.38e-15 2.20e-15   3.88e-15 4.39e-15   3.25e-15 4.98e-15   8.61e-16 1.36e-15   4.79e-16 7.75e-16
    tree64  shared   1.68e-16 2.44e-16   1.13e-16 1.84e-16   2.38e-16 3.87e-16   4.77e-16 6.75e-16   2.03e-16 4.49e-16
    tree64  per      1.68e-16 2.44e-16   4.36e-16 6.22e-16   4.96e-16 3.18e-16   4.32e-16 6.75e-16   2.03e-16 4.49e-16
The value at the final states of the 6-step rollout (section 3): e_ref 2.32e-16, rmx_rollout_cost 1.39e-16, rmx_adjoint_track
1.16e-16.  The testGrad identity (section 4): 2.9e-10 (5-chain) and 6.0e-11 (7-joint tree) of max|ana|.
"""
import numpy as np
import pytest

import proto_point_cost as P
import proto_worldframe as pw
from test_gpu_adjoint_controls import _DevArray
from test_point_cost_proto import terms_of
from test_rollout_feedback_proto import scene as _scene_or_fixed
from test_rollout_vjp_proto import case

B, N = 3, 4
EPS = np.finfo(np.float64).eps
SIZES = [2, 3, "fixed", 5, "tree7", 11, 16, 32, "tree64"]
QUANTITIES = ("x", "Jk", "lx", "Q", "gq")
_CACHE = {}


def _scene(size):
    if size == "tree64":
        from redmax_amd.scenes import sceneTree
        sc = sceneTree(64)
        sc.init()
        return sc
    return _scene_or_fixed(size, 1)


def _case(size):
    """Scene, proto model, terms and the inputs of a size, shared and per rollout: computed once, left unchanged."""
    if size not in _CACHE:
        sc = _scene(size)
        m = pw.build_model(sc.desc())
        nr = sc.nr
        cs = case(sc, 61, nsteps=N, B=B)
        rng = np.random.default_rng(67)
        q = cs["q0"][:, None] + 0.05 * rng.standard_normal((B, N, nr))
        qd = cs["qd0"][:, None] + 0.2 * rng.standard_normal((B, N, nr))
        terms = terms_of(m, N)
        T = len(terms)
        Qp = rng.standard_normal((B, N, 2 * nr, 2 * nr))
        Qp = Qp + Qp.transpose(0, 1, 3, 2)
        xgp = np.concatenate([q, qd], axis=-1) + 0.3 * rng.standard_normal((B, N, 2 * nr))
        xp = np.array([P.points(m, q[b], terms) for b in range(B)])
        dirs = rng.standard_normal((B, T, 3))
        dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
        xtp = xp + dirs * (0.3 * np.linalg.norm(xp, axis=-1, keepdims=True) + 0.3)
        # a shared target: off the rollouts' points by their spread about the mean and 0.3 (|p| + 1) of the farthest of them
        spread = np.linalg.norm(xp - xp.mean(0), axis=-1).max(0)[:, None]
        xts = xp.mean(0) + dirs[0] * (spread + 0.3 * np.linalg.norm(xp, axis=-1).max(0)[:, None] + 0.3)
        gx = rng.standard_normal((B, T, 3))
        _CACHE[size] = dict(sc=sc, m=m, terms=terms, q=q, qd=qd, gx=gx, per=dict(Q=Qp, xgoal=xgp, xtarget=xtp),
                            shared=dict(Q=Qp[0].copy(), xgoal=xgp[0].copy(), xtarget=xts))
    return _CACHE[size]


def _row(a, b, per):
    return a[b] if per else a


def _proto(c, tab, per, dtype):
    """dict(x, Jk, lx, Q, gq, r) over the batch from the proto in dtype."""
    outs = [P.cost(c["m"], c["q"][b], c["qd"][b], _row(tab["Q"], b, per), _row(tab["xgoal"], b, per), c["terms"], _row(tab["xtarget"], b, per),
                   dtype) for b in range(B)]
    res = {k: np.array([o[k] for o in outs]) for k in ("x", "Jk", "lx", "Q", "r")}
    res["gq"] = np.array([P.pullback(c["m"], c["q"][b], c["terms"], c["gx"][b], dtype) for b in range(B)])
    return res


def _gpu(sim, c, tab, want=("Jk", "lx", "Q"), sel=slice(None), **over):
    kw = dict(Q=tab["Q"], xgoal=tab["xgoal"], terms=c["terms"], xtarget=tab["xtarget"])
    kw.update(over)
    return sim.rollout_cost(N, c["q"][sel], c["qd"][sel], want=want, **kw)


# ---------------------------------------------------------------- 1. against the proto

@pytest.mark.gpu
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per"])
@pytest.mark.parametrize("size", SIZES)
def test_outputs_meet_the_extended_proto(size, per):
    from redmax_amd import BatchSim
    c = _case(size)
    tab = c["per" if per else "shared"]
    ref, ext = _proto(c, tab, per, np.float64), _proto(c, tab, per, np.longdouble)
    rn, pn = np.linalg.norm(ext["r"].astype(float), axis=-1), np.linalg.norm(ext["x"].astype(float), axis=-1)
    assert (rn >= 0.1 * pn).all(), (rn / pn).min()
    sim = BatchSim(c["sc"], batch=B)
    gpu = _gpu(sim, c, tab)
    gpu["x"], gpu["gq"] = sim.rollout_points(N, c["q"], c["terms"], gx=c["gx"])
    sim.close()
    ok = True
    line = "%-7s %-6s" % (size, "per" if per else "shared")
    for name in QUANTITIES:
        e_ref, e_gpu = P.rel_err(ref[name], ext[name]), P.rel_err(gpu[name], ext[name])
        bound = 8 * max(e_ref, 16 * EPS)
        line += "   %s %.2e %.2e%s" % (name, e_ref, e_gpu, "" if e_gpu <= bound else " <-- over %.2e" % bound)
        ok = ok and e_gpu <= bound
    print(line)
    assert ok, line


# ---------------------------------------------------------------- 2. exact structure, bit for bit

def _path_mask(c):
    """[N][nr] bool: the reduced DOFs on the path of some term of the step."""
    m, on = c["m"], np.zeros((N, c["sc"].nr), bool)
    for t in c["terms"]:
        for j in range(m["n"]):
            if m["anc"][j, t["body"]] and m["idx"][j] >= 0:
                on[t["step"] - 1, m["idx"][j]] = True
    return on


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["fixed", 5, "tree7", "tree64"])
def test_symmetry_untouched_blocks_and_zeros(size):
    from redmax_amd import BatchSim
    c = _case(size)
    nr, tab = c["sc"].nr, c["per"]
    sim = BatchSim(c["sc"], batch=B)
    out = _gpu(sim, c, tab)
    _, gq = sim.rollout_points(N, c["q"], c["terms"], gx=c["gx"])
    Qo = out["Q"]
    assert np.array_equal(Qo, Qo.transpose(0, 1, 3, 2))
    assert np.array_equal(Qo[:, :, nr:, :], tab["Q"][:, :, nr:, :]) and np.array_equal(Qo[:, :, :, nr:], tab["Q"][:, :, :, nr:])
    # step 2 owns no term: the joint-space part alone, which is what the call without terms returns for every step
    bare = sim.rollout_cost(N, c["q"], c["qd"], Q=tab["Q"], xgoal=tab["xgoal"])
    assert np.array_equal(Qo[:, 1], tab["Q"][:, 1]) and np.array_equal(bare["Q"], tab["Q"])
    for k in ("Jk", "lx"):
        assert np.array_equal(out[k][:, 1], bare[k][:, 1])
    owns = np.array([any(t["step"] == k + 1 for t in c["terms"]) for k in range(N)])
    assert not np.array_equal(out["lx"][:, owns], bare["lx"][:, owns])
    # off the path: exact zeros in gq, the input's bits in Qout
    on = _path_mask(c)
    assert on.any() and (gq[:, ~on] == 0.0).all() and (gq[:, on] != 0.0).any()
    assert np.signbit(gq[:, ~on]).sum() == 0
    for k in range(N):
        off = np.where(~on[k])[0]
        assert np.array_equal(Qo[:, k][:, off, :], tab["Q"][:, k][:, off, :])
        if on[k].any():      # ... and on it the block of the terms has been added
            dofs = np.where(on[k])[0]
            assert (Qo[:, k][:, dofs][:, :, dofs] != tab["Q"][:, k][:, dofs][:, :, dofs]).any()
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, "tree7", 32])
def test_outputs_do_not_depend_on_their_company(size):
    """Which outputs are NULL, the place in the batch, the batch size, shared against per-rollout copies, sc = NULL against zero
    tables, the host against the device form, and a repeated call: the same bits."""
    from redmax_amd import BatchSim
    c = _case(size)
    nr, tab, sh = c["sc"].nr, c["per"], c["shared"]
    sim = BatchSim(c["sc"], batch=B)
    full = _gpu(sim, c, tab)
    x, gq = sim.rollout_points(N, c["q"], c["terms"], gx=c["gx"])
    for k in ("Jk", "lx", "Q"):
        assert np.array_equal(_gpu(sim, c, tab, want=(k,))[k], full[k]), k
    again = _gpu(sim, c, tab)
    assert all(np.array_equal(again[k], full[k]) for k in full)
    assert np.array_equal(sim.rollout_points(N, c["q"], c["terms"])[0], x)
    assert np.array_equal(sim.rollout_points(N, c["q"], c["terms"], gx=c["gx"], points=False)[1], gq)
    # a permuted batch
    perm = np.array([2, 0, 1])
    ptab = {k: v[perm] for k, v in tab.items()}
    pout = sim.rollout_cost(N, c["q"][perm], c["qd"][perm], terms=c["terms"], **ptab)
    assert all(np.array_equal(pout[k], full[k][perm]) for k in full)
    px, pgq = sim.rollout_points(N, c["q"][perm], c["terms"], gx=c["gx"][perm])
    assert np.array_equal(px, x[perm]) and np.array_equal(pgq, gq[perm])
    # shared tables against B copies of them
    shared = _gpu(sim, c, sh)
    copies = _gpu(sim, c, {k: np.broadcast_to(v, (B,) + v.shape).copy() for k, v in sh.items()})
    assert all(np.array_equal(shared[k], copies[k]) for k in shared)
    # no joint-space part against tables of zeros; no terms is covered above
    none = sim.rollout_cost(N, c["q"], c["qd"], terms=c["terms"], xtarget=tab["xtarget"])
    zeros = sim.rollout_cost(N, c["q"], c["qd"], Q=np.zeros((N, 2 * nr, 2 * nr)), xgoal=np.zeros((N, 2 * nr)), terms=c["terms"],
                             xtarget=tab["xtarget"])
    qonly = sim.rollout_cost(N, c["q"], c["qd"], Q=np.zeros((B, N, 2 * nr, 2 * nr)), terms=c["terms"], xtarget=tab["xtarget"])
    for k in none:
        assert np.array_equal(none[k], zeros[k]) and np.array_equal(none[k], qonly[k]), k
        assert np.array_equal(np.signbit(none[k]), np.signbit(zeros[k])), k
    sim.close()
    # another batch size: rollout 1 alone
    one = BatchSim(c["sc"], batch=1)
    o1 = one.rollout_cost(N, c["q"][1:2], c["qd"][1:2], terms=c["terms"], **{k: v[1:2] for k, v in tab.items()})
    x1, gq1 = one.rollout_points(N, c["q"][1:2], c["terms"], gx=c["gx"][1:2])
    assert all(np.array_equal(o1[k][0], full[k][1]) for k in full) and np.array_equal(x1[0], x[1]) and np.array_equal(gq1[0], gq[1])
    one.close()


@pytest.mark.gpu
def test_the_device_forms_return_the_host_forms_bits():
    from redmax_amd import BatchSim
    c = _case("tree7")
    nr, tab, T = c["sc"].nr, c["per"], len(c["terms"])
    sim = BatchSim(c["sc"], batch=B)
    full = _gpu(sim, c, tab)
    x, gq = sim.rollout_points(N, c["q"], c["terms"], gx=c["gx"])
    d = {k: _DevArray(v) for k, v in dict(q=c["q"], qd=c["qd"], Q=tab["Q"], xg=tab["xgoal"], xt=tab["xtarget"], gx=c["gx"]).items()}
    o = {k: _DevArray(np.full(s, np.nan)) for k, s in dict(Jk=(B, N), lx=(B, N, 2 * nr), Q=(B, N, 2 * nr, 2 * nr), x=(B, T, 3), gq=(B, N, nr)).items()}
    sim.rollout_cost_device(N, d["q"].ptr.value, d["qd"].ptr.value, Q_ptr=d["Q"].ptr.value, xgoal_ptr=d["xg"].ptr.value, Q_per_rollout=True,
                            goal_per_rollout=True, terms=c["terms"], xtarget_ptr=d["xt"].ptr.value, target_per_rollout=True,
                            Jk_ptr=o["Jk"].ptr.value, lx_ptr=o["lx"].ptr.value, Qout_ptr=o["Q"].ptr.value)
    sim.rollout_points_device(N, d["q"].ptr.value, c["terms"], x_ptr=o["x"].ptr.value, gx_ptr=d["gx"].ptr.value, gq_ptr=o["gq"].ptr.value)
    assert sim.last_step_kernel() == "k_rollout_cost"
    for k in full:
        assert np.array_equal(o[k].get(), full[k]), k
    assert np.array_equal(o["x"].get(), x) and np.array_equal(o["gq"].get(), gq)
    for k, v in dict(q=c["q"], qd=c["qd"], Q=tab["Q"]).items():      # the inputs are left as they were
        assert np.array_equal(d[k].get(), v)
    for a in list(d.values()) + list(o.values()):
        a.free()
    sim.close()


# ---------------------------------------------------------------- 3. against the library itself

def _rolled(size, nsteps=6):
    """The 5-chain under case's u: (sc, cs, terms on the tip at steps 2 and nsteps and on an inner body at step 4, targets)."""
    sc = _scene_or_fixed(size, 1)
    cs = case(sc, 71, nsteps=nsteps, B=B)
    n = sc.nr
    terms = [dict(body=n - 1, xlocal=[5.0, 0.0, 0.0], step=2, wpos=3.0), dict(body=n // 2, xlocal=[1.0, 0.5, -0.5], step=4, wpos=0.5),
             dict(body=n - 1, xlocal=[5.0, 0.2, 0.1], step=nsteps, wpos=2.0)]
    xt = np.array([[10.0, 0.0, -10.0], [4.0, 1.0, -3.0], [8.0, 1.0, -12.0]])
    return sc, cs, terms, xt, nsteps


@pytest.mark.gpu
def test_the_tape_is_left_alone_and_the_value_is_adjoint_tracks():
    from redmax_amd import BatchSim
    sc, cs, terms, xt, ns = _rolled(5)
    m = pw.build_model(sc.desc())
    sim = BatchSim(sc, batch=B)
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, info = sim.rollout_tape(ns, sc.h, cs["u"], pscale=sc.task["pscale"], stats=True)
    assert (info["status"] & 15 == 0).all()
    state = sim.get_state()
    before = sim.rollout_vjp(ns, cs["c"], cs["d"])
    out = sim.rollout_cost(ns, qt, qdt, terms=terms, xtarget=xt)
    sim.rollout_points(ns, qt, terms, gx=np.ones((B, len(terms), 3)))
    after = sim.rollout_vjp(ns, cs["c"], cs["d"])
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert all(np.array_equal(a, b) for a, b in zip(state, sim.get_state()))
    # the same objective through rmx_adjoint_track (wreg = 0), from the same state under the same torques
    sim.set_state(cs["q0"], cs["qd0"])
    Ptrack, _, _ = sim.adjoint_track(ns, sc.h, dict(terms=terms, xtarget=xt, pscale=sc.task["pscale"], wreg=0.0), cs["u"], gradient=False)
    sim.close()
    ref = np.array([P.cost(m, qt[b], qdt[b], None, None, terms, xt)["Jk"].sum() for b in range(B)])
    ext = np.array([P.cost(m, qt[b], qdt[b], None, None, terms, xt, np.longdouble)["Jk"].sum() for b in range(B)])
    e_ref = P.rel_err(ref, ext)
    bound = 8 * max(e_ref, 16 * EPS)
    e_cost, e_track = P.rel_err(out["Jk"].sum(1), ext), P.rel_err(Ptrack, ext)
    print("value at the final states: e_ref %.2e, rollout_cost %.2e, adjoint_track %.2e (bound %.2e)" % (e_ref, e_cost, e_track, bound))
    assert e_cost <= bound and e_track <= bound


# ---------------------------------------------------------------- 4. the testGrad identity on the GPU's own value

@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, "tree7"])
def test_lx_meets_central_differences_of_the_gpus_value(size):
    """Central differences of sum_k Jk (eps = 1e-5) along 3 random directions in q, one batch of 6 perturbed records, against
    <lx_q, d>: rtol 2e-5, atol 1e-6 max|ana| (test_gpu_rollout_vjp.py::test_gradients_meet_the_testgrad_identity's floor)."""
    from redmax_amd import BatchSim
    c = _case(size)
    nr, tab = c["sc"].nr, c["per"]
    b, nd, eps = 1, 3, 1e-5
    rng = np.random.default_rng(73)
    dirs = rng.standard_normal((nd, N, nr))
    one = BatchSim(c["sc"], batch=1)
    kw = dict(Q=tab["Q"][b], xgoal=tab["xgoal"][b], terms=c["terms"], xtarget=tab["xtarget"][b])
    lx = one.rollout_cost(N, c["q"][b:b + 1], c["qd"][b:b + 1], want=("lx",), **kw)["lx"][0]
    one.close()
    fd = BatchSim(c["sc"], batch=2 * nd)
    qs = np.array([c["q"][b] + s * eps * d for d in dirs for s in (1.0, -1.0)])
    Jk = fd.rollout_cost(N, qs, np.broadcast_to(c["qd"][b], qs.shape), want=("Jk",), **kw)["Jk"]
    fd.close()
    L = Jk.sum(1)
    num = (L[0::2] - L[1::2]) / (2 * eps)
    ana = np.array([(lx[:, :nr] * d).sum() for d in dirs])
    err = np.abs(num - ana)
    print("testgrad %s: |num - ana| / max|ana| = %.3e" % (size, err.max() / np.abs(ana).max()))
    assert np.abs(ana).max() > 0
    assert (err <= 2e-5 * np.abs(ana) + 1e-6 * np.abs(ana).max()).all(), (num, ana)


# ---------------------------------------------------------------- 5. refusals, and the models that are taken

@pytest.mark.gpu
def test_refusals_by_message():
    from redmax_amd import BatchSim, _abi
    import ctypes as C
    c = _case(5)
    nr, tab, T = c["sc"].nr, c["shared"], len(c["terms"])
    sim = BatchSim(c["sc"], batch=B)
    L, bh = sim._L, sim._batch
    q, qd = np.ascontiguousarray(c["q"]), np.ascontiguousarray(c["qd"])
    arr, _ = sim._point_terms(c["terms"], "test", True)
    xt = np.ascontiguousarray(tab["xtarget"])
    out = {k: np.zeros(s) for k, s in dict(Jk=(B, N), lx=(B, N, 2 * nr), Q=(B, N, 2 * nr, 2 * nr)).items()}
    x, gx, gq = np.zeros((B, T, 3)), np.zeros((B, T, 3)), np.zeros((B, N, nr))

    def cost(nsteps=N, q_=q, qd_=qd, sc=None, pts="default", cm="default", fn=L.rmx_rollout_cost):
        pts = _abi.PointTerms(T, arr, xt.ctypes.data, 0) if pts == "default" else pts
        cm = _abi.CostModel(out["Jk"].ctypes.data, out["lx"].ctypes.data, out["Q"].ctypes.data) if cm == "default" else cm
        rc = fn(bh, nsteps, None if q_ is None else q_.ctypes.data, None if qd_ is None else qd_.ctypes.data,
                None if sc is None else C.byref(sc), None if pts is None else C.byref(pts), None if cm is None else C.byref(cm))
        return rc, L.rmx_last_error().decode()

    def points(nsteps=N, q_=q, pts="default", x_=x, gx_=gx, gq_=gq):
        pts = _abi.PointTerms(T, arr, None, 0) if pts == "default" else pts
        rc = L.rmx_rollout_points(bh, nsteps, None if q_ is None else q_.ctypes.data, None if pts is None else C.byref(pts),
                                  None if x_ is None else x_.ctypes.data, None if gx_ is None else gx_.ctypes.data,
                                  None if gq_ is None else gq_.ctypes.data)
        return rc, L.rmx_last_error().decode()

    def refused(res, words):
        assert res[0] != 0 and words in res[1], res

    assert cost()[0] == 0 and points()[0] == 0
    refused(cost(q_=None), "rmx_rollout_cost: null argument")
    refused(cost(qd_=None), "rmx_rollout_cost: null argument")
    refused(cost(cm=None), "rmx_rollout_cost: null argument")
    refused(cost(pts=None), "rmx_rollout_cost: null argument")                       # neither sc nor pts
    refused(cost(pts=_abi.PointTerms(T, arr, None, 0)), "rmx_rollout_cost: null argument")      # no targets
    refused(points(q_=None), "rmx_rollout_points: null argument")
    refused(points(pts=None), "rmx_rollout_points: null argument")
    refused(cost(cm=_abi.CostModel(None, None, None)), "rmx_rollout_cost: all outputs are null")
    refused(points(x_=None, gq_=None), "rmx_rollout_points: all outputs are null")
    refused(points(gx_=None), "gq needs gx")
    refused(cost(pts=_abi.PointTerms(T, arr, xt.ctypes.data, 2)), "per_rollout must be 0 or 1")
    refused(points(pts=_abi.PointTerms(T, arr, None, -1)), "per_rollout must be 0 or 1")
    refused(cost(sc=_abi.StateCost(None, None, 2, 0)), "Q_per_rollout and goal_per_rollout must be 0 or 1")
    refused(cost(sc=_abi.StateCost(None, None, 0, 3)), "Q_per_rollout and goal_per_rollout must be 0 or 1")
    refused(cost(nsteps=0), "nsteps < 1")
    # rmx_track::plan_terms' own messages
    refused(cost(pts=_abi.PointTerms(0, arr, xt.ctypes.data, 0)), "rmx_rollout_cost: nterms < 1")
    refused(points(pts=_abi.PointTerms(T, None, None, 0)), "rmx_rollout_points: null terms")
    bad, _ = sim._point_terms([dict(c["terms"][0], body=nr)], "test", True)
    refused(cost(pts=_abi.PointTerms(1, bad, xt.ctypes.data, 0)), "term 0: body %d is outside the listing of %d bodies" % (nr, nr))
    bad, _ = sim._point_terms(c["terms"][:1] + [dict(c["terms"][1], step=N + 1)], "test", True)
    refused(points(pts=_abi.PointTerms(2, bad, None, 0)), "term 1: step %d is outside [1, %d]" % (N + 1, N))
    # the weights: rmx_rollout_cost alone reads them
    for w in (-1.0, float("nan"), float("inf")):
        bad, _ = sim._point_terms(c["terms"][:2] + [dict(c["terms"][2], wpos=w)], "test", True)
        refused(cost(pts=_abi.PointTerms(3, bad, xt.ctypes.data, 0)), "rmx_rollout_cost: term 2: wpos must be finite and >= 0")
        assert points(pts=_abi.PointTerms(3, bad, None, 0))[0] == 0
    # the Python layer, in the words of its neighbours
    with pytest.raises(ValueError, match="rollout_cost: q and qdot must have shape"):
        sim.rollout_cost(N, c["q"][:, :-1], c["qd"], terms=c["terms"], xtarget=xt)
    with pytest.raises(ValueError, match="rollout_cost: Q must have shape"):
        sim.rollout_cost(N, c["q"], c["qd"], Q=np.zeros((N, nr, nr)))
    with pytest.raises(ValueError, match="rollout_cost: xtarget must have shape"):
        sim.rollout_cost(N, c["q"], c["qd"], terms=c["terms"], xtarget=xt[:-1])
    with pytest.raises(ValueError, match="rollout_points: gx must have shape"):
        sim.rollout_points(N, c["q"], c["terms"], gx=np.zeros((B, T, 2)))
    with pytest.raises(_abi.RedMaxHipError, match="rmx_rollout_cost: null argument"):
        sim.rollout_cost(N, c["q"], c["qd"])
    # and after all of it the entries still answer with the bits they gave
    assert cost()[0] == 0
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["chart", "big"])
def test_models_outside_kinematics_are_refused_in_rollout_tapes_words(kind):
    from redmax_amd import BatchSim, _abi
    from redmax_amd.scenes import sceneChain, scenesRedMax
    sc = scenesRedMax(7) if kind == "chart" else sceneChain(100)
    sc.init()
    words = {"chart": "spherical joints", "big": "more than 64 nodes"}[kind]
    sim = BatchSim(sc, batch=2)
    q = np.zeros((2, 2, sc.nr))
    terms = [dict(body=0, xlocal=[0.0, 0.0, 0.0], step=1, wpos=1.0)]
    with pytest.raises(_abi.RedMaxHipError, match=words) as tape:
        sim.rollout_tape(2, sc.h, np.zeros((2, 2, sc.nr)))
    with pytest.raises(_abi.RedMaxHipError, match=words) as pts:
        sim.rollout_points(2, q, terms)
    with pytest.raises(_abi.RedMaxHipError, match=words) as cst:
        sim.rollout_cost(2, q, q, terms=terms, xtarget=np.zeros((1, 3)))
    tail = str(tape.value).split(": ", 1)[1]
    assert str(pts.value).split(": ", 1)[1] == tail and str(cst.value).split(": ", 1)[1] == tail
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ground", "point forces"])
def test_contact_and_point_forces_do_not_enter_kinematics(kind):
    """A chain over a frictional ground and the 15-joint tree with body-to-body forces: rmx_rollout_tape refuses them, the two entries
    take them and return what the proto gives for the model's kinematics."""
    from redmax_amd import BatchSim, _abi
    if kind == "ground":
        from redmax_amd.scenes import sceneChainGround
        sc = sceneChainGround(6, ground_z=-1.0)
        sc.init()
    else:
        from proto_point_forces import treeWithForces
        sc = treeWithForces(15)
        sc.init()      # (the forces were attached behind the scene's own init)
    m = pw.build_model(sc.desc())
    nr = sc.nr
    rng = np.random.default_rng(79)
    q0, qd0 = sc.getQ()
    q = q0[None, None] + 0.1 * rng.standard_normal((2, N, nr))
    qd = qd0[None, None] + 0.1 * rng.standard_normal((2, N, nr))
    terms = terms_of(m, N)
    xt = rng.standard_normal((len(terms), 3)) * 10.0
    gx = rng.standard_normal((2, len(terms), 3))
    sim = BatchSim(sc, batch=2)
    with pytest.raises(_abi.RedMaxHipError, match="ground contact" if kind == "ground" else "point forces"):
        sim.rollout_tape(N, sc.h, np.zeros((2, N, nr)))
    x, gq = sim.rollout_points(N, q, terms, gx=gx)
    out = sim.rollout_cost(N, q, qd, terms=terms, xtarget=xt)
    sim.close()
    for b in range(2):
        ref = P.cost(m, q[b], qd[b], None, None, terms, xt)
        # (float64 against float64 on short trees: 64 eps of the largest entry, the bound of test_point_cost_proto's Jacobians)
        for name, got, want in (("x", x[b], ref["x"]), ("gq", gq[b], P.pullback(m, q[b], terms, gx[b])), ("Jk", out["Jk"][b], ref["Jk"]),
                                ("lx", out["lx"][b], ref["lx"]), ("Q", out["Q"][b], ref["Q"])):
            assert np.max(np.abs(got - want)) <= 64 * EPS * np.max(np.abs(want)), (kind, name)
