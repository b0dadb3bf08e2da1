"""rmx_rollout_frames / rmx_rollout_cost_frames: position, point velocity and orientation of body frames along a state record and the
cost model of the device iLQR with frame targets (redmax_amd/csrc/rmx_cost.h, the FRAMES instantiation), on the GPU.

The checks, in the order of the sections below:
  1. against tests/proto_frame_cost.py at every padded size: with ext the longdouble proto and ref the float64 proto on IDENTICAL
     inputs, per quantity (x, v, R, gq, gqd, Jk, lx, Q) e = max |. - ext| / max |ext| over the batch and e_gpu <= 8 max(e_ref, 16 eps)
     - the rule of test_gpu_rollout_lqr._judge and test_gpu_rollout_cost.py.  Conditions on the inputs, asserted on the proto:
     |r| >= 0.1 |p|; |rv| >= 0.1 |v| (vtarget = v + dir (0.3 |v| + 0.3)); Rtarget = R exp(theta axis) with theta in [0.5, 2.0] rad,
     so 0.4 <= |e_w| and theta stays away from pi;
  2. exact structure, bit for bit; 3. against the library itself (rmx_rollout_tape, rmx_rollout_points); 4. the testGrad identity
     on the GPU's own value, in q and in qdot; 5. refusals, and the models that are taken.

Scenes, B, N and states: test_gpu_rollout_cost's.  Terms: test_frame_cost_proto.frame_terms_of - step 1 owns a term with all three
weights (tip) and a position-only one, step 2 none, step 3 position-only terms alone, step 4 a term with wrot alone on the root body
and one with wvel alone on an inner body.

Measured on an MI355X (test_outputs_meet_the_extended_proto, pytest -s; e_ref e_gpu per quantity over the batch; the whole table
is profiles/frame_cost.txt): every e_ref is below the floor of 16 eps = 3.55e-15, where the bound is 2.84e-14; the largest e_gpu is
3.21e-15 (Jk, 32-chain, per-rollout tables: e_gpu / bound = 0.11), the smallest 1.13e-16 (R, 7-joint tree).  Its extremes:
    scene   tables   x                   v                   R                   gq                  gqd                 Jk                  lx                  Q
    2       shared   1.88e-16 1.87e-16   1.95e-16 2.14e-16   1.51e-16 1.51e-16   1.51e-16 1.51e-16   2.18e-16 2.02e-16   2.51e-16 2.51e-16   1.17e-16 1.17e-16   3.36e-16 3.53e-16
    16      per      1.56e-15 9.06e-16   7.96e-16 5.89e-16   7.21e-16 3.19e-16   6.82e-16 5.03e-16   5.77e-16 3.52e-16   2.53e-15 1.22e-15   2.16e-15 1.72e-15   5.68e-16 6.74e-16
    32      per      1.02e-15 2.09e-15   5.58e-16 7.54e-16   5.03e-16 5.79e-16   2.96e-16 6.94e-16   7.24e-16 7.35e-16   2.24e-15 3.21e-15   1.88e-15 2.21e-15   1.06e-15 1.31e-15
    tree64  per      1.61e-16 2.65e-16   2.59e-16 2.31e-16   1.27e-16 1.27e-16   3.61e-16 5.75e-16   1.49e-16 2.68e-16   4.55e-16 7.48e-16   3.09e-16 3.24e-16   7.17e-16 5.53e-16
v along the 6-step tape (section 3): e_ref 3.66e-16, rmx_rollout_frames 2.20e-16, Jp qdot from rmx_rollout_points 2.74e-16.  The
testGrad identity (section 4), of max|ana|: 7.0e-10 in q and 3.0e-11 in qdot (5-chain), 1.0e-10 and 7.4e-11 (7-joint tree).
"""
import numpy as np
import pytest

import proto_frame_cost as F
import proto_point_cost as P
import proto_worldframe as pw
from test_frame_cost_proto import frame_terms_of
from test_gpu_adjoint_controls import _DevArray
from test_gpu_rollout_cost import _scene
from test_rollout_feedback_proto import scene as _scene_or_fixed
from test_rollout_vjp_proto import case

B, N = 3, 4
EPS = np.finfo(np.float64).eps
SIZES = [2, 3, "fixed", 5, "tree7", 11, 16, 32, "tree64"]
QUANTITIES = ("x", "v", "R", "gq", "gqd", "Jk", "lx", "Q")
_CACHE = {}
_PROTO = {}


def _case(size):
    """Scene, proto model, terms and the inputs of a size, shared and per rollout: computed once, left unchanged."""
    if size not in _CACHE:
        sc = _scene(size)
        m = pw.build_model(sc.desc())
        nr = sc.nr
        cs = case(sc, 61, nsteps=N, B=B)
        rng = np.random.default_rng(83)
        q = cs["q0"][:, None] + 0.05 * rng.standard_normal((B, N, nr))
        qd = cs["qd0"][:, None] + 0.2 * rng.standard_normal((B, N, nr))
        terms = frame_terms_of(m, N)
        T = len(terms)
        Qp = rng.standard_normal((B, N, 2 * nr, 2 * nr))
        Qp = Qp + Qp.transpose(0, 1, 3, 2)
        xgp = np.concatenate([q, qd], axis=-1) + 0.3 * rng.standard_normal((B, N, 2 * nr))
        fr = [F.frames(m, q[b], qd[b], terms) for b in range(B)]
        xp, vp, Rp = (np.array([f[i] for f in fr]) for i in range(3))

        def off(a):
            d = rng.standard_normal((B, T, 3))
            d /= np.linalg.norm(d, axis=-1, keepdims=True)
            per = a + d * (0.3 * np.linalg.norm(a, axis=-1, keepdims=True) + 0.3)
            # a shared target: off the rollouts' values by their spread about the mean and 0.3 (|.| + 1) of the farthest of them
            spread = np.linalg.norm(a - a.mean(0), axis=-1).max(0)[:, None]
            return per, a.mean(0) + d[0] * (spread + 0.3 * np.linalg.norm(a, axis=-1).max(0)[:, None] + 0.3)

        xtp, xts = off(xp)
        vtp, vts = off(vp)
        Rtp = np.array([[Rp[b, t] @ F.rot(rng.standard_normal(3), rng.uniform(0.5, 2.0)) for t in range(T)] for b in range(B)])
        cot = dict(gx=rng.standard_normal((B, T, 3)), gv=rng.standard_normal((B, T, 3)), gR=rng.standard_normal((B, T, 3, 3)))
        _CACHE[size] = dict(sc=sc, m=m, terms=terms, q=q, qd=qd, cot=cot, per=dict(Q=Qp, xgoal=xgp, xtarget=xtp, vtarget=vtp, Rtarget=Rtp),
                            shared=dict(Q=Qp[0].copy(), xgoal=xgp[0].copy(), xtarget=xts, vtarget=vts, Rtarget=Rtp[0].copy()))
    return _CACHE[size]


def _row(a, b, per):
    return a[b] if per else a


def _proto(size, per, dtype):
    """dict(x, v, R, gq, gqd, Jk, lx, Q, r, rv, ew) over the batch from the proto in dtype (kept: several tests read it)."""
    key = (size, per, dtype)
    if key not in _PROTO:
        c = _case(size)
        tab = c["per" if per else "shared"]
        outs = [F.cost(c["m"], c["q"][b], c["qd"][b], _row(tab["Q"], b, per), _row(tab["xgoal"], b, per), c["terms"], _row(tab["xtarget"], b, per),
                       _row(tab["vtarget"], b, per), _row(tab["Rtarget"], b, per), dtype) for b in range(B)]
        res = {k: np.array([o[k] for o in outs]) for k in ("x", "v", "R", "Jk", "lx", "Q", "r", "rv", "ew")}
        g = [F.pullback(c["m"], c["q"][b], c["qd"][b], c["terms"], c["cot"]["gx"][b], c["cot"]["gv"][b], c["cot"]["gR"][b], dtype) for b in range(B)]
        res["gq"], res["gqd"] = np.array([a for a, _ in g]), np.array([a for _, a in g])
        _PROTO[key] = res
    return _PROTO[key]


def _gpu(sim, c, tab, want=("Jk", "lx", "Q"), sel=slice(None), **over):
    kw = dict(Q=tab["Q"], xgoal=tab["xgoal"], terms=c["terms"], xtarget=tab["xtarget"], vtarget=tab["vtarget"], Rtarget=tab["Rtarget"])
    kw.update(over)
    return sim.rollout_cost_frames(N, c["q"][sel], c["qd"][sel], want=want, **kw)


def _frames(sim, c, **kw):
    out, gq, gqd = sim.rollout_frames(N, c["q"], c["qd"], c["terms"], **dict(c["cot"], **kw))
    return dict(out, gq=gq, gqd=gqd)


# ---------------------------------------------------------------- 1. against the proto

@pytest.mark.gpu
@pytest.mark.parametrize("per", [False, True], ids=["shared", "per"])
@pytest.mark.parametrize("size", SIZES)
def test_outputs_meet_the_extended_proto(size, per):
    from redmax_amd import BatchSim
    c = _case(size)
    tab = c["per" if per else "shared"]
    ref, ext = _proto(size, per, np.float64), _proto(size, per, np.longdouble)
    terms = c["terms"]
    wp, wv, wr = (np.array([F.term_weights(t)[i] > 0 for t in terms]) for i in range(3))
    norm = lambda a: np.linalg.norm(a.astype(float), axis=-1)      # noqa: E731
    assert (norm(ext["r"])[:, wp] >= 0.1 * norm(ext["x"])[:, wp]).all()
    assert (norm(ext["rv"])[:, wv] >= 0.1 * norm(ext["v"])[:, wv]).all()
    assert (norm(ext["ew"])[:, wr] >= 0.4).all()
    sim = BatchSim(c["sc"], batch=B)
    gpu = _gpu(sim, c, tab)
    gpu.update(_frames(sim, c))
    assert sim.last_step_kernel() == "k_rollout_frames"
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

def _masks(c):
    """([N][nr] bool: the reduced DOFs on the path of some term of the step, [N] bool: the step owns a term with wvel > 0)."""
    m, on, vel = c["m"], np.zeros((N, c["sc"].nr), bool), np.zeros(N, bool)
    for t in c["terms"]:
        vel[t["step"] - 1] |= F.term_weights(t)[1] > 0
        for j in range(m["n"]):
            if m["anc"][j, t["body"]] and m["idx"][j] >= 0:
                on[t["step"] - 1, m["idx"][j]] = True
    return on, vel


def _position_only(c, tab):
    """The terms with wvel = wrot = 0 and their rows of the target table, as rollout_cost takes them."""
    keep = [i for i, t in enumerate(c["terms"]) if F.term_weights(t)[1] == 0 and F.term_weights(t)[2] == 0]
    return [dict(body=c["terms"][i]["body"], xlocal=c["terms"][i]["xlocal"], step=c["terms"][i]["step"], wpos=c["terms"][i]["wpos"])
            for i in keep], tab["xtarget"][..., keep, :]


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["fixed", 5, "tree7", 16, 32, "tree64"])
def test_symmetry_untouched_blocks_and_position_only_steps(size):
    from redmax_amd import BatchSim
    c = _case(size)
    nr, tab = c["sc"].nr, c["per"]
    sim = BatchSim(c["sc"], batch=B)
    out = _gpu(sim, c, tab)
    Qo, Qi = out["Q"], tab["Q"]
    assert np.array_equal(Qo, Qo.transpose(0, 1, 3, 2))
    on, vel = _masks(c)
    assert vel.any() and not vel.all()
    for k in range(N):
        off = np.where(~on[k])[0]
        both = np.concatenate([off, nr + off])
        assert np.array_equal(Qo[:, k][:, both, :], Qi[:, k][:, both, :]) and np.array_equal(Qo[:, k][:, :, both], Qi[:, k][:, :, both])
        if not vel[k]:      # the qdot rows and columns are the input's
            assert np.array_equal(Qo[:, k, nr:, :], Qi[:, k, nr:, :]) and np.array_equal(Qo[:, k, :, nr:], Qi[:, k, :, nr:])
        else:      # ... and have taken the velocity term's blocks (a cross block only where the proto's is not zero: G = 0 on a path
            dofs = np.where(on[k])[0]      # of prismatic joints alone)
            Qr = _proto(size, True, np.float64)["Q"]
            for blk in ((dofs, nr + dofs), (nr + dofs, dofs), (nr + dofs, nr + dofs)):
                sub = lambda A: A[:, k][:, blk[0]][:, :, blk[1]]      # noqa: E731
                assert (sub(Qo) != sub(Qi)).any() == (sub(Qr) != sub(Qi)).any()
            assert (Qo[:, k, nr:, nr:] != Qi[:, k, nr:, nr:]).any()
    # steps whose terms weigh position alone, and steps without terms: rmx_rollout_cost's bits on the same call
    pterms, pxt = _position_only(c, tab)
    plain = sim.rollout_cost(N, c["q"], c["qd"], Q=tab["Q"], xgoal=tab["xgoal"], terms=pterms, xtarget=pxt)
    steps = [k for k in range(N) if all(F.term_weights(t)[1] == 0 and F.term_weights(t)[2] == 0 for t in c["terms"] if t["step"] == k + 1)]
    assert steps == [1, 2]
    for k in ("Jk", "lx", "Q"):
        assert np.array_equal(out[k][:, steps], plain[k][:, steps]), k
    other = [k for k in range(N) if k not in steps]
    assert not np.array_equal(out["lx"][:, other], plain["lx"][:, other])
    # the same terms with every wvel and wrot zero: rmx_rollout_cost's bits at every step (wpos = 0 terms add nothing to lx and Q)
    zt = [dict(t, wvel=0.0, wrot=0.0) for t in c["terms"]]
    zero = sim.rollout_cost_frames(N, c["q"], c["qd"], Q=tab["Q"], xgoal=tab["xgoal"], terms=zt, xtarget=tab["xtarget"])
    same = sim.rollout_cost(N, c["q"], c["qd"], Q=tab["Q"], xgoal=tab["xgoal"], terms=[{k: t[k] for k in ("body", "xlocal", "step", "wpos")} for t in zt],
                            xtarget=tab["xtarget"])
    for k in ("Jk", "lx", "Q"):
        assert np.array_equal(zero[k], same[k]), k
    # rmx_rollout_frames with x and gq alone: rmx_rollout_points
    fo, gq, _ = sim.rollout_frames(N, c["q"], c["qd"], c["terms"], gx=c["cot"]["gx"], want=("x",))
    px, pgq = sim.rollout_points(N, c["q"], c["terms"], gx=c["cot"]["gx"])
    assert np.array_equal(fo["x"], px) and np.array_equal(gq, pgq)
    # off the path and at steps without a term: exact zeros in gq and gqd
    fr = _frames(sim, c)
    assert (fr["gq"][:, ~on] == 0.0).all() and (fr["gqd"][:, ~on] == 0.0).all() and (fr["gq"][:, on] != 0.0).any() and (fr["gqd"][:, on] != 0.0).any()
    assert np.signbit(fr["gq"][:, ~on]).sum() == 0 and np.signbit(fr["gqd"][:, ~on]).sum() == 0
    sim.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, "tree7", 32])
def test_outputs_do_not_depend_on_their_company(size):
    """Which outputs are NULL, the place in the batch, the batch size, shared against per-rollout copies, NULL against zero tables and
    a repeated call: the same bits."""
    from redmax_amd import BatchSim
    c = _case(size)
    nr, tab, sh, cot = c["sc"].nr, c["per"], c["shared"], c["cot"]
    sim = BatchSim(c["sc"], batch=B)
    full = _gpu(sim, c, tab)
    fr = _frames(sim, c)
    for k in ("Jk", "lx", "Q"):
        assert np.array_equal(_gpu(sim, c, tab, want=(k,))[k], full[k]), k
    again = _gpu(sim, c, tab)
    assert all(np.array_equal(again[k], full[k]) for k in full)
    for k in ("x", "v", "R"):
        assert np.array_equal(sim.rollout_frames(N, c["q"], c["qd"], c["terms"], want=(k,))[0][k], fr[k]), k
    _, gq, gqd = sim.rollout_frames(N, c["q"], c["qd"], c["terms"], want=(), **cot)
    assert np.array_equal(gq, fr["gq"]) and np.array_equal(gqd, fr["gqd"])
    # the pull-back is the sum of its three parts, each alone (zero cotangents against NULL ones: the same bits)
    z3, z9 = np.zeros((B, len(c["terms"]), 3)), np.zeros((B, len(c["terms"]), 3, 3))
    _, gq0, gqd0 = sim.rollout_frames(N, c["q"], c["qd"], c["terms"], want=(), gx=z3, gv=cot["gv"], gR=z9)
    _, gq1, gqd1 = sim.rollout_frames(N, c["q"], c["qd"], c["terms"], want=(), gv=cot["gv"])
    assert np.array_equal(gq0, gq1) and np.array_equal(gqd0, gqd1) and np.array_equal(gqd1, fr["gqd"])
    # a permuted batch
    perm = np.array([2, 0, 1])
    pout = sim.rollout_cost_frames(N, c["q"][perm], c["qd"][perm], terms=c["terms"], **{k: v[perm] for k, v in tab.items()})
    assert all(np.array_equal(pout[k], full[k][perm]) for k in full)
    po, pgq, pgqd = sim.rollout_frames(N, c["q"][perm], c["qd"][perm], c["terms"], **{k: v[perm] for k, v in cot.items()})
    assert all(np.array_equal(po[k], fr[k][perm]) for k in po) and np.array_equal(pgq, fr["gq"][perm]) and np.array_equal(pgqd, fr["gqd"][perm])
    # shared tables against B copies of them
    shared = _gpu(sim, c, sh)
    copies = _gpu(sim, c, {k: np.broadcast_to(v, (B,) + v.shape).copy() for k, v in sh.items()})
    assert all(np.array_equal(shared[k], copies[k]) for k in shared)
    # no joint-space part against tables of zeros
    tg = {k: tab[k] for k in ("xtarget", "vtarget", "Rtarget")}
    none = sim.rollout_cost_frames(N, c["q"], c["qd"], terms=c["terms"], **tg)
    zeros = sim.rollout_cost_frames(N, c["q"], c["qd"], Q=np.zeros((N, 2 * nr, 2 * nr)), xgoal=np.zeros((N, 2 * nr)), terms=c["terms"], **tg)
    for k in none:
        assert np.array_equal(none[k], zeros[k]) and np.array_equal(np.signbit(none[k]), np.signbit(zeros[k])), k
    # a NULL target table against a table of zeros, where no term weighs it
    nov = [dict(t, wvel=0.0) for t in c["terms"]]
    a = sim.rollout_cost_frames(N, c["q"], c["qd"], Q=tab["Q"], xgoal=tab["xgoal"], terms=nov, xtarget=tab["xtarget"], Rtarget=tab["Rtarget"])
    b = sim.rollout_cost_frames(N, c["q"], c["qd"], Q=tab["Q"], xgoal=tab["xgoal"], terms=nov, xtarget=tab["xtarget"], Rtarget=tab["Rtarget"],
                                vtarget=np.zeros_like(tab["vtarget"]))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    sim.close()
    # another batch size: rollout 1 alone
    one = BatchSim(c["sc"], batch=1)
    o1 = one.rollout_cost_frames(N, c["q"][1:2], c["qd"][1:2], terms=c["terms"], **{k: v[1:2] for k, v in tab.items()})
    f1, gq1, gqd1 = one.rollout_frames(N, c["q"][1:2], c["qd"][1:2], c["terms"], **{k: v[1:2] for k, v in cot.items()})
    assert all(np.array_equal(o1[k][0], full[k][1]) for k in full) and all(np.array_equal(f1[k][0], fr[k][1]) for k in f1)
    assert np.array_equal(gq1[0], fr["gq"][1]) and np.array_equal(gqd1[0], fr["gqd"][1])
    one.close()


@pytest.mark.gpu
def test_the_device_forms_return_the_host_forms_bits():
    from redmax_amd import BatchSim
    c = _case("tree7")
    nr, tab, T, cot = c["sc"].nr, c["per"], len(c["terms"]), c["cot"]
    cm = lambda a: np.ascontiguousarray(np.swapaxes(a, -1, -2))      # noqa: E731  (the library's 3x3 is column-major)
    sim = BatchSim(c["sc"], batch=B)
    full = _gpu(sim, c, tab)
    fr = _frames(sim, c)
    d = {k: _DevArray(v) for k, v in dict(q=c["q"], qd=c["qd"], Q=tab["Q"], xg=tab["xgoal"], xt=tab["xtarget"], vt=tab["vtarget"],
                                          Rt=cm(tab["Rtarget"]), gx=cot["gx"], gv=cot["gv"], gR=cm(cot["gR"])).items()}
    o = {k: _DevArray(np.full(s, np.nan)) for k, s in dict(Jk=(B, N), lx=(B, N, 2 * nr), Q=(B, N, 2 * nr, 2 * nr), x=(B, T, 3), v=(B, T, 3),
                                                           R=(B, T, 3, 3), gq=(B, N, nr), gqd=(B, N, nr)).items()}
    p = lambda a: a.ptr.value      # noqa: E731
    sim.rollout_cost_frames_device(N, p(d["q"]), p(d["qd"]), Q_ptr=p(d["Q"]), xgoal_ptr=p(d["xg"]), Q_per_rollout=True, goal_per_rollout=True,
                                   terms=c["terms"], xtarget_ptr=p(d["xt"]), vtarget_ptr=p(d["vt"]), Rtarget_ptr=p(d["Rt"]),
                                   target_per_rollout=True, Jk_ptr=p(o["Jk"]), lx_ptr=p(o["lx"]), Qout_ptr=p(o["Q"]))
    sim.rollout_frames_device(N, p(d["q"]), p(d["qd"]), c["terms"], x_ptr=p(o["x"]), v_ptr=p(o["v"]), R_ptr=p(o["R"]), gx_ptr=p(d["gx"]),
                              gv_ptr=p(d["gv"]), gR_ptr=p(d["gR"]), gq_ptr=p(o["gq"]), gqd_ptr=p(o["gqd"]))
    assert sim.last_step_kernel() == "k_rollout_frames"
    for k in full:
        assert np.array_equal(o[k].get(), full[k]), k
    for k in ("x", "v", "gq", "gqd"):
        assert np.array_equal(o[k].get(), fr[k]), k
    assert np.array_equal(cm(o["R"].get()), fr["R"])
    for k, v in dict(q=c["q"], qd=c["qd"], Q=tab["Q"]).items():      # the inputs are left as they were
        assert np.array_equal(d[k].get(), v)
    for a in list(d.values()) + list(o.values()):
        a.free()
    sim.close()


# ---------------------------------------------------------------- 3. against the library itself

@pytest.mark.gpu
def test_v_is_jp_qdot_of_rollout_points_and_the_tape_is_left_alone():
    from redmax_amd import BatchSim
    ns = 6
    sc = _scene_or_fixed(5, 1)
    cs = case(sc, 71, nsteps=ns, B=B)
    m = pw.build_model(sc.desc())
    n = sc.nr
    terms = [dict(body=n - 1, xlocal=[5.0, 0.0, 0.0], step=2), dict(body=n // 2, xlocal=[1.0, 0.5, -0.5], step=4),
             dict(body=n - 1, xlocal=[5.0, 0.2, 0.1], step=ns)]
    T = len(terms)
    sim = BatchSim(sc, batch=B)
    sim.set_state(cs["q0"], cs["qd0"])
    qt, qdt, info = sim.rollout_tape(ns, sc.h, cs["u"], pscale=sc.task["pscale"], stats=True)
    assert (info["status"] & 15 == 0).all()
    state = sim.get_state()
    before = sim.rollout_vjp(ns, cs["c"], cs["d"])
    out, gq, gqd = sim.rollout_frames(ns, qt, qdt, terms, gx=np.ones((B, T, 3)), gv=np.ones((B, T, 3)), gR=np.ones((B, T, 3, 3)))
    sim.rollout_cost_frames(ns, qt, qdt, terms=[dict(t, wpos=1.0, wvel=1.0, wrot=1.0) for t in terms], xtarget=np.zeros((T, 3)),
                            vtarget=np.zeros((T, 3)), Rtarget=np.broadcast_to(np.eye(3), (T, 3, 3)))
    after = sim.rollout_vjp(ns, cs["c"], cs["d"])
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert all(np.array_equal(a, b) for a, b in zip(state, sim.get_state()))
    # Jp qdot, row by row of Jp: the pull-back of the unit cotangents through rmx_rollout_points
    v = np.zeros((B, T, 3))
    for comp in range(3):
        gx = np.zeros((B, T, 3))
        gx[:, :, comp] = 1.0
        for t in range(T):      # (one term at a time: terms of one step share a row of gq)
            g1 = np.zeros((B, T, 3))
            g1[:, t, comp] = 1.0
            _, g = sim.rollout_points(ns, qt, terms, gx=g1)
            v[:, t, comp] = (g[:, terms[t]["step"] - 1] * qdt[:, terms[t]["step"] - 1]).sum(-1)
    sim.close()
    ref = np.array([F.frames(m, qt[b], qdt[b], terms)[1] for b in range(B)])
    ext = np.array([F.frames(m, qt[b], qdt[b], terms, np.longdouble)[1] for b in range(B)])
    e_ref = P.rel_err(ref, ext)
    bound = 8 * max(e_ref, 16 * EPS)
    e_v, e_jp = P.rel_err(out["v"], ext), P.rel_err(v, ext)
    print("v along the tape: e_ref %.2e, rollout_frames %.2e, Jp qdot from rollout_points %.2e (bound %.2e)" % (e_ref, e_v, e_jp, bound))
    assert e_v <= bound and e_jp <= bound


# ---------------------------------------------------------------- 4. the testGrad identity on the GPU's own value

@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, "tree7"])
def test_lx_meets_central_differences_of_the_gpus_value(size):
    """Central differences of sum_k Jk (eps = 1e-5) along 3 random directions in q and 3 in qdot, one batch of 12 perturbed records,
    against <lx, d>: rtol 2e-5, atol 1e-6 max|ana| (test_gpu_rollout_cost.py's)."""
    from redmax_amd import BatchSim
    c = _case(size)
    nr, tab = c["sc"].nr, c["per"]
    b, nd, eps = 1, 3, 1e-5
    rng = np.random.default_rng(89)
    dirs = rng.standard_normal((2 * nd, N, nr))
    kw = {k: v[b] for k, v in tab.items()}
    one = BatchSim(c["sc"], batch=1)
    lx = one.rollout_cost_frames(N, c["q"][b:b + 1], c["qd"][b:b + 1], want=("lx",), terms=c["terms"], **kw)["lx"][0]
    one.close()
    fd = BatchSim(c["sc"], batch=4 * nd)
    qs = np.array([c["q"][b] + (s * eps * d if i < nd else 0.0) for i, d in enumerate(dirs) for s in (1.0, -1.0)])
    qds = np.array([c["qd"][b] + (s * eps * d if i >= nd else 0.0) for i, d in enumerate(dirs) for s in (1.0, -1.0)])
    Jk = fd.rollout_cost_frames(N, qs, qds, want=("Jk",), terms=c["terms"], **kw)["Jk"]
    fd.close()
    L = Jk.sum(1)
    num = (L[0::2] - L[1::2]) / (2 * eps)
    ana = np.array([(lx[:, :nr] * d).sum() if i < nd else (lx[:, nr:] * d).sum() for i, d in enumerate(dirs)])
    err = np.abs(num - ana)
    print("testgrad %s: |num - ana| / max|ana| = %.3e (q) %.3e (qdot)" % (size, err[:nd].max() / np.abs(ana[:nd]).max(),
                                                                          err[nd:].max() / np.abs(ana[nd:]).max()))
    for part in (slice(0, nd), slice(nd, None)):
        assert np.abs(ana[part]).max() > 0
        assert (err[part] <= 2e-5 * np.abs(ana[part]) + 1e-6 * np.abs(ana[part]).max()).all(), (num, ana)


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
    arr, _ = sim._frame_terms(c["terms"], "test")
    xt, vt = np.ascontiguousarray(tab["xtarget"]), np.ascontiguousarray(tab["vtarget"])
    Rt = np.ascontiguousarray(np.swapaxes(tab["Rtarget"], -1, -2))
    out = {k: np.zeros(s) for k, s in dict(Jk=(B, N), lx=(B, N, 2 * nr), Q=(B, N, 2 * nr, 2 * nr)).items()}
    x, gx, gq, gqd = np.zeros((B, T, 3)), np.zeros((B, T, 3)), np.zeros((B, N, nr)), np.zeros((B, N, nr))
    ad = lambda a: None if a is None else a.ctypes.data      # noqa: E731

    def terms(n=T, a=arr, x_=xt, v_=vt, R_=Rt, per=0):
        return _abi.FrameTerms(n, a, ad(x_), ad(v_), ad(R_), per)

    def cost(nsteps=N, q_=q, qd_=qd, sc=None, ft="default", cm="default"):
        ft = terms() if ft == "default" else ft
        cm = _abi.CostModel(out["Jk"].ctypes.data, out["lx"].ctypes.data, out["Q"].ctypes.data) if cm == "default" else cm
        rc = L.rmx_rollout_cost_frames(bh, nsteps, ad(q_), ad(qd_), None if sc is None else C.byref(sc), None if ft is None else C.byref(ft),
                                       None if cm is None else C.byref(cm))
        return rc, L.rmx_last_error().decode()

    def frames(nsteps=N, q_=q, qd_=qd, ft="default", x_=x, gx_=gx, gv_=None, gq_=gq, gqd_=None):
        ft = terms(x_=None, v_=None, R_=None) if ft == "default" else ft
        rc = L.rmx_rollout_frames(bh, nsteps, ad(q_), ad(qd_), None if ft is None else C.byref(ft), ad(x_), None, None, ad(gx_), ad(gv_), None,
                                  ad(gq_), ad(gqd_))
        return rc, L.rmx_last_error().decode()

    def refused(res, words):
        assert res[0] != 0 and words in res[1], res

    assert cost()[0] == 0 and frames()[0] == 0
    refused(cost(q_=None), "rmx_rollout_cost_frames: null argument")
    refused(cost(qd_=None), "rmx_rollout_cost_frames: null argument")
    refused(cost(cm=None), "rmx_rollout_cost_frames: null argument")
    refused(cost(ft=None), "rmx_rollout_cost_frames: null argument")                       # neither sc nor ft
    rc = L.rmx_rollout_cost_frames(None, N, ad(q), ad(qd), None, C.byref(terms()), C.byref(_abi.CostModel(ad(out["Jk"]), None, None)))
    assert rc != 0 and "rmx_rollout_cost_frames: null argument" in L.rmx_last_error().decode()
    refused(frames(q_=None), "rmx_rollout_frames: null argument")
    refused(frames(qd_=None), "rmx_rollout_frames: null argument")
    refused(frames(ft=None), "rmx_rollout_frames: null argument")
    refused(cost(cm=_abi.CostModel(None, None, None)), "rmx_rollout_cost_frames: all outputs are null")
    refused(frames(x_=None, gq_=None), "rmx_rollout_frames: all outputs are null")
    refused(frames(gx_=None), "gq needs gx, gv or gR")
    refused(frames(gqd_=gqd), "gqd needs gv")
    # a weight whose table is NULL: the message names the table
    refused(cost(ft=terms(x_=None)), "term 0: wpos > 0 needs xtarget, which is null")
    refused(cost(ft=terms(v_=None)), "term 0: wvel > 0 needs vtarget, which is null")
    refused(cost(ft=terms(R_=None)), "term 0: wrot > 0 needs Rtarget, which is null")
    refused(cost(ft=terms(per=2)), "per_rollout must be 0 or 1")
    refused(frames(ft=terms(per=-1)), "per_rollout must be 0 or 1")
    refused(cost(sc=_abi.StateCost(None, None, 2, 0)), "Q_per_rollout and goal_per_rollout must be 0 or 1")
    refused(cost(sc=_abi.StateCost(None, None, 0, 3)), "Q_per_rollout and goal_per_rollout must be 0 or 1")
    refused(cost(nsteps=0), "nsteps < 1")
    # rmx_track::plan_terms' own messages
    refused(cost(ft=terms(n=0)), "rmx_rollout_cost_frames: nterms < 1")
    refused(frames(ft=terms(a=None)), "rmx_rollout_frames: null terms")
    bad, _ = sim._frame_terms([dict(c["terms"][0], body=nr)], "test")
    refused(cost(ft=terms(n=1, a=bad)), "term 0: body %d is outside the listing of %d bodies" % (nr, nr))
    bad, _ = sim._frame_terms(c["terms"][:1] + [dict(c["terms"][1], step=N + 1)], "test")
    refused(frames(ft=terms(n=2, a=bad)), "term 1: step %d is outside [1, %d]" % (N + 1, N))
    # the weights: rmx_rollout_cost_frames alone reads them
    for name in ("wpos", "wvel", "wrot"):
        for w in (-1.0, float("nan"), float("inf")):
            bad, _ = sim._frame_terms(c["terms"][:2] + [dict(c["terms"][2], **{name: w})], "test")
            refused(cost(ft=terms(n=3, a=bad)), "rmx_rollout_cost_frames: term 2: %s must be finite and >= 0" % name)
            assert frames(ft=terms(n=3, a=bad))[0] == 0
    # the Python layer, in the words of its neighbours
    with pytest.raises(ValueError, match="rollout_cost_frames: q and qdot must have shape"):
        sim.rollout_cost_frames(N, c["q"][:, :-1], c["qd"], terms=c["terms"], xtarget=xt)
    with pytest.raises(ValueError, match="rollout_cost_frames: Rtarget must have shape"):
        sim.rollout_cost_frames(N, c["q"], c["qd"], terms=c["terms"], xtarget=xt, vtarget=vt, Rtarget=np.zeros((T, 9)))
    with pytest.raises(ValueError, match="rollout_frames: gR must have shape"):
        sim.rollout_frames(N, c["q"], c["qd"], c["terms"], gR=np.zeros((B, T, 9)))
    with pytest.raises(_abi.RedMaxHipError, match="rmx_rollout_cost_frames: null argument"):
        sim.rollout_cost_frames(N, c["q"], c["qd"])
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
    terms = [dict(body=0, xlocal=[0.0, 0.0, 0.0], step=1, wpos=1.0, wrot=1.0)]
    with pytest.raises(_abi.RedMaxHipError, match=words) as tape:
        sim.rollout_tape(2, sc.h, np.zeros((2, 2, sc.nr)))
    with pytest.raises(_abi.RedMaxHipError, match=words) as frm:
        sim.rollout_frames(2, q, q, terms)
    with pytest.raises(_abi.RedMaxHipError, match=words) as cst:
        sim.rollout_cost_frames(2, q, q, terms=terms, xtarget=np.zeros((1, 3)), Rtarget=np.eye(3)[None])
    tail = str(tape.value).split(": ", 1)[1]
    assert str(frm.value).split(": ", 1)[1] == tail and str(cst.value).split(": ", 1)[1] == tail
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
    rng = np.random.default_rng(97)
    q0, qd0 = sc.getQ()
    q = q0[None, None] + 0.1 * rng.standard_normal((2, N, nr))
    qd = qd0[None, None] + 0.1 * rng.standard_normal((2, N, nr))
    terms = frame_terms_of(m, N)
    T = len(terms)
    xt, vt = rng.standard_normal((T, 3)) * 10.0, rng.standard_normal((T, 3)) * 10.0
    Rt = np.array([F.rot(rng.standard_normal(3), rng.uniform(0.5, 2.0)) for _ in range(T)])
    cot = dict(gx=rng.standard_normal((2, T, 3)), gv=rng.standard_normal((2, T, 3)), gR=rng.standard_normal((2, T, 3, 3)))
    sim = BatchSim(sc, batch=2)
    with pytest.raises(_abi.RedMaxHipError, match="ground contact" if kind == "ground" else "point forces"):
        sim.rollout_tape(N, sc.h, np.zeros((2, N, nr)))
    fo, gq, gqd = sim.rollout_frames(N, q, qd, terms, **cot)
    out = sim.rollout_cost_frames(N, q, qd, terms=terms, xtarget=xt, vtarget=vt, Rtarget=Rt)
    sim.close()
    gpu = dict(fo, gq=gq, gqd=gqd, **out)
    res = {}
    for dtype in (np.float64, np.longdouble):      # the rule of section 1
        outs = [F.cost(m, q[b], qd[b], None, None, terms, xt, vt, Rt, dtype) for b in range(2)]
        r = {k: np.array([o[k] for o in outs]) for k in ("x", "v", "R", "Jk", "lx", "Q")}
        g = [F.pullback(m, q[b], qd[b], terms, cot["gx"][b], cot["gv"][b], cot["gR"][b], dtype) for b in range(2)]
        r["gq"], r["gqd"] = np.array([a for a, _ in g]), np.array([a for _, a in g])
        res[dtype] = r
    for name in QUANTITIES:
        e_ref, e_gpu = P.rel_err(res[np.float64][name], res[np.longdouble][name]), P.rel_err(gpu[name], res[np.longdouble][name])
        assert e_gpu <= 8 * max(e_ref, 16 * EPS), (kind, name, e_ref, e_gpu)
