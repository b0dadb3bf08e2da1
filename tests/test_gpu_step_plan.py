"""The wiring of the step plan (redmax_amd/csrc/rmx_select.h -> launch_step -> the launchers) on the device: for one small model per row
of DESIGN.md's "Which kernel runs" table, under the environment that selects the row, rmx_last_step_kernel names the expected kernel
and 3 steps of 2 (3) rollouts land on the CPU oracle's states at the single-step bounds of tests/test_gpu_parity.py
(|dq| <= 1e-11 |q| + 1e-10, |dqdot| <= 1e-9 |qdot| + 1e-8).  The tick counters are per call whether a kernel stores or adds them."""
import functools

import numpy as np
import pytest

import proto_point_forces as pf
from redmax_amd.scenes import sceneChain, sceneChainGround, sceneChainSprings, scenesRedMax, sceneTree, syntheticStates

pytestmark = pytest.mark.gpu

NSTEPS = 3
KNOBS = ("RMX_PARK_HALVINGS", "RMX_COOP_MAP", "RMX_W2_RUNAHEAD", "RMX_PAIRC", "RMX_GROUND_FUSED", "RMX_ADJ_HELP",
         "RMX_GCONST_MIN", "RMX_W2_MAX", "RMX_W2C_MIN", "RMX_TREE_SOLVE", "RMX_BIG_LDS_LIMIT")


def _close(a, b, rtol, atol):
    return np.linalg.norm(a - b) <= rtol * np.linalg.norm(b) + atol


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name.startswith("chainsprings"):
        sc = sceneChainSprings(int(name[12:]))
    elif name.startswith("chainground"):
        sc = sceneChainGround(int(name[11:]), ground_z=-0.6)
    elif name.startswith("chain"):
        sc = sceneChain(int(name[5:]))
    elif name.startswith("tree"):
        sc = sceneTree(int(name[4:]))
    else:
        sc = scenesRedMax(int(name))
    sc.init()
    return sc


def _states(name, B):
    sc = _scene(name)
    if name.startswith("chainground"):
        # near horizontal: rollout 0 stays in free flight; the others are tilted about the root so that their far links start in the
        # ground and the steps with the contact terms run from the first step on (the oracle's end state differs by 5e-4 .. 8e-4
        # from the same chain's without a ground)
        rng = np.random.default_rng(77)
        q, qd = 1e-3 * rng.normal(size=(B, sc.nr)), 0.05 * rng.normal(size=(B, sc.nr))
        q[1:, 0] += 0.25 / sc.nr * np.arange(1, B)
        return q, qd
    if name == "7":      # two spherical joints: around the scene's own state
        q0, qd0 = sc.getQ()
        rng = np.random.default_rng(3)
        return q0[None, :] + 0.05 * rng.standard_normal((B, sc.nr)), qd0[None, :] + 0.2 * rng.standard_normal((B, sc.nr))
    return syntheticStates(sc.nr, B)


@functools.lru_cache(maxsize=None)
def _reference_one(name, integ, B, b):
    """(q, qdot) of rollout b after NSTEPS steps on the CPU: the literal oracle; the numpy restatement for the scene with point forces;
    for the 72-link chain the tensor-free CPU code in the kernels' iterate mode (on plain doubles the literal oracle cannot meet
    tol = 1e-9 on a 720 cm cgs chain and takes minutes trying: tests/test_gpu_big_trees.py).  Computed once per rollout and shared by
    the cases that differ in the environment only."""
    from oracle import oracle as orc
    orc.build()
    sc = _scene(name)
    q, qd = _states(name, B)
    if name.startswith("chainsprings"):
        lit = pf.Literal(orc, sc)
        qo, qdo, st, _ = pf.sim_loop(lit.eval, lit.energy, q[b], qd[b], sc.h, NSTEPS, integ, history=True)
        assert st == 0
    elif name == "chain72":
        assert integ == 1
        qo, qdo = np.ascontiguousarray(q[b:b + 1]), np.ascontiguousarray(qd[b:b + 1])
        ref = orc.tensorfree_batch_step_bdf1(sc.desc(), qo, qdo, sc.h, NSTEPS, nthreads=1, tol=1e-9, compensated=True)
        assert (ref["status"] & 15 == 0).all()
        qo, qdo = qo[0], qdo[0]
    else:
        o = orc.Oracle(sc.desc())
        o.set_state(q[b], qd[b])
        st = (o.step_bdf1 if integ == 1 else o.step_bdf2)(sc.h, NSTEPS)
        assert st.diverged == 0 and st.not_converged == 0      # the reference algorithm itself converged on this state
        qo, qdo = o.get_state()
    return np.array(qo), np.array(qdo)


def _reference(name, integ, B):
    # (the states of rollouts 0 .. B - 1 do not depend on B: a batch of 3 shares the first two with the batch of 2)
    return [_reference_one(name, integ, 2 if b < 2 else B, b) for b in range(B)]


# (scene, integrator, environment, batch, label); B = 3 where a batch threshold set in the environment has to be reached
CASES = [
    ("chain3", 1, {}, 2, "k_step_bdf1<4>"),
    ("chain3", 2, {}, 2, "k_step_bdf2<4>"),
    ("chain16", 1, {}, 2, "k_step_bdf1<16,fullchain>"),
    ("chain16", 2, {}, 2, "k_step_bdf2<16,fullchain>"),
    ("chain32", 1, {}, 2, "k_step_bdf1_pair32"),
    ("chain32", 1, {"RMX_PAIRC": "0"}, 2, "k_step_bdf1<32,fullchain>"),
    ("chain32", 1, {"RMX_PAIRC": "0", "RMX_W2C_MIN": "2"}, 3, "k_step_bdf1<32,fullchain,w2>"),
    ("chain32", 2, {}, 2, "k_step_bdf2<32,fullchain>"),
    ("tree64", 1, {}, 2, "k_step_bdf1<64,w2>"),
    ("tree64", 2, {}, 2, "k_step_bdf2<64,w2>"),
    ("tree64", 1, {"RMX_W2_MAX": "0"}, 2, "k_step_bdf1<64,fulln>"),
    ("tree64", 2, {"RMX_W2_MAX": "0"}, 2, "k_step_bdf2<64,fulln>"),
    ("tree64", 1, {"RMX_W2_MAX": "0", "RMX_GCONST_MIN": "2"}, 3, "k_step_bdf1<64,gconst>"),
    ("tree64", 2, {"RMX_W2_MAX": "0", "RMX_GCONST_MIN": "2"}, 3, "k_step_bdf2<64,gconst>"),
    ("tree40", 1, {"RMX_W2_MAX": "0"}, 2, "k_step_bdf1<64>"),
    ("7", 1, {}, 2, "k_step_bdf1<8,ct>"),
    ("7", 2, {}, 2, "k_step_bdf2<8,ct>"),
    # the kernels around newton_pair are built for 32 lanes: the smallest chain that reaches them has 17 links (an 8-link chain pads to
    # 8 lanes and runs the lean launch and the launch with the contact terms of its own size)
    ("chainground17", 2, {}, 2, "k_ground32"),
    ("chainground17", 2, {"RMX_GROUND_FUSED": "0"}, 2, "k_step_pair"),
    ("chainground17", 2, {"RMX_PARK_HALVINGS": "0"}, 2, "k_ground32"),
    ("chainground8", 2, {}, 2, "k_step_bdf2<8,ct>"),
    ("chainsprings8", 1, {}, 2, "k_step_pf<8,bdf1>"),
    ("chain72", 1, {}, 2, "k_big_step"),
]


def _clean_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name,integ,env,B,label", CASES, ids=["%s-bdf%d-%s" % (c[0], c[1], "+".join("%s=%s" % kv for kv in c[2].items()) or "default") for c in CASES])
def test_plan_reaches_the_kernel(monkeypatch, name, integ, env, B, label):
    from redmax_amd import BatchSim
    _clean_env(monkeypatch, env)          # (before the model is created: the thresholds are read there)
    sc = _scene(name)
    q, qd = _states(name, B)
    sim = BatchSim(sc, batch=B)
    sim.set_state(q, qd)
    out = (sim.step_bdf1 if integ == 1 else sim.step_bdf2)(NSTEPS, h=sc.h, stats=True)
    kernel = sim.last_step_kernel()
    qg, qdg = sim.get_state()
    sim.close()
    print("%s BDF%d %s: kernel %s, status %s" % (name, integ, env, kernel, out["status"]))
    assert kernel == label
    assert (out["status"] & 15 == 0).all(), out["status"]
    ref = _reference(name, integ, B)
    for b in range(B):
        qo, qdo = ref[b]
        dq, dqd = np.linalg.norm(qg[b] - qo), np.linalg.norm(qdg[b] - qdo)
        print("   b=%d: |dq| = %.3e (bound %.3e), |dqdot| = %.3e (bound %.3e)" % (
            b, dq, 1e-11 * np.linalg.norm(qo) + 1e-10, dqd, 1e-9 * np.linalg.norm(qdo) + 1e-8))
    for b in range(B):
        qo, qdo = ref[b]
        assert _close(qg[b], qo, 1e-11, 1e-10), (name, integ, b)
        assert _close(qdg[b], qdo, 1e-9, 1e-8), (name, integ, b)


@pytest.mark.parametrize("name,label", [("chain32", "k_step_bdf1_pair32"), ("chain16", "k_step_bdf1<16,fullchain>")], ids=["storing", "adding"])
def test_ticks_are_per_call(monkeypatch, name, label):
    """rmx_step_ticks counts ONE call, for the kernel that stores its count (no fill ahead of it) and for one that adds to it (fill
    ahead): after a warm-up call, two identical calls from the same state.  The work is deterministic, so the second count is the
    first one's; a counter that accumulated across calls would read at least twice that - 1.5 is the midpoint."""
    from redmax_amd import BatchSim
    _clean_env(monkeypatch, {})
    sc = _scene(name)
    B = 2
    q, qd = _states(name, B)
    sim = BatchSim(sc, batch=B)
    ticks = []
    for call in range(3):      # (0: warm-up)
        sim.set_state(q, qd)
        sim.step_bdf1(NSTEPS, h=sc.h)
        assert sim.last_step_kernel() == label
        ticks.append(sim.step_ticks().astype(np.float64))
    sim.close()
    print("%s ticks: warm-up %s, first %s, second %s" % (label, ticks[0], ticks[1], ticks[2]))
    assert (ticks[2] > 0).all()
    assert (ticks[2] <= 1.5 * ticks[1]).all()
