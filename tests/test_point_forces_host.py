"""Host side of the body-to-body forces (no device needed): the reference's class surface, the rest lengths Scene.init computes,
desc() and the ctypes hand-over, what is refused before a device is touched, and that the kernels of force-free models are the
code they were (the fingerprints the roofline calibrations were measured on)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from redmax_amd import _abi, se3
from redmax_amd.redmax import (PF_CABLE, PF_POINTPOINT, PF_SPRINGDAMPER, BodyCuboid, ForceCable, ForcePointPoint, ForceSpringDamper,
                               JointRevolute, Scene)
from redmax_amd.scenes import (COMPOSITE_SCENES, IN_SCOPE_SCENES, POINT_FORCE_SCENES, SPHERICAL_SCENES, sceneChain, sceneChainSprings,
                               scenesRedMax)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_lists_keep_their_values():
    assert IN_SCOPE_SCENES == (0, 1, 2, 3, 14)
    assert COMPOSITE_SCENES == (4, 5, 6, 8)
    assert SPHERICAL_SCENES == (7, 9)
    assert POINT_FORCE_SCENES == (10, 12, 13)


def test_class_surface_and_defaults():
    b = BodyCuboid(1.0, [1, 1, 1])
    pp = ForcePointPoint(b, [0, 0, 1], None, [1, 2, 3])
    assert (pp.stiffness, pp.damping, pp.kind) == (1.0, 0.0, PF_POINTPOINT)          # ForcePointPoint.m:32-33
    sd = ForceSpringDamper([], [0, 0, 0], b, [0, 0, 1])                              # MATLAB's [] is the world
    assert (sd.stiffness, sd.damping, sd.L, sd.kind) == (1.0, 1.0, 0.0, PF_SPRINGDAMPER) and sd.bodies[0] is None
    sd.setStiffness(5)
    sd.setDamping(6)
    sd.setRetLength(7)
    assert (sd.stiffness, sd.damping, sd.L) == (5.0, 6.0, 7.0)
    c = ForceCable()
    c.addBodyPoint(b, [0, 0, 0])
    c.addBodyPoint(None, [1, 0, 0])
    assert (c.stiffness, c.damping, c.L, c.kind, len(c.xls)) == (1.0, 1.0, 0.0, PF_CABLE, 2)


@pytest.mark.parametrize("sid", POINT_FORCE_SCENES)
def test_rest_lengths_are_the_initial_polyline_lengths(sid):
    sc = scenesRedMax(sid)
    sc.init()
    E = sc.bodyTransforms()
    idx = {id(b): i for i, b in enumerate(sc.bodies)}
    for f, d in zip(sc.pointForces(), sc.desc()["point_forces"]):
        xw = [x if b is None else E[idx[id(b)]][:3, :3] @ x + E[idx[id(b)]][:3, 3] for b, x in zip(f.bodies, f.xls)]
        l0 = sum(np.linalg.norm(xw[k + 1] - xw[k]) for k in range(len(xw) - 1))
        if f.kind == PF_POINTPOINT:
            assert f.L == 0.0
        else:
            assert f.L == pytest.approx(l0, rel=1e-15) and f.L > 0
        assert d["kind"] == f.kind and d["L"] == f.L and d["stiffness"] == f.stiffness and d["damping"] == f.damping
        assert list(d["body"]) == [-1 if b is None else idx[id(b)] for b in f.bodies]
        assert np.array_equal(d["x"], np.stack(f.xls))
    # known values: scene 12's world-anchored spring, scene 13's cable at q = (pi/2, -pi/2)
    if sid == 12:
        assert sc.pointForces()[0].L == pytest.approx(np.linalg.norm([15 + 5, 0, -2 + 5]), rel=1e-15)
        assert sc.pointForces()[1].L == pytest.approx(10.0, rel=1e-15)
    if sid == 10:
        assert [j.idxR for j in sc.joints] == [[], [3], [2], [1], [0]]              # listed depth-first: joints 1, 2, 4, 5, 3


def test_body_transforms_follow_the_joints():
    sc = sceneChain(3, q0=0.3)
    sc.init()
    E = sc.bodyTransforms()
    R = se3.aaToMat([0, 1, 0], 0.3)
    assert np.allclose(E[0][:3, 3], R @ [5, 0, 0], atol=1e-15)
    assert np.allclose(E[1][:3, :3], R @ R, atol=1e-15)
    assert np.allclose(E[1][:3, 3], R @ [10, 0, 0] + R @ R @ [5, 0, 0], atol=1e-14)


def test_set_ret_length_wins_over_the_initial_length():
    sc = scenesRedMax(12)
    sc.forces[0].setRetLength(3.25)
    sc.init()
    assert sc.forces[0].L == 3.25 and sc.forces[1].L == pytest.approx(10.0)


def test_desc_is_ignored_by_existing_consumers_and_round_trips(oracle_lib):
    sc = scenesRedMax(13)
    sc.init()
    d = sc.desc()
    assert "contact" not in d and len(d["point_forces"]) == 1
    plain = scenesRedMax(13)
    plain.forces = []
    plain.init()
    o1, o2 = oracle_lib.Oracle(d), oracle_lib.Oracle(plain.desc())                   # the oracle knows nothing of these forces
    q, qd = sc.getQ()
    g1 = o1.eval_bdf1(q, q, qd, sc.h, want_H=False)
    g2 = o2.eval_bdf1(q, q, qd, sc.h, want_H=False)
    assert np.array_equal(g1, g2)
    keep = {}
    arr, n = _abi.make_point_forces(d, keep)
    assert n == 1 and arr[0].kind == PF_CABLE and arr[0].npts == 3
    assert [arr[0].body[k] for k in range(3)] == [3, 1, 2]
    assert [arr[0].x[k] for k in range(9)] == [0, 0, 0, -4, 0, 1, -4, 0, 1]
    assert (arr[0].stiffness, arr[0].damping, arr[0].L) == (1e6, 1e3, sc.forces[0].L)
    assert _abi.make_point_forces(plain.desc(), {}) == (None, 0)
    assert C.sizeof(_abi.PointForce) == 48                                           # int, int, two pointers, three doubles


def test_ground_contact_and_point_forces_are_described_side_by_side():
    from redmax_amd.scenes import sceneChainGround
    sc = sceneChainGround(4, ground_z=-1.0)
    sc.forces.append(ForcePointPoint(sc.bodies[0], [0, 0, 0], sc.bodies[3], [0, 0, 0]))
    sc.init()
    d = sc.desc()
    assert list(d["contact"]) == [1, 1, 1, 1] and len(d["point_forces"]) == 1 and d["njoints"] == 4


def test_scene_init_refuses_what_it_cannot_describe():
    sc = sceneChain(3)
    c = ForceCable()
    c.addBodyPoint(sc.bodies[0], [0, 0, 0])
    sc.forces = [c]
    with pytest.raises(ValueError, match="at least two points"):
        sc.init()
    sc = sceneChain(3)
    sc.forces = [ForcePointPoint(sc.bodies[0], [0, 0, 0], BodyCuboid(1.0, [1, 1, 1]), [0, 0, 0])]
    with pytest.raises(ValueError, match="body of this scene"):
        sc.init()
    sc = sceneChain(3)
    sc.forces = [ForceSpringDamper(sc.bodies[0], [1, 0, 0], sc.bodies[0], [1, 0, 0])]
    with pytest.raises(ValueError, match="initial length is zero"):
        sc.init()
    sc = scenesRedMax(7)                                                             # JointSpherical
    sc.forces = [ForceSpringDamper(None, [0, 0, 0], sc.bodies[-1], [0, 0, 1])]
    with pytest.raises(NotImplementedError, match="JointSpherical"):
        sc.init()

    class Other:
        pass
    sc = sceneChain(3)
    sc.forces = [Other()]
    with pytest.raises(NotImplementedError, match="not in scope"):
        sc.init()


def test_group_sim_refuses_point_forces():
    from redmax_amd import GroupSim, RedMaxHipError
    sc = scenesRedMax(12)
    sc.init()
    with pytest.raises(RedMaxHipError, match="no slot for point forces"):
        GroupSim(sc, batch=2)


def test_chain_springs_scene():
    sc = sceneChainSprings(32)
    sc.init()
    kinds = [f["kind"] for f in sc.desc()["point_forces"]]
    assert kinds == [PF_SPRINGDAMPER, PF_POINTPOINT, PF_CABLE]
    assert list(sc.desc()["point_forces"][0]["body"]) == [-1, 31]
    assert list(sc.desc()["point_forces"][1]["body"]) == [16, 24]
    assert len(sc.desc()["point_forces"][2]["body"]) == 3 and sc.nr == 32


def test_header_declares_the_limits_the_kernels_use():
    hdr = open(os.path.join(ROOT, "include", "redmax_hip.h")).read()
    assert "RMX_PF_MAX_FORCES = 32, RMX_PF_MAX_POINTS = 8, RMX_PF_MAX_TOTAL = 128" in hdr
    assert "int rmx_model_set_point_forces(rmx_model* m, const rmx_point_force* f, int nforces);" in hdr
    assert "rmx_model_set_point_forces" in _abi.SYMBOLS


def test_driver_lists_all_fifteen_scenes():
    src = open(os.path.join(ROOT, "redmax_amd", "driver.py")).read()
    assert "default=list(range(15))" in src


def test_kernels_of_force_free_models_are_unchanged():
    """After build(): every kernel a roofline calibration was measured on has the opcode hash it was measured with (the values
    of the parent commit), so bench.py reports no calibration_stale - the point-force kernels are new symbols only."""
    import bench
    fp_file = os.path.join(ROOT, "redmax_amd", "kernel_fingerprint.json")
    if not os.path.exists(fp_file):
        import __graft_entry__ as g
        g.build()
    cal = json.load(open(os.path.join(ROOT, "profiles", "roofline_calibration.json")))
    fp = json.load(open(fp_file))
    checked = 0
    for key, ent in cal["workloads"].items():
        assert bench.load_calibration(key)[1] is None, (key, bench.load_calibration(key)[1])
        for sym, sha in ent["fingerprints"].items():
            assert fp[sym]["opcode_sha16"] == sha, sym
            checked += 1
    assert checked >= 7
    new = [s for s in fp if "k_step_pf" in s or "k_eval_pf" in s or "k_energy_pf" in s]
    assert len(new) == 25                                                            # 5 sizes x (2 step + 2 eval + 1 energy)
