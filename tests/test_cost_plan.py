"""The plan of rmx_rollout_points / rmx_rollout_cost (redmax_amd/csrc/rmx_select.h select_rollout_cost), on the CPU: one wavefront
per (rollout, step) in the object of the model's padded size, 64 included; ground contact and point forces do not enter kinematics
and are taken; spherical joints, trees of more than 64 nodes and a grid of more than 2^31 - 1 wavefronts are refused."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE, REFUSED_SPHERICAL, REFUSED_NODES, REFUSED_GRID = range(4)      # CostKernel, in the order of the enum


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(ROOT, "build", "costplan", "libcost_plan_shim.so")
    src = os.path.join(ROOT, "tests", "costplan", "cost_plan_shim.cpp")
    inc = os.path.join(ROOT, "redmax_amd", "csrc")
    deps = [src, os.path.join(inc, "rmx_select.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", inc, "-o", so, src])
    shim = C.CDLL(so)
    shim.cp_max_grid.restype = C.c_ulonglong
    return shim


def _select(shim, NP, n, B=3, nsteps=4, big=False, spherical=False, contact=False, point_forces=False):
    np_, block, grid = C.c_int(-1), C.c_int(-1), C.c_ulonglong(0)
    kernel = shim.cp_select(NP, n, int(big), int(spherical), int(contact), int(point_forces), B, nsteps, C.byref(np_), C.byref(block),
                            C.byref(grid))
    return kernel, np_.value, block.value, grid.value


def test_every_padded_size_runs_its_own_object_one_wavefront_per_rollout_and_step(shim):
    for NP, n in ((4, 2), (4, 4), (8, 5), (8, 7), (16, 11), (16, 16), (32, 17), (32, 32), (64, 33), (64, 64)):
        assert _select(shim, NP, n) == (WAVE, NP, 64, 12), (NP, n)
    assert _select(shim, 32, 32, B=1024, nsteps=100) == (WAVE, 32, 64, 102400)


def test_contact_and_point_forces_do_not_enter_kinematics(shim):
    assert _select(shim, 32, 32, contact=True) == (WAVE, 32, 64, 12)
    assert _select(shim, 16, 15, point_forces=True) == (WAVE, 16, 64, 12)


def test_spherical_joints_and_big_trees_are_refused(shim):
    assert _select(shim, 8, 6, spherical=True)[0] == REFUSED_SPHERICAL
    assert _select(shim, 64, 128, big=True)[0] == REFUSED_NODES
    assert _select(shim, 8, 6, spherical=True)[3] == 0 and _select(shim, 64, 128, big=True)[3] == 0


def test_the_grid_limit(shim):
    top = shim.cp_max_grid()
    assert top == 2 ** 31 - 1
    assert _select(shim, 8, 5, B=1 << 16, nsteps=(1 << 15) - 1) == (WAVE, 8, 64, (1 << 16) * ((1 << 15) - 1))
    assert _select(shim, 8, 5, B=1 << 16, nsteps=1 << 15)[0] == REFUSED_GRID
    assert _select(shim, 8, 5, B=3, nsteps=0)[0] == REFUSED_GRID
