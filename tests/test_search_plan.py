"""The plan of rmx_rollout_search (redmax_amd/csrc/rmx_select.h select_rollout_search), on the CPU: one wavefront per rollout at
every padded size the Riccati sweep exists for, and that sweep's refusals."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE, REFUSED_NR, REFUSED_NODES = range(3)      # SearchKernel, in the order of the enum


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(ROOT, "build", "stepplan", "libsearch_plan_shim.so")
    src = os.path.join(ROOT, "tests", "stepplan", "search_plan_shim.cpp")
    inc = os.path.join(ROOT, "redmax_amd", "csrc")
    deps = [src, os.path.join(inc, "rmx_select.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", inc, "-o", so, src])
    lib = C.CDLL(so)
    lib.sp_label.restype = C.c_char_p
    return lib


def _select(shim, NP, n, nr, big=False):
    np_, block = C.c_int(-1), C.c_int(-1)
    kernel = shim.sp_select(NP, n, int(big), nr, C.byref(np_), C.byref(block))
    return kernel, np_.value, block.value


def test_every_padded_size_up_to_32_runs_one_wavefront_per_rollout(shim):
    for NP, n, nr in ((4, 2, 2), (4, 3, 3), (8, 5, 5), (8, 5, 3), (16, 11, 11), (16, 16, 16), (32, 17, 17), (32, 32, 32), (32, 32, 1)):
        assert _select(shim, NP, n, nr) == (WAVE, NP, 64), (NP, n, nr)


def test_nr_33_is_refused(shim):
    assert _select(shim, 64, 33, 33)[0] == REFUSED_NR
    assert _select(shim, 64, 64, 64)[0] == REFUSED_NR and _select(shim, 64, 128, 128, True)[0] == REFUSED_NR


def test_a_40_node_tree_with_few_dofs_is_refused(shim):
    assert _select(shim, 64, 40, 20)[0] == REFUSED_NODES
    assert _select(shim, 64, 150, 30, True)[0] == REFUSED_NODES


def test_label_and_alphas(shim):
    assert shim.sp_label() == b"k_rollout_search<bdf1,tape,feedback>"
    assert shim.sp_max_alphas() == 16
