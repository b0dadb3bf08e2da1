"""The plan of rmx_rollout_lqr (redmax_amd/csrc/rmx_select.h select_rollout_lqr), on the CPU: the LDS-resident kernel for every
padded size up to 32 with the LDS it asks for, a refusal that names nr above 32 reduced DOFs, and a refusal of its own for a tree of
more than 32 nodes whose reduced DOFs would fit."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS, REFUSED_NR, REFUSED_NODES = range(3)      # LqrKernel, in the order of the enum
CU_LDS = 160 * 1024                            # bytes of LDS of a CU of the MI355X


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(ROOT, "build", "lqrplan", "liblqr_plan_shim.so")
    src = os.path.join(ROOT, "tests", "lqrplan", "lqr_plan_shim.cpp")
    inc = os.path.join(ROOT, "redmax_amd", "csrc")
    deps = [src, os.path.join(inc, "rmx_select.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", inc, "-o", so, src])
    return C.CDLL(so)


def _select(shim, NP, n, nr, big=False):
    block, lds = C.c_int(-1), C.c_ulonglong(0)
    kernel = shim.lp_select(NP, n, int(big), nr, C.byref(block), C.byref(lds))
    return kernel, block.value, lds.value


def test_every_padded_size_up_to_32_runs_the_lds_kernel(shim):
    assert shim.lp_max_nr() == 32
    for NP, n, nr in ((4, 2, 2), (4, 4, 4), (8, 5, 5), (8, 7, 7), (16, 16, 16), (16, 11, 9), (32, 17, 17), (32, 32, 32), (32, 32, 1)):
        kernel, block, lds = _select(shim, NP, n, nr)
        assert (kernel, block) == (LDS, 256), (NP, n, nr)
        # 17 blocks of (NP + 1) * NP doubles and 8 vectors of NP doubles (the header comment of rmx_lqr.h)
        assert lds == 8 * (17 * (NP + 1) * NP + 8 * NP), (NP, lds)
        assert lds <= CU_LDS
    assert _select(shim, 32, 32, 32)[2] == 145664      # the headline chain: 143 616 bytes of blocks + 2 048 of vectors


def test_more_than_32_reduced_dofs_are_refused(shim):
    for NP, n, nr, big in ((64, 33, 33, False), (64, 40, 40, False), (64, 64, 64, False), (64, 128, 128, True)):
        kernel, _, lds = _select(shim, NP, n, nr, big)
        assert (kernel, lds) == (REFUSED_NR, 0), (NP, n, nr)


def test_a_tree_of_more_than_32_nodes_is_refused_even_where_nr_fits(shim):
    assert _select(shim, 64, 40, 20)[0] == REFUSED_NODES      # (fixed joints: the elimination runs at the padded size of the nodes)
    assert _select(shim, 64, 150, 30, big=True)[0] == REFUSED_NODES
    assert _select(shim, 32, 32, 20)[0] == LDS
