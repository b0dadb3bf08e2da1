"""The plan of rmx_rollout_lqr_box (redmax_amd/csrc/rmx_select.h select_rollout_lqr_box), on the CPU: the LDS bytes of the box
kernel for every padded size, under the CU's limit, and the refusals of select_rollout_lqr."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS, REFUSED_NR, REFUSED_NODES = range(3)      # LqrKernel, in the order of the enum
CU_LDS = 160 * 1024                            # bytes of LDS of a CU of the MI355X


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(ROOT, "build", "lqrplan", "liblqr_box_plan_shim.so")
    src = os.path.join(ROOT, "tests", "lqrplan", "lqr_box_plan_shim.cpp")
    inc = os.path.join(ROOT, "redmax_amd", "csrc")
    deps = [src, os.path.join(inc, "rmx_select.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", inc, "-o", so, src])
    lib = C.CDLL(so)
    lib.lbp_label.restype = C.c_char_p
    lib.lbp_label_feedback.restype = C.c_char_p
    return lib


def _select(shim, NP, n, nr, big=False):
    block, lds, plain = C.c_int(-1), C.c_ulonglong(0), C.c_ulonglong(0)
    kernel = shim.lbp_select(NP, n, int(big), nr, C.byref(block), C.byref(lds))
    return kernel, block.value, lds.value, shim.lbp_select_plain(NP, n, int(big), nr, C.byref(plain)), plain.value


def test_every_padded_size_up_to_32_runs_the_box_kernel_with_its_own_lds(shim):
    assert shim.lbp_vectors() == 16 and shim.lbp_default_max_iter() == 64
    for NP, n, nr in ((4, 2, 2), (4, 3, 3), (8, 5, 5), (8, 5, 3), (16, 11, 11), (16, 16, 16), (32, 17, 17), (32, 32, 32), (32, 32, 1)):
        kernel, block, lds, plain_kernel, plain_lds = _select(shim, NP, n, nr)
        assert (kernel, block, plain_kernel) == (LDS, 256, LDS), (NP, n, nr)
        # 17 blocks of (NP + 1) * NP doubles and 16 vectors of NP doubles: the unconstrained kernel's and the 8 vectors of the QP
        assert lds == 8 * (17 * (NP + 1) * NP + 16 * NP) == plain_lds + 8 * 8 * NP, (NP, lds)
        assert lds <= CU_LDS
    assert {NP: _select(shim, NP, NP, NP)[2] for NP in (4, 8, 16, 32)} == {4: 3232, 8: 10816, 16: 39040, 32: 147712}


def test_the_refusals_are_those_of_the_unconstrained_sweep(shim):
    for NP, n, nr, big in ((64, 33, 33, False), (64, 40, 40, False), (64, 64, 64, False), (64, 128, 128, True), (64, 40, 20, False),
                           (64, 150, 30, True), (32, 32, 20, False), (32, 32, 32, False)):
        kernel, _, lds, plain_kernel, _ = _select(shim, NP, n, nr, big)
        assert kernel == plain_kernel, (NP, n, nr)
        assert (lds == 0) == (kernel != LDS)
    assert _select(shim, 64, 33, 33)[0] == REFUSED_NR and _select(shim, 64, 40, 20)[0] == REFUSED_NODES


def test_labels(shim):
    assert shim.lbp_label() == b"k_rollout_lqr<box>"
    assert shim.lbp_label_feedback(1) == b"k_adjoint_fwd<bdf1,tape,feedback,box>" and shim.lbp_label_feedback(2) == b"k_adjoint_fwd<bdf2,tape,feedback,box>"
