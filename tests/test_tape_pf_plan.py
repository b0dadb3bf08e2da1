"""The plan of the taped rollouts of a model with point forces (redmax_amd/csrc/rmx_select.h select_rollout_tape_pf), on the CPU:
always the one-wavefront kernel of the model's padded size, for both integrators, with or without the feedback stage - whatever
the tree is (a full chain, a tree the helper-wave form would take) - under the four labels rmx_last_step_kernel reports; and its
refusals."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE, REFUSED = range(2)      # TapePfKernel, in the order of the enum
BDF1, BDF2 = 1, 2
LABELS = {(BDF1, 0): b"k_adjoint_fwd<bdf1,tape,pf>", (BDF2, 0): b"k_adjoint_fwd<bdf2,tape,pf>",
          (BDF1, 1): b"k_adjoint_fwd<bdf1,tape,feedback,pf>", (BDF2, 1): b"k_adjoint_fwd<bdf2,tape,feedback,pf>"}


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(ROOT, "build", "stepplan", "libtape_pf_plan_shim.so")
    src = os.path.join(ROOT, "tests", "stepplan", "tape_pf_plan_shim.cpp")
    inc = os.path.join(ROOT, "redmax_amd", "csrc")
    deps = [src, os.path.join(inc, "rmx_select.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", inc, "-o", so, src])
    lib = C.CDLL(so)
    lib.tp_select.restype = C.c_char_p
    lib.tp_label.restype = C.c_char_p
    return lib


def _select(shim, NP, n, integ, feedback, chain=False, pf=True, big=False, contact=False, sph=False, adj_max=0):
    kernel, out = C.c_int(-1), (C.c_int * 3)(-1, -1, -1)
    label = shim.tp_select(NP, n, int(chain), int(pf), int(big), int(contact), int(sph), adj_max, integ, int(feedback), C.byref(kernel), out)
    return kernel.value, label, tuple(out)


def test_every_size_integrator_and_loop_runs_the_one_wavefront_kernel(shim):
    for NP, n in ((4, 2), (4, 4), (8, 5), (8, 8), (16, 9), (16, 16), (32, 17), (32, 32), (64, 33), (64, 64)):
        for integ in (BDF1, BDF2):
            for fb in (0, 1):
                assert _select(shim, NP, n, integ, fb) == (WAVE, LABELS[(integ, fb)], (NP, fb, 64)), (NP, n, integ, fb)


def test_neither_the_full_chain_nor_the_helper_wave_changes_the_plan(shim):
    """H is dense: the full 16-link chain and a batch the helper-wave form would take run the same kernel as any tree."""
    want = (WAVE, LABELS[(BDF1, 0)], (16, 0, 64))
    assert _select(shim, 16, 16, BDF1, 0, chain=True) == want
    assert _select(shim, 16, 11, BDF1, 0, adj_max=512) == want
    assert _select(shim, 16, 16, BDF1, 0, chain=True, adj_max=512) == want
    assert _select(shim, 32, 32, BDF2, 1, chain=True) == (WAVE, LABELS[(BDF2, 1)], (32, 1, 64))


def test_refusals(shim):
    assert _select(shim, 8, 5, BDF1, 0, pf=False)[0] == REFUSED          # no force table: the other plans' business
    assert _select(shim, 64, 128, BDF1, 0, big=True)[0] == REFUSED
    assert _select(shim, 32, 20, BDF1, 0, contact=True)[0] == REFUSED
    assert _select(shim, 32, 20, BDF2, 1, sph=True)[0] == REFUSED
    assert _select(shim, 8, 5, 3, 0)[0] == REFUSED                       # not an integrator
    assert _select(shim, 8, 5, 3, 0)[1] == b""


def test_labels(shim):
    for (integ, fb), label in LABELS.items():
        assert shim.tp_label(integ, fb) == label
