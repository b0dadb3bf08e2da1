"""The kernel choice of rmx_rollout_tape_feedback (redmax_amd/csrc/rmx_select.h select_rollout_feedback), on the CPU: always the
generic one-wavefront kernel - also for the models and batches whose open-loop taped rollout takes the helper wave or the full-chain
instantiation - with a label of its own per integrator."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELP16, FULLCHAIN16, GENERIC = range(3)      # AdjKernel, in the order of the enum


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(ROOT, "build", "stepplan", "libfeedback_plan_shim.so")
    src = os.path.join(ROOT, "tests", "stepplan", "feedback_plan_shim.cpp")
    inc = os.path.join(ROOT, "redmax_amd", "csrc")
    deps = [src, os.path.join(inc, "rmx_select.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", inc, "-o", so, src])
    L = C.CDLL(so)
    L.fp_select.restype = C.c_char_p
    return L


def test_feedback_rollout_is_always_the_generic_kernel(shim):
    seen = set()
    for NP, n, chain in ((4, 3, True), (8, 5, True), (8, 7, False), (16, 11, True), (16, 16, True), (16, 16, False), (32, 32, True), (64, 40, True)):
        for B in (1, 3, 512, 513, 4096):
            for integ in (1, 2):
                for help_ in (0, 1):
                    kernel, fc = C.c_int(-1), C.c_int(-1)
                    label = shim.fp_select(NP, n, int(chain), 512, B, integ, help_, C.byref(kernel), C.byref(fc)).decode()
                    assert (kernel.value, fc.value) == (GENERIC, 0), (NP, n, chain, B, integ, help_)
                    assert label == ("k_adjoint_fwd<bdf1,tape,feedback>" if integ == 1 else "k_adjoint_fwd<bdf2,tape,feedback>")
                    seen.add(shim.fp_select_tape(NP, n, int(chain), 512, B, integ, help_))
    assert seen == {HELP16, FULLCHAIN16, GENERIC}       # (the open-loop plans the cases cover: all three)
