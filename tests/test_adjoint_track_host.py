"""rmx_adjoint_track, the checks that need no GPU: the term plan (redmax_amd/csrc/rmx_track.h behind tests/trackplan/track_plan_shim.cpp,
plain g++), the MEX command's place in the gateway, and the scratch the TRK instantiations take next to their CTL siblings."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from test_mex_gateway import MexError, gw  # noqa: F401  (gw: the fixture that builds and loads the gateway stub)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(ROOT, "build", "trackplan", "libtrack_plan_shim.so")
    src = os.path.join(ROOT, "tests", "trackplan", "track_plan_shim.cpp")
    inc = os.path.join(ROOT, "redmax_amd", "csrc")
    abi = os.path.join(ROOT, "include")
    deps = [src, os.path.join(inc, "rmx_track.h"), os.path.join(abi, "redmax_hip.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", inc, "-I", abi, "-o", so, src])
    return C.CDLL(so)


def plan(L, terms, nsteps, node_of_listing, null_terms=False):
    """terms: [(body, step, wpos, xlocal)].  Returns the sorted table as a dict, or the refusal's text."""
    n = len(terms)
    ia = lambda v: (C.c_int * max(len(v), 1))(*v)          # noqa: E731
    da = lambda v: (C.c_double * max(len(v), 1))(*v)       # noqa: E731
    node, orig, begin = ia([0] * n), ia([0] * n), ia([0] * (nsteps + 1 if nsteps > 0 else 1))
    wout, xout = da([0.0] * n), da([0.0] * 3 * n)
    err = C.create_string_buffer(256)
    rc = L.tp_plan(n, ia([t[0] for t in terms]), ia([t[1] for t in terms]), da([t[2] for t in terms]),
                   da([x for t in terms for x in t[3]]), nsteps, len(node_of_listing), ia(node_of_listing), int(null_terms),
                   node, orig, wout, xout, begin, err, len(err))
    if rc:
        return err.value.decode()
    return dict(node=list(node)[:n], orig=list(orig)[:n], wpos=list(wout)[:n], xl=np.array(list(xout)[:3 * n]).reshape(n, 3),
                begin=list(begin)[:nsteps + 1])


XL = (5.0, 0.5, 0.25)


def test_plan_sorts_by_step_and_keeps_the_callers_order_within_a_step(shim):
    ident = list(range(6))
    #        index:   0             1             2             3             4             5             6
    terms = [(5, 4, 1.0, XL), (5, 2, 0.5, XL), (3, 2, 2.0, XL), (0, 1, 1.5, XL), (3, 4, 0.25, XL), (5, 4, 3.0, XL), (1, 2, 7.0, XL)]
    p = plan(shim, terms, 6, ident)
    assert p["orig"] == [3, 1, 2, 6, 0, 4, 5]                       # stable: 1, 2, 6 on step 2 and 0, 4, 5 on step 4 in the caller's order
    assert p["begin"] == [0, 1, 4, 4, 7, 7, 7]                      # step 3 and the steps behind the last term own nothing
    assert p["node"] == [terms[i][0] for i in p["orig"]]
    assert p["wpos"] == [terms[i][2] for i in p["orig"]]
    assert np.array_equal(p["xl"], np.array([terms[i][3] for i in p["orig"]]))


def test_plan_of_one_term_and_of_a_term_on_every_step(shim):
    p = plan(shim, [(2, 3, 1.0, XL)], 3, [0, 1, 2])
    assert p["orig"] == [0] and p["begin"] == [0, 0, 0, 1]
    p = plan(shim, [(0, k, 1.0, XL) for k in (4, 3, 2, 1)], 4, [0])
    assert p["orig"] == [3, 2, 1, 0] and p["begin"] == [0, 1, 2, 3, 4]


def test_plan_maps_bodies_to_nodes_on_a_branching_listing(shim):
    # a listing whose depth-first node order differs from the listing order (a tree listed breadth first)
    node_of_listing = [0, 1, 4, 2, 3, 5, 6]
    terms = [(6, 2, 1.0, (1.0, 2.0, 3.0)), (2, 1, 1.0, (4.0, 5.0, 6.0)), (3, 2, 1.0, XL), (2, 2, 1.0, XL)]
    p = plan(shim, terms, 2, node_of_listing)
    assert p["orig"] == [1, 0, 2, 3]
    assert p["node"] == [4, 6, 2, 4]
    assert p["xl"][0].tolist() == [4.0, 5.0, 6.0] and p["xl"][1].tolist() == [1.0, 2.0, 3.0]
    assert p["begin"] == [0, 1, 4]


def test_plan_refusals_name_the_term(shim):
    ident = [0, 1, 2]
    good = (1, 2, 1.0, XL)
    assert "null terms" in plan(shim, [good], 4, ident, null_terms=True)
    assert "nterms < 1" in plan(shim, [], 4, ident)
    assert "nsteps < 1" in plan(shim, [good], 0, ident)
    for bad_body in (-1, 3):
        msg = plan(shim, [good, good, (bad_body, 2, 1.0, XL)], 4, ident)
        assert msg.startswith("term 2:") and "body" in msg, msg
    for bad_step in (0, 5, -3):
        msg = plan(shim, [good, (1, bad_step, 1.0, XL), good], 4, ident)
        assert msg.startswith("term 1:") and "step" in msg, msg
    # the first bad term is the one that is named
    assert plan(shim, [(7, 1, 1.0, XL), (0, 9, 1.0, XL)], 4, ident).startswith("term 0:")
    assert isinstance(plan(shim, [(0, 1, 1.0, XL), (2, 4, 1.0, XL)], 4, ident), dict)       # the edges of both ranges hold


def test_mex_command_checks_its_handle(gw):  # noqa: F811
    """'adjoint_track' is a command of the gateway and, like every command that names a handle, refuses a made-up one and a missing one."""
    with pytest.raises(MexError, match="handle"):
        gw.call(1, "adjoint_track", np.array([[12345]], dtype=np.uint64), 1e-2, 4.0, {}, np.zeros((2, 4, 1)))
    with pytest.raises(MexError, match="handle"):
        gw.call(1, "adjoint_track")


def _adjoint_kernels():
    """{(kind, NP, MODE, flags): entry} of the k_adjoint_fwd / k_adjoint_bwd instantiations in the fingerprint build() wrote."""
    import __graft_entry__ as g
    g.build()
    fp = json.load(open(os.path.join(ROOT, "redmax_amd", "kernel_fingerprint.json")))
    out = {}
    for v in fp.values():
        m = re.search(r"k_adjoint_(fwd|bwd)<(\d+), (\d+)((?:, (?:true|false))*)>", v["name"])
        if m:
            out[(m.group(1), int(m.group(2)), int(m.group(3)), m.group(4))] = v
    return out


def test_trk_instantiations_exist_and_take_no_more_scratch_than_their_ctl_siblings():
    """Every launcher family has its TRK pair (MODE = integrator | 4 | 8 = 13, 14), and up to 32 lanes no TRK kernel takes more
    scratch than the CTL kernel of the same size, integrator, helper wave and chain flag.  The 64-lane figures are reported, not
    bounded: that kernel spills in every form (built with HIP 7.2: forward 2104 against 2156 bytes per lane under BDF1, 3832 against
    3880 under BDF2; backward 0 in all four)."""
    ks = _adjoint_kernels()
    fwd = sorted(k for k in ks if k[0] == "fwd" and k[2] & 8)
    bwd = sorted(k for k in ks if k[0] == "bwd" and k[2] & 8)
    want_fwd = {(NP, mode, ", false, false") for NP in (4, 8, 16, 32, 64) for mode in (13, 14)}
    want_fwd |= {(16, mode, flags) for mode in (13, 14) for flags in (", false, true", ", true, false", ", true, true")}
    assert {k[1:] for k in fwd} == want_fwd
    want_bwd = {(NP, mode, ", false") for NP in (4, 8, 16, 32, 64) for mode in (13, 14)} | {(16, mode, ", true") for mode in (13, 14)}
    assert {k[1:] for k in bwd} == want_bwd
    for k in fwd + bwd:
        sib = ks[(k[0], k[1], k[2] & ~8, k[3])]
        print("k_adjoint_%s<%d, %d%s>: scratch %d B/lane, VGPR %d; CTL sibling: scratch %d, VGPR %d"
              % (k[0], k[1], k[2], k[3], ks[k]["scratch_bytes"], ks[k]["vgpr"], sib["scratch_bytes"], sib["vgpr"]))
        if k[1] <= 32:
            assert ks[k]["scratch_bytes"] <= sib["scratch_bytes"], (k, ks[k]["scratch_bytes"], sib["scratch_bytes"])
