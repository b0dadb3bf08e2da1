"""The kernel choice of a step / adjoint call (redmax_amd/csrc/rmx_select.h), on the CPU: the header is compiled with plain g++ behind
a small C shim (tests/stepplan/step_plan_shim.cpp) and every row, sub-case and threshold edge of DESIGN.md's "Which kernel runs"
table is asserted against labels written out here."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BDF1, BDF2 = 1, 2
# StepKernel, in the order of the enum
BIG, PF, CT, GROUND32, STEPPAIR32, W2_64, PAIRCHAIN32, W2CHAIN32, FULLCHAIN, GCONST64, FULLN64, PLAIN = range(12)
HELP16, FULLCHAIN16, GENERIC = range(3)
COOP_G = 8
N_SIMD = 1024          # 256 CUs
# the thresholds a model takes on such a device (redmax_hip.hip model_create_flat)
W2_MAX, W2C_MIN, GCONST_MIN, ADJ_MAX = N_SIMD // 2, 128, N_SIMD // 2 + 1, N_SIMD // 2


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(ROOT, "build", "stepplan", "libstep_plan_shim.so")
    src = os.path.join(ROOT, "tests", "stepplan", "step_plan_shim.cpp")
    inc = os.path.join(ROOT, "redmax_amd", "csrc")
    deps = [src, os.path.join(inc, "rmx_select.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", inc, "-o", so, src])
    L = C.CDLL(so)
    L.sp_select_step.restype = C.c_char_p
    return L


def traits(NP, n, chain=False, big=False, pf=False, contact=False, sph=False, n_simd=N_SIMD, w2_max=None, w2_min=None, gconst_min=None):
    """StepTraits as model_create_flat fills them for such a model (thresholds only where the model takes them)."""
    plain = not sph
    full32 = NP == 32 and plain and chain and n == 32
    if w2_max is None:
        w2_max = W2_MAX if ((NP == 64 and plain) or full32) and not big else 0
    if w2_min is None:
        w2_min = W2C_MIN if full32 else 0
    gconst = NP == 64 and plain and not big
    if gconst_min is None:
        gconst_min = GCONST_MIN if gconst else 0
    adj = ADJ_MAX if NP == 16 and not big else 0
    return (C.c_int * 14)(NP, n, big, pf, contact, sph, chain, gconst, n_simd, COOP_G, w2_max, w2_min, gconst_min, adj)


def plan(L, t, B, integ, energy=False, park=24, coop_map=0, runahead=1, pairc=1, fused=1, adj_help=1):
    out = (C.c_int * 11)()
    label = L.sp_select_step(t, B, integ, int(energy), (C.c_int * 6)(park, coop_map, runahead, pairc, fused, adj_help), 0, out)
    keys = ("kernel", "stores_ticks", "parks", "park_halvings", "fused", "contact_pass", "fullchain", "fulln", "energy", "block", "full32")
    d = dict(zip(keys, out))
    d["label"] = label.decode()
    return d


ALL_NP = (4, 8, 16, 32, 64)


def test_row1_big(shim):
    for integ in (BDF1, BDF2):
        for contact in (False, True):
            p = plan(shim, traits(256, 72, chain=True, big=True, contact=contact), 2, integ)
            assert (p["kernel"], p["label"]) == (BIG, "k_big_step")
            assert not p["stores_ticks"] and not p["parks"]
    # ... ahead of point forces
    assert plan(shim, traits(256, 72, big=True, pf=True), 2, BDF1)["label"] == "k_big_step"


def test_row2_point_forces(shim):
    want = {4: ("k_step_pf<4,bdf1>", "k_step_pf<4,bdf2>"), 8: ("k_step_pf<8,bdf1>", "k_step_pf<8,bdf2>"),
            16: ("k_step_pf<16,bdf1>", "k_step_pf<16,bdf2>"), 32: ("k_step_pf<32,bdf1>", "k_step_pf<32,bdf2>"),
            64: ("k_step_pf<64,bdf1>", "k_step_pf<64,bdf2>")}
    for NP in ALL_NP:
        for i, integ in enumerate((BDF1, BDF2)):
            # a full chain, so that every later row would match too: point forces come first
            p = plan(shim, traits(NP, NP, chain=True, pf=True), 2, integ)
            assert (p["kernel"], p["label"]) == (PF, want[NP][i])
            assert not p["stores_ticks"] and p["block"] == 64
    # ... ahead of contact and Euler charts
    assert plan(shim, traits(32, 8, chain=True, pf=True, contact=True), 2, BDF1)["label"] == "k_step_pf<32,bdf1>"
    assert plan(shim, traits(8, 5, pf=True, sph=True), 2, BDF2)["label"] == "k_step_pf<8,bdf2>"


def test_row3_contact_or_euler_charts(shim):
    want = {4: ("k_step_bdf1<4,ct>", "k_step_bdf2<4,ct>"), 8: ("k_step_bdf1<8,ct>", "k_step_bdf2<8,ct>"),
            16: ("k_step_bdf1<16,ct>", "k_step_bdf2<16,ct>"), 32: ("k_step_bdf1<32,ct>", "k_step_bdf2<32,ct>"),
            64: ("k_step_bdf1<64,ct>", "k_step_bdf2<64,ct>")}
    for NP in ALL_NP:
        for i, integ in enumerate((BDF1, BDF2)):
            for contact, sph in ((True, False), (False, True), (True, True)):
                # (a tree: the 32-node serial chain with contact and no charts is row 4)
                p = plan(shim, traits(NP, NP, chain=False, contact=contact, sph=sph), 2, integ)
                assert (p["kernel"], p["label"]) == (CT, want[NP][i])
                assert bool(p["contact_pass"]) == contact      # the launch with the contact terms iff there is contact
                assert not p["stores_ticks"] and not p["parks"] and p["fused"] == 0 and p["block"] == 64
    # NP = 32 beside row 4: a tree with contact, a chain with contact AND charts, a chain with charts only
    for integ, lab in ((BDF1, "k_step_bdf1<32,ct>"), (BDF2, "k_step_bdf2<32,ct>")):
        assert plan(shim, traits(32, 20, chain=False, contact=True), 2, integ)["label"] == lab
        assert plan(shim, traits(32, 20, chain=True, contact=True, sph=True), 2, integ)["label"] == lab
        assert plan(shim, traits(32, 20, chain=True, sph=True), 2, integ)["label"] == lab
    # a serial chain with contact at another size is row 3 too
    assert plan(shim, traits(16, 16, chain=True, contact=True), 2, BDF1)["label"] == "k_step_bdf1<16,ct>"
    assert plan(shim, traits(64, 40, chain=True, contact=True), 2, BDF2)["label"] == "k_step_bdf2<64,ct>"


def test_row4_chain32_with_ground(shim):
    for integ in (BDF1, BDF2):
        for n in (8, 32):
            t = traits(32, n, chain=True, contact=True)
            p = plan(shim, t, 2, integ)      # defaults: fused 1, 24 halvings
            assert (p["kernel"], p["label"], p["fused"], p["parks"], p["park_halvings"]) == (GROUND32, "k_ground32", 1, 1, 24)
            assert not p["stores_ticks"]
            for fused in (2, 3):      # modes 2 and 3 stay what they are
                p = plan(shim, t, 2, integ, fused=fused)
                assert (p["kernel"], p["label"], p["fused"], p["parks"]) == (GROUND32, "k_ground32", fused, 1)
            p = plan(shim, t, 2, integ, fused=0)
            assert (p["kernel"], p["label"], p["fused"], p["parks"], p["park_halvings"]) == (STEPPAIR32, "k_step_pair", 0, 1, 24)
            p = plan(shim, t, 2, integ, park=7)
            assert (p["parks"], p["park_halvings"]) == (1, 7)


def test_row4_parking_and_fused_1_becomes_2(shim):
    for integ in (BDF1, BDF2):
        t = traits(32, 8, chain=True, contact=True)
        # RMX_PARK_HALVINGS = 0: no parking, and "one launch for rollouts and groups" turns into mode 2
        p = plan(shim, t, 2, integ, park=0)
        assert (p["kernel"], p["label"], p["fused"], p["parks"], p["park_halvings"]) == (GROUND32, "k_ground32", 2, 0, 0)
        # fewer SIMDs than a group has members: the same, whatever RMX_PARK_HALVINGS says
        p = plan(shim, traits(32, 8, chain=True, contact=True, n_simd=COOP_G - 1), 2, integ)
        assert (p["kernel"], p["label"], p["fused"], p["parks"], p["park_halvings"]) == (GROUND32, "k_ground32", 2, 0, 0)
        # exactly COOP_G SIMDs: parking is on
        p = plan(shim, traits(32, 8, chain=True, contact=True, n_simd=COOP_G), 2, integ)
        assert (p["fused"], p["parks"]) == (1, 1)
        # the other modes do not change without parking
        for fused, kern, lab in ((0, STEPPAIR32, "k_step_pair"), (2, GROUND32, "k_ground32"), (3, GROUND32, "k_ground32")):
            p = plan(shim, t, 2, integ, park=0, fused=fused)
            assert (p["kernel"], p["label"], p["fused"], p["parks"]) == (kern, lab, fused, 0)


def test_parks_iff_row4(shim):
    """parks only in row 4 (with enough SIMDs and halvings > 0); every other row, whatever the knobs: no."""
    others = [traits(256, 72, big=True, contact=True), traits(32, 8, chain=True, pf=True, contact=True), traits(32, 8, chain=False, contact=True),
              traits(16, 16, chain=True, contact=True), traits(64, 64), traits(32, 32, chain=True), traits(16, 16, chain=True), traits(64, 40),
              traits(4, 3, chain=True)]
    for t in others:
        for integ in (BDF1, BDF2):
            for B in (2, 600):
                p = plan(shim, t, B, integ, park=24, fused=1)
                assert (p["parks"], p["park_halvings"], p["fused"]) == (0, 0, 0), p


def test_row5_w2_64(shim):
    lab = {BDF1: "k_step_bdf1<64,w2>", BDF2: "k_step_bdf2<64,w2>"}
    for integ in (BDF1, BDF2):
        for energy in (False, True):
            # full chain
            p = plan(shim, traits(64, 64, chain=True), 2, integ, energy=energy)
            assert (p["kernel"], p["label"], p["fullchain"], p["fulln"], p["energy"], p["block"]) == (W2_64, lab[integ], 1, 0, 1, 128)
            # n == 64, a tree: the instantiation without energies under BDF1 when none are recorded, and only then
            p = plan(shim, traits(64, 64), 2, integ, energy=energy)
            assert (p["kernel"], p["label"], p["fullchain"], p["fulln"], p["block"]) == (W2_64, lab[integ], 0, 1, 128)
            assert bool(p["energy"]) == (energy or integ == BDF2)
            # n < 64 (tree or chain)
            for chain in (False, True):
                p = plan(shim, traits(64, 40, chain=chain), 2, integ, energy=energy)
                assert (p["kernel"], p["label"], p["fullchain"], p["fulln"], p["energy"], p["block"]) == (W2_64, lab[integ], 0, 0, 1, 128)
            assert not p["stores_ticks"]


def test_row5_threshold_edges(shim):
    for integ, w2, fulln, gconst in ((BDF1, "k_step_bdf1<64,w2>", "k_step_bdf1<64,fulln>", "k_step_bdf1<64,gconst>"),
                                     (BDF2, "k_step_bdf2<64,w2>", "k_step_bdf2<64,fulln>", "k_step_bdf2<64,gconst>")):
        t = traits(64, 64, w2_max=100, gconst_min=300)
        assert plan(shim, t, 100, integ)["label"] == w2           # B == w2_max_batch
        assert plan(shim, t, 101, integ)["label"] == fulln        # + 1
        assert plan(shim, t, 1, integ)["label"] == w2
        # the default thresholds meet: w2 up to n_simd / 2, gconst from n_simd / 2 + 1
        t = traits(64, 64)
        assert plan(shim, t, W2_MAX, integ)["label"] == w2
        assert plan(shim, t, W2_MAX + 1, integ)["label"] == gconst
        # RMX_W2_MAX=0: never
        assert plan(shim, traits(64, 64, w2_max=0), 1, integ)["label"] == fulln


def test_row6_pairchain32_is_the_only_storing_plan(shim):
    t = traits(32, 32, chain=True)
    for energy in (False, True):
        for B in (1, 2, 127, 128, 512, 513, 4096):      # (inside and outside the window of row 7: row 6 comes first)
            p = plan(shim, t, B, BDF1, energy=energy)
            assert (p["kernel"], p["label"], p["stores_ticks"], p["block"], p["full32"]) == (PAIRCHAIN32, "k_step_bdf1_pair32", 1, 64, 1)
            assert bool(p["energy"]) == energy      # the energy instantiation iff T, V are recorded
    # BDF2 never
    assert plan(shim, t, 2, BDF2)["label"] == "k_step_bdf2<32,fullchain>"
    # stores_ticks iff row 6: a sweep over shapes, integrators, batch sizes and knobs
    shapes = [traits(256, 72, big=True), traits(32, 32, chain=True, pf=True), traits(32, 32, chain=True, contact=True),
              traits(32, 32, chain=True, sph=True), traits(32, 32, chain=False), traits(32, 31, chain=True), traits(32, 32, chain=True),
              traits(16, 16, chain=True), traits(64, 64, chain=True), traits(64, 64), traits(64, 40), traits(4, 3, chain=True), traits(8, 8, chain=True)]
    n = 0
    for ti, tt in enumerate(shapes):
        for integ in (BDF1, BDF2):
            for B in (1, 128, 600):
                for pairc in (0, 1):
                    p = plan(shim, tt, B, integ, pairc=pairc)
                    row6 = ti == 6 and integ == BDF1 and pairc == 1
                    assert bool(p["stores_ticks"]) == row6 == (p["kernel"] == PAIRCHAIN32) == (p["label"] == "k_step_bdf1_pair32"), (ti, integ, B, pairc, p)
                    n += row6
    assert n == 3


def test_row7_w2chain32_edges(shim):
    t = traits(32, 32, chain=True)      # w2_min_batch 128, w2_max_batch 512
    w2c, fc = "k_step_bdf1<32,fullchain,w2>", "k_step_bdf1<32,fullchain>"
    p = plan(shim, t, W2C_MIN, BDF1, pairc=0)            # B == w2_min_batch
    assert (p["kernel"], p["label"], p["block"], p["stores_ticks"]) == (W2CHAIN32, w2c, 128, 0)
    p = plan(shim, t, W2C_MIN - 1, BDF1, pairc=0)        # - 1
    assert (p["kernel"], p["label"], p["block"]) == (FULLCHAIN, fc, 64)
    assert plan(shim, t, W2_MAX, BDF1, pairc=0)["label"] == w2c          # B == w2_max_batch
    assert plan(shim, t, W2_MAX + 1, BDF1, pairc=0)["label"] == fc      # + 1
    # BDF2 has no such kernel
    assert plan(shim, t, W2C_MIN, BDF2, pairc=0)["label"] == "k_step_bdf2<32,fullchain>"
    # RMX_W2_MAX=0: never; RMX_W2C_MIN=2: from two rollouts on
    assert plan(shim, traits(32, 32, chain=True, w2_max=0), 200, BDF1, pairc=0)["label"] == fc
    assert plan(shim, traits(32, 32, chain=True, w2_min=2), 2, BDF1, pairc=0)["label"] == w2c
    assert plan(shim, traits(32, 32, chain=True, w2_min=2), 1, BDF1, pairc=0)["label"] == fc
    # not a full chain: neither row 6 nor row 7 (thresholds as a full chain's, to show that they are not what decides)
    for tt in (traits(32, 31, chain=True, w2_max=W2_MAX, w2_min=W2C_MIN), traits(32, 32, chain=False, w2_max=W2_MAX, w2_min=W2C_MIN)):
        p = plan(shim, tt, 200, BDF1)
        assert (p["kernel"], p["label"], p["full32"]) == (PLAIN, "k_step_bdf1<32>", 0)


def test_row8_fullchain(shim):
    want = {16: ("k_step_bdf1<16,fullchain>", "k_step_bdf2<16,fullchain>"), 32: ("k_step_bdf1<32,fullchain>", "k_step_bdf2<32,fullchain>"),
            64: ("k_step_bdf1<64,fullchain>", "k_step_bdf2<64,fullchain>")}
    for NP in (16, 32, 64):
        for i, integ in enumerate((BDF1, BDF2)):
            # (NP = 64: beyond the two-wave batches; a full chain wins over gconst, row 9)
            p = plan(shim, traits(NP, NP, chain=True), 600, integ, pairc=0)
            assert (p["kernel"], p["label"], p["block"]) == (FULLCHAIN, want[NP][i], 64)
    # below 16 nodes there is no such specialisation; nor for a chain that leaves slots free, nor for a tree
    for integ, pre in ((BDF1, "k_step_bdf1<"), (BDF2, "k_step_bdf2<")):
        assert plan(shim, traits(4, 4, chain=True), 2, integ)["label"] == pre + "4>"
        assert plan(shim, traits(8, 8, chain=True), 2, integ)["label"] == pre + "8>"
        assert plan(shim, traits(16, 15, chain=True), 2, integ)["label"] == pre + "16>"
        assert plan(shim, traits(16, 16, chain=False), 2, integ)["label"] == pre + "16>"


def test_row9_gconst_edges(shim):
    for integ, gc, fulln, plain in ((BDF1, "k_step_bdf1<64,gconst>", "k_step_bdf1<64,fulln>", "k_step_bdf1<64>"),
                                    (BDF2, "k_step_bdf2<64,gconst>", "k_step_bdf2<64,fulln>", "k_step_bdf2<64>")):
        for n, below in ((64, fulln), (40, plain)):
            t = traits(64, n, w2_max=0, gconst_min=300)
            p = plan(shim, t, 300, integ)                    # B == gconst_min_batch
            assert (p["kernel"], p["label"], bool(p["fulln"]), p["block"]) == (GCONST64, gc, n == 64, 64)
            assert plan(shim, t, 299, integ)["label"] == below      # - 1
            # 0: never
            assert plan(shim, traits(64, n, w2_max=0, gconst_min=0), 5000, integ)["label"] == below
    # no table in global memory (a model with Euler charts never gets here; the flag alone)
    t = traits(64, 64, w2_max=0, gconst_min=2)
    t[7] = 0
    assert plan(shim, t, 3, BDF1)["label"] == "k_step_bdf1<64,fulln>"


def test_rows10_11_fulln_and_plain(shim):
    for integ, pre in ((BDF1, "k_step_bdf1<"), (BDF2, "k_step_bdf2<")):
        p = plan(shim, traits(64, 64, w2_max=0), 2, integ)
        assert (p["kernel"], p["label"]) == (FULLN64, pre + "64,fulln>")
        p = plan(shim, traits(64, 40, w2_max=0), 2, integ)
        assert (p["kernel"], p["label"]) == (PLAIN, pre + "64>")
        for NP, n, lab in ((4, 3, "4>"), (8, 7, "8>"), (16, 11, "16>"), (32, 20, "32>"), (32, 32, "32>")):
            p = plan(shim, traits(NP, n, chain=False), 2, integ)
            assert (p["kernel"], p["label"], p["block"], p["stores_ticks"], p["parks"]) == (PLAIN, pre + lab, 64, 0, 0)


def test_adjoint_choices(shim):
    fc = C.c_int()
    sel = lambda t, B, help_=1: (shim.sp_select_adjoint(t, B, help_, C.byref(fc)), fc.value)
    chain16, tree16 = traits(16, 16, chain=True), traits(16, 11)
    assert sel(chain16, ADJ_MAX) == (HELP16, 1)             # B == adj_help_max_batch
    assert sel(chain16, ADJ_MAX + 1) == (FULLCHAIN16, 1)    # + 1
    assert sel(chain16, 2, 0) == (FULLCHAIN16, 1)           # RMX_ADJ_HELP=0
    assert sel(tree16, ADJ_MAX) == (HELP16, 0)
    assert sel(tree16, ADJ_MAX + 1) == (GENERIC, 0)
    assert sel(tree16, 2, 0) == (GENERIC, 0)
    assert sel(traits(16, 15, chain=True), ADJ_MAX + 1) == (GENERIC, 0)      # a chain that leaves a slot free
    # the other sizes: generic, full chain or not
    for NP in (4, 8, 32, 64):
        assert sel(traits(NP, NP, chain=True), 2) == (GENERIC, 0)
    # a threshold of 0 switches the helper wave off
    t = traits(16, 16, chain=True)
    t[13] = 0
    assert sel(t, 1) == (FULLCHAIN16, 1)


def test_knobs_from_environment(shim, monkeypatch):
    """One function reads the per-call switches: names and defaults as they have always been, read again at every call."""
    names = ("RMX_PARK_HALVINGS", "RMX_COOP_MAP", "RMX_W2_RUNAHEAD", "RMX_PAIRC", "RMX_GROUND_FUSED", "RMX_ADJ_HELP")
    for nm in names:
        monkeypatch.delenv(nm, raising=False)
    out = (C.c_int * 6)()
    shim.sp_knobs_from_env(out)
    assert list(out) == [24, 0, 1, 1, 1, 1]
    for nm, v in zip(names, ("5", "1", "0", "0", "3", "0")):
        monkeypatch.setenv(nm, v)
    shim.sp_knobs_from_env(out)
    assert list(out) == [5, 1, 0, 0, 3, 0]
    # ... and select_step sees them
    res = (C.c_int * 11)()
    assert shim.sp_select_step(traits(32, 32, chain=True), 2, BDF1, 0, None, 1, res) == b"k_step_bdf1<32,fullchain>"
    monkeypatch.setenv("RMX_PAIRC", "1")
    assert shim.sp_select_step(traits(32, 32, chain=True), 2, BDF1, 0, None, 1, res) == b"k_step_bdf1_pair32"
    assert shim.sp_select_step(traits(32, 8, chain=True, contact=True), 2, BDF2, 0, None, 1, res) == b"k_ground32"
    assert (res[4], res[2], res[3]) == (3, 1, 5)
