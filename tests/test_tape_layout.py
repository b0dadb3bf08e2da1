"""The arithmetic of redmax_amd/csrc/rmx_tape.h, on the CPU: where the parts of a tape lie in the adjoint workspace (the layout every
entry of the taped-rollout family reads), and where the arrays of a host form lie in their staging room.  Sizes and total are
compared with an independent restatement below."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = ("H", "M", "D", "stage_traj0", "stage_traj1", "stage_traj2", "stage_state0", "stage_state1", "Q0", "QD0", "QT", "QDT", "ZS", "PG")
SHAPES = ((1, 1, 1, 1, 1), (3, 2, 5, 4, 7), (2, 1, 3, 0, 3), (512, 20, 16, 16, 16))      # (B, nsteps, n, nr, nlist)


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(ROOT, "build", "tapeplan", "libtape_layout_shim.so")
    src = os.path.join(ROOT, "tests", "tapeplan", "tape_layout_shim.cpp")
    inc = os.path.join(ROOT, "redmax_amd", "csrc")
    deps = [src, os.path.join(inc, "rmx_tape.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", inc, "-o", so, src])
    L = C.CDLL(so)
    L.tl_round256.restype = C.c_ulonglong
    L.tl_round256.argtypes = [C.c_ulonglong]
    L.tl_stage.restype = C.c_ulonglong
    return L


def up256(x):
    return -(-x // 256) * 256


def layout(shim, B, nsteps, integ, n, nr, nlist):
    off, size = (C.c_ulonglong * 14)(), (C.c_ulonglong * 14)()
    scal, pg_off, pg_bytes = (C.c_ulonglong * 2)(), (C.c_ulonglong * 5)(), (C.c_ulonglong * 5)()
    shim.tl_layout(B, nsteps, integ, n, nr, nlist, off, size, scal, pg_off, pg_bytes)
    return list(off), list(size), scal[0], scal[1], list(pg_off), list(pg_bytes)


def test_round256(shim):
    for x in (0, 1, 255, 256, 257, 511, 512, 8 * 3 * 2 * 4, (1 << 40) + 1):
        assert shim.tl_round256(x) == up256(x)


@pytest.mark.parametrize("integ", (1, 2))
@pytest.mark.parametrize("shape", SHAPES)
def test_tape_layout(shim, shape, integ):
    B, nsteps, n, nr, nlist = shape
    off, size, nslots, total, pg_off, pg_bytes = layout(shim, B, nsteps, integ, n, nr, nlist)
    assert nslots == nsteps + (1 if integ == 2 else 0)
    # the independent restatement
    hist, traj, state = B * nslots * n * n * 8, B * nsteps * nr * 8, B * nr * 8
    pg = [state, state, state, B * nlist * 6 * 8, B * 3 * 8]
    want = dict(zip(PARTS, [hist] * 3 + [traj] * 3 + [state] * 2 + [state] * 2 + [traj] * 2 + [B * nslots * n * 8, sum(up256(x) for x in pg)]))
    assert dict(zip(PARTS, size)) == want
    assert total == sum(up256(x) for x in want.values())
    # every part at a 256-byte boundary, in the documented order, each holding its size rounded up: none overlaps the next
    assert all(o % 256 == 0 for o in off)
    at = 0
    for name, o, s in zip(PARTS, off, size):
        assert o == at, name
        at += up256(s)
    assert at == total
    nonempty = [(o, s) for o, s in zip(off, size) if s]
    assert all(o0 + s0 <= o1 for (o0, s0), (o1, _) in zip(nonempty, nonempty[1:]))
    assert nonempty[-1][0] + nonempty[-1][1] <= total
    # the five gradient arrays inside part PG
    assert pg_bytes == pg
    assert all(o % 256 == 0 for o in pg_off)
    assert pg_off == [sum(up256(x) for x in pg[:i]) for i in range(5)]
    assert pg_off[4] + pg_bytes[4] <= size[13]


def test_tape_layout_empty_parts(shim):
    # nr = 0: the parts shaped as u or as the state are empty and take no room
    off, size, _, _, _, _ = layout(shim, 2, 1, 1, 3, 0, 3)
    empty = [name for name, s in zip(PARTS, size) if s == 0]
    assert empty == [p for p in PARTS if p.startswith("stage_") or p in ("Q0", "QD0", "QT", "QDT")]
    assert len({off[PARTS.index(p)] for p in empty}) == 1


def stage(shim, items):
    n = len(items)
    bytes_ = (C.c_ulonglong * n)(*[b for b, _ in items])
    present = (C.c_int * n)(*[int(p) for _, p in items])
    off = (C.c_ulonglong * n)()
    total = shim.tl_stage(n, bytes_, present, off)
    return total, list(off)


@pytest.mark.parametrize("items", (
    [(1, True)],
    [(96, True), (96, False), (96, True)],                                     # an absent array in the middle
    [(0, True), (300, True), (256, True), (1, True)],                          # an empty array that is given
    [(480, False), (480, False), (48, False)],                                 # nothing given
    [(48, True), (48, True), (48, False), (384, True), (96, False), (48, True), (384, False), (96, True), (24, True), (24, True)],
))
def test_stage_plan(shim, items):
    assert len(items) <= shim.tl_stage_max()
    total, off = stage(shim, items)
    assert total == sum(up256(b) for b, p in items if p)                       # absent arrays take no room
    given = [(o, b) for o, (b, p) in zip(off, items) if p]
    assert all(o % 256 == 0 for o, _ in given)
    at = 0
    for o, b in given:                                                         # in order, disjoint, each with its rounded size
        assert o == at
        at += up256(b)
    assert at == total
    # dropping the absent arrays from the list changes nothing for the others
    total2, off2 = stage(shim, [it for it in items if it[1]])
    assert total2 == total and off2 == [o for o, _ in given]
