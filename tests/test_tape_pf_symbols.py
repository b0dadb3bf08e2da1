"""The switch of the taped rollouts with point forces (rmx_model_tape_point_forces, rmx_model_get_tape_point_forces) is declared,
exported by the built library and bound; and what the entries and the Python layer refuse without a device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rmx_model_tape_point_forces", "rmx_model_get_tape_point_forces")


def test_the_two_names_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from redmax_amd import _abi
    raw = C.CDLL(_abi.LIB_PATH)
    L = _abi.lib()
    header = open(os.path.join(ROOT, "include", "redmax_hip.h")).read()
    for name in NAMES:
        assert name in _abi.SYMBOLS, name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
        assert "int %s(" % name in header, name
    assert L.rmx_model_tape_point_forces.argtypes == [C.c_void_p, C.c_int]
    assert L.rmx_version() == 111          # no new ABI version: callers probe for the symbols


def test_a_null_model_is_refused():
    import __graft_entry__ as g
    g.build()
    from redmax_amd import _abi
    L = _abi.lib()
    assert L.rmx_model_tape_point_forces(None, 1) != 0
    assert b"rmx_model_tape_point_forces: null argument" in L.rmx_last_error()
    assert L.rmx_model_get_tape_point_forces(None) < 0


def test_a_group_refuses_the_keyword():
    from redmax_amd import _abi, scenesRedMax
    from redmax_amd.batch import GroupSim
    sc = scenesRedMax(0)
    sc.init()
    with pytest.raises(_abi.RedMaxHipError, match="tape_forces"):
        GroupSim(sc, 2, devices=(0,), tape_forces=True)
