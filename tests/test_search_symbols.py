"""The line-search entries (rmx_rollout_search and its _device form) are declared, exported by the built library and bound; and what
the entry and the Python layer refuse without a device."""
import ctypes as C

import pytest

NAMES = ("rmx_rollout_search", "rmx_rollout_search_device")


def test_the_two_names_are_listed_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from redmax_amd import _abi
    raw = C.CDLL(_abi.LIB_PATH)
    L = _abi.lib()
    for name in NAMES:
        assert name in _abi.SYMBOLS, name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
    vp, i = C.sizeof(C.c_void_p), C.sizeof(C.c_int)
    assert [f[0] for f in _abi.SearchCost._fields_] == ["sc", "ft", "R"] and C.sizeof(_abi.SearchCost) == 3 * vp
    assert [f[0] for f in _abi.Search._fields_] == ["kff", "alphas", "nalpha", "Jbar"] and C.sizeof(_abi.Search) == 4 * vp
    assert _abi.Search.nalpha.offset == 2 * vp and _abi.Search.nalpha.size == i and _abi.Search.Jbar.offset == 3 * vp
    assert [f[0] for f in _abi.SearchOut._fields_] == ["J", "alpha", "trials", "status"] and C.sizeof(_abi.SearchOut) == 4 * vp
    assert _abi.SEARCH_MAX_ALPHAS == 16
    # feedback, box, search, cost; the record and uapp; the outputs; the stats - as the header declares them
    a = L.rmx_rollout_search.argtypes
    assert len(a) == 13 and a[4] == C.POINTER(_abi.Feedback) and a[5] == C.POINTER(_abi.Box) and a[6] == C.POINTER(_abi.Search)
    assert a[7] == C.POINTER(_abi.SearchCost) and a[11] == C.POINTER(_abi.SearchOut) and a[12] == C.POINTER(_abi.Stats)
    assert L.rmx_rollout_search_device.argtypes == a


def test_the_header_declares_the_structs_and_keeps_the_version():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "redmax_hip.h")).read()
    assert re.search(r"#define RMX_VERSION 111\b", txt) and re.search(r"#define RMX_SEARCH_MAX_ALPHAS 16\b", txt)
    for name in ("rmx_search_cost", "rmx_search", "rmx_search_out"):
        assert re.search(r"\}\s*%s;" % name, txt), name


def test_a_null_batch_is_refused_by_name():
    """The refusals that need no device: the entries answer for themselves, in their own name."""
    import __graft_entry__ as g
    g.build()
    from redmax_amd import _abi
    L = _abi.lib()
    for name in NAMES:
        assert getattr(L, name)(None, None, 1, 1.0, None, None, None, None, None, None, None, None, None) != 0
        assert b"rmx_rollout_search: null argument" in L.rmx_last_error()


def test_solve_refuses_a_device_search_without_the_device_backward_pass():
    from redmax_amd import ilqr
    with pytest.raises(ValueError, match="search='device' needs backward='device'"):
        ilqr.solve(None, None, None, None, None, backward="torch", search="device")
    with pytest.raises(ValueError, match="search must be 'host' or 'device'"):
        ilqr.solve(None, None, None, None, None, search="gpu")


def test_solve_names_the_costs_the_device_search_knows():
    from redmax_amd import ilqr

    class Other:
        pass

    with pytest.raises(ValueError, match="QuadraticCost and TrackingCost"):
        ilqr.solve(None, None, None, None, Other(), backward="device", search="device")
