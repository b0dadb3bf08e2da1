"""The torque-limit entries (rmx_rollout_tape_feedback_box, rmx_rollout_lqr_box and their _device forms) are declared, exported by
the built library and bound; and what the Python layer refuses without a device."""
import ctypes as C

import pytest

NAMES = ("rmx_rollout_tape_feedback_box", "rmx_rollout_tape_feedback_box_device", "rmx_rollout_lqr_box", "rmx_rollout_lqr_box_device")


def test_the_four_names_are_listed_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from redmax_amd import _abi
    raw = C.CDLL(_abi.LIB_PATH)
    L = _abi.lib()
    for name in NAMES:
        assert name in _abi.SYMBOLS, name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
    box = _abi.Box(None, None)
    assert [f[0] for f in _abi.Box._fields_] == ["ulo", "uhi"] and C.sizeof(box) == 2 * C.sizeof(C.c_void_p)
    # the box sits between the feedback table and the record / between the cost and ubar, as the header declares it
    assert L.rmx_rollout_tape_feedback_box.argtypes[6] == C.POINTER(_abi.Box) and len(L.rmx_rollout_tape_feedback_box.argtypes) == 11
    assert L.rmx_rollout_lqr_box.argtypes[3] == C.POINTER(_abi.Box) and len(L.rmx_rollout_lqr_box.argtypes) == 8


def test_a_null_batch_is_refused_by_name():
    """The refusals that need no device: the entries answer for themselves, in their own names."""
    import __graft_entry__ as g
    g.build()
    from redmax_amd import _abi
    L = _abi.lib()
    assert L.rmx_rollout_lqr_box(None, 1, None, None, None, 0, None, None) != 0
    assert b"rmx_rollout_lqr_box: null argument" in L.rmx_last_error()
    assert L.rmx_rollout_tape_feedback_box(None, None, 1, 1, 1.0, None, None, None, None, None, None) != 0
    assert b"rmx_rollout_tape_feedback_box: null argument" in L.rmx_last_error()


def test_solve_with_limits_needs_the_device_backward_pass():
    from redmax_amd import ilqr
    with pytest.raises(ValueError, match="backward='device'"):
        ilqr.solve(None, None, None, None, None, backward="torch", ulim=(None, None))
