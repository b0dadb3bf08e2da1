"""The frame-target entries (rmx_rollout_frames, rmx_rollout_cost_frames and their _device forms) are declared, exported by the built
library and bound; the structs are the header's; and what they refuse without a device."""
import ctypes as C

import pytest

NAMES = ("rmx_rollout_frames", "rmx_rollout_frames_device", "rmx_rollout_cost_frames", "rmx_rollout_cost_frames_device")


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
    # the structs as the header declares them
    assert [f[0] for f in _abi.FrameTerm._fields_] == ["body", "xlocal", "step", "wpos", "wvel", "wrot"]
    assert [f[0] for f in _abi.FrameTerms._fields_] == ["nterms", "terms", "xtarget", "vtarget", "Rtarget", "per_rollout"]
    # int, 3 doubles, int, 3 doubles with C's padding: 8 + 24 + 8 + 24; int, four pointers, int
    assert C.sizeof(_abi.FrameTerm) == 64 and _abi.FrameTerm.xlocal.offset == 8 and _abi.FrameTerm.step.offset == 32
    assert _abi.FrameTerm.wpos.offset == 40 and _abi.FrameTerm.wrot.offset == 56
    assert C.sizeof(_abi.FrameTerms) == 48 and _abi.FrameTerms.per_rollout.offset == 40
    assert L.rmx_rollout_frames.argtypes[4] == C.POINTER(_abi.FrameTerms) and len(L.rmx_rollout_frames.argtypes) == 13
    assert L.rmx_rollout_cost_frames.argtypes[4] == C.POINTER(_abi.StateCost) and L.rmx_rollout_cost_frames.argtypes[5] == C.POINTER(_abi.FrameTerms)
    assert len(L.rmx_rollout_cost_frames.argtypes) == 7 and L.rmx_rollout_cost_frames.argtypes[6] == C.POINTER(_abi.CostModel)


def test_the_header_declares_the_structs_as_bound():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "redmax_hip.h")).read()
    assert re.search(r"typedef struct rmx_frame_term \{ int body; double xlocal\[3\]; int step; double wpos, wvel, wrot; \} rmx_frame_term;", text)
    body = re.search(r"typedef struct rmx_frame_terms \{(.*?)\} rmx_frame_terms;", text, re.S).group(1)
    names = re.findall(r"\b(nterms|terms|xtarget|vtarget|Rtarget|per_rollout)\b", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == ["nterms", "terms", "xtarget", "vtarget", "Rtarget", "per_rollout"]
    assert "#define RMX_VERSION 111" in text


def test_a_null_batch_is_refused_by_name():
    import __graft_entry__ as g
    g.build()
    from redmax_amd import _abi
    L = _abi.lib()
    assert L.rmx_rollout_frames(None, 1, None, None, None, None, None, None, None, None, None, None, None) != 0
    assert b"rmx_rollout_frames: null argument" in L.rmx_last_error()
    assert L.rmx_rollout_frames_device(None, 1, None, None, None, None, None, None, None, None, None, None, None) != 0
    assert b"rmx_rollout_frames: null argument" in L.rmx_last_error()
    assert L.rmx_rollout_cost_frames(None, 1, None, None, None, None, None) != 0
    assert b"rmx_rollout_cost_frames: null argument" in L.rmx_last_error()
    assert L.rmx_rollout_cost_frames_device(None, 1, None, None, None, None, None) != 0
    assert b"rmx_rollout_cost_frames: null argument" in L.rmx_last_error()


def test_the_python_layers_are_there():
    import inspect
    from redmax_amd import diff, ilqr
    from redmax_amd.batch import BatchSim
    assert all(callable(getattr(BatchSim, n)) for n in ("rollout_frames", "rollout_frames_device", "rollout_cost_frames", "rollout_cost_frames_device"))
    assert callable(diff.frames)
    for fn in (diff.cost_model, ilqr.TrackingCost.__init__):
        p = inspect.signature(fn).parameters
        assert p["vtarget"].default is None and p["Rtarget"].default is None
    with pytest.raises(ValueError, match="want must name distinct outputs"):
        diff.cost_model(None, None, None, want=("J", "J"), vtarget=None, Rtarget=None)
