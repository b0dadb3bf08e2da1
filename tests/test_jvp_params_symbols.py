"""rmx_rollout_jvp_params / rmx_rollout_jvp_params_device: declared in the header, listed in _abi.SYMBOLS, exported by the library and
bound with their argument types; rmx_param_tangents as the header lays it out; RMX_VERSION stays 111; a null batch is refused by name."""
import ctypes
import os
import re

import __graft_entry__ as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rmx_rollout_jvp_params", "rmx_rollout_jvp_params_device")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "redmax_hip.h")).read(), flags=re.S)


def test_entry_points_are_declared_listed_exported_and_bound():
    g.build()
    from redmax_amd import _abi
    src = _header()
    L = ctypes.CDLL(_abi.LIB_PATH)
    lib = _abi.lib()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _abi.SYMBOLS
        assert hasattr(L, name), name
        args = getattr(lib, name).argtypes
        assert len(args) == 9 and args[1] is ctypes.c_int and args[2] is ctypes.c_int and args[3] is ctypes.POINTER(_abi.ParamTangents)
    assert lib.rmx_rollout_jvp_params.argtypes[4] is ctypes.POINTER(ctypes.c_double)
    assert lib.rmx_rollout_jvp_params_device.argtypes[4] is ctypes.c_void_p
    assert lib.rmx_version() == 111 and re.search(r"#define\s+RMX_VERSION\s+111\b", open(os.path.join(ROOT, "include", "redmax_hip.h")).read())


def test_the_struct_is_the_headers():
    from redmax_amd import _abi
    body = re.search(r"typedef struct rmx_param_tangents\s*\{(.*?)\}\s*rmx_param_tangents;", _header(), flags=re.S).group(1)
    fields = re.findall(r"const double\*\s*(\w+);", body)
    assert tuple(fields) == _abi.PARAM_NAMES == tuple(n for n, _ in _abi.ParamTangents._fields_)
    assert all(t is ctypes.c_void_p for _, t in _abi.ParamTangents._fields_)
    assert ctypes.sizeof(_abi.ParamTangents) == 5 * ctypes.sizeof(ctypes.c_void_p)


def test_a_null_batch_is_refused_by_name():
    g.build()
    from redmax_amd import _abi
    lib = _abi.lib()
    tp = _abi.ParamTangents()
    out = (ctypes.c_double * 4)()
    for name in NAMES:
        rc = getattr(lib, name)(None, 1, 1, ctypes.byref(tp), None, None, None, ctypes.cast(out, getattr(lib, name).argtypes[7]),
                                ctypes.cast(out, getattr(lib, name).argtypes[8]))
        assert rc != 0 and lib.rmx_last_error() == b"rmx_rollout_jvp_params: null argument", name
