"""ctypes binding of the C ABI in include/redmax_hip.h (libredmax_hip.so, built in-tree).

This is the only place the product touches native code.  There is deliberately no fallback:
if the shared library is missing or no HIP device is visible, calls raise RedMaxHipError.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libredmax_hip.so")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

# every symbol include/redmax_hip.h and include/redmax_hip_profile.h (the measurement hooks) declare (tests/test_abi_symbols.py checks the .so exports them all)
SYMBOLS = (
    "rmx_last_error", "rmx_version", "rmx_device_count", "rmx_opts_default",
    "rmx_model_create", "rmx_model_destroy", "rmx_model_nr", "rmx_model_nm", "rmx_model_idxR",
    "rmx_model_set_ground_contact", "rmx_model_set_point_forces", "rmx_model_nsph", "rmx_get_charts", "rmx_set_charts",
    "rmx_batch_create", "rmx_batch_destroy", "rmx_batch_size",
    "rmx_set_state", "rmx_get_state", "rmx_set_state_device", "rmx_get_state_device",
    "rmx_eval", "rmx_eval_mfd", "rmx_compute_values", "rmx_step_bdf1", "rmx_step_bdf2", "rmx_step_history", "rmx_step_euler", "rmx_adjoint_bdf1", "rmx_adjoint_bdf2", "rmx_adjoint_bdf1_device", "rmx_adjoint_bdf2_device", "rmx_adjoint_controls", "rmx_adjoint_controls_device", "rmx_adjoint_track", "rmx_adjoint_track_device", "rmx_energy",
    "rmx_rollout_tape", "rmx_rollout_vjp", "rmx_rollout_tape_device", "rmx_rollout_vjp_device",
    "rmx_rollout_tape_bdf2", "rmx_rollout_tape_bdf2_device",
    "rmx_rollout_tape_feedback", "rmx_rollout_tape_feedback_device",
    "rmx_rollout_vjp_feedback", "rmx_rollout_vjp_feedback_device",
    "rmx_rollout_linearize", "rmx_rollout_linearize_device",
    "rmx_rollout_vjp_params", "rmx_rollout_vjp_params_device",
    "rmx_rollout_vjp_forces", "rmx_rollout_vjp_forces_device",
    "rmx_rollout_jvp", "rmx_rollout_jvp_device",
    "rmx_rollout_jvp_params", "rmx_rollout_jvp_params_device",
    "rmx_rollout_lqr", "rmx_rollout_lqr_device",
    "rmx_rollout_tape_feedback_box", "rmx_rollout_tape_feedback_box_device", "rmx_rollout_lqr_box", "rmx_rollout_lqr_box_device",
    "rmx_rollout_points", "rmx_rollout_points_device", "rmx_rollout_cost", "rmx_rollout_cost_device",
    "rmx_rollout_frames", "rmx_rollout_frames_device", "rmx_rollout_cost_frames", "rmx_rollout_cost_frames_device",
    "rmx_rollout_search", "rmx_rollout_search_device",
    "rmx_model_tape_point_forces", "rmx_model_get_tape_point_forces",
    "rmx_last_step_ms", "rmx_last_step_kernel", "rmx_batch_stream", "rmx_step_bdf1_async", "rmx_step_bdf2_async", "rmx_step_history_async", "rmx_sync",
    "rmx_history_read", "rmx_stats_reset", "rmx_stats_read", "rmx_profile_phases", "rmx_step_ticks",
    "rmx_group_create", "rmx_group_destroy", "rmx_group_batch_size", "rmx_group_nshards", "rmx_group_shard", "rmx_group_shard_batch",
    "rmx_group_shard_model", "rmx_group_set_state", "rmx_group_get_state", "rmx_group_step", "rmx_group_step_async", "rmx_group_sync",
    "rmx_group_energy", "rmx_group_timing", "rmx_group_gather_device", "rmx_group_gather_path", "rmx_group_gather", "rmx_group_gathered",
    "rmx_group_gathered_read",
)
REC_ENERGY, REC_STATE, REC_CHARTS = 1, 2, 4      # RMX_REC_*


class RedMaxHipError(RuntimeError):
    pass


class ModelDesc(C.Structure):
    _fields_ = [
        ("njoints", C.c_int),
        ("parent", _ip), ("type", _ip),
        ("axis", _dp), ("E0_pj", _dp), ("E0_ji", _dp), ("I_i", _dp),
        ("qRest", _dp), ("tau", _dp), ("stiffness", _dp), ("damping", _dp),
        ("qLimL", _dp), ("qLimU", _dp), ("qLimK", _dp), ("qLimD", _dp),
        ("grav", C.c_double * 3),
        ("plane", _dp), ("qRestR", _dp),
    ]


class Opts(C.Structure):
    _fields_ = [("h", C.c_double), ("tol", C.c_double), ("dxMax", C.c_double),
                ("iterMaxPerDof", C.c_int), ("iterLsMax", C.c_int), ("lu_mode", C.c_int), ("compensated", C.c_int), ("ls_fail_limit", C.c_int)]


class TaskPointPos(C.Structure):
    _fields_ = [("body", C.c_int), ("xlocal", C.c_double * 3), ("xtarget", C.c_double * 3), ("step", C.c_int),
                ("pscale", C.c_double), ("wreg", C.c_double), ("wpos", C.c_double)]


class TrackTerm(C.Structure):
    _fields_ = [("body", C.c_int), ("xlocal", C.c_double * 3), ("step", C.c_int), ("wpos", C.c_double)]


class TaskTrack(C.Structure):
    _fields_ = [("nterms", C.c_int), ("terms", C.POINTER(TrackTerm)), ("xtarget", _dp), ("per_rollout", C.c_int),
                ("pscale", C.c_double), ("wreg", C.c_double)]


class GroundContact(C.Structure):
    _fields_ = [("flags", _ip), ("sides", _dp), ("E", C.c_double * 16), ("kn", C.c_double), ("kt", C.c_double),
                ("mu", C.c_double), ("kd", C.c_double), ("E_body", _dp), ("kn_body", _dp), ("kt_body", _dp), ("mu_body", _dp),
                ("kd_body", _dp)]


class PointForce(C.Structure):
    _fields_ = [("kind", C.c_int), ("npts", C.c_int), ("body", _ip), ("x", _dp), ("stiffness", C.c_double), ("damping", C.c_double),
                ("L", C.c_double)]


class ParamGrads(C.Structure):
    _fields_ = [("stiffness", C.c_void_p), ("damping", C.c_void_p), ("qrest", C.c_void_p), ("inertia", C.c_void_p), ("grav", C.c_void_p)]


class ParamTangents(C.Structure):      # rmx_param_tangents: host pointers in the host form, device pointers in the _device form
    _fields_ = [("stiffness", C.c_void_p), ("damping", C.c_void_p), ("qrest", C.c_void_p), ("inertia", C.c_void_p), ("grav", C.c_void_p)]


class ForceGrads(C.Structure):      # rmx_force_grads: host pointers in the host form, device pointers in the _device form
    _fields_ = [("stiffness", C.c_void_p), ("damping", C.c_void_p), ("L", C.c_void_p)]


class Feedback(C.Structure):      # rmx_feedback: host pointers in the host form, device pointers in the _device form
    _fields_ = [("uff", C.c_void_p), ("K", C.c_void_p), ("xref", C.c_void_p), ("per_rollout", C.c_int)]


class FeedbackGrads(C.Structure):      # rmx_feedback_grads: host pointers in the host form, device pointers in the _device form
    _fields_ = [("duff", C.c_void_p), ("dK", C.c_void_p), ("dxref", C.c_void_p), ("dq0", C.c_void_p), ("dqd0", C.c_void_p)]


class LqrCost(C.Structure):      # rmx_lqr_cost: host pointers in the host form, device pointers in the _device form
    _fields_ = [("lx", C.c_void_p), ("lu", C.c_void_p), ("Q", C.c_void_p), ("R", C.c_void_p), ("per_rollout", C.c_int), ("mu", C.c_double),
                ("mu_b", C.c_void_p)]


class LqrGains(C.Structure):      # rmx_lqr_gains
    _fields_ = [("kff", C.c_void_p), ("K", C.c_void_p), ("expected", C.c_void_p), ("status", C.c_void_p)]


class Box(C.Structure):      # rmx_box: host pointers in the host form, device pointers in the _device form
    _fields_ = [("ulo", C.c_void_p), ("uhi", C.c_void_p)]


class PointTerms(C.Structure):      # rmx_point_terms: terms is a host array in both forms, xtarget a device pointer in the _device form
    _fields_ = [("nterms", C.c_int), ("terms", C.POINTER(TrackTerm)), ("xtarget", C.c_void_p), ("per_rollout", C.c_int)]


class StateCost(C.Structure):      # rmx_state_cost: host pointers in the host form, device pointers in the _device form
    _fields_ = [("Q", C.c_void_p), ("xgoal", C.c_void_p), ("Q_per_rollout", C.c_int), ("goal_per_rollout", C.c_int)]


class CostModel(C.Structure):      # rmx_cost_model
    _fields_ = [("Jk", C.c_void_p), ("lx", C.c_void_p), ("Q", C.c_void_p)]


class FrameTerm(C.Structure):      # rmx_frame_term
    _fields_ = [("body", C.c_int), ("xlocal", C.c_double * 3), ("step", C.c_int), ("wpos", C.c_double), ("wvel", C.c_double), ("wrot", C.c_double)]


class FrameTerms(C.Structure):      # rmx_frame_terms: terms is a host array in both forms, the targets device pointers in the _device form
    _fields_ = [("nterms", C.c_int), ("terms", C.POINTER(FrameTerm)), ("xtarget", C.c_void_p), ("vtarget", C.c_void_p), ("Rtarget", C.c_void_p),
                ("per_rollout", C.c_int)]


SEARCH_MAX_ALPHAS = 16      # RMX_SEARCH_MAX_ALPHAS


class SearchCost(C.Structure):      # rmx_search_cost: sc and ft host structs; R a host pointer in the host form, a device pointer in the _device form
    _fields_ = [("sc", C.POINTER(StateCost)), ("ft", C.POINTER(FrameTerms)), ("R", C.c_void_p)]


class Search(C.Structure):      # rmx_search: alphas is a host array in both forms; kff and Jbar device pointers in the _device form
    _fields_ = [("kff", C.c_void_p), ("alphas", _dp), ("nalpha", C.c_int), ("Jbar", C.c_void_p)]


class SearchOut(C.Structure):      # rmx_search_out
    _fields_ = [("J", C.c_void_p), ("alpha", C.c_void_p), ("trials", C.c_void_p), ("status", C.c_void_p)]


FEEDBACK_GRAD_NAMES = ("duff", "dK", "dxref", "dq0", "dqd0")      # the members of rmx_feedback_grads, in their order
PARAM_NAMES = ("stiffness", "damping", "qrest", "inertia", "grav")      # the members of rmx_param_grads, in their order
FORCE_PARAM_NAMES = ("force_stiffness", "force_damping", "force_L")      # the members of rmx_force_grads, in their order


class History(C.Structure):
    _fields_ = [("T", _dp), ("V", _dp), ("q", _dp), ("qdot", _dp), ("charts", _ip)]


class Stats(C.Structure):
    _fields_ = [("newton_iters", _ip), ("ls_halvings", _ip), ("status", _ip)]


_lib = None


def lib():
    """Load libredmax_hip.so (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RedMaxHipError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.rmx_last_error.restype = C.c_char_p
    L.rmx_version.restype = C.c_int
    L.rmx_device_count.restype = C.c_int
    L.rmx_opts_default.argtypes = [C.POINTER(Opts)]
    L.rmx_model_create.argtypes = [C.POINTER(ModelDesc), C.c_int, C.POINTER(vp)]
    L.rmx_model_destroy.argtypes = [vp]
    L.rmx_model_nr.argtypes = [vp]
    L.rmx_model_nm.argtypes = [vp]
    L.rmx_model_idxR.argtypes = [vp, _ip]
    L.rmx_model_set_ground_contact.argtypes = [vp, C.POINTER(GroundContact)]
    L.rmx_model_set_point_forces.argtypes = [vp, C.POINTER(PointForce), C.c_int]
    L.rmx_model_tape_point_forces.argtypes = [vp, C.c_int]
    L.rmx_model_get_tape_point_forces.argtypes = [vp]
    L.rmx_model_nsph.argtypes = [vp]
    L.rmx_get_charts.argtypes = [vp, _ip]
    L.rmx_set_charts.argtypes = [vp, _ip]
    L.rmx_batch_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.rmx_batch_destroy.argtypes = [vp]
    L.rmx_batch_size.argtypes = [vp]
    L.rmx_set_state.argtypes = [vp, _dp, _dp]
    L.rmx_get_state.argtypes = [vp, _dp, _dp]
    L.rmx_set_state_device.argtypes = [vp, vp, vp]
    L.rmx_get_state_device.argtypes = [vp, vp, vp]
    L.rmx_eval.argtypes = [vp, _dp, _dp, _dp, C.c_double, _dp, _dp]
    L.rmx_eval_mfd.argtypes = [vp, _dp, _dp, _dp, _dp, _dp]
    L.rmx_compute_values.argtypes = [vp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
    L.rmx_step_bdf1.argtypes = [vp, C.POINTER(Opts), C.c_int, C.POINTER(Stats), _dp, _dp]
    L.rmx_step_bdf2.argtypes = [vp, C.POINTER(Opts), C.c_int, C.POINTER(Stats), _dp, _dp]
    L.rmx_step_history.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.POINTER(Stats), C.POINTER(History)]
    L.rmx_step_euler.argtypes = [vp, C.c_double, C.c_int, _dp, _dp]
    L.rmx_adjoint_bdf1.argtypes = [vp, C.POINTER(Opts), C.c_int, C.POINTER(TaskPointPos), _dp, _dp, _dp, C.POINTER(Stats)]
    L.rmx_adjoint_bdf2.argtypes = L.rmx_adjoint_bdf1.argtypes
    L.rmx_adjoint_bdf1_device.argtypes = [vp, C.POINTER(Opts), C.c_int, C.POINTER(TaskPointPos), vp, vp, vp, C.POINTER(Stats)]
    L.rmx_adjoint_bdf2_device.argtypes = L.rmx_adjoint_bdf1_device.argtypes
    L.rmx_adjoint_controls.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.POINTER(TaskPointPos), _dp, _dp, _dp, C.POINTER(Stats)]
    L.rmx_adjoint_controls_device.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.POINTER(TaskPointPos), vp, vp, vp, C.POINTER(Stats)]
    L.rmx_adjoint_track.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.POINTER(TaskTrack), _dp, _dp, _dp, C.POINTER(Stats)]
    L.rmx_adjoint_track_device.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.POINTER(TaskTrack), vp, vp, vp, vp, C.POINTER(Stats)]
    L.rmx_rollout_tape.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_double, _dp, _dp, _dp, C.POINTER(Stats)]
    L.rmx_rollout_tape_device.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_double, vp, vp, vp, C.POINTER(Stats)]
    L.rmx_rollout_tape_feedback.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.c_double, C.POINTER(Feedback), _dp, _dp, _dp, C.POINTER(Stats)]
    L.rmx_rollout_tape_feedback_device.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.c_double, C.POINTER(Feedback), vp, vp, vp, C.POINTER(Stats)]
    L.rmx_rollout_vjp_feedback.argtypes = [vp, C.c_int, C.POINTER(Feedback), _dp, _dp, _dp, C.POINTER(FeedbackGrads)]
    L.rmx_rollout_vjp_feedback_device.argtypes = [vp, C.c_int, C.POINTER(Feedback), vp, vp, vp, C.POINTER(FeedbackGrads)]
    L.rmx_rollout_tape_bdf2.argtypes = L.rmx_rollout_tape.argtypes
    L.rmx_rollout_tape_bdf2_device.argtypes = L.rmx_rollout_tape_device.argtypes
    L.rmx_rollout_vjp.argtypes = [vp, C.c_int, _dp, _dp, _dp, _dp, _dp]
    L.rmx_rollout_vjp_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.rmx_rollout_linearize.argtypes = [vp, C.c_int, _dp, _dp, _dp]
    L.rmx_rollout_linearize_device.argtypes = [vp, C.c_int, vp, vp, vp]
    L.rmx_rollout_jvp.argtypes = [vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp]
    L.rmx_rollout_jvp_device.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.rmx_rollout_jvp_params.argtypes = [vp, C.c_int, C.c_int, C.POINTER(ParamTangents), _dp, _dp, _dp, _dp, _dp]
    L.rmx_rollout_jvp_params_device.argtypes = [vp, C.c_int, C.c_int, C.POINTER(ParamTangents), vp, vp, vp, vp, vp]
    L.rmx_rollout_lqr.argtypes = [vp, C.c_int, C.POINTER(LqrCost), C.POINTER(LqrGains)]
    L.rmx_rollout_lqr_device.argtypes = L.rmx_rollout_lqr.argtypes
    L.rmx_rollout_tape_feedback_box.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.c_double, C.POINTER(Feedback), C.POINTER(Box), _dp, _dp, _dp,
                                                C.POINTER(Stats)]
    L.rmx_rollout_tape_feedback_box_device.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.c_double, C.POINTER(Feedback), C.POINTER(Box), vp, vp,
                                                       vp, C.POINTER(Stats)]
    L.rmx_rollout_lqr_box.argtypes = [vp, C.c_int, C.POINTER(LqrCost), C.POINTER(Box), vp, C.c_int, C.POINTER(LqrGains), vp]
    L.rmx_rollout_lqr_box_device.argtypes = L.rmx_rollout_lqr_box.argtypes
    L.rmx_rollout_points.argtypes = [vp, C.c_int, vp, C.POINTER(PointTerms), vp, vp, vp]
    L.rmx_rollout_points_device.argtypes = L.rmx_rollout_points.argtypes
    L.rmx_rollout_cost.argtypes = [vp, C.c_int, vp, vp, C.POINTER(StateCost), C.POINTER(PointTerms), C.POINTER(CostModel)]
    L.rmx_rollout_cost_device.argtypes = L.rmx_rollout_cost.argtypes
    L.rmx_rollout_frames.argtypes = [vp, C.c_int, vp, vp, C.POINTER(FrameTerms), vp, vp, vp, vp, vp, vp, vp, vp]
    L.rmx_rollout_frames_device.argtypes = L.rmx_rollout_frames.argtypes
    L.rmx_rollout_cost_frames.argtypes = [vp, C.c_int, vp, vp, C.POINTER(StateCost), C.POINTER(FrameTerms), C.POINTER(CostModel)]
    L.rmx_rollout_cost_frames_device.argtypes = L.rmx_rollout_cost_frames.argtypes
    L.rmx_rollout_search.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_double, C.POINTER(Feedback), C.POINTER(Box), C.POINTER(Search),
                                     C.POINTER(SearchCost), vp, vp, vp, C.POINTER(SearchOut), C.POINTER(Stats)]
    L.rmx_rollout_search_device.argtypes = L.rmx_rollout_search.argtypes
    L.rmx_rollout_vjp_params.argtypes = [vp, C.c_int, _dp, _dp, _dp, _dp, _dp, C.POINTER(ParamGrads)]
    L.rmx_rollout_vjp_params_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(ParamGrads)]
    L.rmx_rollout_vjp_forces.argtypes = [vp, C.c_int, _dp, _dp, _dp, _dp, _dp, C.POINTER(ParamGrads), C.POINTER(ForceGrads)]
    L.rmx_rollout_vjp_forces_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(ParamGrads), C.POINTER(ForceGrads)]
    L.rmx_step_ticks.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    L.rmx_energy.argtypes = [vp, _dp, _dp]
    L.rmx_last_step_ms.argtypes = [vp]
    L.rmx_last_step_ms.restype = C.c_double
    L.rmx_last_step_kernel.argtypes = [vp]
    L.rmx_last_step_kernel.restype = C.c_char_p
    L.rmx_batch_stream.argtypes = [vp]
    L.rmx_batch_stream.restype = vp
    L.rmx_step_bdf1_async.argtypes = [vp, C.POINTER(Opts), C.c_int]
    L.rmx_sync.argtypes = [vp]
    L.rmx_step_bdf2_async.argtypes = [vp, C.POINTER(Opts), C.c_int]
    L.rmx_step_history_async.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.c_int]
    L.rmx_history_read.argtypes = [vp, C.POINTER(History)]
    L.rmx_group_create.argtypes = [C.POINTER(ModelDesc), C.POINTER(GroundContact), C.c_int, _ip, C.c_int, C.POINTER(vp)]
    L.rmx_group_destroy.argtypes = [vp]
    L.rmx_group_batch_size.argtypes = [vp]
    L.rmx_group_nshards.argtypes = [vp]
    L.rmx_group_shard.argtypes = [vp, C.c_int, _ip, _ip, _ip]
    L.rmx_group_shard_batch.argtypes = [vp, C.c_int]
    L.rmx_group_shard_batch.restype = vp
    L.rmx_group_shard_model.argtypes = [vp, C.c_int]
    L.rmx_group_shard_model.restype = vp
    L.rmx_group_set_state.argtypes = [vp, _dp, _dp]
    L.rmx_group_get_state.argtypes = [vp, _dp, _dp]
    L.rmx_group_step.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.POINTER(Stats), C.POINTER(History)]
    L.rmx_group_step_async.argtypes = [vp, C.POINTER(Opts), C.c_int, C.c_int, C.c_int]
    L.rmx_group_sync.argtypes = [vp, C.POINTER(Stats), C.POINTER(History)]
    L.rmx_group_energy.argtypes = [vp, _dp, _dp]
    L.rmx_group_gather_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    L.rmx_group_gather_path.argtypes = [vp]
    L.rmx_group_gather_path.restype = C.c_char_p
    L.rmx_group_gather.argtypes = [vp, C.c_int]
    L.rmx_group_gathered.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.rmx_group_gathered_read.argtypes = [vp, C.c_int, _dp, _dp]
    L.rmx_group_timing.argtypes = [vp, _dp, _dp, _dp, _dp]
    L.rmx_stats_reset.argtypes = [vp]
    L.rmx_profile_phases.argtypes = [vp, C.c_int, C.c_double, _dp]
    L.rmx_stats_read.argtypes = [vp, C.POINTER(Stats)]
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        msg = lib().rmx_last_error()
        raise RedMaxHipError("%s failed (%d): %s" % (what or "redmax_hip call", rc, msg.decode() if msg else "?"))


def dptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def iptr(a):
    return a.ctypes.data_as(_ip) if a is not None else None


def make_ground_contact(d, keep):
    """scene.forces (ForceGroundCuboid objects) of a Scene.desc() dict -> GroundContact, or None when the scene has none."""
    if d.get("contact") is None or not np.any(d["contact"]):
        return None
    g = d["ground"]
    gc = GroundContact()
    keep["contact"] = np.ascontiguousarray(d["contact"], dtype=np.int32)
    keep["sides"] = np.ascontiguousarray(d["sides"], dtype=np.float64)
    gc.flags, gc.sides = iptr(keep["contact"]), dptr(keep["sides"])
    gc.E[:] = list(np.asarray(g["E"], dtype=np.float64).reshape(4, 4).T.reshape(16))
    gc.kn, gc.kt, gc.mu, gc.kd = float(g["kn"]), float(g["kt"]), float(g["mu"]), float(g["kd"])
    gb = d.get("ground_body")
    if gb is not None:        # force objects with their own frames / constants, listing order; [n][4][4] row-major -> column-major
        keep["gE"] = np.ascontiguousarray(np.asarray(gb["E"], dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1).reshape(-1, 16))
        gc.E_body = dptr(keep["gE"])
        for k in ("kn", "kt", "mu", "kd"):
            keep["g" + k] = np.ascontiguousarray(gb[k], dtype=np.float64)
            setattr(gc, k + "_body", dptr(keep["g" + k]))
    return gc


def make_point_forces(d, keep):
    """desc()["point_forces"] (ForcePointPoint / ForceSpringDamper / ForceCable of a Scene) -> (array of PointForce, count), or
    (None, 0) when the scene has none."""
    pfs = d.get("point_forces")
    if not pfs:
        return None, 0
    arr = (PointForce * len(pfs))()
    keep["pf"] = []
    for a, f in zip(arr, pfs):
        body = np.ascontiguousarray(f["body"], dtype=np.int32)
        x = np.ascontiguousarray(f["x"], dtype=np.float64).reshape(-1, 3)
        if len(body) != len(x):
            raise ValueError("point force: body and x must have one entry per point")
        keep["pf"].append((body, x))
        a.kind, a.npts = int(f["kind"]), len(body)
        a.body, a.x = iptr(body), dptr(x)
        a.stiffness, a.damping, a.L = float(f["stiffness"]), float(f["damping"]), float(f.get("L", 0.0))
    return arr, len(pfs)


def make_desc(d):
    """dict from redmax.Scene.desc() -> (ModelDesc, keepalive)."""
    keep = {}

    def f64(k):
        keep[k] = np.ascontiguousarray(d[k], dtype=np.float64)
        return keep[k].ctypes.data_as(_dp)

    def i32(k):
        keep[k] = np.ascontiguousarray(d[k], dtype=np.int32)
        return keep[k].ctypes.data_as(_ip)

    s = ModelDesc()
    s.njoints = int(d["njoints"])
    s.parent, s.type = i32("parent"), i32("type")
    for k in ("axis", "E0_pj", "E0_ji", "I_i", "qRest", "tau", "stiffness", "damping", "qLimL", "qLimU", "qLimK", "qLimD"):
        setattr(s, k, f64(k))
    for i in range(3):
        s.grav[i] = float(d["grav"][i])
    s.plane = f64("plane") if d.get("plane") is not None else None
    s.qRestR = f64("qRestR") if d.get("qRestR") is not None and len(d["qRestR"]) else None
    return s, keep
