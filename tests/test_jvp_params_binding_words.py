"""The words of the argument checks of BatchSim.rollout_jvp_params, diff.jvp_params and diff.param_jacobian, on a CPU: every
ValueError they raise before their first call into the library, whole message by whole message, in the shell of
tests/test_binding_words.py (a BatchSim without a library: B = 3 rollouts, nr = 2 DOFs, 2 joints; fake "cuda:0" tensors).
"""
import torch

from redmax_amd import diff
from test_binding_words import B, CPU, F32, N, NR, TYPE, fake, reaches_library, refused, shell, t64, z  # noqa: F401  (fake: the fixture)

KNOWN = "stiffness, damping, qrest, inertia, grav"
AXIS = " - or, every %s alike, that shape without the direction axis -, got "


def test_rollout_jvp_params():
    s = shell()
    who = "rollout_jvp_params: "
    call = s.rollout_jvp_params
    refused(who + "tparams must be a dict of arrays over " + KNOWN + ", got list", call, N, [z(B, NR)])
    refused(who + "unknown model parameter 'mass' (known: " + KNOWN + ")", call, N, {"grav": z(B, 3), "mass": z(B, NR)})
    refused(who + "tparams names no parameter (rollout_jvp is the call for tangents of u, q0 and qdot0 alone)", call, N, {})
    refused(who + "tparams names no parameter (rollout_jvp is the call for tangents of u, q0 and qdot0 alone)", call, N, {}, tu=z(B, N, NR))
    refused(who + "every tangent must carry the same number of directions, got 2 and 3", call, N, {"grav": z(B, 2, 3), "damping": z(B, 3, NR)})
    refused(who + "every tangent must carry the same number of directions, got 1, 2 and 5", call, N,
            {"grav": z(B, 2, 3), "inertia": z(B, 5, 2, 6)}, tq0=z(B, 1, NR))
    refused(who + "tparams['grav'] must have shape (3, 1, 3)" + AXIS % "input" + "(3, 2)", call, N, {"grav": z(B, 2)})
    refused(who + "tparams['inertia'] must have shape (3, 2, 2, 6)" + AXIS % "input" + "(3, 2, 3, 6)", call, N,
            {"stiffness": z(B, 2, NR), "inertia": z(B, 2, 3, 6)})
    refused(who + "tparams['qrest'] must have shape (3, 2, 2)" + AXIS % "input" + "(3, 2)", call, N, {"grav": z(B, 2, 3), "qrest": z(B, NR)})
    refused(who + "tu must have shape (3, 1, 4, 2)" + AXIS % "input" + "(3, 5, 2)", call, N, {"grav": z(B, 3)}, tu=z(B, 5, NR))
    refused(who + "tqd0 must have shape (3, 2, 2)" + AXIS % "input" + "(3, 2, 3)", call, N, {"damping": z(B, 2, NR)}, tqd0=z(B, 2, 3))
    refused(who + "tparams['stiffness'] must have shape (3, 2, 2)" + AXIS % "input" + "(2, 2, 2)", call, N, {"stiffness": z(2, 2, NR)})
    # what passes every check stops at the library handle the shell does not have
    reaches_library(call, N, {"grav": z(B, 3)})
    reaches_library(call, N, {"inertia": z(B, 4, 2, 6), "stiffness": z(B, 4, NR)}, tu=z(B, 4, N, NR), tq0=z(B, 4, NR))
    assert s.tape_count == 0


def test_diff_jvp_params(fake):  # noqa: F811
    s = shell()
    q0, u = t64(B, NR), t64(B, N, NR)
    who = "jvp_params: "

    def call(tparams, **kw):
        return diff.jvp_params(s, q0, q0, u, tparams, h=0.01, **kw)

    grav = {"grav": t64(B, 3)}
    refused("rollout: integrator must be 1 (BDF1) or 2 (BDF2), got 3", call, grav, integrator=3)
    refused("rollout: qdot0 must have shape (3, 2), got (3, 3)", diff.jvp_params, s, q0, t64(B, 3), u, grav, h=0.01)
    refused(who + "tparams must be a dict of tensors over " + KNOWN + ", got list", call, [t64(B, 3)])
    refused(who + "unknown model parameter 'mass' (known: " + KNOWN + ")", call, {"mass": t64(B, NR)})
    refused(who + "tparams names no parameter (jvp is the call for tangents of u, q0 and qdot0 alone)", call, {})
    refused(TYPE % ("jvp_params", "tparams['grav']"), call, {"grav": z(B, 3)})
    refused(F32 % ("jvp_params", "tparams['stiffness']"), call, {"stiffness": t64(B, NR, dtype=torch.float32)})
    refused(CPU % ("jvp_params", "tu"), call, grav, tu=t64(B, N, NR, device="cpu"))
    refused(who + "every tangent must carry the same number of directions, got 2 and 3", call, {"grav": t64(B, 2, 3)}, tq0=t64(B, 3, NR))
    refused(who + "tparams['inertia'] must have shape (3, 1, 2, 6)" + AXIS % "tangent" + "(3, 6)", call, {"inertia": t64(B, 6)})
    refused(who + "tqdot0 must have shape (3, 2, 2)" + AXIS % "tangent" + "(3, 2)", call, {"grav": t64(B, 2, 3)}, tqdot0=t64(B, NR))
    refused(who + "tparams['damping'] must have shape (3, 2, 2)" + AXIS % "tangent" + "(3, 2, 3)", call,
            {"grav": t64(B, 2, 3), "damping": t64(B, 2, 3)})
    assert s.tape_count == 0


def test_diff_param_jacobian(fake):  # noqa: F811
    s = shell()
    who = "param_jacobian: names must name distinct parameters among 'stiffness', 'damping', 'qrest', 'inertia', 'grav', got "
    refused(who + "('mass',)", diff.param_jacobian, s, N, names="mass")
    refused(who + "()", diff.param_jacobian, s, N, names=())
    refused(who + "('grav', 'grav')", diff.param_jacobian, s, N, names=("grav", "grav"))
    refused("param_jacobian: nsteps must be the number of steps of the sim's tape, got 0", diff.param_jacobian, s, 0)
