"""The words of the Python bindings' argument checks, on a CPU.

Every ValueError that BatchSim's taped-rollout and adjoint_controls / adjoint_track entries and the functions of redmax_amd.diff
raise before their first call into the library is API: the GPU tests match on the text.  None of those checks needs a device, so they
are pinned here, whole message by whole message, through the public entry points: a BatchSim made with __new__ (no library, no
model: B = 3 rollouts, nr = 2 DOFs) stands for the sim, and the tensors of the diff functions are made under FakeTensorMode, where a
"cuda:0" tensor has its device, dtype and shape and no memory.  A check that lets a call through ends in an AttributeError on the
library handle the shell does not have.
"""
import types

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from redmax_amd import _abi, diff
from redmax_amd.batch import BatchSim

B, NR, N = 3, 2, 4


def shell(**extra):
    s = BatchSim.__new__(BatchSim)
    s.B, s.nr, s.device, s._tape_integrator, s.tape_count = B, NR, 0, 1, 0
    s.opts = _abi.Opts()                                    # (a plain struct: rollout_feedback copies it before it reads ulim)
    s._desc = types.SimpleNamespace(njoints=2)              # (_param_shapes reads the joint count)
    for k, v in extra.items():
        setattr(s, k, v)
    return s


def refused(msg, fn, *args, **kw):
    """fn(*args, **kw) raises ValueError with exactly msg."""
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == msg


def reaches_library(fn, *args, **kw):
    """fn(*args, **kw) passes every check: the shell's missing library handle is what stops it."""
    with pytest.raises(AttributeError) as e:
        fn(*args, **kw)
    assert "_L" in str(e.value)


def z(*shape):
    return np.zeros(shape)


TASK = dict(body=0, xlocal=[0.0, 0.0, 0.0], xtarget=[0.0, 0.0, 0.0], step=N, pscale=1.0, wreg=0.0, wpos=1.0)
TERM = dict(body=0, xlocal=[0.0, 0.0, 0.0], step=N, wpos=1.0)
WANT_FB = "'duff', 'dK', 'dxref', 'dq0', 'dqd0'"
WANT_P = "'stiffness', 'damping', 'qrest', 'inertia', 'grav'"


# ---- BatchSim ----

def test_adjoint_controls():
    s = shell()
    refused("adjoint_controls: u is None", s.adjoint_controls, N, 0.01, TASK, None)
    refused("adjoint_controls: u must have shape (3, 4, 2) or (4, 2), got (3, 5, 2)", s.adjoint_controls, N, 0.01, TASK, z(B, 5, NR))
    refused("adjoint_controls: u must have shape (3, 4, 2) or (4, 2), got (4, 3)", s.adjoint_controls, N, 0.01, TASK, z(N, 3))
    assert s.tape_count == 0


def test_adjoint_track():
    s = shell()
    task = dict(terms=[TERM], xtarget=z(1, 3), pscale=1.0, wreg=0.0)
    refused("adjoint_track: u is None", s.adjoint_track, N, 0.01, task, None)
    refused("adjoint_track: u must have shape (3, 4, 2) or (4, 2), got (3, 4, 3)", s.adjoint_track, N, 0.01, task, z(B, N, 3))
    u = z(B, N, NR)
    bad = dict(task, terms=[dict(TERM, xlocal=[0.0, 0.0])])
    refused("adjoint_track: a term's xlocal must have shape (3,), got (2,)", s.adjoint_track, N, 0.01, bad, u)
    refused("adjoint_track: xtarget is None", s.adjoint_track, N, 0.01, dict(task, xtarget=None), u)
    refused("adjoint_track: xtarget must have shape (1, 3) or (3, 1, 3), got (2, 3)", s.adjoint_track, N, 0.01, dict(task, xtarget=z(2, 3)), u)
    refused("adjoint_track: xtarget must have shape (2, 3) or (3, 2, 3), got (3, 1, 3)", s.adjoint_track, N, 0.01,
            dict(task, terms=[TERM, dict(TERM, t=0.02)], xtarget=z(B, 1, 3)), u)
    assert s.tape_count == 0


def test_rollout_tape():
    # (the entry is looked up by name behind the integrator check and before the checks of u: the shell needs the two names)
    s = shell(_L=types.SimpleNamespace(rmx_rollout_tape=None, rmx_rollout_tape_bdf2=None))
    refused("rollout_tape: integrator must be 1 (BDF1) or 2 (BDF2), got 3", s.rollout_tape, N, 0.01, z(B, N, NR), integrator=3)
    refused("rollout_tape: integrator must be 1 (BDF1) or 2 (BDF2), got 3", s.rollout_tape, N, 0.01, None, integrator=3)
    refused("rollout_tape: u is None", s.rollout_tape, N, 0.01, None)
    refused("rollout_tape: u is None", s.rollout_tape, N, 0.01, None, integrator=2)
    refused("rollout_tape: u must have shape (3, 4, 2) or (4, 2), got (3, 4, 3)", s.rollout_tape, N, 0.01, z(B, N, 3))
    refused("rollout_tape: integrator must be 1 (BDF1) or 2 (BDF2), got 0", s.rollout_tape_device, N, 0.01, 0, 0, 0, integrator=0)
    assert s.tape_count == 0 and s._tape_integrator == 1


def test_rollout_feedback():
    s = shell()
    uff = z(B, N, NR)
    refused("rollout_feedback: integrator must be 1 (BDF1) or 2 (BDF2), got 3", s.rollout_feedback, N, 0.01, None, integrator=3)
    refused("rollout_feedback: uff is None", s.rollout_feedback, N, 0.01, None)
    refused("rollout_feedback: uff must have shape (3, 4, 2) or (4, 2), got (4, 3)", s.rollout_feedback, N, 0.01, z(N, 3))
    refused("rollout_feedback: K must have shape (4, 4, 2) or (3, 4, 4, 2), got (4, 4, 3)", s.rollout_feedback, N, 0.01, uff, K=z(N, 4, 3))
    refused("rollout_feedback: xref must have shape (4, 4) or (3, 4, 4), got (4, 5)", s.rollout_feedback, N, 0.01, uff, xref=z(N, 5))
    mixed = "rollout_feedback: K and xref must both be shared by the batch or both hold one table per rollout"
    refused(mixed, s.rollout_feedback, N, 0.01, uff, K=z(N, 4, 2), xref=z(B, N, 4))
    refused(mixed, s.rollout_feedback, N, 0.01, uff, K=z(B, N, 4, 2), xref=z(N, 4))
    refused("rollout_feedback: integrator must be 1 (BDF1) or 2 (BDF2), got 3", s.rollout_feedback_device, N, 0.01, 0, 0, 0, 0, 0, 0,
            integrator=3)
    assert s.tape_count == 0
    # ulim is read behind the point where the call has claimed the tape
    refused("rollout_feedback: ulim must be a pair (ulo, uhi), either may be None", s.rollout_feedback, N, 0.01, uff, ulim=z(NR))
    assert s.tape_count == 1
    refused("rollout_feedback: ulim must be a pair (ulo, uhi), either may be None", s.rollout_feedback, N, 0.01, uff, ulim=(None,))
    refused("rollout_feedback: ulo must have shape (2,), got (3,)", s.rollout_feedback, N, 0.01, uff, ulim=(z(3), None), integrator=2)
    refused("rollout_feedback: uhi must have shape (2,), got (1, 2)", s.rollout_feedback, N, 0.01, uff, ulim=(None, z(1, NR)))
    assert s.tape_count == 4 and s._tape_integrator == 1


def test_rollout_vjp():
    s = shell()
    refused("rollout_vjp: gq and gqd must have shape (3, 4, 2), got (3, 4, 2) and (3, 5, 2)", s.rollout_vjp, N, z(B, N, NR), z(B, 5, NR))
    refused("rollout_vjp: gq and gqd must have shape (3, 4, 2), got (4, 2) and (3, 4, 2)", s.rollout_vjp, N, z(N, NR), z(B, N, NR))
    reaches_library(s.rollout_vjp, N, z(B, N, NR), z(B, N, NR))
    assert s.tape_count == 0


def test_rollout_vjp_feedback():
    s = shell()
    g = z(B, N, NR)
    refused("rollout_vjp_feedback: want must name distinct outputs among %s, got ('nope',)" % WANT_FB, s.rollout_vjp_feedback, N, g, g,
            want="nope")
    refused("rollout_vjp_feedback: want must name distinct outputs among %s, got ('duff', 'duff')" % WANT_FB, s.rollout_vjp_feedback, N, g,
            g, want=("duff", "duff"))
    refused("rollout_vjp_feedback: gq and gqd must have shape (3, 4, 2), got (3, 4, 3) and (3, 4, 2)", s.rollout_vjp_feedback, N,
            z(B, N, 3), g)
    refused("rollout_vjp_feedback: gu must have shape (3, 4, 2), got (3, 4, 3)", s.rollout_vjp_feedback, N, g, g, gu=z(B, N, 3))
    refused("rollout_vjp_feedback: K must have shape (4, 4, 2) or (3, 4, 4, 2), got (4, 2, 4)", s.rollout_vjp_feedback, N, g, g,
            K=z(N, 2, 4))
    refused("rollout_vjp_feedback: xref must have shape (4, 4) or (3, 4, 4), got (3, 4)", s.rollout_vjp_feedback, N, g, g, K=z(N, 4, 2),
            xref=z(B, 4))
    refused("rollout_vjp_feedback: K and xref must both be shared by the batch or both hold one table per rollout",
            s.rollout_vjp_feedback, N, g, g, K=z(N, 4, 2), xref=z(B, N, 4))
    reaches_library(s.rollout_vjp_feedback, N, g, g, want=())      # an empty list is the library's to refuse
    assert s.tape_count == 0


def test_rollout_vjp_params():
    s = shell()
    g = z(B, N, NR)
    refused("rollout_vjp_params: want must name distinct outputs among %s, got ()" % WANT_P, s.rollout_vjp_params, N, g, g, want=())
    refused("rollout_vjp_params: want must name distinct outputs among %s, got ('mass',)" % WANT_P, s.rollout_vjp_params, N, g, g,
            want="mass")
    refused("rollout_vjp_params: want must name distinct outputs among %s, got ('grav', 'grav')" % WANT_P, s.rollout_vjp_params, N, g, g,
            want=["grav", "grav"])
    refused("rollout_vjp_params: gq and gqd must have shape (3, 4, 2), got (3, 4, 2) and (3, 4)", s.rollout_vjp_params, N, g, z(B, N))
    assert s._param_shapes() == {"stiffness": (2,), "damping": (2,), "qrest": (2,), "inertia": (2, 6), "grav": (3,)}
    reaches_library(s.rollout_vjp_params, N, g, g, want="grav")
    assert s.tape_count == 0


def test_rollout_linearize():
    s = shell()
    refused("rollout_linearize: which must name distinct outputs among 'XA', 'XB', 'XU', got ('XA', 'XA')", s.rollout_linearize, N,
            which=("XA", "XA"))
    refused("rollout_linearize: which must name distinct outputs among 'XA', 'XB', 'XU', got ('XC',)", s.rollout_linearize, N, which="XC")
    reaches_library(s.rollout_linearize, N, which=())      # an empty list is the library's to refuse
    assert s.tape_count == 0


def test_rollout_jvp():
    s = shell()
    refused("rollout_jvp: all tangents are None", s.rollout_jvp, N)
    refused("rollout_jvp: tu must have shape (3, 2, 4, 2) - or, every input alike, that shape without the direction axis -, "
            "got (3, 2, 5, 2)", s.rollout_jvp, N, tu=z(B, 2, 5, NR))
    refused("rollout_jvp: tu must have shape (3, 1, 4, 2) - or, every input alike, that shape without the direction axis -, "
            "got (3, 5, 2)", s.rollout_jvp, N, tu=z(B, 5, NR))
    refused("rollout_jvp: tqd0 must have shape (3, 2, 2) - or, every input alike, that shape without the direction axis -, "
            "got (3, 2)", s.rollout_jvp, N, tq0=z(B, 2, NR), tqd0=z(B, NR))
    reaches_library(s.rollout_jvp, N, tq0=z(B, NR))
    assert s.tape_count == 0


@pytest.mark.parametrize("box", [False, True])
def test_rollout_lqr(box):
    s = shell()
    who = "rollout_lqr_box" if box else "rollout_lqr"
    lx, lu, Q, R, ubar = z(B, N, 4), z(B, N, NR), z(N, 4, 4), z(NR, NR), z(B, N, NR)

    def call(lx=lx, lu=lu, Q=Q, R=R, ubar=ubar, ulim=(None, None), **kw):
        if box:
            return s.rollout_lqr_box(N, lx, lu, Q, R, ubar, ulim, **kw)
        return s.rollout_lqr(N, lx, lu, Q, R, **kw)

    if box:
        refused("rollout_lqr_box: lx, lu and ubar must have shapes (3, 4, 4), (3, 4, 2) and (3, 4, 2), got (3, 4, 4), (3, 4, 2) and "
                "(3, 4, 3)", call, ubar=z(B, N, 3))
        refused("rollout_lqr_box: lx, lu and ubar must have shapes (3, 4, 4), (3, 4, 2) and (3, 4, 2), got (3, 4, 3), (3, 4, 2) and "
                "(3, 4, 2)", call, lx=z(B, N, 3))
    else:
        refused("rollout_lqr: lx and lu must have shapes (3, 4, 4) and (3, 4, 2), got (3, 4, 3) and (3, 4, 2)", call, lx=z(B, N, 3))
        refused("rollout_lqr: lx and lu must have shapes (3, 4, 4) and (3, 4, 2), got (3, 4, 4) and (4, 2)", call, lu=z(N, NR))
    refused("%s: Q must have shape (4, 4, 4) or (3, 4, 4, 4), got (4, 4, 3)" % who, call, Q=z(N, 4, 3))
    refused("%s: R must have shape (2, 2), got (2, 3)" % who, call, R=z(NR, 3))
    refused("%s: R must have shape (2, 2), got (2, 3)" % who, call, R=z(NR, 3), mu_b=z(2))      # (R is looked at first)
    refused("%s: mu_b must have shape (3,), got (2,)" % who, call, Q=z(B, N, 4, 4), mu_b=z(2))
    if box:
        refused("rollout_lqr_box: ulim must be a pair (ulo, uhi), either may be None", call, ulim=None)
        refused("rollout_lqr_box: uhi must have shape (2,), got (3,)", call, ulim=[z(NR), z(3)])
    reaches_library(call, mu_b=z(B))
    assert s.tape_count == 0


def test_rollout_points():
    s = shell()
    q = z(B, N, NR)
    refused("rollout_points: q must have shape (3, 4, 2), got (3, 4, 3)", s.rollout_points, N, z(B, N, 3), [TERM])
    refused("rollout_points: a term's xlocal must have shape (3,), got (2,)", s.rollout_points, N, q, [dict(TERM, xlocal=[1.0, 2.0])])
    refused("rollout_points: gx must have shape (3, 1, 3), got (3, 2, 3)", s.rollout_points, N, q, [TERM], gx=z(B, 2, 3))
    refused("rollout_points_device: a term's xlocal must have shape (3,), got (4,)", s.rollout_points_device, N, 0, [dict(TERM, xlocal=z(2, 2))])
    reaches_library(s.rollout_points, N, q, [dict(body=1, xlocal=[[0.0], [0.0], [0.0]], step=1)])      # (no wpos; xlocal is flattened)
    assert s.tape_count == 0


def test_rollout_cost():
    s = shell()
    q = z(B, N, NR)
    refused("rollout_cost: want must name distinct outputs among 'Jk', 'lx', 'Q', got ()", s.rollout_cost, N, q, q, want=())
    refused("rollout_cost: want must name distinct outputs among 'Jk', 'lx', 'Q', got ('J',)", s.rollout_cost, N, q, q, want="J")
    refused("rollout_cost: want must name distinct outputs among 'Jk', 'lx', 'Q', got ('lx', 'lx')", s.rollout_cost, N, q, q, want=("lx", "lx"))
    refused("rollout_cost: q and qdot must have shape (3, 4, 2), got (3, 4, 2) and (3, 5, 2)", s.rollout_cost, N, q, z(B, 5, NR))
    refused("rollout_cost: Q must have shape (4, 4, 4) or (3, 4, 4, 4), got (4, 4, 3)", s.rollout_cost, N, q, q, Q=z(N, 4, 3))
    refused("rollout_cost: xgoal must have shape (4, 4) or (3, 4, 4), got (4, 5)", s.rollout_cost, N, q, q, Q=z(N, 4, 4), xgoal=z(N, 5))
    refused("rollout_cost: a term's xlocal must have shape (3,), got (1,)", s.rollout_cost, N, q, q, terms=[dict(TERM, xlocal=[0.0])])
    refused("rollout_cost: xtarget is None", s.rollout_cost, N, q, q, terms=[TERM])
    refused("rollout_cost: xtarget must have shape (1, 3) or (3, 1, 3), got (2, 3)", s.rollout_cost, N, q, q, terms=[TERM], xtarget=z(2, 3))
    refused("rollout_cost_device: a term's xlocal must have shape (3,), got (1,)", s.rollout_cost_device, N, 0, 0, terms=[dict(TERM, xlocal=[0.0])])
    reaches_library(s.rollout_cost, N, q, q, xgoal=z(B, N, 4), terms=[TERM], xtarget=z(B, 1, 3), want="Jk")
    assert s.tape_count == 0


def test_private_helpers_keep_their_shape():
    """What tests and tools call by name: _tape_opts, _track_task, _point_terms."""
    s = shell()
    s.opts.h, s.opts.iterMaxPerDof, s.opts.tol = 0.5, 9, 1e-7
    o = s._tape_opts(0.01)
    assert (o.h, o.iterMaxPerDof, o.tol) == (0.01, 5, 1e-7) and s._tape_opts(None).h == 0.5 and s.opts.iterMaxPerDof == 9
    terms = [dict(body=2, xlocal=[1.0, 2.0, 3.0], t=0.03, wpos=4.0), dict(body=0, xlocal=(0.0, 0.0, 1.0), step=2, wpos=0.5)]
    xt = np.arange(6.0).reshape(2, 3)
    tk, opts, keep = s._track_task(dict(terms=terms, xtarget=xt, pscale=2.0, wreg=0.25), 0.01, N)
    assert s.tape_count == 1 and (opts.h, opts.iterMaxPerDof) == (0.01, 5)
    assert (tk.nterms, tk.per_rollout, tk.pscale, tk.wreg) == (2, 0, 2.0, 0.25)
    assert [(tk.terms[i].body, tk.terms[i].step, tk.terms[i].wpos, list(tk.terms[i].xlocal)) for i in range(2)] == \
        [(2, 3, 4.0, [1.0, 2.0, 3.0]), (0, 2, 0.5, [0.0, 0.0, 1.0])]
    assert [tk.xtarget[i] for i in range(6)] == list(range(6)) and len(keep) == 2
    tk, _, _ = s._track_task(dict(terms=terms, xtarget=np.zeros((B, 2, 3)), pscale=1.0, wreg=0.0), 0.01, N)
    assert tk.per_rollout == 1
    tk, _, keep = s._track_task(dict(terms=terms, per_rollout=True, pscale=1.0, wreg=0.0), 0.01, N, device_targets=True)
    assert tk.per_rollout == 1 and not tk.xtarget and s.tape_count == 3
    arr, n = BatchSim._point_terms([dict(body=1, xlocal=[0.0, 1.0, 0.0], step=3)], "who", False)
    assert n == 1 and (arr[0].body, arr[0].step, arr[0].wpos, list(arr[0].xlocal)) == (1, 3, 0.0, [0.0, 1.0, 0.0])
    arr, n = BatchSim._point_terms([], "who", True)
    assert n == 0 and len(arr) == 1
    with pytest.raises(KeyError):
        BatchSim._point_terms([dict(body=1, xlocal=[0.0, 1.0, 0.0], step=3)], "who", True)


# ---- redmax_amd.diff ----

@pytest.fixture(scope="module")
def fake():
    with FakeTensorMode() as mode:
        yield mode


def t64(*shape, dtype=torch.float64, device="cuda:0"):
    return torch.empty(shape, dtype=dtype, device=device)


TYPE = "%s: %s must be a torch.Tensor, got ndarray"
F32 = "%s: %s must be float64, got torch.float32"
CPU = "%s: %s must be on cuda:0 (the sim's device), got cpu"


def test_diff_rollout(fake):
    s = shell()
    q0, u = t64(B, NR), t64(B, N, NR)
    refused("rollout: integrator must be 1 (BDF1) or 2 (BDF2), got 3", diff.rollout, s, q0, q0, u, h=0.01, integrator=3)
    refused(TYPE % ("rollout", "q0"), diff.rollout, s, z(B, NR), q0, u, h=0.01)
    refused("rollout: u must be a torch.Tensor, got NoneType", diff.rollout, s, q0, q0, None, h=0.01)
    refused(F32 % ("rollout", "u"), diff.rollout, s, q0, q0, t64(B, N, NR, dtype=torch.float32), h=0.01)
    refused(CPU % ("rollout", "qdot0"), diff.rollout, s, q0, t64(B, NR, device="cpu"), u, h=0.01)
    refused(F32 % ("rollout", "q0"), diff.rollout, s, t64(B, NR, dtype=torch.float32), z(B, NR), u, h=0.01)      # (input by input)
    refused("rollout: u must have shape (3, nsteps, 2), got (3, 4, 3)", diff.rollout, s, q0, q0, t64(B, N, 3), h=0.01)
    refused("rollout: u must have shape (3, nsteps, 2), got (3, 0, 2)", diff.rollout, s, q0, q0, t64(B, 0, NR), h=0.01)
    refused("rollout: u must have shape (3, nsteps, 2), got (4, 2)", diff.rollout, s, q0, q0, t64(N, NR), h=0.01)
    refused("rollout: qdot0 must have shape (3, 2), got (3, 3)", diff.rollout, s, q0, t64(B, 3), u, h=0.01)
    refused("rollout: q0 must have shape (3, 2), got (2,)", diff.rollout, s, t64(NR), q0, u, h=0.01)
    diff._check_inputs(s, q0, q0, u)

    def params(p):
        return diff.rollout(s, q0, q0, u, h=0.01, params=p)

    refused("rollout: params must be a dict of tensors (model_params(sim) or part of it), got list", params, [q0])
    refused("rollout: unknown model parameter 'mass' (known: stiffness, damping, qrest, inertia, grav)", params, {"grav": t64(3), "mass": q0})
    refused("rollout: params names no parameter (pass None for a rollout without parameter gradients)", params, {})
    refused("rollout: params['stiffness'] must be a torch.Tensor, got ndarray", params, {"stiffness": z(NR)})
    refused("rollout: params['damping'] must be float64, got torch.float32", params, {"damping": t64(NR, dtype=torch.float32)})
    refused("rollout: params['qrest'] must be on cuda:0 (the sim's device), got cpu", params, {"qrest": t64(NR, device="cpu")})
    refused("rollout: params['inertia'] must have shape (2, 6), got (2, 5)", params, {"grav": t64(3), "inertia": t64(2, 5)})
    refused("rollout: params['grav'] must have shape (3,), got (2,)", params, {"grav": t64(2)})
    assert s.tape_count == 0


def test_diff_linearize(fake):
    s = shell()
    q0, u = t64(B, NR), t64(B, N, NR)
    refused("linearize: integrator must be 1 (BDF1), got 2: the BDF2 assembly needs the augmented state "
            "(BatchSim.rollout_linearize returns the per-solve sensitivities of a BDF2 tape)", diff.linearize, s, q0, q0, u, h=0.01,
            integrator=2)
    refused("rollout: u must have shape (3, nsteps, 2), got (3, 4, 3)", diff.linearize, s, q0, q0, t64(B, N, 3), h=0.01)
    assert s.tape_count == 0


def test_diff_rollout_feedback(fake):
    s = shell()
    q0, u = t64(B, NR), t64(B, N, NR)

    def call(**kw):
        return diff.rollout_feedback(s, q0, q0, u, h=0.01, **kw)

    refused("rollout: integrator must be 1 (BDF1) or 2 (BDF2), got 0", call, integrator=0)
    refused("rollout: integrator must be 1 (BDF1) or 2 (BDF2), got 0", diff.rollout_closed_loop, s, q0, q0, u, None, h=0.01, integrator=0)
    refused(F32 % ("rollout", "u"), diff.rollout_feedback, s, q0, q0, t64(B, N, NR, dtype=torch.float32), h=0.01)
    refused(TYPE % ("rollout", "K"), call, K=z(N, 4, 2))
    refused(F32 % ("rollout", "K"), call, K=t64(N, 4, 2, dtype=torch.float32))
    refused(CPU % ("rollout", "xref"), call, K=t64(N, 4, 2), xref=t64(N, 4, device="cpu"))
    refused("rollout: K must have shape (4, 4, 2) or (3, 4, 4, 2), got (4, 4, 3)", call, K=t64(N, 4, 3))
    refused("rollout: xref must have shape (4, 4) or (3, 4, 4), got (4, 5)", call, xref=t64(N, 5))
    refused("rollout: K and xref must both be shared by the batch or both hold one table per rollout", call, K=t64(N, 4, 2), xref=t64(B, N, 4))
    refused("rollout: ulim must be a pair (ulo, uhi), either may be None", call, ulim=t64(NR))
    refused("rollout: ulo must be a float64 tensor of shape (2,) on cuda:0", call, ulim=(t64(3), None))
    refused("rollout: uhi must be a float64 tensor of shape (2,) on cuda:0", call, ulim=(None, t64(NR, dtype=torch.float32)))
    refused("rollout: uhi must be a float64 tensor of shape (2,) on cuda:0", call, ulim=(t64(NR), z(NR)))
    refused("rollout: ulo must be a float64 tensor of shape (2,) on cuda:0", call, ulim=[t64(NR, device="cpu"), t64(NR)])
    assert s.tape_count == 0


@pytest.mark.parametrize("box", [False, True])
def test_diff_lqr_backward(fake, box):
    s = shell()
    who = "lqr_backward_box" if box else "lqr_backward"
    lx, lu, Q, R, ubar = t64(B, N, 4), t64(B, N, NR), t64(N, 4, 4), t64(NR, NR), t64(B, N, NR)

    def call(lx=lx, lu=lu, Q=Q, R=R, ubar=ubar, ulim=(None, None)):
        if box:
            return diff.lqr_backward_box(s, lx, lu, Q, R, ubar, ulim)
        return diff.lqr_backward(s, lx, lu, Q, R)

    refused(TYPE % (who, "lu"), call, lu=z(B, N, NR))
    refused(F32 % (who, "lx"), call, lx=t64(B, N, 4, dtype=torch.float32))
    refused(CPU % (who, "Q"), call, Q=t64(N, 4, 4, device="cpu"))
    refused(F32 % (who, "R"), call, R=t64(NR, NR, dtype=torch.float32))
    refused("%s: lu must have shape (3, nsteps, 2), got (3, 4, 3)" % who, call, lu=t64(B, N, 3))
    if box:
        refused(F32 % (who, "ubar"), call, ubar=t64(B, N, NR, dtype=torch.float32))
        refused("lqr_backward_box: lx and ubar must have shapes (3, 4, 4) and (3, 4, 2), got (3, 4, 3) and (3, 4, 2)", call, lx=t64(B, N, 3))
        refused("lqr_backward_box: lx and ubar must have shapes (3, 4, 4) and (3, 4, 2), got (3, 4, 4) and (3, 5, 2)", call, ubar=t64(B, 5, NR))
    else:
        refused("lqr_backward: lx must have shape (3, 4, 4), got (3, 4, 3)", call, lx=t64(B, N, 3))
    refused("%s: Q must have shape (4, 4, 4) or (3, 4, 4, 4), got (4, 4, 3)" % who, call, Q=t64(N, 4, 3))
    refused("%s: R must have shape (2, 2), got (2, 3)" % who, call, R=t64(NR, 3))
    if box:
        refused("lqr_backward_box: ulim must be a pair (ulo, uhi), either may be None", call, ulim=None)
        refused("lqr_backward_box: uhi must be a float64 tensor of shape (2,) on cuda:0", call, ulim=(None, t64(3)))
    assert s.tape_count == 0


def test_diff_points(fake):
    s = shell()
    refused(TYPE % ("points", "q"), diff.points, s, z(B, N, NR), [TERM])
    refused("points: q must have shape (3, nsteps, 2), got (3, 4, 3)", diff.points, s, t64(B, N, 3), [TERM])
    refused("points: terms is empty", diff.points, s, t64(B, N, NR), [])


def test_diff_cost_model(fake):
    s = shell()
    q = t64(B, N, NR)
    refused("cost_model: want must name distinct outputs among 'J', 'lx', 'Q', got ('Jk',)", diff.cost_model, s, q, q, want="Jk")
    refused("cost_model: want must name distinct outputs among 'J', 'lx', 'Q', got ()", diff.cost_model, s, q, q, want=())
    refused(F32 % ("cost_model", "qdtraj"), diff.cost_model, s, q, t64(B, N, NR, dtype=torch.float32))
    refused(CPU % ("cost_model", "xtarget"), diff.cost_model, s, q, q, xtarget=t64(1, 3, device="cpu"))
    refused("cost_model: qtraj must have shape (3, nsteps, 2), got (3, 4, 3)", diff.cost_model, s, t64(B, N, 3), q)
    refused("cost_model: qdtraj must have shape (3, 4, 2), got (3, 5, 2)", diff.cost_model, s, q, t64(B, 5, NR))
    refused("cost_model: Q must have shape (4, 4, 4) or (3, 4, 4, 4), got (4, 4, 3)", diff.cost_model, s, q, q, Q=t64(N, 4, 3))
    refused("cost_model: xgoal must have shape (4, 4) or (3, 4, 4), got (4, 5)", diff.cost_model, s, q, q, xgoal=t64(N, 5))
    refused("cost_model: neither a joint-space cost (Q, xgoal) nor terms", diff.cost_model, s, q, q)
    refused("cost_model: xtarget is None", diff.cost_model, s, q, q, terms=[TERM])
    refused("cost_model: xtarget must have shape (1, 3) or (3, 1, 3), got (2, 3)", diff.cost_model, s, q, q, terms=[TERM], xtarget=t64(2, 3))


def test_diff_jvp(fake):
    s = shell()
    q0, u = t64(B, NR), t64(B, N, NR)

    def call(**kw):
        return diff.jvp(s, q0, q0, u, h=0.01, **kw)

    refused("rollout: integrator must be 1 (BDF1) or 2 (BDF2), got 3", call, integrator=3)
    refused("rollout: qdot0 must have shape (3, 2), got (3, 3)", diff.jvp, s, q0, t64(B, 3), u, h=0.01)
    refused("rollout: all tangents are None", call)
    refused(TYPE % ("rollout", "tq0"), call, tq0=z(B, NR))
    refused(F32 % ("rollout", "tu"), call, tu=t64(B, N, NR, dtype=torch.float32))
    refused(CPU % ("rollout", "tqdot0"), call, tqdot0=t64(B, NR, device="cpu"))
    refused("rollout: tu must have shape (3, 1, 4, 2) - or, every tangent alike, that shape without the direction axis -, got (3, 5, 2)",
            call, tu=t64(B, 5, NR))
    refused("rollout: tu must have shape (3, 2, 4, 2) - or, every tangent alike, that shape without the direction axis -, got (3, 2, 5, 2)",
            call, tu=t64(B, 2, 5, NR))
    refused("rollout: tqdot0 must have shape (3, 2, 2) - or, every tangent alike, that shape without the direction axis -, got (3, 2)",
            call, tq0=t64(B, 2, NR), tqdot0=t64(B, NR))
    assert s.tape_count == 0
