"""A differentiable controlled BDF1 or BDF2 rollout for PyTorch: ``rollout(sim, q0, qdot0, u)`` returns the trajectory, and
``backward()`` of any loss on it yields dL/du, dL/dq0 and dL/dqdot0 - and, with ``params=model_params(sim)``, the gradient with respect to
the model's own parameters (joint stiffness, damping and rest position, body inertia and mass, gravity; rmx_rollout_vjp_params_device).
On a sim whose tape carries point forces (BatchSim(..., tape_forces=True)) ``force_params=force_params(sim)`` adds the stiffness, damping
and rest length of every spring, damper and cable, and both keywords go through rmx_rollout_vjp_forces_device.

Forward is rmx_rollout_tape_device (rmx_rollout_tape_bdf2_device under integrator=2), backward rmx_rollout_vjp_device (include/redmax_hip.h): device pointers end to end, the
objective lives wholly on the PyTorch side.  Forward mode (torch.autograd.forward_ad, torch.func.jvp, torch.func.jacfwd) runs
rmx_rollout_jvp_device on the same tape; ``jvp(sim, q0, qdot0, u, ...)`` pushes several tangent directions through one tape in one
call, ``jvp_params`` does the same for tangents of the model's parameters (rmx_rollout_jvp_params_device) and ``param_jacobian`` returns
whole columns of the trajectory's Jacobian in them.  ``rollout_closed_loop`` is the same for a rollout under state feedback (rmx_rollout_tape_feedback_device forward,
rmx_rollout_vjp_feedback_device backward): autograd reaches the gains K, the reference xref and the feed-forward uff through the
closed loop.  torch is imported inside the functions: ``import redmax_amd`` does not need it.
"""
from __future__ import annotations

from ._abi import PARAM_NAMES      # (the members of rmx_param_grads / rmx_param_tangents, in their order)

_BAD_STATUS = 1 | 2 | 4      # RMX_ST_DIVERGED, RMX_ST_MAXITER, RMX_ST_NAN

_Function = None


def _function():
    """The torch.autograd.Function, made on first use (torch is not imported before)."""
    global _Function
    if _Function is not None:
        return _Function
    import torch

    class _Rollout(torch.autograd.Function):
        @staticmethod
        def forward(q0, qdot0, u, sim, h, pscale, check, integrator, names=(), *ptensors):
            # (names, ptensors: the model parameters of rollout(params=...) and the force constants of rollout(force_params=...), in
            # that order; the forward does not read their values)
            return _tape_forward(sim, q0.contiguous(), qdot0.contiguous(), u.contiguous(), h, pscale, check, integrator)

        @staticmethod
        def setup_context(ctx, inputs, output):
            # (forward and setup_context apart: the form torch.func's transforms ask of an autograd.Function)
            u, sim = inputs[2], inputs[3]
            ctx.names = tuple(inputs[8]) if len(inputs) > 8 else ()
            ctx.sim, ctx.nsteps, ctx.tape = sim, u.shape[1], sim.tape_count
            # a tape that carries point forces: rmx_rollout_vjp_forces is the entry for every parameter gradient on it
            ctx.pf_tape = bool(getattr(sim, "nforces", 0)) and bool(sim.tapes_point_forces)

        @staticmethod
        def backward(ctx, gq, gqd):
            sim, nsteps = ctx.sim, ctx.nsteps
            if sim.tape_count != ctx.tape:
                raise RuntimeError("the tape of this rollout has been replaced")
            dev = torch.device("cuda", sim.device)
            sh = (sim.B, nsteps, sim.nr)
            gq = torch.zeros(sh, dtype=torch.float64, device=dev) if gq is None else gq.contiguous()
            gqd = torch.zeros(sh, dtype=torch.float64, device=dev) if gqd is None else gqd.contiguous()
            du = torch.empty(sh, dtype=torch.float64, device=dev)
            dq0 = torch.empty((sim.B, sim.nr), dtype=torch.float64, device=dev)
            dqd0 = torch.empty_like(dq0)
            torch.cuda.current_stream(dev).synchronize()
            if not ctx.names:
                sim.rollout_vjp_device(nsteps, gq.data_ptr(), gqd.data_ptr(), du.data_ptr(), dq0.data_ptr(), dqd0.data_ptr())
                return dq0, dqd0, du, None, None, None, None, None, None      # (apply binds forward's default names=())
            from . import _abi
            shapes = {n: (sim.nforces,) for n in _abi.FORCE_PARAM_NAMES} if ctx.pf_tape else {}
            shapes.update(sim._param_shapes())
            rows = {n: torch.zeros((sim.B,) + shapes[n], dtype=torch.float64, device=dev) for n in ctx.names}
            entry = sim.rollout_vjp_forces_device if ctx.pf_tape else sim.rollout_vjp_params_device
            entry(nsteps, gq.data_ptr(), gqd.data_ptr(), du.data_ptr(), dq0.data_ptr(), dqd0.data_ptr(),
                  **{n + "_ptr": rows[n].data_ptr() for n in ctx.names})
            # one row per rollout from the library; the rollouts share the model, so the parameter's gradient is their sum
            return (dq0, dqd0, du, None, None, None, None, None, None) + tuple(rows[n].sum(dim=0) for n in ctx.names)

        @staticmethod
        def jvp(ctx, tq0, tqd0, tu, *rest):
            # forward mode (torch.autograd.forward_ad, torch.func.jvp): one rmx_rollout_jvp_device call on the tape of this rollout
            sim, nsteps = ctx.sim, ctx.nsteps
            if sim.tape_count != ctx.tape:
                raise RuntimeError("the tape of this rollout has been replaced")
            if any(t is not None for t in rest):
                raise RuntimeError("rollout: forward-mode tangents of the model parameters are not available (rmx_rollout_jvp takes "
                                   "tangents of q0, qdot0 and u)")
            if tq0 is None and tqd0 is None and tu is None:
                z = torch.zeros((sim.B, nsteps, sim.nr), dtype=torch.float64, device=torch.device("cuda", sim.device))
                return z, z.clone()
            return _Tangents.apply(tq0, tqd0, tu, sim, nsteps)

        @staticmethod
        def vmap(info, in_dims, *args):
            # (torch.func.jacfwd is vmap over jvp: the rollout itself is reached with unbatched inputs and never gets here)
            raise RuntimeError("rollout: torch.func.vmap over q0, qdot0 or u is not available - the batch axis of the sim is the batch")

    class _Tangents(torch.autograd.Function):
        """rmx_rollout_jvp_device on the sim's tape.  Under torch.func.vmap (jacfwd) the mapped axis becomes the directions of ONE call."""

        @staticmethod
        def forward(tq0, tqd0, tu, sim, nsteps):
            return _Tangents.run(sim, nsteps, 1, tq0, tqd0, tu, (sim.B, nsteps, sim.nr))

        @staticmethod
        def setup_context(ctx, inputs, output):
            pass

        @staticmethod
        def run(sim, nsteps, ntan, tq0, tqd0, tu, shape):
            dev = torch.device("cuda", sim.device)
            tq0, tqd0, tu = (None if t is None else t.contiguous() for t in (tq0, tqd0, tu))
            tq = torch.empty(shape, dtype=torch.float64, device=dev)
            tqd = torch.empty_like(tq)
            torch.cuda.current_stream(dev).synchronize()
            sim.rollout_jvp_device(nsteps, ntan, *(0 if t is None else t.data_ptr() for t in (tu, tq0, tqd0)), tq.data_ptr(), tqd.data_ptr())
            return tq, tqd

        @staticmethod
        def vmap(info, in_dims, tq0, tqd0, tu, sim, nsteps):
            T = info.batch_size

            def directions(t, dim):      # [B][T][...]: the mapped axis behind the rollouts; an unmapped tangent is the same in all
                if t is None:
                    return None
                return t.unsqueeze(1).expand(t.shape[:1] + (T,) + t.shape[1:]) if dim is None else t.movedim(dim, 1)

            tq0, tqd0, tu = (directions(t, d) for t, d in zip((tq0, tqd0, tu), in_dims[:3]))
            return _Tangents.run(sim, nsteps, T, tq0, tqd0, tu, (sim.B, T, nsteps, sim.nr)), (1, 1)

    _Function = _Rollout
    return _Function


def _check_tensors(who, sim, named):
    """float64 tensors on the sim's device: THE place that says so.  named: (name, tensor) pairs.  Returns the device."""
    import torch
    dev = torch.device("cuda", sim.device)
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a torch.Tensor, got %s" % (who, name, type(t).__name__))
        if t.dtype != torch.float64:
            raise ValueError("%s: %s must be float64, got %s" % (who, name, t.dtype))
        if t.device != dev:
            raise ValueError("%s: %s must be on %s (the sim's device), got %s" % (who, name, dev, t.device))
    return dev


def _check_integrator(integrator):
    if integrator not in (1, 2):
        raise ValueError("rollout: integrator must be 1 (BDF1) or 2 (BDF2), got %r" % (integrator,))


def _check_ulim(who, ulim, nr, dev):
    """(ulo, uhi) of a ``ulim`` argument as contiguous tensors or None each."""
    import torch
    if not isinstance(ulim, (tuple, list)) or len(ulim) != 2:
        raise ValueError("%s: ulim must be a pair (ulo, uhi), either may be None" % who)
    out = []
    for name, t in zip(("ulo", "uhi"), ulim):
        if t is not None:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != dev or tuple(t.shape) != (nr,):
                raise ValueError("%s: %s must be a float64 tensor of shape (%d,) on %s" % (who, name, nr, dev))
            t = t.detach().contiguous()
        out.append(t)
    return out


def _raise_newton_failed(info):
    """RuntimeError when the status words of a taped rollout's info say that a Newton solve failed."""
    if (info["status"] & _BAD_STATUS).any():
        bad = [(int(b), int(s)) for b, s in enumerate(info["status"]) if s & _BAD_STATUS]
        raise RuntimeError("rollout: Newton failed (rollout, status bits; 1 diverged, 2 iteration limit, 4 NaN): %r" % (bad[:8],))


def _tape_forward(sim, q0c, qd0c, uc, h, pscale, check, integrator):
    """The open-loop taped rollout of contiguous device tensors: (qtraj, qdtraj), the tape left in the sim.  The forward of rollout,
    linearize and jvp; whatever else the caller allocates, it allocates before."""
    import torch
    B, nsteps, nr = uc.shape
    qtraj = torch.empty((B, nsteps, nr), dtype=torch.float64, device=uc.device)
    qdtraj = torch.empty_like(qtraj)
    # the library works on a stream of its own and returns when its kernels have finished: what torch has queued for the
    # inputs must be done before it starts
    torch.cuda.current_stream(uc.device).synchronize()
    sim.set_state_device(q0c.data_ptr(), qd0c.data_ptr())
    info = sim.rollout_tape_device(nsteps, h, uc.data_ptr(), qtraj.data_ptr(), qdtraj.data_ptr(), pscale=pscale, stats=check,
                                   integrator=integrator)
    if check:
        _raise_newton_failed(info)
    return qtraj, qdtraj


def _check_inputs(sim, q0, qdot0, u):
    """The argument checks rollout, linearize, jvp and rollout_feedback share (and their words)."""
    _check_tensors("rollout", sim, (("q0", q0), ("qdot0", qdot0), ("u", u)))
    if u.dim() != 3 or u.shape[0] != sim.B or u.shape[2] != sim.nr or u.shape[1] < 1:
        raise ValueError("rollout: u must have shape (%d, nsteps, %d), got %r" % (sim.B, sim.nr, tuple(u.shape)))
    for name, t in (("q0", q0), ("qdot0", qdot0)):
        if tuple(t.shape) != (sim.B, sim.nr):
            raise ValueError("rollout: %s must have shape (%d, %d), got %r" % (name, sim.B, sim.nr, tuple(t.shape)))


def model_params(sim):
    """The model parameters of ``sim`` (a BatchSim) the taped rollout can be differentiated by, as float64 leaf tensors on the sim's
    device that hold the model's values and require grad: "stiffness", "damping", "qrest" [nr] in reduced DOF order (a value the
    scene sets per joint is repeated for every DOF of a multi-DOF joint), "inertia" [njoints][6] in listing order (the layout of
    desc.I_i: the rotational inertia, then three times the mass) and "grav" [3].  Pass the dict, or part of it, as ``params`` of rollout."""
    import numpy as np
    import torch
    from . import _abi
    n, nr = int(sim._desc.njoints), sim.nr
    idx = np.zeros(n, dtype=np.int32)
    _abi.check(sim._L.rmx_model_idxR(sim._model, _abi.iptr(idx)), "rmx_model_idxR")
    keep = sim._keep
    qrr = keep.get("qRestR")
    vals = {k: np.zeros(nr) for k in ("stiffness", "damping", "qrest")}
    starts = sorted(int(i) for i in idx if i >= 0) + [nr]
    for j in range(n):
        if idx[j] < 0:
            continue
        end = starts[starts.index(int(idx[j])) + 1]      # the DOFs of joint j: idx[j] .. the next joint's first DOF
        for k, r in enumerate(range(int(idx[j]), end)):
            vals["stiffness"][r] = keep["stiffness"][j]
            vals["damping"][r] = keep["damping"][j]
            vals["qrest"][r] = qrr[r] if qrr is not None and len(qrr) == nr else (keep["qRest"][j] if k == 0 else 0.0)
    vals["inertia"] = np.asarray(keep["I_i"], dtype=np.float64).reshape(n, 6)
    vals["grav"] = np.array([sim._desc.grav[i] for i in range(3)])
    dev = torch.device("cuda", sim.device)
    return {k: torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for k, v in vals.items()}


def _check_params(sim, params):
    """params of rollout -> (names, tensors) in the order of rmx_param_grads; ValueError for anything the library cannot fill."""
    from . import _abi
    if not isinstance(params, dict):
        raise ValueError("rollout: params must be a dict of tensors (model_params(sim) or part of it), got %s" % type(params).__name__)
    unknown = [k for k in params if k not in _abi.PARAM_NAMES]
    if unknown:
        raise ValueError("rollout: unknown model parameter %r (known: %s)" % (unknown[0], ", ".join(_abi.PARAM_NAMES)))
    if not params:
        raise ValueError("rollout: params names no parameter (pass None for a rollout without parameter gradients)")
    shapes = sim._param_shapes()
    names = tuple(n for n in _abi.PARAM_NAMES if n in params)
    for n in names:      # (tensor by tensor: the first tensor that is wrong in any way is the one named)
        _check_tensors("rollout", sim, [("params[%r]" % n, params[n])])
        if tuple(params[n].shape) != shapes[n]:
            raise ValueError("rollout: params[%r] must have shape %r, got %r" % (n, shapes[n], tuple(params[n].shape)))
    return names, tuple(params[n] for n in names)


def force_params(sim):
    """The constants of the point forces of ``sim`` (a BatchSim built with tape_forces=True) the taped rollout can be differentiated
    by, as float64 leaf tensors [nforces] on the sim's device that hold the force table's values and require grad, in the order of the
    scene's point forces: "force_stiffness", "force_damping" and "force_L" (the rest length; a point-point force has none, its entry
    takes no gradient).  Pass the dict, or part of it, as ``force_params`` of rollout."""
    import torch
    from . import _abi
    dev = torch.device("cuda", sim.device)
    return {n: torch.tensor(sim._force_values[:, i].copy(), dtype=torch.float64, device=dev, requires_grad=True)
            for i, n in enumerate(_abi.FORCE_PARAM_NAMES)}


def _check_force_params(sim, force_params):
    """force_params of rollout -> (names, tensors) in the order of rmx_force_grads; ValueError for anything the library cannot fill."""
    from . import _abi
    if not isinstance(force_params, dict):
        raise ValueError("rollout: force_params must be a dict of tensors (force_params(sim) or part of it), got %s" % type(force_params).__name__)
    unknown = [k for k in force_params if k not in _abi.FORCE_PARAM_NAMES]
    if unknown:
        raise ValueError("rollout: unknown force parameter %r (known: %s)" % (unknown[0], ", ".join(_abi.FORCE_PARAM_NAMES)))
    if not force_params:
        raise ValueError("rollout: force_params names no parameter (pass None for a rollout without force gradients)")
    if not getattr(sim, "nforces", 0) or not sim.tapes_point_forces:
        raise ValueError("rollout: force_params needs a sim whose tape carries point forces (a scene with point forces, BatchSim(..., tape_forces=True))")
    names = tuple(n for n in _abi.FORCE_PARAM_NAMES if n in force_params)
    for n in names:
        _check_tensors("rollout", sim, [("force_params[%r]" % n, force_params[n])])
        if tuple(force_params[n].shape) != (sim.nforces,):
            raise ValueError("rollout: force_params[%r] must have shape %r, got %r" % (n, (sim.nforces,), tuple(force_params[n].shape)))
    return names, tuple(force_params[n] for n in names)


def rollout(sim, q0, qdot0, u, h=None, pscale=1.0, check=True, integrator=1, params=None, force_params=None):
    """A controlled BDF1 (integrator=1) or BDF2 (integrator=2) rollout of every trajectory of ``sim`` (a BatchSim) that autograd can differentiate.

    q0, qdot0: [B][nr]; u: [B][nsteps][nr], one torque per joint and step (tau + pscale*u at step k) - float64 tensors on the sim's
    device.  h: step size (None: sim.opts.h).  Returns (qtraj, qdtraj), both [B][nsteps][nr]: row k-1 is the state after step k.
    The sim is left at the end of the rollout.  check=True raises RuntimeError when a rollout's Newton solve diverged, hit its
    iteration limit or met a NaN.  backward() must run before the next rollout or adjoint_* call on the same sim: both replace
    the tape, and backward raises RuntimeError("the tape of this rollout has been replaced") then.
    Under integrator=2 the rollout starts itself with SDIRK2 from (q0, qdot0): row 0 is the state after the two-stage start step
    (u[:, 0] holds for both stages), row k-1 for k >= 2 the state after the BDF2 step from steps k-1 and k-2; the gradients are
    exact through the start step too.  Any other integrator raises ValueError.
    Forward mode works too: under torch.autograd.forward_ad or torch.func.jvp the tangents of q0, qdot0 and u (any subset) go through
    one rmx_rollout_jvp_device call on the tape just recorded, and torch.func.jacfwd runs all its directions in ONE such call; a
    tangent on a params tensor raises RuntimeError (the forward never reads the params tensors; ``jvp_params`` is the call for
    forward-mode parameter tangents, ``param_jacobian`` for whole columns), torch.func.vmap over q0, qdot0 or u too.
    params: None, or a dict of model-parameter tensors - model_params(sim) or any part of it ("stiffness", "damping", "qrest",
    "inertia", "grav").  backward() then also accumulates into each given tensor's .grad the gradient of the loss with respect to
    that parameter, summed over the batch (one rmx_rollout_vjp_params call).  The forward does NOT read the tensors' values: the sim
    simulates the model it was built from, so the tensors must describe that model, and a parameter update means building a new
    BatchSim from the updated scene.  Unknown names and tensors of another shape, dtype or device raise ValueError.
    force_params: None, or a dict of force-constant tensors - force_params(sim) or any part of it ("force_stiffness", "force_damping",
    "force_L"), on a sim whose tape carries point forces (tape_forces=True).  backward() then accumulates the gradient with respect to
    the constants of the scene's point forces in the same way (one rmx_rollout_vjp_forces call, which on such a sim also serves
    ``params``); the rules of ``params`` hold: the forward does not read the values, errors are ValueError."""
    _check_integrator(integrator)
    _check_inputs(sim, q0, qdot0, u)
    args = (q0, qdot0, u, sim, float(sim.opts.h if h is None else h), float(pscale), bool(check), integrator)
    if params is None and force_params is None:
        return _function().apply(*args)
    names, tensors = _check_params(sim, params) if params is not None else ((), ())
    fnames, ftensors = _check_force_params(sim, force_params) if force_params is not None else ((), ())
    return _function().apply(*args, names + fnames, *tensors, *ftensors)


def linearize(sim, q0, qdot0, u, h=None, pscale=1.0, check=True, integrator=1):
    """The controlled BDF1 rollout of ``rollout`` and its linearisation, step by step: (qtraj, qdtraj, A, Bm) with

        A[b, k-1]  = d(q_k, qdot_k)/d(q_{k-1}, qdot_{k-1})   [B][nsteps][2nr][2nr]
        Bm[b, k-1] = d(q_k, qdot_k)/du_k                      [B][nsteps][2nr][nr]

    in the state order (q, qdot) - what iLQR / DDP, time-varying LQR and Gauss-Newton shooting take.  Arguments, checks and words
    are rollout's; no autograd graph is made.  Forward is rmx_rollout_tape_device, the per-solve sensitivities XA, XB, XU come
    from rmx_rollout_linearize_device (include/redmax_hip.h) and are assembled here with torch ops:

        A = [[XA + XB, h XB], [(XA + XB - I)/h, XB]]        Bm = [[XU], [XU/h]]

    The call replaces the sim's tape, as rollout does, and leaves the sim at the end of the rollout.  integrator=2 raises
    ValueError: BDF2 needs the augmented state (q_k, qdot_k, q_{k-1}, qdot_{k-1}) and a composite start step; the per-solve
    sensitivities of a BDF2 tape are available from BatchSim.rollout_linearize, their assembly is left to a later change."""
    import torch
    if integrator != 1:
        raise ValueError("linearize: integrator must be 1 (BDF1), got %r: the BDF2 assembly needs the augmented state "
                         "(BatchSim.rollout_linearize returns the per-solve sensitivities of a BDF2 tape)" % (integrator,))
    _check_inputs(sim, q0, qdot0, u)
    h = float(sim.opts.h if h is None else h)
    B, nsteps, nr = u.shape
    X = torch.empty((3, B, nsteps, nr, nr), dtype=torch.float64, device=u.device)
    qtraj, qdtraj = _tape_forward(sim, q0.detach().contiguous(), qdot0.detach().contiguous(), u.detach().contiguous(), h, float(pscale),
                                  bool(check), 1)
    sim.rollout_linearize_device(nsteps, X[0].data_ptr(), X[1].data_ptr(), X[2].data_ptr())
    XA, XB, XU = (X[i].transpose(-1, -2) for i in range(3))      # the ABI's last index is column-major: [.., i, j] = dx_i/d(.)_j
    S = XA + XB
    eye = torch.eye(nr, dtype=torch.float64, device=u.device)
    A = torch.cat([torch.cat([S, h * XB], dim=-1), torch.cat([(S - eye) / h, XB], dim=-1)], dim=-2)
    Bm = torch.cat([XU, XU / h], dim=-2)
    return qtraj, qdtraj, A, Bm


def rollout_feedback(sim, q0, qdot0, uff, K=None, xref=None, h=None, pscale=1.0, check=True, integrator=1, status=False, ulim=None):
    """The controlled rollout of ``rollout`` in CLOSED LOOP: (qtraj, qdtraj, uapp), with the torque of step k

        uapp[b, k-1] = uff[b, k-1] + K[.., k-1].T @ (x - xref[.., k-1]),      x = (q, qdot) at the START of step k

    formed on the device from the state the rollout itself has reached - all steps in one launch (rmx_rollout_tape_feedback_device):
    the forward pass of iLQR / DDP, time-varying-LQR tracking.  uff: [B][nsteps][nr].  K: [nsteps][2nr][nr], shared by the batch,
    or [B][nsteps][2nr][nr]; the index order is (step, STATE entry j, torque i): K[.., k-1, j, i] = du_i/dx_j with the q block
    first - a tensor whose memory is the ABI's column-major table (for a gain matrix G[i, j] in the usual order pass
    G.transpose(-1, -2)).  xref: [nsteps][2nr] or [B][nsteps][2nr], row k-1 the reference for the state at the start of step k (row
    0 belongs to (q0, qdot0)); K and xref both shared or both per rollout.  None: no feedback / a zero reference.
    No autograd graph is made: the tape the call leaves is the open-loop tape under uapp.  Gradients through the feedback law
    (dL/dK, dL/dxref, the closed-loop dL/duff) come from ``rollout_closed_loop``, the same rollout as an autograd function.  Arguments, checks and words are rollout's (uff in the place of u).  The call replaces the sim's tape, as
    rollout does, and leaves the sim at the end of the rollout.  status=True appends the rollouts' status words (a bool tensor [B] on
    the sim's device: did a Newton solve diverge, hit its iteration limit or meet a NaN) - for a caller that passes check=False and
    sorts the rollouts itself, as a line search does.
    ulim=(ulo, uhi), float64 tensors [nr] on the sim's device or None each: the applied torque is clamped into the limits behind the
    feedback sum, uapp = min(max(uff + K'(x - xref), ulo), uhi), with K None too (rmx_rollout_tape_feedback_box_device).
    ``rollout_closed_loop`` does not know about the clamp: gradients through a saturated feedback law are not formed."""
    import torch
    _check_integrator(integrator)
    _check_inputs(sim, q0, qdot0, uff)
    B, nsteps, nr = uff.shape
    dev = torch.device("cuda", sim.device)
    per = []
    for name, t, tail in (("K", K, (nsteps, 2 * nr, nr)), ("xref", xref, (nsteps, 2 * nr))):
        if t is None:
            continue
        _check_tensors("rollout", sim, [(name, t)])
        if tuple(t.shape) not in (tail, (B,) + tail):
            raise ValueError("rollout: %s must have shape %r or %r, got %r" % (name, tail, (B,) + tail, tuple(t.shape)))
        per.append(t.dim() == len(tail) + 1)
    if len(set(per)) > 1:
        raise ValueError("rollout: K and xref must both be shared by the batch or both hold one table per rollout")
    h = float(sim.opts.h if h is None else h)
    lim = None if ulim is None else _check_ulim("rollout", ulim, nr, dev)
    q0c, qd0c, uc = q0.detach().contiguous(), qdot0.detach().contiguous(), uff.detach().contiguous()
    Kc = None if K is None else K.detach().contiguous()
    xc = None if xref is None else xref.detach().contiguous()
    qtraj = torch.empty((B, nsteps, nr), dtype=torch.float64, device=dev)
    qdtraj = torch.empty_like(qtraj)
    uapp = torch.empty_like(qtraj)
    torch.cuda.current_stream(dev).synchronize()      # (the library works on a stream of its own: see _tape_forward)
    sim.set_state_device(q0c.data_ptr(), qd0c.data_ptr())
    info = sim.rollout_feedback_device(nsteps, h, uc.data_ptr(), 0 if Kc is None else Kc.data_ptr(), 0 if xc is None else xc.data_ptr(),
                                       qtraj.data_ptr(), qdtraj.data_ptr(), uapp.data_ptr(), per_rollout=bool(per and per[0]),
                                       pscale=float(pscale), stats=bool(check or status), integrator=integrator,
                                       ulim=None if lim is None else tuple(0 if t is None else t.data_ptr() for t in lim))
    if check:
        _raise_newton_failed(info)
    if status:
        return qtraj, qdtraj, uapp, torch.as_tensor((info["status"] & _BAD_STATUS) != 0, device=dev)
    return qtraj, qdtraj, uapp


def _lqr_arguments(who, sim, lx, lu, Q, R, ubar=None, box=False):
    """The checks lqr_backward and lqr_backward_box share (ubar: the box form's) -> (the sim's device, the tape's steps N)."""
    dev = _check_tensors(who, sim, [("lx", lx), ("lu", lu), ("Q", Q), ("R", R)] + ([("ubar", ubar)] if box else []))
    B, nr = sim.B, sim.nr
    if lu.dim() != 3 or lu.shape[0] != B or lu.shape[2] != nr or lu.shape[1] < 1:
        raise ValueError("%s: lu must have shape (%d, nsteps, %d), got %r" % (who, B, nr, tuple(lu.shape)))
    N = lu.shape[1]
    if box and (tuple(lx.shape) != (B, N, 2 * nr) or tuple(ubar.shape) != (B, N, nr)):
        raise ValueError("%s: lx and ubar must have shapes %r and %r, got %r and %r"
                         % (who, (B, N, 2 * nr), (B, N, nr), tuple(lx.shape), tuple(ubar.shape)))
    if tuple(lx.shape) != (B, N, 2 * nr):
        raise ValueError("%s: lx must have shape %r, got %r" % (who, (B, N, 2 * nr), tuple(lx.shape)))
    tail = (N, 2 * nr, 2 * nr)
    if tuple(Q.shape) not in (tail, (B,) + tail):
        raise ValueError("%s: Q must have shape %r or %r, got %r" % (who, tail, (B,) + tail, tuple(Q.shape)))
    if tuple(R.shape) != (nr, nr):
        raise ValueError("%s: R must have shape %r, got %r" % (who, (nr, nr), tuple(R.shape)))
    return dev, N


def _lqr_outputs(sim, N, dev):
    """kff [B][N][nr], K [B][N][2nr][nr], expected [B] and the int32 status [B] of a Riccati sweep, on the device."""
    import torch
    B, nr = sim.B, sim.nr
    return (torch.empty((B, N, nr), dtype=torch.float64, device=dev), torch.empty((B, N, 2 * nr, nr), dtype=torch.float64, device=dev),
            torch.empty(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))


def lqr_backward_box(sim, lx, lu, Q, R, ubar, ulim, mu=0.0, max_iter=0):
    """``lqr_backward`` under the torque limits ulim=(ulo, uhi) (rmx_rollout_lqr_box_device, include/redmax_hip.h): control-limited
    DDP - at every step the box QP over ulo - ubar_k <= k <= uhi - ubar_k in the place of the solve, the feedback rows of the
    torques on a bound zero.  ubar [B][N][nr]: the nominal applied torques (the uapp of the launch that left the tape); ulo, uhi:
    float64 tensors [nr] on the sim's device or None; max_iter: the cap on the QP iterations of a step (0: 64); the rest is
    lqr_backward's.  Returns (kff, K, expected, status [B] int32, clamped [B][N] int32 holding the bit masks): status 0, 1 (a pivot
    not > 0) or 2 (a QP did not terminate); a rollout with status != 0 has zero gains and expected 0.  One box for all steps and
    rollouts; BDF1 tapes only."""
    import torch
    dev, N = _lqr_arguments("lqr_backward_box", sim, lx, lu, Q, R, ubar, box=True)
    ulo, uhi = _check_ulim("lqr_backward_box", ulim, sim.nr, dev)
    lxc, luc, Qc, Rc, ubc = (t.detach().contiguous() for t in (lx, lu, Q, R, ubar))
    kff, K, expected, status = _lqr_outputs(sim, N, dev)
    clamped = torch.zeros((sim.B, N), dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()      # (the library works on a stream of its own: see _tape_forward)
    sim.rollout_lqr_box_device(N, lxc.data_ptr(), luc.data_ptr(), Qc.data_ptr(), Rc.data_ptr(), ubc.data_ptr(),
                               0 if ulo is None else ulo.data_ptr(), 0 if uhi is None else uhi.data_ptr(), kff.data_ptr(), K.data_ptr(),
                               expected.data_ptr(), status.data_ptr(), clamped.data_ptr(), per_rollout=Q.dim() == 4, mu=float(mu),
                               max_iter=int(max_iter))
    return kff, K, expected, status, clamped


def lqr_backward(sim, lx, lu, Q, R, mu=0.0):
    """The Riccati sweep of iLQR on the tape ``sim`` holds (rmx_rollout_lqr_device, include/redmax_hip.h): the recursion of
    ``ilqr.backward_pass`` in one launch, the per-step linearisation formed inside it - no rollout is run and no A_k, B_k are written.

    lx [B][N][2nr], lu [B][N][nr]: the cost's gradients at the nominal the tape was recorded at; Q [N][2nr][2nr], shared by the batch,
    or [B][N][2nr][2nr]; R [nr][nr]; both symmetric; mu >= 0 - float64 tensors on the sim's device, N the tape's steps.  The tape must
    be a BDF1 tape (rollout, linearize, rollout_feedback with integrator=1).  Returns (kff [B][N][nr], K [B][N][2nr][nr],
    expected [B], notpd [B] bool): K is what ``rollout_feedback`` takes as is (K[b, k-1, j, i] = du_i/dx_j, the transpose of
    backward_pass's), and a rollout whose Quu + mu I was not positive definite has notpd set, zero gains and expected 0."""
    import torch
    dev, N = _lqr_arguments("lqr_backward", sim, lx, lu, Q, R)
    lxc, luc, Qc, Rc = (t.detach().contiguous() for t in (lx, lu, Q, R))
    kff, K, expected, status = _lqr_outputs(sim, N, dev)
    torch.cuda.current_stream(dev).synchronize()      # (the library works on a stream of its own: see _tape_forward)
    sim.rollout_lqr_device(N, lxc.data_ptr(), luc.data_ptr(), Qc.data_ptr(), Rc.data_ptr(), kff.data_ptr(), K.data_ptr(),
                           expected.data_ptr(), status.data_ptr(), per_rollout=Q.dim() == 4, mu=float(mu))
    return kff, K, expected, status != 0


_Points = None


def _points_function():
    """The torch.autograd.Function of points, made on first use."""
    global _Points
    if _Points is not None:
        return _Points
    import torch
    from torch.autograd.function import once_differentiable

    class _PointsFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q, sim, terms):
            B, N, _ = q.shape
            qc = q.detach().contiguous()
            x = torch.empty((B, len(terms), 3), dtype=torch.float64, device=q.device)
            torch.cuda.current_stream(q.device).synchronize()      # (the library works on a stream of its own: see _tape_forward)
            sim.rollout_points_device(N, qc.data_ptr(), terms, x_ptr=x.data_ptr())
            ctx.sim, ctx.terms = sim, terms
            ctx.save_for_backward(qc)
            return x

        @staticmethod
        @once_differentiable
        def backward(ctx, gx):
            (qc,) = ctx.saved_tensors
            gxc = gx.contiguous()
            gq = torch.empty_like(qc)
            torch.cuda.current_stream(qc.device).synchronize()
            ctx.sim.rollout_points_device(qc.shape[1], qc.data_ptr(), ctx.terms, gx_ptr=gxc.data_ptr(), gq_ptr=gq.data_ptr())
            return gq, None, None

    _Points = _PointsFn
    return _Points


def points(sim, q, terms):
    """World positions of body points along a state record, differentiable: q [B][N][nr] -> x [B][nterms][3]
    (rmx_rollout_points_device forward and, with the cotangents gx, backward).  terms: a list of dict(body, xlocal, step) -
    ``BatchSim.adjoint_track``'s term without its weight; the point of term t is read at the posture q[:, step_t - 1].  It composes
    with ``rollout``: any task-space loss on ``points(sim, rollout(...)[0], terms)`` backpropagates to u, q0 and qdot0.  The Jacobian
    is taken at the given state.  Needs no tape and leaves the sim's tape alone."""
    _check_tensors("points", sim, (("q", q),))
    if q.dim() != 3 or q.shape[0] != sim.B or q.shape[2] != sim.nr or q.shape[1] < 1:
        raise ValueError("points: q must have shape (%d, nsteps, %d), got %r" % (sim.B, sim.nr, tuple(q.shape)))
    terms = [dict(t) for t in terms]
    if not terms:
        raise ValueError("points: terms is empty")
    return _points_function().apply(q, sim, terms)


_Frames = None


def _frames_function():
    """The torch.autograd.Function of frames, made on first use."""
    global _Frames
    if _Frames is not None:
        return _Frames
    import torch
    from torch.autograd.function import once_differentiable

    class _FramesFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q, qdot, sim, terms):
            B, N, _ = q.shape
            qc, qdc = q.detach().contiguous(), qdot.detach().contiguous()
            T = len(terms)
            x, v = (torch.empty((B, T, 3), dtype=torch.float64, device=q.device) for _ in range(2))
            Rcm = torch.empty((B, T, 3, 3), dtype=torch.float64, device=q.device)      # the library's 3x3 is column-major
            torch.cuda.current_stream(q.device).synchronize()      # (the library works on a stream of its own: see _tape_forward)
            sim.rollout_frames_device(N, qc.data_ptr(), qdc.data_ptr(), terms, x_ptr=x.data_ptr(), v_ptr=v.data_ptr(), R_ptr=Rcm.data_ptr())
            ctx.sim, ctx.terms = sim, terms
            ctx.save_for_backward(qc, qdc)
            ctx.set_materialize_grads(False)
            return x, v, Rcm.transpose(-1, -2).contiguous()

        @staticmethod
        @once_differentiable
        def backward(ctx, gx, gv, gR):
            qc, qdc = ctx.saved_tensors
            gq, gqd = torch.zeros_like(qc), torch.zeros_like(qc)
            if gx is None and gv is None and gR is None:
                return gq, gqd, None, None
            gxc, gvc = (None if g is None else g.contiguous() for g in (gx, gv))
            gRc = None if gR is None else gR.transpose(-1, -2).contiguous()
            ptr = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
            torch.cuda.current_stream(qc.device).synchronize()
            ctx.sim.rollout_frames_device(qc.shape[1], qc.data_ptr(), qdc.data_ptr(), ctx.terms, gx_ptr=ptr(gxc), gv_ptr=ptr(gvc), gR_ptr=ptr(gRc),
                                          gq_ptr=gq.data_ptr(), gqd_ptr=gqd.data_ptr() if gvc is not None else 0)
            return gq, gqd, None, None

    _Frames = _FramesFn
    return _Frames


def frames(sim, q, qdot, terms):
    """Position, point velocity and orientation of body frames along a state record, differentiable: q, qdot [B][N][nr] ->
    (x [B][nterms][3], v [B][nterms][3], R [B][nterms][3][3] with R[..., r, c]) (rmx_rollout_frames_device forward and, with the
    cotangents, backward: gq = sum_t Jp'gx + G'gv + Jw'a(gR R'), gqd = sum_t Jp'gv).  terms: a list of dict(body, xlocal, step | t) -
    weights are not read; the frame of term t is read at the state of row step_t - 1.  It composes with ``rollout``: a loss on
    ``frames(sim, *rollout(...), terms)`` backpropagates to u, q0 and qdot0.  The Jacobians are taken at the given state.  Needs no
    tape and leaves the sim's tape alone."""
    _check_tensors("frames", sim, (("q", q), ("qdot", qdot)))
    if q.dim() != 3 or q.shape[0] != sim.B or q.shape[2] != sim.nr or q.shape[1] < 1:
        raise ValueError("frames: q must have shape (%d, nsteps, %d), got %r" % (sim.B, sim.nr, tuple(q.shape)))
    if tuple(qdot.shape) != tuple(q.shape):
        raise ValueError("frames: qdot must have shape %r, got %r" % (tuple(q.shape), tuple(qdot.shape)))
    terms = [dict(t) for t in terms]
    if not terms:
        raise ValueError("frames: terms is empty")
    return _frames_function().apply(q, qdot, sim, terms)


def _frame_weighted(terms):
    """Does a term carry a velocity or an orientation weight (then the cost goes through rmx_rollout_cost_frames)."""
    return terms is not None and any(float(t.get("wvel", 0.0)) != 0.0 or float(t.get("wrot", 0.0)) != 0.0 for t in terms)


def _check_frame_targets(sim, terms, vtarget, Rtarget):
    """The checks of cost_model's two frame tables (xtarget has its own, older words)."""
    B, T = sim.B, len(terms)
    _check_tensors("cost_model", sim, [(n, t) for n, t in (("vtarget", vtarget), ("Rtarget", Rtarget)) if t is not None])
    for name, t, tail in (("vtarget", vtarget, (3,)), ("Rtarget", Rtarget, (3, 3))):
        if t is not None and tuple(t.shape) not in ((T,) + tail, (B, T) + tail):
            raise ValueError("cost_model: %s must have shape %r or %r, got %r" % (name, (T,) + tail, (B, T) + tail, tuple(t.shape)))


def _cost_model_frames(sim, N, qc, qdc, xtarget, vtarget, Rtarget, common):
    """cost_model's call where a term weighs velocity or orientation: the three target tables share one per-rollout flag, so a shared
    table beside a per-rollout one is repeated; Rtarget [..][3][3] goes column-major.  common: the arguments both entries take."""
    B = sim.B
    per = any(t is not None and t.dim() == len(tail) + 2 for t, tail in ((xtarget, (3,)), (vtarget, (3,)), (Rtarget, (3, 3))))

    def table(t, tail):
        if t is None:
            return None
        t = t.detach()
        if per and t.dim() == len(tail) + 1:
            t = t.unsqueeze(0).expand((B,) + tuple(t.shape))
        return (t.transpose(-1, -2) if len(tail) == 2 else t).contiguous()

    xt, vt, Rt = table(xtarget, (3,)), table(vtarget, (3,)), table(Rtarget, (3, 3))
    ptr = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    sim.rollout_cost_frames_device(N, qc.data_ptr(), qdc.data_ptr(), xtarget_ptr=ptr(xt), vtarget_ptr=ptr(vt), Rtarget_ptr=ptr(Rt),
                                   target_per_rollout=per, **common)


def cost_model(sim, qtraj, qdtraj, Q=None, xgoal=None, terms=None, xtarget=None, want=("J", "lx", "Q"), vtarget=None, Rtarget=None):
    """The cost of a trajectory and its second-order model for ``lqr_backward`` (rmx_rollout_cost_device, include/redmax_hip.h): a
    joint-space quadratic - Q [N][2nr][2nr] or [B][N][2nr][2nr], symmetric; xgoal [N][2nr] or [B][N][2nr]; None: zero - plus point
    targets - terms: a list of dict(body, xlocal, step, wpos), wpos >= 0; xtarget [nterms][3] or [B][nterms][3].  qtraj, qdtraj
    [B][N][nr]: float64 tensors on the sim's device, as every table.  Returns a dict with the names in `want`: "J" [B], the cost
    summed over the steps (Jk.sum(1)); "lx" [B][N][2nr], its exact gradient by the states; "Q" [B][N][2nr][2nr], the Gauss-Newton
    model Q + sum_t w_t Jp_t'Jp_t (the curvature of the points is dropped), symmetric bit for bit - the per-rollout table
    ``lqr_backward`` takes.  No rollout is run and the sim's tape is left alone.
    A term may also carry wvel and wrot (frame targets, rmx_rollout_cost_frames_device): wvel/2 |v - vtarget|^2 on the point's velocity
    and wrot/4 |R - Rtarget|_F^2 = wrot (1 - cos theta) on the body's orientation, with vtarget [nterms][3] and Rtarget [nterms][3][3]
    (R[..., r, c]), shared or [B][..]; a table may be None where no term weighs it.  Then "lx" has qdot rows and "Q" the velocity
    terms' cross blocks.  Without such a term the call is the one above, bit for bit."""
    import torch
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in ("J", "lx", "Q") for w in want) or len(set(want)) != len(want):
        raise ValueError("cost_model: want must name distinct outputs among 'J', 'lx', 'Q', got %r" % (want,))
    named = [("qtraj", qtraj), ("qdtraj", qdtraj)] + [(n, t) for n, t in (("Q", Q), ("xgoal", xgoal), ("xtarget", xtarget)) if t is not None]
    dev = _check_tensors("cost_model", sim, named)
    B, nr = sim.B, sim.nr
    if qtraj.dim() != 3 or qtraj.shape[0] != B or qtraj.shape[2] != nr or qtraj.shape[1] < 1:
        raise ValueError("cost_model: qtraj must have shape (%d, nsteps, %d), got %r" % (B, nr, tuple(qtraj.shape)))
    N = qtraj.shape[1]
    if tuple(qdtraj.shape) != (B, N, nr):
        raise ValueError("cost_model: qdtraj must have shape %r, got %r" % ((B, N, nr), tuple(qdtraj.shape)))
    if Q is not None and tuple(Q.shape) not in ((N, 2 * nr, 2 * nr), (B, N, 2 * nr, 2 * nr)):
        raise ValueError("cost_model: Q must have shape %r or %r, got %r" % ((N, 2 * nr, 2 * nr), (B, N, 2 * nr, 2 * nr), tuple(Q.shape)))
    if xgoal is not None and tuple(xgoal.shape) not in ((N, 2 * nr), (B, N, 2 * nr)):
        raise ValueError("cost_model: xgoal must have shape %r or %r, got %r" % ((N, 2 * nr), (B, N, 2 * nr), tuple(xgoal.shape)))
    if Q is None and xgoal is None and terms is None:
        raise ValueError("cost_model: neither a joint-space cost (Q, xgoal) nor terms")
    nterms = 0
    if terms is not None:
        terms = [dict(t) for t in terms]
        nterms = len(terms)
        if xtarget is None and (not _frame_weighted(terms) or any(float(t.get("wpos", 0.0)) != 0.0 for t in terms)):
            raise ValueError("cost_model: xtarget is None")
        if xtarget is not None and tuple(xtarget.shape) not in ((nterms, 3), (B, nterms, 3)):
            raise ValueError("cost_model: xtarget must have shape (%d, 3) or (%d, %d, 3), got %r" % (nterms, B, nterms, tuple(xtarget.shape)))
        if _frame_weighted(terms):
            _check_frame_targets(sim, terms, vtarget, Rtarget)
    qc, qdc = qtraj.detach().contiguous(), qdtraj.detach().contiguous()
    Qc, xgc, xtc = (None if t is None else t.detach().contiguous() for t in (Q, xgoal, xtarget if terms is not None else None))
    Jk = torch.empty((B, N), dtype=torch.float64, device=dev) if "J" in want else None
    lx = torch.empty((B, N, 2 * nr), dtype=torch.float64, device=dev) if "lx" in want else None
    Qo = torch.empty((B, N, 2 * nr, 2 * nr), dtype=torch.float64, device=dev) if "Q" in want else None
    torch.cuda.current_stream(dev).synchronize()      # (the library works on a stream of its own: see _tape_forward)
    ptr = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    common = dict(Q_ptr=ptr(Qc), xgoal_ptr=ptr(xgc), Q_per_rollout=Q is not None and Q.dim() == 4, goal_per_rollout=xgoal is not None and xgoal.dim() == 3,
                  terms=terms, Jk_ptr=ptr(Jk), lx_ptr=ptr(lx), Qout_ptr=ptr(Qo))
    if _frame_weighted(terms):
        _cost_model_frames(sim, N, qc, qdc, xtarget, vtarget, Rtarget, common)
    else:
        sim.rollout_cost_device(N, qc.data_ptr(), qdc.data_ptr(), xtarget_ptr=ptr(xtc), target_per_rollout=xtc is not None and xtc.dim() == 3, **common)
    out = {}
    if Jk is not None:
        out["J"] = Jk.sum(1)
    if lx is not None:
        out["lx"] = lx
    if Qo is not None:
        out["Q"] = Qo
    return out


def rollout_search(sim, q0, qdot0, ubar, kff, K, xref, alphas, Jbar, cost=None, ulim=None, h=None, pscale=1.0):
    """The backtracking line search of iLQR in ONE launch (rmx_rollout_search_device, include/redmax_hip.h), BDF1:
    (qtraj, qdtraj, uapp, J, alpha, status).  From (q0, qdot0) every rollout runs the closed loop of ``rollout_feedback`` (K, xref and
    ulim as there) under uff = ubar + a*kff for a in ``alphas``, in order, and keeps the first pass without a failed Newton solve whose
    cost is below Jbar[b]; a rollout no alpha helps - and every rollout when ``alphas`` is empty, where kff and Jbar may be None -
    runs the nominal pass uff = ubar.  cost: an ``ilqr.QuadraticCost`` or ``ilqr.TrackingCost`` (its Q, xgoal, R and terms with
    their targets), evaluated inside the launch on the states each pass produces.  J [B]: the cost of the trajectory each rollout
    ended on; alpha [B]: the accepted step length, 0: none; status [B] int32: the Newton status word of that pass.  The record,
    uapp, the sim's state and its tape (the open-loop tape under uapp) belong to that pass.
    NOT differentiable: no autograd graph is made and none can be - the accepted alpha is a discrete choice.  Differentiate the
    trajectory it returns with ``rollout`` / ``rollout_closed_loop`` at uapp."""
    import torch
    _check_inputs(sim, q0, qdot0, ubar)
    if cost is None:
        raise ValueError("rollout_search: cost is None (an ilqr.QuadraticCost or ilqr.TrackingCost)")
    B, N, nr = ubar.shape
    dev = torch.device("cuda", sim.device)
    alphas = tuple(float(a) for a in (() if alphas is None else alphas))
    named = [(n, t) for n, t in (("kff", kff), ("K", K), ("xref", xref), ("Jbar", Jbar)) if t is not None]
    Qc, Rc, xg = getattr(cost, "Q", None), getattr(cost, "R", None), getattr(cost, "xgoal", None)
    terms = getattr(cost, "terms", None)
    xt, vt, Rt = (getattr(cost, n, None) for n in ("xtarget", "vtarget", "Rtarget"))
    named += [(n, t) for n, t in (("cost.Q", Qc), ("cost.R", Rc), ("cost.xgoal", xg), ("cost.xtarget", xt), ("cost.vtarget", vt),
                                  ("cost.Rtarget", Rt)) if t is not None]
    _check_tensors("rollout_search", sim, named)
    if alphas and (kff is None or Jbar is None):
        raise ValueError("rollout_search: alphas need kff and Jbar")
    if kff is not None and tuple(kff.shape) != (B, N, nr):
        raise ValueError("rollout_search: kff must have shape %r, got %r" % ((B, N, nr), tuple(kff.shape)))
    if Jbar is not None and tuple(Jbar.shape) != (B,):
        raise ValueError("rollout_search: Jbar must have shape %r, got %r" % ((B,), tuple(Jbar.shape)))
    per = []
    for name, t, tail in (("K", K, (N, 2 * nr, nr)), ("xref", xref, (N, 2 * nr))):
        if t is None:
            continue
        if tuple(t.shape) not in (tail, (B,) + tail):
            raise ValueError("rollout_search: %s must have shape %r or %r, got %r" % (name, tail, (B,) + tail, tuple(t.shape)))
        per.append(t.dim() == len(tail) + 1)
    if len(set(per)) > 1:
        raise ValueError("rollout_search: K and xref must both be shared by the batch or both hold one table per rollout")
    if xg is not None and xg.dim() == 3 and xg.shape[0] == 1:
        xg = xg[0]
    if Qc is not None and tuple(Qc.shape) not in ((N, 2 * nr, 2 * nr), (B, N, 2 * nr, 2 * nr)):
        raise ValueError("rollout_search: cost.Q must have shape %r or %r, got %r" % ((N, 2 * nr, 2 * nr), (B, N, 2 * nr, 2 * nr), tuple(Qc.shape)))
    if xg is not None and tuple(xg.shape) not in ((N, 2 * nr), (B, N, 2 * nr)):
        raise ValueError("rollout_search: cost.xgoal must have shape %r or %r, got %r" % ((N, 2 * nr), (B, N, 2 * nr), tuple(xg.shape)))
    if Rc is not None and tuple(Rc.shape) != (nr, nr):
        raise ValueError("rollout_search: cost.R must have shape %r, got %r" % ((nr, nr), tuple(Rc.shape)))
    tper = False
    if terms is not None:
        terms = [dict(t) for t in terms]
        T = len(terms)
        tabs = ((xt, (3,), "xtarget"), (vt, (3,), "vtarget"), (Rt, (3, 3), "Rtarget"))
        for t, tail, name in tabs:
            if t is not None and tuple(t.shape) not in ((T,) + tail, (B, T) + tail):
                raise ValueError("rollout_search: cost.%s must have shape %r or %r, got %r" % (name, (T,) + tail, (B, T) + tail, tuple(t.shape)))
        tper = any(t is not None and t.dim() == len(tail) + 2 for t, tail, _ in tabs)

        def table(t, tail):      # (the three tables share one per-rollout flag; Rtarget [..][3][3] goes column-major)
            if t is None:
                return None
            t = t.detach()
            if tper and t.dim() == len(tail) + 1:
                t = t.unsqueeze(0).expand((B,) + tuple(t.shape))
            return (t.transpose(-1, -2) if len(tail) == 2 else t).contiguous()

        xt, vt, Rt = table(xt, (3,)), table(vt, (3,)), table(Rt, (3, 3))
    else:
        xt = vt = Rt = None
    h = float(sim.opts.h if h is None else h)
    lim = None if ulim is None else _check_ulim("rollout_search", ulim, nr, dev)
    c = lambda t: None if t is None else t.detach().contiguous()      # noqa: E731
    q0c, qd0c, uc, kc, Kc, xc, Jc, Qd, xgd, Rd = (c(t) for t in (q0, qdot0, ubar, kff, K, xref, Jbar, Qc, xg, Rc))
    qtraj = torch.empty((B, N, nr), dtype=torch.float64, device=dev)
    qdtraj, uapp = torch.empty_like(qtraj), torch.empty_like(qtraj)
    J = torch.empty(B, dtype=torch.float64, device=dev)
    alpha = torch.empty_like(J)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    torch.cuda.current_stream(dev).synchronize()      # (the library works on a stream of its own: see _tape_forward)
    sim.set_state_device(q0c.data_ptr(), qd0c.data_ptr())
    sim.rollout_search_device(N, h, uc.data_ptr(), ptr(kc) if alphas else 0, ptr(Kc), ptr(xc), alphas, ptr(Jc) if alphas else 0, qtraj.data_ptr(),
                              qdtraj.data_ptr(), uapp.data_ptr(), J.data_ptr(), alpha_ptr=alpha.data_ptr(), status_ptr=status.data_ptr(),
                              per_rollout=bool(per and per[0]), Q_ptr=ptr(Qd), xgoal_ptr=ptr(xgd), Q_per_rollout=Qd is not None and Qd.dim() == 4,
                              goal_per_rollout=xgd is not None and xgd.dim() == 3, R_ptr=ptr(Rd), terms=terms, xtarget_ptr=ptr(xt),
                              vtarget_ptr=ptr(vt), Rtarget_ptr=ptr(Rt), target_per_rollout=tper, pscale=float(pscale),
                              ulim=None if lim is None else tuple(0 if t is None else t.data_ptr() for t in lim))
    return qtraj, qdtraj, uapp, J, alpha, status


_ClosedLoop = None


def _closed_loop_function():
    """The torch.autograd.Function of rollout_closed_loop, made on first use."""
    global _ClosedLoop
    if _ClosedLoop is not None:
        return _ClosedLoop
    import torch
    from torch.autograd.function import once_differentiable

    class _Closed(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q0, qdot0, uff, K, xref, sim, h, pscale, check, integrator):
            qtraj, qdtraj, uapp = rollout_feedback(sim, q0, qdot0, uff, K, xref, h=h, pscale=pscale, check=check, integrator=integrator)
            ctx.sim, ctx.nsteps, ctx.tape = sim, uff.shape[1], sim.tape_count
            ctx.per = K is not None and K.dim() == 4
            ctx.has = (K is not None, xref is not None)
            keep = [q0.detach(), qdot0.detach(), qtraj, qdtraj]
            keep += [t.detach().contiguous() for t in (K, xref) if t is not None]
            ctx.save_for_backward(*keep)
            return qtraj, qdtraj, uapp

        @staticmethod
        @once_differentiable
        def backward(ctx, gq, gqd, gu):
            sim, nsteps = ctx.sim, ctx.nsteps
            if sim.tape_count != ctx.tape:
                raise RuntimeError("the tape of this rollout has been replaced")
            saved = list(ctx.saved_tensors)
            q0, qd0, qtraj, qdtraj = saved[:4]
            K = saved[4] if ctx.has[0] else None
            xref = saved[4 + int(ctx.has[0])] if ctx.has[1] else None
            dev = torch.device("cuda", sim.device)
            B, nr = sim.B, sim.nr
            sh = (B, nsteps, nr)
            gq = torch.zeros(sh, dtype=torch.float64, device=dev) if gq is None else gq.contiguous()
            gqd = torch.zeros(sh, dtype=torch.float64, device=dev) if gqd is None else gqd.contiguous()
            gu = None if gu is None else gu.contiguous()
            need = ctx.needs_input_grad
            duff = torch.empty(sh, dtype=torch.float64, device=dev)
            dq0 = torch.empty((B, nr), dtype=torch.float64, device=dev)
            dqd0 = torch.empty_like(dq0)
            rows_K = torch.empty((B, nsteps, 2 * nr, nr), dtype=torch.float64, device=dev) if (K is not None and ctx.per and need[3]) else None
            rows_x = torch.empty((B, nsteps, 2 * nr), dtype=torch.float64, device=dev) if (K is not None and xref is not None and need[4]) else None
            torch.cuda.current_stream(dev).synchronize()
            sim.rollout_vjp_feedback_device(nsteps, gq.data_ptr(), gqd.data_ptr(), 0 if gu is None else gu.data_ptr(),
                                            0 if K is None else K.data_ptr(), 0 if (K is None or xref is None) else xref.data_ptr(),
                                            per_rollout=ctx.per, duff_ptr=duff.data_ptr(), dK_ptr=0 if rows_K is None else rows_K.data_ptr(),
                                            dxref_ptr=0 if rows_x is None else rows_x.data_ptr(), dq0_ptr=dq0.data_ptr(), dqd0_ptr=dqd0.data_ptr())
            dK = dx = None
            if K is not None and need[3]:
                if ctx.per:
                    dK = rows_K
                else:      # a shared table: one contraction of duff with the states the steps started from, no [B][nsteps][2nr][nr] tensor
                    x = torch.cat([torch.cat([q0[:, None], qtraj[:, :-1]], dim=1), torch.cat([qd0[:, None], qdtraj[:, :-1]], dim=1)], dim=2)
                    if xref is not None:
                        x = x - xref
                    dK = torch.einsum("bkj,bki->kji", x, duff)
            if xref is not None and need[4]:
                if K is None:
                    dx = torch.zeros_like(xref)
                else:
                    dx = rows_x if ctx.per else rows_x.sum(dim=0)
            return dq0, dqd0, duff, dK, dx, None, None, None, None, None

    _ClosedLoop = _Closed
    return _ClosedLoop


def rollout_closed_loop(sim, q0, qdot0, uff, K, xref=None, h=None, pscale=1.0, check=True, integrator=1):
    """``rollout_feedback`` as a function autograd can differentiate: (qtraj, qdtraj, uapp), every one of them differentiable with
    respect to q0, qdot0, uff, K and xref - gain tuning, learning a tracking reference, a torch policy that emits K, xref or uff,
    differentiating an iLQR result through its own feedback policy.  Shapes and meaning are rollout_feedback's; K and xref may be
    shared by the batch or hold one table per rollout (both alike).  Forward is rmx_rollout_tape_feedback_device, backward ONE
    rmx_rollout_vjp_feedback_device call (include/redmax_hip.h) with the cotangent of uapp as gu.  The library returns one gradient row per
    rollout: for a shared xref the rows are summed over the batch, and for a shared K the gradient is one einsum of duff with the
    states the steps started from (no [B][nsteps][2nr][nr] tensor is made).  Arguments, checks and words are rollout_feedback's.
    backward() must run before the next rollout or adjoint_* call on the same sim: those replace the tape, and backward raises
    RuntimeError("the tape of this rollout has been replaced") then.  First derivatives only."""
    _check_integrator(integrator)
    return _closed_loop_function().apply(q0, qdot0, uff, K, xref, sim, float(sim.opts.h if h is None else h), float(pscale), bool(check),
                                         integrator)


def jvp(sim, q0, qdot0, u, tq0=None, tqdot0=None, tu=None, h=None, pscale=1.0, check=True, integrator=1):
    """The controlled rollout of ``rollout`` and the forward-mode tangents of its whole trajectory: (qtraj, qdtraj, tq, tqd).

    tu: [B][T][nsteps][nr], tq0, tqdot0: [B][T][nr] - T tangent directions per rollout, float64 tensors on the sim's device; any of
    them may be None (zero), not all.  tq, tqd: [B][T][nsteps][nr], row k-1 the tangent of the state after step k.  A tu of
    [B][nsteps][nr] or a tq0 / tqdot0 of [B][nr] (every given input alike) is one direction, and tq, tqd come back without the T axis.
    One tape (rmx_rollout_tape_device, or its BDF2 form under integrator=2) and one rmx_rollout_jvp_device call for all directions -
    one elimination per step whatever T is; no autograd graph is made.  Arguments, checks and words are rollout's.  The call
    replaces the sim's tape, as rollout does, and leaves the sim at the end of the rollout."""
    import torch
    _check_integrator(integrator)
    _check_inputs(sim, q0, qdot0, u)
    B, nsteps, nr = u.shape
    tans = {n: t for n, t in (("tu", tu), ("tq0", tq0), ("tqdot0", tqdot0)) if t is not None}
    if not tans:
        raise ValueError("rollout: all tangents are None")
    tail = {"tu": (nsteps, nr), "tq0": (nr,), "tqdot0": (nr,)}
    dev = _check_tensors("rollout", sim, tans.items())
    single = all(t.dim() == 1 + len(tail[n]) for n, t in tans.items())
    if single:
        tans = {n: t.unsqueeze(1) for n, t in tans.items()}
    T = max([t.shape[1] for t in tans.values() if t.dim() >= 2] + [1])
    for n, t in tans.items():
        if tuple(t.shape) != (B, T) + tail[n]:
            raise ValueError("rollout: %s must have shape %r - or, every tangent alike, that shape without the direction axis -, got %r"
                             % (n, (B, T) + tail[n], tuple(t.shape[:1] + t.shape[2:]) if single else tuple(t.shape)))
    tans = {n: t.detach().contiguous() for n, t in tans.items()}
    h = float(sim.opts.h if h is None else h)
    tq = torch.empty((B, T, nsteps, nr), dtype=torch.float64, device=dev)
    tqd = torch.empty_like(tq)
    qtraj, qdtraj = _tape_forward(sim, q0.detach().contiguous(), qdot0.detach().contiguous(), u.detach().contiguous(), h, float(pscale),
                                  bool(check), integrator)
    sim.rollout_jvp_device(nsteps, T, *(tans[n].data_ptr() if n in tans else 0 for n in ("tu", "tq0", "tqdot0")), tq.data_ptr(),
                           tqd.data_ptr())
    return (qtraj, qdtraj, tq[:, 0], tqd[:, 0]) if single else (qtraj, qdtraj, tq, tqd)


def _check_tparams(who, tparams):
    """tparams of jvp_params -> {name: tensor}, in the order of rmx_param_tangents; ValueError for anything the library cannot read."""
    from . import _abi
    if not isinstance(tparams, dict):
        raise ValueError("%s: tparams must be a dict of tensors over %s, got %s" % (who, ", ".join(_abi.PARAM_NAMES), type(tparams).__name__))
    unknown = [k for k in tparams if k not in _abi.PARAM_NAMES]
    if unknown:
        raise ValueError("%s: unknown model parameter %r (known: %s)" % (who, unknown[0], ", ".join(_abi.PARAM_NAMES)))
    if not tparams:
        raise ValueError("%s: tparams names no parameter (jvp is the call for tangents of u, q0 and qdot0 alone)" % who)
    return {n: tparams[n] for n in _abi.PARAM_NAMES if n in tparams}


def jvp_params(sim, q0, qdot0, u, tparams, tq0=None, tqdot0=None, tu=None, h=None, pscale=1.0, check=True, integrator=1):
    """The controlled rollout of ``rollout`` and the forward-mode tangents of its whole trajectory with respect to the model's
    parameters: (qtraj, qdtraj, tq, tqd), what ``jvp`` returns.

    tparams: a dict of float64 tensors on the sim's device over "stiffness", "damping", "qrest" ([B][T][nr]), "inertia"
    ([B][T][njoints][6]; a mass tangent is the same number in entries 3 .. 5) and "grav" ([B][T][3]), at least one: direction t of
    rollout b moves the model's parameters by the rows (b, t), and u, q0, qdot0 by tu, tq0, tqdot0 where given (jvp's shapes).
    Every given tensor without its T axis is one direction, and tq, tqd come back without it.  One tape and one
    rmx_rollout_jvp_params_device call for all directions; no autograd graph is made.  The forward does not read parameter values:
    the sim simulates the model it was built from.  Arguments, checks and words are rollout's; the call replaces the sim's tape and
    leaves the sim at the end of the rollout.  It is the transpose of rollout(..., params=...).backward()."""
    import torch
    from . import _abi
    who = "jvp_params"
    _check_integrator(integrator)
    _check_inputs(sim, q0, qdot0, u)
    B, nsteps, nr = u.shape
    tp = _check_tparams(who, tparams)
    tans = {"tparams[%r]" % n: t for n, t in tp.items()}
    tans.update({n: t for n, t in (("tu", tu), ("tq0", tq0), ("tqdot0", tqdot0)) if t is not None})
    tail = {"tparams[%r]" % n: s for n, s in sim._param_shapes().items()}
    tail.update({"tu": (nsteps, nr), "tq0": (nr,), "tqdot0": (nr,)})
    dev = _check_tensors(who, sim, tans.items())
    single = all(t.dim() == 1 + len(tail[n]) for n, t in tans.items())
    if single:
        tans = {n: t.unsqueeze(1) for n, t in tans.items()}
    Ts = sorted({int(t.shape[1]) for n, t in tans.items() if t.dim() == 2 + len(tail[n])})
    if len(Ts) > 1:
        raise ValueError("%s: every tangent must carry the same number of directions, got %s" % (who, " and ".join("%d" % t for t in Ts)))
    T = Ts[0] if Ts else 1
    for n, t in tans.items():
        if tuple(t.shape) != (B, T) + tail[n]:
            raise ValueError("%s: %s must have shape %r - or, every tangent alike, that shape without the direction axis -, got %r"
                             % (who, n, (B, T) + tail[n], tuple(t.shape[:1] + t.shape[2:]) if single else tuple(t.shape)))
    tans = {n: t.detach().contiguous() for n, t in tans.items()}
    h = float(sim.opts.h if h is None else h)
    tq = torch.empty((B, T, nsteps, nr), dtype=torch.float64, device=dev)
    tqd = torch.empty_like(tq)
    qtraj, qdtraj = _tape_forward(sim, q0.detach().contiguous(), qdot0.detach().contiguous(), u.detach().contiguous(), h, float(pscale),
                                  bool(check), integrator)

    def ptr(n):
        return tans[n].data_ptr() if n in tans else 0
    sim.rollout_jvp_params_device(nsteps, T, tq.data_ptr(), tqd.data_ptr(), *(ptr("tparams[%r]" % n) for n in _abi.PARAM_NAMES),
                                  tu_ptr=ptr("tu"), tq0_ptr=ptr("tq0"), tqd0_ptr=ptr("tqdot0"))
    return (qtraj, qdtraj, tq[:, 0], tqd[:, 0]) if single else (qtraj, qdtraj, tq, tqd)


def param_jacobian(sim, nsteps, names=PARAM_NAMES):
    """The Jacobian of the taped trajectory with respect to the model's parameters, on the sim's CURRENT tape (the last rollout,
    jvp or rollout_tape call): name -> (Jq, Jqd), float64 tensors on the sim's device of shape [B][nsteps][nr] + the parameter's
    shape ("stiffness", "damping", "qrest": [nr]; "inertia": [njoints][6]; "grav": [3]), Jq[b, k-1, i, ...] = d q_k[i] / d theta[...]
    for rollout b.  One unit direction per parameter entry, and all entries of all names go in ONE rmx_rollout_jvp_params_device
    call - one elimination per taped solve however many parameters there are.  names: distinct names among the five (default: all).
    An "inertia" column of entry 3, 4 or 5 alone is the derivative in that entry; the derivative in the physical mass is their sum.
    Memory: the call holds tq and tqd of [B][T][nsteps][nr] doubles and the library a parameter term of [B][T][nslots][n], with T the
    number of parameter entries asked for (all five names: 3 nr + 6 njoints + 3) - at 512 rollouts of a 32-link chain and 100 steps
    about 3.8 GB per array.  ``names`` restricts T to the groups wanted; for a large batch take the groups, or the rollouts, in turn.
    Neither the state nor the tape changes."""
    import torch
    from . import _abi
    who = "param_jacobian"
    given = (names,) if isinstance(names, str) else tuple(names)
    if not given or any(n not in _abi.PARAM_NAMES for n in given) or len(set(given)) != len(given):
        raise ValueError("%s: names must name distinct parameters among %s, got %r" % (who, ", ".join(repr(n) for n in _abi.PARAM_NAMES), given))
    nsteps = int(nsteps)
    if nsteps < 1:
        raise ValueError("%s: nsteps must be the number of steps of the sim's tape, got %d" % (who, nsteps))
    shapes = sim._param_shapes()
    B, nr = sim.B, sim.nr
    dev = torch.device("cuda", sim.device)
    order = [n for n in _abi.PARAM_NAMES if n in given]
    count = {n: int(torch.Size(shapes[n]).numel()) for n in order}
    T = sum(count.values())
    tans, off = {}, {}
    at = 0
    for n in order:
        t = torch.zeros((B, T, count[n]), dtype=torch.float64, device=dev)
        t[:, at:at + count[n]] = torch.eye(count[n], dtype=torch.float64, device=dev)
        tans[n], off[n] = t.reshape((B, T) + shapes[n]).contiguous(), at
        at += count[n]
    tq = torch.empty((B, T, nsteps, nr), dtype=torch.float64, device=dev)
    tqd = torch.empty_like(tq)
    torch.cuda.current_stream(dev).synchronize()      # (the library works on a stream of its own: _tape_forward)
    sim.rollout_jvp_params_device(nsteps, T, tq.data_ptr(), tqd.data_ptr(), *(tans[n].data_ptr() if n in tans else 0 for n in _abi.PARAM_NAMES))

    def cols(t, n):
        return t[:, off[n]:off[n] + count[n]].permute(0, 2, 3, 1).reshape((B, nsteps, nr) + shapes[n]).contiguous()
    return {n: (cols(tq, n), cols(tqd, n)) for n in given}
