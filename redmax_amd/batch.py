"""Batched rollouts of one scene on one MI355X: the host-side handle around the C ABI.

``BatchSim`` is what replaces the body of ``simLoop`` (matlab-diff/driverRedMaxBDF1.m:57-91):
the scene is flattened once (``Scene.desc()``), B independent (q, qdot) states live in HBM and
``step_bdf1(nsteps)`` advances all of them in one kernel launch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi


# ---- argument checks and marshalling of the entries below: every check, and its words, is written here once ----
def _and(items):
    items = list(items)
    return ", ".join(items[:-1]) + " and " + items[-1]


def _f64(who, name, a, *shapes):
    """`a` as a contiguous float64 array whose shape is one of `shapes` (one or two)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape not in shapes:
        raise ValueError("%s: %s must have shape %s, got %r" % (who, name, " or ".join("%r" % (s,) for s in shapes), a.shape))
    return a


def _f64_joint(who, names, arrays, shapes):
    """Arrays that are refused together ("gq and gqd must have shape .., got .. and ..").  shapes: one shape for all of them (a
    tuple), or a list with one shape each."""
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    each = shapes if isinstance(shapes, list) else [shapes] * len(arrays)
    if any(a.shape != s for a, s in zip(arrays, each)):
        want = "shapes " + _and("%r" % (s,) for s in each) if isinstance(shapes, list) else "shape %r" % (shapes,)
        raise ValueError("%s: %s must have %s, got %s" % (who, _and(names), want, _and("%r" % (a.shape,) for a in arrays)))
    return arrays


def _table(who, name, a, tail, B):
    """A table the batch shares, shape `tail`, or one per rollout, (B,) + tail: (the array, 1 if per rollout else 0)."""
    a = _f64(who, name, a, tail, (B,) + tail)
    return a, int(a.ndim > len(tail))


def _names(who, arg, given, allowed, empty_ok):
    """A `want` / `which` list as a tuple of distinct names among `allowed`."""
    given = (given,) if isinstance(given, str) else tuple(given)
    if (not given and not empty_ok) or any(w not in allowed for w in given) or len(set(given)) != len(given):
        raise ValueError("%s: %s must name distinct outputs among %s, got %r" % (who, arg, ", ".join(repr(n) for n in allowed), given))
    return given


def _vp(ptr):
    """A device pointer (an integer; 0 / None: null) as the c_void_p of a call."""
    return C.c_void_p(ptr or None)


def _addr(a):
    """The address of an array for a c_void_p struct member (None: null).  The struct does not hold the array: its caller does."""
    return None if a is None else a.ctypes.data


def _stats_arrays(B):
    """The three per-rollout counters of a step call and the Stats that points into them."""
    out = {k: np.zeros(B, dtype=np.int32) for k in ("newton_iters", "ls_halvings", "status")}
    return out, _abi.Stats(_abi.iptr(out["newton_iters"]), _abi.iptr(out["ls_halvings"]), _abi.iptr(out["status"]))


def _history_arrays(B, nr, nsph, nsteps, record):
    """The per-step arrays `record` (REC_ENERGY | REC_STATE | REC_CHARTS) asks for and the History that points into them."""
    out, hist = {}, _abi.History()
    if record & _abi.REC_ENERGY:
        out["T"], out["V"] = np.empty((nsteps, B)), np.empty((nsteps, B))
        hist.T, hist.V = _abi.dptr(out["T"]), _abi.dptr(out["V"])
    if record & _abi.REC_STATE:
        out["q"], out["qdot"] = np.empty((nsteps, B, nr)), np.empty((nsteps, B, nr))
        hist.q, hist.qdot = _abi.dptr(out["q"]), _abi.dptr(out["qdot"])
    if record & _abi.REC_CHARTS and nsph:
        out["charts"] = np.full((nsteps, B, nsph), 7, dtype=np.int32)
        hist.charts = _abi.iptr(out["charts"])
    return out, hist


class BatchSim:
    def __init__(self, scene_or_desc, batch=1, device=0, tape_forces=False):
        """tape_forces: the taped rollouts take the scene's point forces (tape_point_forces); off, they refuse such a scene."""
        d = scene_or_desc.desc() if hasattr(scene_or_desc, "desc") else scene_or_desc
        self._L = _abi.lib()
        self._async = None                               # (nsteps, record) of a step_history_async whose record has not been replaced
        self._desc, self._keep = _abi.make_desc(d)
        self._model = C.c_void_p()
        self._batch = C.c_void_p()
        _abi.check(self._L.rmx_model_create(C.byref(self._desc), int(device), C.byref(self._model)), "rmx_model_create")
        self.nr = self._L.rmx_model_nr(self._model)
        self.nm = self._L.rmx_model_nm(self._model)
        gc = _abi.make_ground_contact(d, self._keep)      # scene.forces: ForceGroundCuboid
        if gc is not None:
            _abi.check(self._L.rmx_model_set_ground_contact(self._model, C.byref(gc)), "rmx_model_set_ground_contact")
        pf, npf = _abi.make_point_forces(d, self._keep)   # scene.forces: ForcePointPoint / ForceSpringDamper / ForceCable
        if npf:
            rc = self._L.rmx_model_set_point_forces(self._model, pf, npf)
            if rc != 0:
                msg = self._L.rmx_last_error()
                self._L.rmx_model_destroy(self._model)
                self._model = None
                raise _abi.RedMaxHipError("rmx_model_set_point_forces failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        self.nforces = int(npf)                          # rows of the force table (the rows of rollout_vjp_forces' force gradients)
        self._force_values = np.array([[pf[i].stiffness, pf[i].damping, pf[i].L] for i in range(npf)], dtype=np.float64).reshape(npf, 3)
        self.nsph = self._L.rmx_model_nsph(self._model)
        self.B = int(batch)
        self.device = int(device)
        _abi.check(self._L.rmx_batch_create(self._model, self.B, C.byref(self._batch)), "rmx_batch_create")
        self.opts = _abi.Opts()
        self._L.rmx_opts_default(C.byref(self.opts))
        self._tape_integrator = 1                          # the integrator of the last rollout_tape* call: the slots rollout_linearize returns
        self.tape_count = 0                                # calls that rewrote the adjoint workspace (rollout_tape*, adjoint_*): see diff.rollout
        if tape_forces:
            self.tape_point_forces(True)

    def tape_point_forces(self, enable=True):
        """rmx_model_tape_point_forces: with the switch on, rollout_tape and rollout_feedback (both integrators, limits included)
        take a scene with ForcePointPoint / ForceSpringDamper / ForceCable, and the tape they leave - H and D carry the forces -
        is read by rollout_vjp, rollout_linearize, rollout_jvp, rollout_vjp_feedback, rollout_lqr unchanged.  Off (the default)
        restores the refusal.  A scene without such forces is not affected.  Takes effect at the next tape call."""
        _abi.check(self._L.rmx_model_tape_point_forces(self._model, 1 if enable else 0), "rmx_model_tape_point_forces")

    @property
    def tapes_point_forces(self):
        return self._L.rmx_model_get_tape_point_forces(self._model) == 1

    def close(self):
        if getattr(self, "_batch", None):
            self._L.rmx_batch_destroy(self._batch)
            self._batch = None
        if getattr(self, "_model", None):
            self._L.rmx_model_destroy(self._model)
            self._model = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- Joint.setQ / getQ for the batch, reference (leaf-to-root) DOF order ----
    def _arr(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (self.B, self.nr):
            a = np.ascontiguousarray(np.broadcast_to(a, (self.B, self.nr)))
        return a

    def charts(self):
        """JointSpherical.chart of every spherical joint and trajectory, [B][nsph] (reference numbering 1..12)."""
        c = np.zeros((self.B, max(self.nsph, 1)), dtype=np.int32)
        if self.nsph:
            c = np.zeros((self.B, self.nsph), dtype=np.int32)
            _abi.check(self._L.rmx_get_charts(self._batch, _abi.iptr(c)), "rmx_get_charts")
            return c
        return c[:, :0]

    def set_charts(self, charts):
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(charts, dtype=np.int32), (self.B, self.nsph)))
        _abi.check(self._L.rmx_set_charts(self._batch, _abi.iptr(c)), "rmx_set_charts")

    def idxR(self):
        idx = np.zeros(self._desc.njoints, dtype=np.int32)
        _abi.check(self._L.rmx_model_idxR(self._model, _abi.iptr(idx)), "rmx_model_idxR")
        return idx

    def set_state(self, q, qdot):
        q, qdot = self._arr(q), self._arr(qdot)
        _abi.check(self._L.rmx_set_state(self._batch, _abi.dptr(q), _abi.dptr(qdot)), "rmx_set_state")

    def get_state(self):
        q = np.empty((self.B, self.nr))
        qd = np.empty((self.B, self.nr))
        _abi.check(self._L.rmx_get_state(self._batch, _abi.dptr(q), _abi.dptr(qd)), "rmx_get_state")
        return q, qd

    def get_state_device(self, q_ptr, qdot_ptr):
        """Copy the state into caller-owned DEVICE buffers (e.g. torch tensors' data_ptr())."""
        _abi.check(self._L.rmx_get_state_device(self._batch, C.c_void_p(q_ptr), C.c_void_p(qdot_ptr)), "rmx_get_state_device")

    def set_state_device(self, q_ptr, qdot_ptr):
        _abi.check(self._L.rmx_set_state_device(self._batch, C.c_void_p(q_ptr), C.c_void_p(qdot_ptr)), "rmx_set_state_device")

    # ---- evalBDF1 & friends: g (and H) for every trajectory ----
    def eval_residual(self, q, qA, qB, eta, want_H=True):
        q, qA, qB = self._arr(q), self._arr(qA), self._arr(qB)
        g = np.empty((self.B, self.nr))
        H = np.empty((self.B, self.nr * self.nr)) if want_H else None
        _abi.check(self._L.rmx_eval(self._batch, _abi.dptr(q), _abi.dptr(qA), _abi.dptr(qB), float(eta), _abi.dptr(g), _abi.dptr(H)), "rmx_eval")
        if want_H:
            return g, H.reshape(self.B, self.nr, self.nr).transpose(0, 2, 1)   # column-major -> [b][row][col]
        return g

    def eval_bdf1(self, q1, q0, qdot0, h, want_H=True):
        q0 = self._arr(q0)
        return self.eval_residual(q1, q0, q0 + h * self._arr(qdot0), h, want_H)

    def eval_mfd(self, q, qdot):
        """computeValues (driverRedMaxBDF1.m:190-243) at (q, qdot): M [B][nr][nr], f [B][nr], D = df/dqdot [B][nr][nr]."""
        q, qdot = self._arr(q), self._arr(qdot)
        M = np.empty((self.B, self.nr * self.nr))
        D = np.empty((self.B, self.nr * self.nr))
        f = np.empty((self.B, self.nr))
        _abi.check(self._L.rmx_eval_mfd(self._batch, _abi.dptr(q), _abi.dptr(qdot), _abi.dptr(M), _abi.dptr(f), _abi.dptr(D)), "rmx_eval_mfd")
        sh = (self.B, self.nr, self.nr)
        return M.reshape(sh).transpose(0, 2, 1), f, D.reshape(sh).transpose(0, 2, 1)      # column-major -> [b][row][col]

    def compute_values(self, q, qdot, v=None, tensor=False):
        """computeValues' full output (driverRedMaxBDF1.m:188-243) at (q, qdot), any tree size: dict with M, D, K [B][nr][nr], f [B][nr],
        dMv (with v: column i = dMdq(:,:,i) v) and, with tensor=True, dMdq [B][nr][nr][nr] indexed [b][r][c][i]."""
        q, qdot = self._arr(q), self._arr(qdot)
        nr, B = self.nr, self.B
        out = {k: np.empty((B, nr * nr)) for k in ("M", "D", "K")}
        out["f"] = np.empty((B, nr))
        vv = None
        if v is not None:
            vv = self._arr(v)
            out["dMv"] = np.empty((B, nr * nr))
        if tensor:
            out["dMdq"] = np.empty((B, nr * nr * nr))
        _abi.check(self._L.rmx_compute_values(self._batch, _abi.dptr(q), _abi.dptr(qdot), _abi.dptr(vv) if vv is not None else None,
                                              _abi.dptr(out["M"]), _abi.dptr(out["f"]), _abi.dptr(out["D"]), _abi.dptr(out["K"]),
                                              _abi.dptr(out["dMv"]) if vv is not None else None,
                                              _abi.dptr(out["dMdq"]) if tensor else None), "rmx_compute_values")
        sh = (B, nr, nr)
        for k in ("M", "D", "K", "dMv"):
            if k in out:
                out[k] = out[k].reshape(sh).transpose(0, 2, 1)          # column-major -> [b][row][col]
        if tensor:
            out["dMdq"] = out["dMdq"].reshape((B, nr, nr, nr)).transpose(0, 3, 2, 1)    # (i, c, r) storage order -> [b][r][c][i]
        return out

    # ---- stepping ----
    def _step(self, fn, nsteps, h, stats, history):
        if h is not None:
            self.opts.h = float(h)
        self._async = None                                 # any step call replaces the record of an earlier step_history_async
        out, st = _stats_arrays(self.B) if stats else ({}, None)
        stp = C.byref(st) if st is not None else None
        # history "full" is Scene.saveHistory: q, qdot and JointSpherical.chart of every step as well (Scene.m:134-161)
        record = 0 if not history else _abi.REC_ENERGY | (_abi.REC_STATE | _abi.REC_CHARTS if history == "full" else 0)
        rec, hist = _history_arrays(self.B, self.nr, self.nsph, nsteps, record)
        out.update(rec)
        if history == "full":
            out.setdefault("charts", np.full((nsteps, self.B, 0), 7, dtype=np.int32))     # (a model without spherical joints)
            _abi.check(self._L.rmx_step_history(self._batch, C.byref(self.opts), int(nsteps), 1 if fn == "bdf1" else 2, stp,
                                                C.byref(hist)), "rmx_step_history")
        else:
            f = self._L.rmx_step_bdf1 if fn == "bdf1" else self._L.rmx_step_bdf2
            _abi.check(f(self._batch, C.byref(self.opts), int(nsteps), stp, _abi.dptr(out.get("T")), _abi.dptr(out.get("V"))), "rmx_step")
        out["ms"] = self._L.rmx_last_step_ms(self._batch)
        return out

    def step_bdf1(self, nsteps, h=None, stats=False, history=False):
        """history: False | True (T, V per step) | "full" (T, V, q, qdot per step: Scene.saveHistory)."""
        return self._step("bdf1", nsteps, h, stats, history)

    def step_bdf2(self, nsteps, h=None, stats=False, history=False):
        return self._step("bdf2", nsteps, h, stats, history)

    def step_euler(self, nsteps, h, history=False):
        """euler() of matlab-simple/testRedMax.m:67-109 (linearly-implicit Euler, config 1)."""
        out = {}
        T = V = None
        if history:
            T = np.empty((nsteps, self.B))
            V = np.empty((nsteps, self.B))
            out["T"], out["V"] = T, V
        _abi.check(self._L.rmx_step_euler(self._batch, float(h), int(nsteps), _abi.dptr(T), _abi.dptr(V)), "rmx_step_euler")
        out["ms"] = self._L.rmx_last_step_ms(self._batch)
        return out

    def adjoint_bdf2(self, nsteps, h, task, p, stats=False):
        """taskObjective of driverRedMaxAdjointBDF2.m:38-62 (TaskBDF2PointPos): SDIRK2 start step + BDF2 forward, TaskBDF2.calcFinal
        backward.  Arguments and results as adjoint_bdf1."""
        return self.adjoint_bdf1(nsteps, h, task, p, stats, _fn="rmx_adjoint_bdf2")

    def adjoint_bdf1(self, nsteps, h, task, p, stats=False, _fn="rmx_adjoint_bdf1"):
        """taskObjective (driverRedMaxAdjointBDF1.m:39-62) for every trajectory: forward rollout from the current state
        under torques pscale*p, then the backward sweep.  task: dict(body, xlocal, xtarget, t | step, pscale, wreg, wpos);
        p: [B][nr].  Returns (P[B], dPdp[B][nr], info)."""
        tk, opts = self._task_and_opts(task, h)
        p = self._arr(p)
        P = np.empty(self.B)
        dPdp = np.empty((self.B, self.nr))
        info, st = self._tape_stats(stats)
        _abi.check(getattr(self._L, _fn)(self._batch, C.byref(opts), int(nsteps), C.byref(tk), _abi.dptr(p), _abi.dptr(P),
                                         _abi.dptr(dPdp), st), _fn)
        info["ms"] = self._L.rmx_last_step_ms(self._batch)
        return P, dPdp, info

    def adjoint_bdf1_device(self, nsteps, h, task, p_ptr, P_ptr, dPdp_ptr, stats=False, _fn="rmx_adjoint_bdf1_device"):
        """adjoint_bdf1 with DEVICE pointers (integers, e.g. torch.Tensor.data_ptr()) for p [B][nr], P [B] and dPdp [B][nr]: nothing
        crosses the host boundary but the optional counters.  Returns info."""
        tk, opts = self._task_and_opts(task, h)
        info, st = self._tape_stats(stats)
        _abi.check(getattr(self._L, _fn)(self._batch, C.byref(opts), int(nsteps), C.byref(tk), C.c_void_p(p_ptr), C.c_void_p(P_ptr),
                                         C.c_void_p(dPdp_ptr), st), _fn)
        info["ms"] = self._L.rmx_last_step_ms(self._batch)
        return info

    def adjoint_bdf2_device(self, nsteps, h, task, p_ptr, P_ptr, dPdp_ptr, stats=False):
        return self.adjoint_bdf1_device(nsteps, h, task, p_ptr, P_ptr, dPdp_ptr, stats=stats, _fn="rmx_adjoint_bdf2_device")

    def _task_and_opts(self, task, h):
        tk = _abi.TaskPointPos()
        tk.body = int(task["body"])
        for i in range(3):
            tk.xlocal[i] = float(task["xlocal"][i])
            tk.xtarget[i] = float(task["xtarget"][i])
        tk.step = int(task["step"]) if "step" in task else int(round(float(task["t"]) / float(h)))
        tk.pscale, tk.wreg, tk.wpos = float(task["pscale"]), float(task["wreg"]), float(task["wpos"])
        opts = self._tape_opts(float(h))
        self.tape_count += 1                        # (every adjoint_* call comes through here or _track_task: it ends a rollout_tape's tape)
        return tk, opts

    def _controls(self, who, name, u, nsteps):
        """u / uff of an entry with one torque per joint and step: [B][nsteps][nr], or [nsteps][nr] for every rollout alike."""
        if u is None:
            raise ValueError("%s: %s is None" % (who, name))
        full = (self.B, nsteps, self.nr)
        u = _f64(who, name, u, full, full[1:])
        return u if u.shape == full else np.ascontiguousarray(np.broadcast_to(u, full))

    def adjoint_controls(self, nsteps, h, task, u, integrator=1, stats=False, gradient=True):
        """rmx_adjoint_controls: the adjoint with one torque per joint and STEP.  u: [B][nsteps][nr] (a [nsteps][nr] array holds for
        every trajectory); at step k the joint torque is tau + pscale*u[:, k-1].  integrator: 1 (BDF1) or 2 (BDF2).  task as
        adjoint_bdf1.  Returns (P[B], dPdu[B][nsteps][nr], info); gradient=False runs the forward rollout alone and returns None for
        dPdu.  Under BDF2 the k = 1 rows of dPdu carry the reference's start-step approximation (include/redmax_hip.h)."""
        nsteps = int(nsteps)
        u = self._controls("adjoint_controls", "u", u, nsteps)
        tk, opts = self._task_and_opts(task, h)
        P = np.empty(self.B)
        dPdu = np.empty((self.B, nsteps, self.nr)) if gradient else None
        info, st = self._tape_stats(stats)
        _abi.check(self._L.rmx_adjoint_controls(self._batch, C.byref(opts), nsteps, int(integrator), C.byref(tk), _abi.dptr(u),
                                                _abi.dptr(P), _abi.dptr(dPdu), st), "rmx_adjoint_controls")
        info["ms"] = self._L.rmx_last_step_ms(self._batch)
        return P, dPdu, info

    def adjoint_controls_device(self, nsteps, h, task, u_ptr, P_ptr, dPdu_ptr, integrator=1, stats=False):
        """adjoint_controls with DEVICE pointers (integers) for u [B][nsteps][nr], P [B] and dPdu [B][nsteps][nr]; dPdu_ptr 0 / None:
        the forward rollout alone.  Returns info."""
        tk, opts = self._task_and_opts(task, h)
        info, st = self._tape_stats(stats)
        _abi.check(self._L.rmx_adjoint_controls_device(self._batch, C.byref(opts), int(nsteps), int(integrator), C.byref(tk),
                                                       _vp(u_ptr), _vp(P_ptr), _vp(dPdu_ptr), st), "rmx_adjoint_controls_device")
        info["ms"] = self._L.rmx_last_step_ms(self._batch)
        return info

    def _targets(self, who, xtarget, nterms):
        """The point targets of `nterms` terms, [nterms][3] or [B][nterms][3]: (the array, 1 if per rollout else 0)."""
        if xtarget is None:
            raise ValueError("%s: xtarget is None" % who)
        return _table(who, "xtarget", xtarget, (nterms, 3), self.B)

    def _track_task(self, task, h, nsteps, device_targets=False):
        """task dict of adjoint_track -> (TaskTrack, Opts, keepalive).  Shapes are checked here, before any call into the library."""
        arr, nterms = self._point_terms(task["terms"], "adjoint_track", True, h)
        tk = _abi.TaskTrack()
        tk.nterms, tk.terms = nterms, arr
        tk.pscale, tk.wreg = float(task["pscale"]), float(task["wreg"])
        xt = None
        if device_targets:
            tk.per_rollout = 1 if task.get("per_rollout") else 0
        else:
            xt, tk.per_rollout = self._targets("adjoint_track", task.get("xtarget"), nterms)
            tk.xtarget = _abi.dptr(xt)
        opts = self._tape_opts(float(h))
        self.tape_count += 1
        return tk, opts, (arr, xt)

    def adjoint_track(self, nsteps, h, task, u, integrator=1, stats=False, gradient=True):
        """rmx_adjoint_track: adjoint_controls with a tracking objective - point targets on several bodies at several steps.
        task: dict(terms=[dict(body, xlocal, step | t, wpos), ...], xtarget, pscale, wreg); xtarget: (nterms, 3), one target table
        for the batch, or (B, nterms, 3), one per rollout, indexed by the term's position in `terms`.
        P[b] = sum_i wpos_i/2 |x_i(step_i) - xtarget[b][i]|^2 + wreg/2 sum u[b]^2.  u, integrator, stats, gradient and the result
        (P[B], dPdu[B][nsteps][nr] or None, info) as adjoint_controls."""
        nsteps = int(nsteps)
        u = self._controls("adjoint_track", "u", u, nsteps)
        tk, opts, keep = self._track_task(task, h, nsteps)
        P = np.empty(self.B)
        dPdu = np.empty((self.B, nsteps, self.nr)) if gradient else None
        info, st = self._tape_stats(stats)
        _abi.check(self._L.rmx_adjoint_track(self._batch, C.byref(opts), nsteps, int(integrator), C.byref(tk), _abi.dptr(u),
                                             _abi.dptr(P), _abi.dptr(dPdu), st), "rmx_adjoint_track")
        del keep
        info["ms"] = self._L.rmx_last_step_ms(self._batch)
        return P, dPdu, info

    def adjoint_track_device(self, nsteps, h, task, xtarget_ptr, u_ptr, P_ptr, dPdu_ptr, integrator=1, stats=False):
        """adjoint_track with DEVICE pointers (integers) for the targets ([nterms][3], or [B][nterms][3] with task["per_rollout"] true;
        task["xtarget"] is not read), u [B][nsteps][nr], P [B] and dPdu [B][nsteps][nr]; dPdu_ptr 0 / None: the forward rollout alone.
        Returns info."""
        tk, opts, keep = self._track_task(task, h, int(nsteps), device_targets=True)
        info, st = self._tape_stats(stats)
        _abi.check(self._L.rmx_adjoint_track_device(self._batch, C.byref(opts), int(nsteps), int(integrator), C.byref(tk),
                                                    _vp(xtarget_ptr), _vp(u_ptr), _vp(P_ptr), _vp(dPdu_ptr), st), "rmx_adjoint_track_device")
        del keep
        info["ms"] = self._L.rmx_last_step_ms(self._batch)
        return info

    def _tape_opts(self, h):
        """The options of one taped-rollout or adjoint_* call: a copy of self.opts under the step size h (None: self.opts.h)."""
        opts = _abi.Opts()
        C.memmove(C.byref(opts), C.byref(self.opts), C.sizeof(opts))
        if h is not None:
            opts.h = float(h)
        opts.iterMaxPerDof = 5                      # driverRedMaxAdjointBDF1.m:108
        return opts

    def _tape_stats(self, stats):
        """(info, the rmx_stats argument of the call or None): with stats, info holds the counters the call fills."""
        if not stats:
            return {}, None
        info = {"newton_iters": np.zeros(self.B, dtype=np.int32), "status": np.zeros(self.B, dtype=np.int32)}
        return info, C.byref(_abi.Stats(_abi.iptr(info["newton_iters"]), None, _abi.iptr(info["status"])))

    def _tape_entry(self, integrator, device):
        """(function, name) of the rollout_tape entry of an integrator: 1 BDF1, 2 BDF2 (rmx_rollout_tape_bdf2)."""
        if integrator not in (1, 2):
            raise ValueError("rollout_tape: integrator must be 1 (BDF1) or 2 (BDF2), got %r" % (integrator,))
        name = ("rmx_rollout_tape" if integrator == 1 else "rmx_rollout_tape_bdf2") + ("_device" if device else "")
        return getattr(self._L, name), name

    def _begin_tape(self, h, stats, integrator):
        """What every call that records a tape does once its arguments stand: (opts, info, stats argument), and the tape is claimed."""
        opts = self._tape_opts(h)
        info, st = self._tape_stats(stats)
        self.tape_count += 1
        self._tape_integrator = integrator
        return opts, info, st

    def rollout_tape(self, nsteps, h, u, pscale=1.0, stats=False, trajectory=True, integrator=1):
        """rmx_rollout_tape: a controlled BDF1 rollout from the current state that records its trajectory and keeps H, M, D of every
        step (the tape rollout_vjp reads).  u: [B][nsteps][nr] (a [nsteps][nr] array holds for every trajectory); at step k the joint
        torque is tau + pscale*u[:, k-1].  Returns (qtraj[B][nsteps][nr], qdtraj[B][nsteps][nr], info), row k-1 the state after step
        k; trajectory=False returns None for both.  integrator=2: rmx_rollout_tape_bdf2 - the BDF2 rollout, which always takes its
        SDIRK2 start step from the current state (step 1; its torque holds for both stages) and leaves the BDF2 history in place;
        rollout_vjp follows the integrator of the tape."""
        fn, fname = self._tape_entry(integrator, False)
        nsteps = int(nsteps)
        u = self._controls("rollout_tape", "u", u, nsteps)
        qtraj = np.empty((self.B, nsteps, self.nr)) if trajectory else None
        qdtraj = np.empty((self.B, nsteps, self.nr)) if trajectory else None
        opts, info, st = self._begin_tape(h, stats, integrator)
        _abi.check(fn(self._batch, C.byref(opts), nsteps, float(pscale), _abi.dptr(u), _abi.dptr(qtraj), _abi.dptr(qdtraj), st), fname)
        info["ms"] = self._L.rmx_last_step_ms(self._batch)
        return qtraj, qdtraj, info

    def rollout_tape_device(self, nsteps, h, u_ptr, qtraj_ptr, qdtraj_ptr, pscale=1.0, stats=False, integrator=1):
        """rollout_tape with DEVICE pointers (integers) for u, qtraj and qdtraj, all [B][nsteps][nr]; qtraj_ptr and qdtraj_ptr 0 /
        None together: no record.  Returns info."""
        fn, fname = self._tape_entry(integrator, True)
        opts, info, st = self._begin_tape(h, stats, integrator)
        _abi.check(fn(self._batch, C.byref(opts), int(nsteps), float(pscale), _vp(u_ptr), _vp(qtraj_ptr), _vp(qdtraj_ptr), st), fname)
        info["ms"] = self._L.rmx_last_step_ms(self._batch)
        return info

    def _feedback_tables(self, nsteps, K, xref, who="rollout_feedback"):
        """K and xref of rollout_feedback as contiguous float64 arrays, and whether they hold one table per rollout.  K:
        [nsteps][2nr][nr] or [B][nsteps][2nr][nr], K[.., k-1, j, i] = du_i/dx_j of step k with x = (q, qdot) - the ABI's column-major
        table as a C array -; xref: [nsteps][2nr] or [B][nsteps][2nr].  Both shared or both per rollout."""
        nr, per = self.nr, []
        if K is not None:
            K, p = _table(who, "K", K, (nsteps, 2 * nr, nr), self.B)
            per.append(p)
        if xref is not None:
            xref, p = _table(who, "xref", xref, (nsteps, 2 * nr), self.B)
            per.append(p)
        if len(set(per)) > 1:
            raise ValueError("%s: K and xref must both be shared by the batch or both hold one table per rollout" % who)
        return K, xref, int(bool(per and per[0]))

    def _ulim(self, ulim, who):
        """The torque limits of a ``ulim`` keyword, (ulo, uhi) with [nr] or None each -> (rmx_box, the arrays it points into)."""
        if not isinstance(ulim, (tuple, list)) or len(ulim) != 2:
            raise ValueError("%s: ulim must be a pair (ulo, uhi), either may be None" % who)
        keep = [None if a is None else _f64(who, name, a, (self.nr,)) for name, a in zip(("ulo", "uhi"), ulim)]
        return _abi.Box(_addr(keep[0]), _addr(keep[1])), keep

    def _feedback_call(self, device, opts, nsteps, integrator, pscale, fb, box, outs, st):
        """THE call of rmx_rollout_tape_feedback[_box][_device]: box None selects the plain entry, the argument list is formed once."""
        name = "rmx_rollout_tape_feedback" + ("" if box is None else "_box") + ("_device" if device else "")
        args = (self._batch, C.byref(opts), int(nsteps), int(integrator), float(pscale), C.byref(fb))
        args += (() if box is None else (C.byref(box),)) + tuple(outs) + (st,)
        _abi.check(getattr(self._L, name)(*args), name)

    def rollout_feedback(self, nsteps, h, uff, K=None, xref=None, pscale=1.0, stats=False, integrator=1, ulim=None):
        """rmx_rollout_tape_feedback: rollout_tape in closed loop - at step k the joint torque is tau + pscale*uapp[:, k-1] with
            uapp[b, k-1] = uff[b, k-1] + K[k-1].T @ (x - xref[k-1]),    x = (q, qdot) at the START of step k,
        formed on the device from the state the rollout has reached (one launch for all steps).  uff: [B][nsteps][nr] (or
        [nsteps][nr] for every rollout).  K: [nsteps][2nr][nr] shared by the batch or [B][nsteps][2nr][nr], K[.., k-1, j, i] =
        du_i/dx_j (the row index is the STATE entry, q block first: the memory is the ABI's column-major table); None: no feedback,
        uapp is uff bit for bit.  xref: [nsteps][2nr] or [B][nsteps][2nr], None: zero.  Returns (qtraj, qdtraj, uapp[, info]) - info
        with stats=True.  The tape it leaves is the open-loop tape under uapp: rollout_vjp, rollout_linearize, rollout_jvp and
        rollout_vjp_params differentiate that open-loop rollout, not the feedback law; rollout_vjp_feedback differentiates the closed loop.
        ulim=(ulo, uhi), each [nr] or None: rmx_rollout_tape_feedback_box - uapp is clamped into the limits behind the feedback sum
        (with K None too: actuator saturation).  rollout_vjp_feedback does not know about the clamp."""
        if integrator not in (1, 2):
            raise ValueError("rollout_feedback: integrator must be 1 (BDF1) or 2 (BDF2), got %r" % (integrator,))
        nsteps = int(nsteps)
        uff = self._controls("rollout_feedback", "uff", uff, nsteps)
        K, xref, per = self._feedback_tables(nsteps, K, xref)
        fb = _abi.Feedback(_addr(uff), _addr(K), _addr(xref), per)
        qtraj, qdtraj, uapp = (np.empty((self.B, nsteps, self.nr)) for _ in range(3))
        opts, info, st = self._begin_tape(h, stats, integrator)
        box, keep = self._ulim(ulim, "rollout_feedback") if ulim is not None else (None, None)
        self._feedback_call(False, opts, nsteps, integrator, pscale, fb, box, (_abi.dptr(qtraj), _abi.dptr(qdtraj), _abi.dptr(uapp)), st)
        del keep      # (the limits box points into: held until the call has returned)
        if not stats:
            return qtraj, qdtraj, uapp
        info["ms"] = self._L.rmx_last_step_ms(self._batch)
        return qtraj, qdtraj, uapp, info

    def rollout_feedback_device(self, nsteps, h, uff_ptr, K_ptr, xref_ptr, qtraj_ptr, qdtraj_ptr, uapp_ptr, per_rollout=False, pscale=1.0,
                                stats=False, integrator=1, ulim=None):
        """rollout_feedback with DEVICE pointers (integers): uff, qtraj, qdtraj, uapp [B][nsteps][nr]; K [nsteps][2nr][nr] and xref
        [nsteps][2nr], or one table per rollout with per_rollout=True.  K_ptr 0 / None: no feedback; xref_ptr 0 / None: zero;
        qtraj_ptr and qdtraj_ptr 0 / None together: no record; uapp_ptr 0 / None: not stored.  ulim=(ulo_ptr, uhi_ptr), DEVICE
        pointers to [nr] doubles, either 0 / None: rmx_rollout_tape_feedback_box_device.  Returns info."""
        if integrator not in (1, 2):
            raise ValueError("rollout_feedback: integrator must be 1 (BDF1) or 2 (BDF2), got %r" % (integrator,))
        fb = _abi.Feedback(uff_ptr or None, K_ptr or None, xref_ptr or None, int(bool(per_rollout)))
        opts, info, st = self._begin_tape(h, stats, integrator)
        box = None if ulim is None else _abi.Box(ulim[0] or None, ulim[1] or None)
        self._feedback_call(True, opts, nsteps, integrator, pscale, fb, box, (_vp(qtraj_ptr), _vp(qdtraj_ptr), _vp(uapp_ptr)), st)
        info["ms"] = self._L.rmx_last_step_ms(self._batch)
        return info

    def rollout_vjp(self, nsteps, gq, gqd, initial_state=True):
        """rmx_rollout_vjp on the tape of the last rollout_tape: gq, gqd [B][nsteps][nr] are dL/dq_k, dL/dqdot_k.  Returns
        (du[B][nsteps][nr], dq0[B][nr], dqd0[B][nr]) = dL/du, dL/dq0, dL/dqdot0; initial_state=False returns None for the last two.
        Neither the state nor the tape changes: the call may be repeated with other cotangents."""
        nsteps = int(nsteps)
        gq, gqd = _f64_joint("rollout_vjp", ("gq", "gqd"), (gq, gqd), (self.B, nsteps, self.nr))
        du, dq0, dqd0 = self._vjp_outputs(nsteps, initial_state)
        _abi.check(self._L.rmx_rollout_vjp(self._batch, nsteps, _abi.dptr(gq), _abi.dptr(gqd), _abi.dptr(du), _abi.dptr(dq0),
                                           _abi.dptr(dqd0)), "rmx_rollout_vjp")
        return du, dq0, dqd0

    def _vjp_outputs(self, nsteps, initial_state):
        """du [B][nsteps][nr] and dq0, dqd0 [B][nr] (None each without initial_state) of rollout_vjp and rollout_vjp_params."""
        dq0, dqd0 = (np.empty((self.B, self.nr)), np.empty((self.B, self.nr))) if initial_state else (None, None)
        return np.empty((self.B, nsteps, self.nr)), dq0, dqd0

    def rollout_vjp_device(self, nsteps, gq_ptr, gqd_ptr, du_ptr, dq0_ptr=None, dqd0_ptr=None):
        """rollout_vjp with DEVICE pointers (integers): gq, gqd, du [B][nsteps][nr]; dq0, dqd0 [B][nr], 0 / None together: not formed."""
        _abi.check(self._L.rmx_rollout_vjp_device(self._batch, int(nsteps), _vp(gq_ptr), _vp(gqd_ptr), _vp(du_ptr), _vp(dq0_ptr),
                                                  _vp(dqd0_ptr)), "rmx_rollout_vjp_device")

    def rollout_vjp_feedback(self, nsteps, gq, gqd, K=None, xref=None, gu=None, want=None):
        """rmx_rollout_vjp_feedback on the tape of the last rollout_feedback: the closed-loop adjoint.  gq, gqd [B][nsteps][nr] are
        dL/dq_k, dL/dqdot_k, gu (or None: zero) the cotangent of the applied torque uapp; K, xref: the tables of the forward call
        (rollout_feedback's shapes; the library cannot check that the tape was recorded under them).  Returns a dict with the names in
        `want` among "duff" [B][nsteps][nr], "dK" [B][nsteps][2nr][nr], "dxref" [B][nsteps][2nr], "dq0" (which brings "dqd0", both
        [B][nr]; None: all of them with gains, "duff" and "dq0" without): ALWAYS one row per rollout - for tables the batch shares, sum over the batch.  K None: no gains ("dK", "dxref"
        are refused); with gu None too the call is rollout_vjp, the same bits.  Neither the state nor the tape changes."""
        nsteps = int(nsteps)
        if want is None:
            want = ("duff", "dq0") if K is None else ("duff", "dK", "dxref", "dq0")
        names = _abi.FEEDBACK_GRAD_NAMES
        want = _names("rollout_vjp_feedback", "want", want, names, True)
        if "dq0" in want or "dqd0" in want:
            want = tuple(w for w in want if w not in ("dq0", "dqd0")) + ("dq0", "dqd0")
        sh = (self.B, nsteps, self.nr)
        gq, gqd = _f64_joint("rollout_vjp_feedback", ("gq", "gqd"), (gq, gqd), sh)
        if gu is not None:
            gu = _f64("rollout_vjp_feedback", "gu", gu, sh)
        K, xref, per = self._feedback_tables(nsteps, K, xref, who="rollout_vjp_feedback")
        fb = _abi.Feedback(None, _addr(K), _addr(xref), per)
        shapes = {"duff": sh, "dK": (self.B, nsteps, 2 * self.nr, self.nr), "dxref": (self.B, nsteps, 2 * self.nr),
                  "dq0": (self.B, self.nr), "dqd0": (self.B, self.nr)}
        out = {w: np.zeros(shapes[w]) for w in want}
        fg = _abi.FeedbackGrads(*[_addr(out.get(n)) for n in names])
        _abi.check(self._L.rmx_rollout_vjp_feedback(self._batch, nsteps, C.byref(fb), _abi.dptr(gq), _abi.dptr(gqd), _abi.dptr(gu),
                                                    C.byref(fg)), "rmx_rollout_vjp_feedback")
        return out

    def rollout_vjp_feedback_device(self, nsteps, gq_ptr, gqd_ptr, gu_ptr=None, K_ptr=None, xref_ptr=None, per_rollout=False, duff_ptr=None,
                                    dK_ptr=None, dxref_ptr=None, dq0_ptr=None, dqd0_ptr=None):
        """rollout_vjp_feedback with DEVICE pointers (integers): gq, gqd, gu, duff [B][nsteps][nr]; K [nsteps][2nr][nr] and xref
        [nsteps][2nr], or one table per rollout with per_rollout=True; dK [B][nsteps][2nr][nr], dxref [B][nsteps][2nr], dq0, dqd0
        [B][nr].  0 / None: gu zero, no gains, a zero reference, that output not formed (dq0 and dqd0 together; not all outputs)."""
        fb = _abi.Feedback(None, K_ptr or None, xref_ptr or None, int(bool(per_rollout)))
        fg = _abi.FeedbackGrads(duff_ptr or None, dK_ptr or None, dxref_ptr or None, dq0_ptr or None, dqd0_ptr or None)
        _abi.check(self._L.rmx_rollout_vjp_feedback_device(self._batch, int(nsteps), C.byref(fb), _vp(gq_ptr), _vp(gqd_ptr), _vp(gu_ptr),
                                                           C.byref(fg)), "rmx_rollout_vjp_feedback_device")

    def _param_shapes(self):
        """The shape of one rollout's row of every rmx_param_grads member."""
        return {"stiffness": (self.nr,), "damping": (self.nr,), "qrest": (self.nr,), "inertia": (int(self._desc.njoints), 6), "grav": (3,)}

    def rollout_vjp_params(self, nsteps, gq, gqd, want=_abi.PARAM_NAMES, initial_state=True):
        """rmx_rollout_vjp_params on the tape of the last rollout_tape: rollout_vjp's sweep for the cotangents gq, gqd [B][nsteps][nr],
        and the gradient with respect to the model's parameters.  Returns (du, dq0, dqd0, grads): the first three are rollout_vjp's
        (the same bits), grads maps every name in `want` to one row per rollout - stiffness, damping, qrest [B][nr] in reduced DOF
        order, inertia [B][njoints][6] in listing order (the layout of desc.I_i: the rotational inertia, then three times the mass),
        grav [B][3].  The gradient of a parameter the rollouts share is the sum over the batch; of a stiffness or damping set per
        joint the sum over that joint's DOFs.  Neither the state nor the tape changes."""
        nsteps = int(nsteps)
        want = _names("rollout_vjp_params", "want", want, _abi.PARAM_NAMES, False)
        gq, gqd = _f64_joint("rollout_vjp_params", ("gq", "gqd"), (gq, gqd), (self.B, nsteps, self.nr))
        du, dq0, dqd0 = self._vjp_outputs(nsteps, initial_state)
        shapes = self._param_shapes()
        grads = {w: np.zeros((self.B,) + shapes[w]) for w in want}
        pg = _abi.ParamGrads(*[_addr(grads.get(n)) for n in _abi.PARAM_NAMES])
        _abi.check(self._L.rmx_rollout_vjp_params(self._batch, nsteps, _abi.dptr(gq), _abi.dptr(gqd), _abi.dptr(du), _abi.dptr(dq0),
                                                  _abi.dptr(dqd0), C.byref(pg)), "rmx_rollout_vjp_params")
        return du, dq0, dqd0, grads

    def rollout_vjp_params_device(self, nsteps, gq_ptr, gqd_ptr, du_ptr, dq0_ptr=None, dqd0_ptr=None, stiffness_ptr=None, damping_ptr=None,
                                  qrest_ptr=None, inertia_ptr=None, grav_ptr=None):
        """rollout_vjp_params with DEVICE pointers (integers): gq, gqd, du [B][nsteps][nr]; dq0, dqd0 [B][nr], 0 / None together: not
        formed; stiffness, damping, qrest [B][nr], inertia [B][njoints][6], grav [B][3], 0 / None: that output is neither computed
        nor stored (not all five)."""
        pg = _abi.ParamGrads(stiffness_ptr or None, damping_ptr or None, qrest_ptr or None, inertia_ptr or None, grav_ptr or None)
        _abi.check(self._L.rmx_rollout_vjp_params_device(self._batch, int(nsteps), _vp(gq_ptr), _vp(gqd_ptr), _vp(du_ptr), _vp(dq0_ptr),
                                                         _vp(dqd0_ptr), C.byref(pg)), "rmx_rollout_vjp_params_device")

    def rollout_vjp_forces(self, nsteps, gq, gqd, want=_abi.FORCE_PARAM_NAMES, model=(), initial_state=True):
        """rmx_rollout_vjp_forces on the tape of the last rollout_tape / rollout_feedback of a sim whose tape carries point forces
        (tape_forces): rollout_vjp's sweep for the cotangents gq, gqd [B][nsteps][nr], the gradient with respect to the constants of
        the force table and, with `model`, rollout_vjp_params' gradients on such a tape.  Returns (du, dq0, dqd0, grads): the first
        three are rollout_vjp's (the same bits); grads maps every name in `want` ("force_stiffness", "force_damping", "force_L":
        [B][nforces] each, one row per rollout in the order of the scene's point forces; a point-point force has no rest length, its
        "force_L" entry is 0) and every name in `model` (rollout_vjp_params' names and shapes) to its rows.  `want` and `model` may
        each be empty, not both.  The gradient of a constant the rollouts share is the sum over the batch.  Neither the state nor the
        tape changes."""
        nsteps = int(nsteps)
        want = _names("rollout_vjp_forces", "want", want, _abi.FORCE_PARAM_NAMES, True)
        model = _names("rollout_vjp_forces", "model", model, _abi.PARAM_NAMES, True)
        if not want and not model:
            raise ValueError("rollout_vjp_forces: want and model name no output")
        gq, gqd = _f64_joint("rollout_vjp_forces", ("gq", "gqd"), (gq, gqd), (self.B, nsteps, self.nr))
        du, dq0, dqd0 = self._vjp_outputs(nsteps, initial_state)
        shapes = self._param_shapes()
        grads = {w: np.zeros((self.B, self.nforces)) for w in want}
        grads.update({w: np.zeros((self.B,) + shapes[w]) for w in model})
        pg = _abi.ParamGrads(*[_addr(grads.get(n)) for n in _abi.PARAM_NAMES])
        fg = _abi.ForceGrads(*[_addr(grads.get(n)) for n in _abi.FORCE_PARAM_NAMES])
        _abi.check(self._L.rmx_rollout_vjp_forces(self._batch, nsteps, _abi.dptr(gq), _abi.dptr(gqd), _abi.dptr(du), _abi.dptr(dq0),
                                                  _abi.dptr(dqd0), C.byref(pg) if model else None, C.byref(fg) if want else None),
                   "rmx_rollout_vjp_forces")
        return du, dq0, dqd0, grads

    def rollout_vjp_forces_device(self, nsteps, gq_ptr, gqd_ptr, du_ptr, dq0_ptr=None, dqd0_ptr=None, force_stiffness_ptr=None,
                                  force_damping_ptr=None, force_L_ptr=None, stiffness_ptr=None, damping_ptr=None, qrest_ptr=None,
                                  inertia_ptr=None, grav_ptr=None):
        """rollout_vjp_forces with DEVICE pointers (integers): gq, gqd, du [B][nsteps][nr]; dq0, dqd0 [B][nr], 0 / None together: not
        formed; force_stiffness, force_damping, force_L [B][nforces]; stiffness .. grav as rollout_vjp_params_device.  0 / None: that
        output is neither computed nor stored (not all eight)."""
        pg = _abi.ParamGrads(stiffness_ptr or None, damping_ptr or None, qrest_ptr or None, inertia_ptr or None, grav_ptr or None)
        fg = _abi.ForceGrads(force_stiffness_ptr or None, force_damping_ptr or None, force_L_ptr or None)
        _abi.check(self._L.rmx_rollout_vjp_forces_device(self._batch, int(nsteps), _vp(gq_ptr), _vp(gqd_ptr), _vp(du_ptr), _vp(dq0_ptr),
                                                         _vp(dqd0_ptr), C.byref(pg), C.byref(fg)), "rmx_rollout_vjp_forces_device")

    def rollout_linearize(self, nsteps, which=("XA", "XB", "XU")):
        """rmx_rollout_linearize on the tape of the last rollout_tape: the forward sensitivities of every taped solve x(qA, qB, u),
        XA = dx/dqA, XB = dx/dqB, XU = dx/du (include/redmax_hip.h has the assembly of A_k, B_k from them).  Returns one array per
        name in `which`, in that order, each [B][nslots][nr][nr] with [.., i, j] = dx_i/d(.)_j; nslots = nsteps for a BDF1 tape,
        nsteps + 1 for a BDF2 tape (slot nsteps: the SDIRK2a solve).  Neither the state nor the tape changes."""
        nsteps = int(nsteps)
        which = _names("rollout_linearize", "which", which, ("XA", "XB", "XU"), True)
        nslots = max(nsteps, 0) + (1 if self._tape_integrator == 2 else 0)
        out = {w: np.empty((self.B, nslots, self.nr, self.nr)) for w in which}
        _abi.check(self._L.rmx_rollout_linearize(self._batch, nsteps, _abi.dptr(out.get("XA")), _abi.dptr(out.get("XB")),
                                                 _abi.dptr(out.get("XU"))), "rmx_rollout_linearize")
        # the ABI's last index is column-major (j*nr + i): [.., j, i] as numpy reads it
        return tuple(np.ascontiguousarray(out[w].transpose(0, 1, 3, 2)) for w in which)

    def rollout_linearize_device(self, nsteps, XA_ptr, XB_ptr, XU_ptr):
        """rollout_linearize with DEVICE pointers (integers), each [B][nslots][nr*nr] with entry j*nr + i = dx_i/d(.)_j (column-major
        in the last index); 0 / None: that output is neither computed nor stored (not all three)."""
        _abi.check(self._L.rmx_rollout_linearize_device(self._batch, int(nsteps), _vp(XA_ptr), _vp(XB_ptr), _vp(XU_ptr)),
                   "rmx_rollout_linearize_device")

    def rollout_jvp(self, nsteps, tu=None, tq0=None, tqd0=None):
        """rmx_rollout_jvp on the tape of the last rollout_tape: the tangents of the whole trajectory for tangents of the controls,
        tu [B][T][nsteps][nr], and of the initial state, tq0, tqd0 [B][T][nr] - T directions per rollout in one sweep over the tape.
        Any of the three may be None (zero), not all.  Returns (tq, tqd), both [B][T][nsteps][nr]: row k-1 is the tangent of the state
        after step k.  T comes from the inputs; a tu of [B][nsteps][nr] or a tq0 / tqd0 of [B][nr] is one direction, and the T axis is
        dropped again in the result.  Neither the state nor the tape changes."""
        nsteps = int(nsteps)
        arrs = {n: np.ascontiguousarray(a, dtype=np.float64) for n, a in (("tu", tu), ("tq0", tq0), ("tqd0", tqd0)) if a is not None}
        if not arrs:
            raise ValueError("rollout_jvp: all tangents are None")
        tail = {"tu": (nsteps, self.nr), "tq0": (self.nr,), "tqd0": (self.nr,)}
        single = all(a.ndim == 1 + len(tail[n]) for n, a in arrs.items())
        if single:
            arrs = {n: np.ascontiguousarray(a[:, None]) for n, a in arrs.items()}
        T = max([a.shape[1] for a in arrs.values() if a.ndim >= 2] + [1])
        for n, a in arrs.items():
            if a.shape != (self.B, T) + tail[n]:
                raise ValueError("rollout_jvp: %s must have shape %r - or, every input alike, that shape without the direction axis -, "
                                 "got %r" % (n, (self.B, T) + tail[n], a.shape[:1] + a.shape[2:] if single else a.shape))
        tq = np.empty((self.B, T, nsteps, self.nr))
        tqd = np.empty_like(tq)
        _abi.check(self._L.rmx_rollout_jvp(self._batch, nsteps, T, _abi.dptr(arrs.get("tu")), _abi.dptr(arrs.get("tq0")),
                                           _abi.dptr(arrs.get("tqd0")), _abi.dptr(tq), _abi.dptr(tqd)), "rmx_rollout_jvp")
        return (tq[:, 0], tqd[:, 0]) if single else (tq, tqd)

    def rollout_jvp_device(self, nsteps, ntan, tu_ptr, tq0_ptr, tqd0_ptr, tq_ptr, tqd_ptr):
        """rollout_jvp with DEVICE pointers (integers): tu [B][ntan][nsteps][nr], tq0, tqd0 [B][ntan][nr], 0 / None: zero (not all
        three); tq, tqd [B][ntan][nsteps][nr]."""
        _abi.check(self._L.rmx_rollout_jvp_device(self._batch, int(nsteps), int(ntan), _vp(tu_ptr), _vp(tq0_ptr), _vp(tqd0_ptr), _vp(tq_ptr),
                                                  _vp(tqd_ptr)), "rmx_rollout_jvp_device")

    def rollout_jvp_params(self, nsteps, tparams, tu=None, tq0=None, tqd0=None):
        """rmx_rollout_jvp_params on the tape of the last rollout_tape: the tangents of the whole trajectory for tangents of the model's
        parameters - rollout_jvp with the parameter term on the right of every taped solve.  tparams: a dict over "stiffness",
        "damping", "qrest" ([B][T][nr], reduced DOF order), "inertia" ([B][T][njoints][6], listing order, the layout of desc.I_i: a
        mass tangent is the same number in entries 3 .. 5) and "grav" ([B][T][3]); at least one name.  Direction t of rollout b moves
        the parameters by the rows (b, t) and, where given, u, q0 and qdot0 by tu, tq0, tqd0 (rollout_jvp's shapes).  Returns
        (tq, tqd), both [B][T][nsteps][nr].  Every input without its T axis ([B] + shape) is one direction, and the T axis is dropped
        again in the result.  It is the transpose of rollout_vjp_params.  Neither the state nor the tape changes."""
        who = "rollout_jvp_params"
        nsteps = int(nsteps)
        if not isinstance(tparams, dict):
            raise ValueError("%s: tparams must be a dict of arrays over %s, got %s" % (who, ", ".join(_abi.PARAM_NAMES), type(tparams).__name__))
        unknown = [k for k in tparams if k not in _abi.PARAM_NAMES]
        if unknown:
            raise ValueError("%s: unknown model parameter %r (known: %s)" % (who, unknown[0], ", ".join(_abi.PARAM_NAMES)))
        if not tparams:
            raise ValueError("%s: tparams names no parameter (rollout_jvp is the call for tangents of u, q0 and qdot0 alone)" % who)
        tail = {"tparams[%r]" % n: s for n, s in self._param_shapes().items()}
        tail.update({"tu": (nsteps, self.nr), "tq0": (self.nr,), "tqd0": (self.nr,)})
        given = [("tparams[%r]" % n, tparams[n]) for n in _abi.PARAM_NAMES if n in tparams] + [("tu", tu), ("tq0", tq0), ("tqd0", tqd0)]
        arrs = {n: np.ascontiguousarray(a, dtype=np.float64) for n, a in given if a is not None}
        single = all(a.ndim == 1 + len(tail[n]) for n, a in arrs.items())
        if single:
            arrs = {n: np.ascontiguousarray(a[:, None]) for n, a in arrs.items()}
        Ts = sorted({a.shape[1] for n, a in arrs.items() if a.ndim == 2 + len(tail[n])})
        if len(Ts) > 1:
            raise ValueError("%s: every tangent must carry the same number of directions, got %s" % (who, _and("%d" % t for t in Ts)))
        T = Ts[0] if Ts else 1
        for n, a in arrs.items():
            if a.shape != (self.B, T) + tail[n]:
                raise ValueError("%s: %s must have shape %r - or, every input alike, that shape without the direction axis -, got %r"
                                 % (who, n, (self.B, T) + tail[n], a.shape[:1] + a.shape[2:] if single else a.shape))
        tp = _abi.ParamTangents(*[_addr(arrs.get("tparams[%r]" % n)) for n in _abi.PARAM_NAMES])
        tq = np.empty((self.B, T, nsteps, self.nr))
        tqd = np.empty_like(tq)
        _abi.check(self._L.rmx_rollout_jvp_params(self._batch, nsteps, T, C.byref(tp), _abi.dptr(arrs.get("tu")), _abi.dptr(arrs.get("tq0")),
                                                  _abi.dptr(arrs.get("tqd0")), _abi.dptr(tq), _abi.dptr(tqd)), "rmx_rollout_jvp_params")
        return (tq[:, 0], tqd[:, 0]) if single else (tq, tqd)

    def rollout_jvp_params_device(self, nsteps, ntan, tq_ptr, tqd_ptr, stiffness_ptr=None, damping_ptr=None, qrest_ptr=None,
                                  inertia_ptr=None, grav_ptr=None, tu_ptr=None, tq0_ptr=None, tqd0_ptr=None):
        """rollout_jvp_params with DEVICE pointers (integers): stiffness, damping, qrest [B][ntan][nr], inertia [B][ntan][njoints][6],
        grav [B][ntan][3], 0 / None: zero (not all five); tu [B][ntan][nsteps][nr], tq0, tqd0 [B][ntan][nr], 0 / None: zero; tq, tqd
        [B][ntan][nsteps][nr]."""
        tp = _abi.ParamTangents(stiffness_ptr or None, damping_ptr or None, qrest_ptr or None, inertia_ptr or None, grav_ptr or None)
        _abi.check(self._L.rmx_rollout_jvp_params_device(self._batch, int(nsteps), int(ntan), C.byref(tp), _vp(tu_ptr), _vp(tq0_ptr),
                                                         _vp(tqd0_ptr), _vp(tq_ptr), _vp(tqd_ptr)), "rmx_rollout_jvp_params_device")

    def rollout_lqr(self, nsteps, lx, lu, Q, R, mu=0.0, mu_b=None):
        """rmx_rollout_lqr on the BDF1 tape of the last rollout_tape / rollout_feedback: the Riccati sweep of iLQR (the recursion of
        ilqr.backward_pass, include/redmax_hip.h) for the cost's gradients lx [B][nsteps][2nr], lu [B][nsteps][nr] at the nominal and
        its Hessians Q [nsteps][2nr][2nr] (shared) or [B][nsteps][2nr][2nr], R [nr][nr], both symmetric; mu >= 0 regularises Quu,
        mu_b [B] replaces it rollout by rollout.  Returns (kff [B][nsteps][nr], K [B][nsteps][2nr][nr], expected [B], notpd [B] bool):
        K[b, k-1, j, i] = du_i/dx_j, the table rollout_feedback takes per rollout; a rollout whose Quu + mu I was not positive
        definite has notpd set and zero gains.  Neither the state nor the tape changes."""
        nsteps = int(nsteps)
        cost, keep = self._lqr_cost("rollout_lqr", nsteps, [("lx", lx), ("lu", lu)], Q, R, mu, mu_b)
        gains, (kff, K, expected, status) = self._lqr_gains(nsteps)
        _abi.check(self._L.rmx_rollout_lqr(self._batch, nsteps, C.byref(cost), C.byref(gains)), "rmx_rollout_lqr")
        del keep
        return kff, K, expected, status != 0

    def _lqr_cost(self, who, nsteps, named, Q, R, mu, mu_b):
        """The checked cost of rollout_lqr / rollout_lqr_box -> (LqrCost, the arrays it points into).  named: ("lx", lx), ("lu", lu)
        and, for the box form, ("ubar", ubar) - refused together; the arrays come back in that order at the head of the second item."""
        B, nr = self.B, self.nr
        shapes = [(B, nsteps, 2 * nr)] + [(B, nsteps, nr)] * (len(named) - 1)
        keep = _f64_joint(who, [n for n, _ in named], [a for _, a in named], shapes)
        Q, per = _table(who, "Q", Q, (nsteps, 2 * nr, 2 * nr), B)
        R = _f64(who, "R", R, (nr, nr))
        if mu_b is not None:
            mu_b = _f64(who, "mu_b", mu_b, (B,))
        # (Q and R are symmetric: their row-major memory is the ABI's column-major table)
        return _abi.LqrCost(_addr(keep[0]), _addr(keep[1]), _addr(Q), _addr(R), per, float(mu), _addr(mu_b)), keep + [Q, R, mu_b]

    def _lqr_gains(self, nsteps):
        """The outputs of a Riccati sweep -> (LqrGains, (kff, K, expected, status))."""
        B, nr = self.B, self.nr
        out = (np.empty((B, nsteps, nr)), np.empty((B, nsteps, 2 * nr, nr)), np.empty(B), np.zeros(B, dtype=np.int32))
        return _abi.LqrGains(*[a.ctypes.data for a in out]), out

    def rollout_lqr_box(self, nsteps, lx, lu, Q, R, ubar, ulim, mu=0.0, mu_b=None, max_iter=0):
        """rmx_rollout_lqr_box: rollout_lqr under the torque limits ulim=(ulo, uhi) ([nr] each or None) - at every step the box QP of
        control-limited DDP over ulo - ubar_k <= k <= uhi - ubar_k in the place of the solve, ubar [B][nsteps][nr] the nominal
        applied torques (the uapp of the launch that left the tape).  max_iter caps the QP iterations of a step (0: 64).  Returns
        (kff, K, expected, status [B] int32, clamped [B][nsteps] uint32): a DOF on a bound has kff = bound - ubar exactly, a zero
        row of K and its bit set in clamped; status 0, 1 (a pivot not > 0) or 2 (a QP did not terminate) - a rollout with status != 0
        has zero kff, K, clamped and expected 0.  With no finite bound: rollout_lqr's bits."""
        nsteps = int(nsteps)
        cost, keep = self._lqr_cost("rollout_lqr_box", nsteps, [("lx", lx), ("lu", lu), ("ubar", ubar)], Q, R, mu, mu_b)
        box, lim = self._ulim(ulim, "rollout_lqr_box")
        gains, (kff, K, expected, status) = self._lqr_gains(nsteps)
        clamped = np.zeros((self.B, nsteps), dtype=np.uint32)
        _abi.check(self._L.rmx_rollout_lqr_box(self._batch, nsteps, C.byref(cost), C.byref(box), keep[2].ctypes.data, int(max_iter),
                                               C.byref(gains), clamped.ctypes.data), "rmx_rollout_lqr_box")
        del keep, lim
        return kff, K, expected, status, clamped

    @staticmethod
    def _lqr_device(lx_ptr, lu_ptr, Q_ptr, R_ptr, per_rollout, mu, mu_b_ptr, kff_ptr, K_ptr, expected_ptr, status_ptr):
        """(LqrCost, LqrGains) of the _device forms of the two Riccati sweeps, from DEVICE pointers."""
        return (_abi.LqrCost(lx_ptr or None, lu_ptr or None, Q_ptr or None, R_ptr or None, int(bool(per_rollout)), float(mu), mu_b_ptr or None),
                _abi.LqrGains(kff_ptr or None, K_ptr or None, expected_ptr or None, status_ptr or None))

    def rollout_lqr_box_device(self, nsteps, lx_ptr, lu_ptr, Q_ptr, R_ptr, ubar_ptr, ulo_ptr, uhi_ptr, kff_ptr, K_ptr, expected_ptr=None,
                               status_ptr=None, clamped_ptr=None, per_rollout=False, mu=0.0, mu_b_ptr=None, max_iter=0):
        """rollout_lqr_box with DEVICE pointers (integers): as rollout_lqr_device, and ubar [B][nsteps][nr], ulo, uhi [nr] (0 / None:
        that side is unbounded), clamped [B][nsteps] uint32 (0 / None: not stored)."""
        cost, gains = self._lqr_device(lx_ptr, lu_ptr, Q_ptr, R_ptr, per_rollout, mu, mu_b_ptr, kff_ptr, K_ptr, expected_ptr, status_ptr)
        box = _abi.Box(ulo_ptr or None, uhi_ptr or None)
        _abi.check(self._L.rmx_rollout_lqr_box_device(self._batch, int(nsteps), C.byref(cost), C.byref(box), _vp(ubar_ptr), int(max_iter),
                                                      C.byref(gains), _vp(clamped_ptr)), "rmx_rollout_lqr_box_device")

    def rollout_lqr_device(self, nsteps, lx_ptr, lu_ptr, Q_ptr, R_ptr, kff_ptr, K_ptr, expected_ptr=None, status_ptr=None, per_rollout=False,
                           mu=0.0, mu_b_ptr=None):
        """rollout_lqr with DEVICE pointers (integers): lx [B][nsteps][2nr], lu, kff [B][nsteps][nr], Q [nsteps][2nr*2nr] or, with
        per_rollout=True, one table per rollout, R [nr*nr], K [B][nsteps][2nr*nr]; expected [B] doubles, status [B] int32 and mu_b
        [B] doubles may be 0 / None."""
        cost, gains = self._lqr_device(lx_ptr, lu_ptr, Q_ptr, R_ptr, per_rollout, mu, mu_b_ptr, kff_ptr, K_ptr, expected_ptr, status_ptr)
        _abi.check(self._L.rmx_rollout_lqr_device(self._batch, int(nsteps), C.byref(cost), C.byref(gains)), "rmx_rollout_lqr_device")

    @staticmethod
    def _terms(ctype, terms, who, weights, need, h):
        """The body of _point_terms / _frame_terms: terms (a list of dicts) -> (array of ctype, count).  weights: the names read; need:
        a missing one is a KeyError and not 0."""
        terms = list(terms)
        arr = (ctype * max(len(terms), 1))()
        for a, t in zip(arr, terms):
            xl = np.asarray(t["xlocal"], dtype=np.float64).reshape(-1)
            if xl.shape != (3,):
                raise ValueError("%s: a term's xlocal must have shape (3,), got %r" % (who, xl.shape))
            a.body = int(t["body"])
            a.step = int(t["step"]) if "step" in t or h is None else int(round(float(t["t"]) / float(h)))
            for k in weights:
                setattr(a, k, float(t[k]) if need else float(t.get(k, 0.0)))
            for i in range(3):
                a.xlocal[i] = float(xl[i])
        return arr, len(terms)

    @staticmethod
    def _point_terms(terms, who, need_wpos, h=None):
        """terms (a list of dict(body, xlocal, step[, wpos]), adjoint_track's) -> (array of TrackTerm, count).  With the step size h a
        term may give its time `t` in the place of `step`."""
        return BatchSim._terms(_abi.TrackTerm, terms, who, ("wpos",), need_wpos, h)

    def rollout_points(self, nsteps, q, terms, gx=None, points=True):
        """rmx_rollout_points: the world positions of body points along a state record q [B][nsteps][nr] (any record, typically a
        qtraj), and the pull-back of cotangents through them.  terms: a list of dict(body, xlocal, step) - adjoint_track's term, a
        wpos is not read; the point of term t is taken at the posture q[:, step_t - 1].  Returns (x [B][nterms][3] or None with
        points=False, gq [B][nsteps][nr] or None without gx): gq[b][k-1] = sum over the terms of step k of Jp_t' gx[b][t], with Jp_t
        the Jacobian of the point at that posture.  Needs no tape and changes neither the state nor the tape."""
        nsteps = int(nsteps)
        B, nr = self.B, self.nr
        q = _f64("rollout_points", "q", q, (B, nsteps, nr))
        arr, nterms = self._point_terms(terms, "rollout_points", False)
        if gx is not None:
            gx = _f64("rollout_points", "gx", gx, (B, nterms, 3))
        x = np.empty((B, nterms, 3)) if points else None
        gq = np.empty((B, nsteps, nr)) if gx is not None else None
        pts = _abi.PointTerms(nterms, arr, None, 0)
        _abi.check(self._L.rmx_rollout_points(self._batch, nsteps, q.ctypes.data, C.byref(pts), _addr(x), _addr(gx), _addr(gq)),
                   "rmx_rollout_points")
        return x, gq

    def rollout_points_device(self, nsteps, q_ptr, terms, x_ptr=None, gx_ptr=None, gq_ptr=None):
        """rollout_points with DEVICE pointers (integers): q, gq [B][nsteps][nr]; x, gx [B][nterms][3]; 0 / None: x not stored, gq
        not formed (not both; gq needs gx).  terms stays the host list."""
        arr, nterms = self._point_terms(terms, "rollout_points_device", False)
        pts = _abi.PointTerms(nterms, arr, None, 0)
        _abi.check(self._L.rmx_rollout_points_device(self._batch, int(nsteps), _vp(q_ptr), C.byref(pts), _vp(x_ptr), _vp(gx_ptr), _vp(gq_ptr)),
                   "rmx_rollout_points_device")

    def _cost_inputs(self, who, nsteps, q, qdot, Q, xgoal, want):
        """The checked inputs rollout_cost / rollout_cost_frames share -> (want, q, qdot, StateCost or None, the arrays it points into)."""
        B, nr = self.B, self.nr
        want = _names(who, "want", want, ("Jk", "lx", "Q"), False)
        q, qdot = _f64_joint(who, ("q", "qdot"), (q, qdot), (B, nsteps, nr))
        sc = None
        if Q is not None or xgoal is not None:
            sc = _abi.StateCost(None, None, 0, 0)
            if Q is not None:      # (symmetric: row-major memory is the column-major table)
                Q, sc.Q_per_rollout = _table(who, "Q", Q, (nsteps, 2 * nr, 2 * nr), B)
                sc.Q = Q.ctypes.data
            if xgoal is not None:
                xgoal, sc.goal_per_rollout = _table(who, "xgoal", xgoal, (nsteps, 2 * nr), B)
                sc.xgoal = xgoal.ctypes.data
        return want, q, qdot, sc, (Q, xgoal)

    def _cost_call(self, entry, nsteps, q, qdot, sc, terms, want):
        """The outputs named in want, packed as a CostModel, and the call of a cost-model entry -> the dict of outputs."""
        B, nr = self.B, self.nr
        shapes = {"Jk": (B, nsteps), "lx": (B, nsteps, 2 * nr), "Q": (B, nsteps, 2 * nr, 2 * nr)}
        out = {w: np.empty(shapes[w]) for w in want}
        cm = _abi.CostModel(*[_addr(out.get(n)) for n in ("Jk", "lx", "Q")])
        _abi.check(getattr(self._L, entry)(self._batch, nsteps, q.ctypes.data, qdot.ctypes.data, None if sc is None else C.byref(sc),
                                           None if terms is None else C.byref(terms), C.byref(cm)), entry)
        return out

    def _cost_call_device(self, entry, nsteps, q_ptr, qdot_ptr, Q_ptr, xgoal_ptr, Q_per_rollout, goal_per_rollout, terms, Jk_ptr, lx_ptr, Qout_ptr):
        """The StateCost and CostModel of DEVICE pointers and the call of a cost-model entry's _device form."""
        sc = _abi.StateCost(Q_ptr or None, xgoal_ptr or None, int(bool(Q_per_rollout)), int(bool(goal_per_rollout)))
        cm = _abi.CostModel(Jk_ptr or None, lx_ptr or None, Qout_ptr or None)
        _abi.check(getattr(self._L, entry)(self._batch, int(nsteps), _vp(q_ptr), _vp(qdot_ptr), C.byref(sc) if (Q_ptr or xgoal_ptr) else None,
                                           None if terms is None else C.byref(terms), C.byref(cm)), entry)

    def rollout_cost(self, nsteps, q, qdot, Q=None, xgoal=None, terms=None, xtarget=None, want=("Jk", "lx", "Q")):
        """rmx_rollout_cost: the cost of a state record q, qdot [B][nsteps][nr] and its second-order model for rollout_lqr -
        a joint-space quadratic (Q [nsteps][2nr][2nr] or [B][..], symmetric; xgoal [nsteps][2nr] or [B][..]; None: zero) plus point
        targets (terms: a list of dict(body, xlocal, step, wpos), wpos >= 0; xtarget [nterms][3] or [B][nterms][3]).  With
        x = (q, qdot), dx = x - xgoal, r_t = p_t(q_k) - xtarget_t, returns a dict with the names in `want`:
        "Jk" [B][nsteps] = 1/2 dx'Q dx + sum_t w_t/2 |r_t|^2, "lx" [B][nsteps][2nr] its exact gradient, "Q" [B][nsteps][2nr][2nr] =
        Q + sum_t w_t Jp_t'Jp_t in the q block (Gauss-Newton: the curvature of the points is dropped), symmetric bit for bit.  Needs
        no tape and changes neither the state nor the tape."""
        nsteps = int(nsteps)
        want, q, qdot, sc, keep = self._cost_inputs("rollout_cost", nsteps, q, qdot, Q, xgoal, want)
        pts = None
        if terms is not None:
            arr, nterms = self._point_terms(terms, "rollout_cost", True)
            xtarget, per = self._targets("rollout_cost", xtarget, nterms)
            pts = _abi.PointTerms(nterms, arr, xtarget.ctypes.data, per)
        out = self._cost_call("rmx_rollout_cost", nsteps, q, qdot, sc, pts, want)
        del keep
        return out

    def rollout_cost_device(self, nsteps, q_ptr, qdot_ptr, Q_ptr=None, xgoal_ptr=None, Q_per_rollout=False, goal_per_rollout=False, terms=None,
                            xtarget_ptr=None, target_per_rollout=False, Jk_ptr=None, lx_ptr=None, Qout_ptr=None):
        """rollout_cost with DEVICE pointers (integers): q, qdot [B][nsteps][nr]; Q [nsteps][2nr*2nr] and xgoal [nsteps][2nr], or one
        table per rollout with the flag set, 0 / None: zero; xtarget [nterms][3] or [B][nterms][3]; Jk [B][nsteps], lx
        [B][nsteps][2nr], Qout [B][nsteps][2nr*2nr], 0 / None: not formed (not all three).  terms stays the host list (None: no
        point targets)."""
        pts = None
        if terms is not None:
            arr, nterms = self._point_terms(terms, "rollout_cost_device", True)
            pts = _abi.PointTerms(nterms, arr, xtarget_ptr or None, int(bool(target_per_rollout)))
        self._cost_call_device("rmx_rollout_cost_device", nsteps, q_ptr, qdot_ptr, Q_ptr, xgoal_ptr, Q_per_rollout, goal_per_rollout, pts, Jk_ptr,
                               lx_ptr, Qout_ptr)

    @staticmethod
    def _frame_terms(terms, who, h=None):
        """terms (a list of dict(body, xlocal, step | t, wpos, wvel, wrot); a missing weight is 0) -> (array of FrameTerm, count)."""
        return BatchSim._terms(_abi.FrameTerm, terms, who, ("wpos", "wvel", "wrot"), False, h)

    def _frame_targets(self, who, nterms, xtarget, vtarget, Rtarget):
        """The target tables of frame terms, each None or shared or one per rollout: ([xtarget, vtarget, Rtarget] as the library reads
        them - Rtarget column-major - and the one per-rollout flag; a shared table beside a per-rollout one is repeated)."""
        B = self.B
        tabs = [None if a is None else _table(who, name, a, (nterms,) + tail, B)
                for name, a, tail in (("xtarget", xtarget, (3,)), ("vtarget", vtarget, (3,)), ("Rtarget", Rtarget, (3, 3)))]
        per = int(any(t is not None and t[1] for t in tabs))
        out = [None if t is None else (np.broadcast_to(t[0], (B,) + t[0].shape) if per and not t[1] else t[0]) for t in tabs]
        if out[2] is not None:      # R[..., r, c] -> column-major
            out[2] = np.swapaxes(out[2], -1, -2)
        return [None if a is None else np.ascontiguousarray(a) for a in out], per

    def rollout_frames(self, nsteps, q, qdot, terms, gx=None, gv=None, gR=None, want=("x", "v", "R")):
        """rmx_rollout_frames: position x [B][nterms][3], point velocity v [B][nterms][3] and orientation R [B][nterms][3][3]
        (R[..., r, c]) of body frames along a state record q, qdot [B][nsteps][nr], and the pull-back of cotangents gx, gv, gR (the
        shapes of x, v, R; None: zero) through them.  terms: a list of dict(body, xlocal, step | t) - weights are not read; the frame
        of term t is taken at the state of row step_t - 1.  Returns (a dict with the names in `want`, gq, gqd): gq, gqd
        [B][nsteps][nr] = sum over the terms of a step of Jp'gx + G'gv + Jw'a(gR R') and Jp'gv, or None, None without a cotangent.
        Needs no tape and changes neither the state nor the tape."""
        nsteps = int(nsteps)
        B, nr = self.B, self.nr
        want = _names("rollout_frames", "want", want, ("x", "v", "R"), any(g is not None for g in (gx, gv, gR)))
        q, qdot = _f64_joint("rollout_frames", ("q", "qdot"), (q, qdot), (B, nsteps, nr))
        arr, nterms = self._frame_terms(terms, "rollout_frames", self.opts.h)
        if gx is not None:
            gx = _f64("rollout_frames", "gx", gx, (B, nterms, 3))
        if gv is not None:
            gv = _f64("rollout_frames", "gv", gv, (B, nterms, 3))
        if gR is not None:
            gR = np.ascontiguousarray(np.swapaxes(_f64("rollout_frames", "gR", gR, (B, nterms, 3, 3)), -1, -2))
        pull = any(g is not None for g in (gx, gv, gR))
        shapes = {"x": (B, nterms, 3), "v": (B, nterms, 3), "R": (B, nterms, 3, 3)}
        out = {w: np.empty(shapes[w]) for w in want}
        gq = np.empty((B, nsteps, nr)) if pull else None
        gqd = np.empty((B, nsteps, nr)) if gv is not None else (np.zeros((B, nsteps, nr)) if pull else None)
        ft = _abi.FrameTerms(nterms, arr, None, None, None, 0)
        _abi.check(self._L.rmx_rollout_frames(self._batch, nsteps, q.ctypes.data, qdot.ctypes.data, C.byref(ft), _addr(out.get("x")),
                                              _addr(out.get("v")), _addr(out.get("R")), _addr(gx), _addr(gv), _addr(gR), _addr(gq),
                                              _addr(gqd) if gv is not None else None), "rmx_rollout_frames")
        if "R" in out:
            out["R"] = np.ascontiguousarray(np.swapaxes(out["R"], -1, -2))
        return out, gq, gqd

    def rollout_frames_device(self, nsteps, q_ptr, qdot_ptr, terms, x_ptr=None, v_ptr=None, R_ptr=None, gx_ptr=None, gv_ptr=None, gR_ptr=None,
                              gq_ptr=None, gqd_ptr=None):
        """rollout_frames with DEVICE pointers (integers): q, qdot, gq, gqd [B][nsteps][nr]; x, v, gx, gv [B][nterms][3]; R, gR
        [B][nterms][9], COLUMN-MAJOR as the library stores a 3x3; 0 / None: not stored / zero.  terms stays the host list."""
        arr, nterms = self._frame_terms(terms, "rollout_frames_device", self.opts.h)
        ft = _abi.FrameTerms(nterms, arr, None, None, None, 0)
        _abi.check(self._L.rmx_rollout_frames_device(self._batch, int(nsteps), _vp(q_ptr), _vp(qdot_ptr), C.byref(ft), _vp(x_ptr), _vp(v_ptr),
                                                     _vp(R_ptr), _vp(gx_ptr), _vp(gv_ptr), _vp(gR_ptr), _vp(gq_ptr), _vp(gqd_ptr)),
                   "rmx_rollout_frames_device")

    def rollout_cost_frames(self, nsteps, q, qdot, Q=None, xgoal=None, terms=None, xtarget=None, vtarget=None, Rtarget=None,
                            want=("Jk", "lx", "Q")):
        """rmx_rollout_cost_frames: rollout_cost with frame terms - dict(body, xlocal, step | t, wpos, wvel, wrot), a missing weight is
        0 - and the targets xtarget, vtarget [nterms][3] and Rtarget [nterms][3][3] (R[..., r, c]), each shared or [B][..]; a table may
        be None where no term weighs it.  Per term the cost is wpos/2 |p - xtarget|^2 + wvel/2 |v - vtarget|^2 + wrot/4 |R -
        Rtarget|_F^2 (the last: wrot (1 - cos theta)); "lx" is its exact gradient in (q, qdot), "Q" the Gauss-Newton table with the
        velocity terms' q, qdot cross blocks, symmetric bit for bit.  Needs no tape and changes neither the state nor the tape."""
        nsteps = int(nsteps)
        want, q, qdot, sc, keep = self._cost_inputs("rollout_cost_frames", nsteps, q, qdot, Q, xgoal, want)
        ft = None
        if terms is not None:
            arr, nterms = self._frame_terms(terms, "rollout_cost_frames", self.opts.h)
            tabs, per = self._frame_targets("rollout_cost_frames", nterms, xtarget, vtarget, Rtarget)
            ft = _abi.FrameTerms(nterms, arr, _addr(tabs[0]), _addr(tabs[1]), _addr(tabs[2]), per)
        out = self._cost_call("rmx_rollout_cost_frames", nsteps, q, qdot, sc, ft, want)
        del keep
        return out

    def rollout_cost_frames_device(self, nsteps, q_ptr, qdot_ptr, Q_ptr=None, xgoal_ptr=None, Q_per_rollout=False, goal_per_rollout=False,
                                   terms=None, xtarget_ptr=None, vtarget_ptr=None, Rtarget_ptr=None, target_per_rollout=False, Jk_ptr=None,
                                   lx_ptr=None, Qout_ptr=None):
        """rollout_cost_frames with DEVICE pointers (integers), as rollout_cost_device; vtarget [nterms][3] and Rtarget [nterms][9]
        (COLUMN-MAJOR) or one table per rollout with the flag set - the three target tables share the flag."""
        ft = None
        if terms is not None:
            arr, nterms = self._frame_terms(terms, "rollout_cost_frames_device", self.opts.h)
            ft = _abi.FrameTerms(nterms, arr, xtarget_ptr or None, vtarget_ptr or None, Rtarget_ptr or None, int(bool(target_per_rollout)))
        self._cost_call_device("rmx_rollout_cost_frames_device", nsteps, q_ptr, qdot_ptr, Q_ptr, xgoal_ptr, Q_per_rollout, goal_per_rollout, ft,
                               Jk_ptr, lx_ptr, Qout_ptr)

    @staticmethod
    def _search_alphas(who, alphas):
        """The trial step lengths of a search as a host array (kept by the caller until the call returns) and their count."""
        al = np.ascontiguousarray(np.asarray(() if alphas is None else alphas, dtype=np.float64).reshape(-1))
        if al.size > _abi.SEARCH_MAX_ALPHAS:
            raise ValueError("%s: at most %d alphas, got %d" % (who, _abi.SEARCH_MAX_ALPHAS, al.size))
        return al, int(al.size)

    def rollout_search(self, nsteps, h, ubar, kff=None, K=None, xref=None, alphas=(), Jbar=None, Q=None, xgoal=None, R=None, terms=None,
                       xtarget=None, vtarget=None, Rtarget=None, ulim=None, pscale=1.0, stats=False, want=("alpha", "trials", "status")):
        """rmx_rollout_search: the backtracking line search of iLQR in one launch, BDF1.  Every rollout runs the closed loop of
        rollout_feedback (K, xref, ulim as there) from the current state under uff = ubar + a*kff for a in `alphas`, in order, and
        stops at the first pass without a failed solve whose cost is below Jbar[b]; with none (or no alphas) it runs the nominal
        pass, uff = ubar.  The cost is that of rollout_cost_frames (Q, xgoal, terms and their targets; each may be None) plus
        1/2 u'R u on the applied torques (R [nr][nr] symmetric, or None), summed over the steps inside the launch.  Returns
        (qtraj, qdtraj, uapp, out): the record and applied torques of the pass each rollout ended on, and a dict with "J" [B] and the
        names in `want` - "alpha" [B] (0: none accepted), "trials" [B] int32 (passes run), "status" [B] int32 (Newton status of the
        last pass) - and, with stats=True, "info".  The tape it leaves is the open-loop tape under uapp.  Not differentiable."""
        who = "rollout_search"
        nsteps = int(nsteps)
        B, nr = self.B, self.nr
        want = _names(who, "want", want, ("alpha", "trials", "status"), True)
        ubar = self._controls(who, "ubar", ubar, nsteps)
        al, nalpha = self._search_alphas(who, alphas)
        if nalpha:
            if kff is None or Jbar is None:
                raise ValueError("%s: alphas need kff and Jbar" % who)
            kff = _f64(who, "kff", kff, (B, nsteps, nr))
            Jbar = _f64(who, "Jbar", Jbar, (B,))
        else:
            kff = Jbar = None
        K, xref, per = self._feedback_tables(nsteps, K, xref, who)
        fb = _abi.Feedback(_addr(ubar), _addr(K), _addr(xref), per)
        sc = None
        if Q is not None or xgoal is not None:
            sc = _abi.StateCost(None, None, 0, 0)
            if Q is not None:      # (symmetric: row-major memory is the column-major table)
                Q, sc.Q_per_rollout = _table(who, "Q", Q, (nsteps, 2 * nr, 2 * nr), B)
                sc.Q = Q.ctypes.data
            if xgoal is not None:
                xgoal, sc.goal_per_rollout = _table(who, "xgoal", xgoal, (nsteps, 2 * nr), B)
                sc.xgoal = xgoal.ctypes.data
        ft, keep = None, None
        if terms is not None:
            arr, nterms = self._frame_terms(terms, who, self.opts.h if h is None else h)
            tabs, tper = self._frame_targets(who, nterms, xtarget, vtarget, Rtarget)
            ft = _abi.FrameTerms(nterms, arr, _addr(tabs[0]), _addr(tabs[1]), _addr(tabs[2]), tper)
            keep = (arr, tabs)
        if R is not None:
            R = _f64(who, "R", R, (nr, nr))
        cost = _abi.SearchCost(None if sc is None else C.pointer(sc), None if ft is None else C.pointer(ft), _addr(R))
        srch = _abi.Search(_addr(kff), _abi.dptr(al) if nalpha else None, nalpha, _addr(Jbar))
        qtraj, qdtraj, uapp = (np.empty((B, nsteps, nr)) for _ in range(3))
        out = {"J": np.empty(B)}
        for w in want:
            out[w] = np.empty(B) if w == "alpha" else np.zeros(B, dtype=np.int32)
        so = _abi.SearchOut(_addr(out["J"]), _addr(out.get("alpha")), _addr(out.get("trials")), _addr(out.get("status")))
        box, lim = self._ulim(ulim, who) if ulim is not None else (None, None)
        opts, info, st = self._begin_tape(h, stats, 1)
        _abi.check(self._L.rmx_rollout_search(self._batch, C.byref(opts), nsteps, float(pscale), C.byref(fb), None if box is None else C.byref(box),
                                              C.byref(srch), C.byref(cost), qtraj.ctypes.data, qdtraj.ctypes.data, uapp.ctypes.data, C.byref(so), st),
                   "rmx_rollout_search")
        del keep, lim
        if stats:
            info["ms"] = self._L.rmx_last_step_ms(self._batch)
            out["info"] = info
        return qtraj, qdtraj, uapp, out

    def rollout_search_device(self, nsteps, h, ubar_ptr, kff_ptr, K_ptr, xref_ptr, alphas, Jbar_ptr, qtraj_ptr, qdtraj_ptr, uapp_ptr, J_ptr,
                              alpha_ptr=None, trials_ptr=None, status_ptr=None, per_rollout=False, Q_ptr=None, xgoal_ptr=None,
                              Q_per_rollout=False, goal_per_rollout=False, R_ptr=None, terms=None, xtarget_ptr=None, vtarget_ptr=None,
                              Rtarget_ptr=None, target_per_rollout=False, ulim=None, pscale=1.0, stats=False):
        """rollout_search with DEVICE pointers (integers): ubar, kff, qtraj, qdtraj, uapp [B][nsteps][nr]; K, xref as
        rollout_feedback_device; Jbar, J, alpha [B] doubles; trials, status [B] int32; the cost's tables as rollout_cost_frames_device
        (Rtarget COLUMN-MAJOR), R [nr*nr]; ulim=(ulo_ptr, uhi_ptr).  alphas and terms stay host objects.  0 / None: kff and Jbar with
        no alphas, K (no feedback), xref (zero), qtraj and qdtraj together (no record), uapp, alpha, trials, status (not stored), any
        part of the cost (not all of Q/xgoal, terms and R).  Returns info."""
        who = "rollout_search_device"
        al, nalpha = self._search_alphas(who, alphas)
        fb = _abi.Feedback(ubar_ptr or None, K_ptr or None, xref_ptr or None, int(bool(per_rollout)))
        sc = _abi.StateCost(Q_ptr or None, xgoal_ptr or None, int(bool(Q_per_rollout)), int(bool(goal_per_rollout)))
        ft, arr = None, None
        if terms is not None:
            arr, nterms = self._frame_terms(terms, who, self.opts.h if h is None else h)
            ft = _abi.FrameTerms(nterms, arr, xtarget_ptr or None, vtarget_ptr or None, Rtarget_ptr or None, int(bool(target_per_rollout)))
        cost = _abi.SearchCost(C.pointer(sc) if (Q_ptr or xgoal_ptr) else None, None if ft is None else C.pointer(ft), R_ptr or None)
        srch = _abi.Search(kff_ptr or None, _abi.dptr(al) if nalpha else None, nalpha, Jbar_ptr or None)
        so = _abi.SearchOut(J_ptr or None, alpha_ptr or None, trials_ptr or None, status_ptr or None)
        box = None if ulim is None else _abi.Box(ulim[0] or None, ulim[1] or None)
        opts, info, st = self._begin_tape(h, stats, 1)
        _abi.check(self._L.rmx_rollout_search_device(self._batch, C.byref(opts), int(nsteps), float(pscale), C.byref(fb),
                                                     None if box is None else C.byref(box), C.byref(srch), C.byref(cost), _vp(qtraj_ptr),
                                                     _vp(qdtraj_ptr), _vp(uapp_ptr), C.byref(so), st), "rmx_rollout_search_device")
        del arr
        info["ms"] = self._L.rmx_last_step_ms(self._batch)
        return info

    def last_step_kernel(self):
        """Label of the step kernel the last step call launched (rmx_last_step_kernel): which size / batch / environment dependent
        variant the library chose."""
        return self._L.rmx_last_step_kernel(self._batch).decode()

    def step_ticks(self):
        """Shader-clock ticks each rollout's wavefront spent in the kernel(s) of the last step call (rmx_step_ticks): [B] uint64."""
        t = np.zeros(self.B, dtype=np.uint64)
        _abi.check(self._L.rmx_step_ticks(self._batch, t.ctypes.data_as(C.POINTER(C.c_ulonglong))), "rmx_step_ticks")
        return t

    def step_bdf1_async(self, nsteps, h=None):
        if h is not None:
            self.opts.h = float(h)
        self._async = None
        _abi.check(self._L.rmx_step_bdf1_async(self._batch, C.byref(self.opts), int(nsteps)), "rmx_step_bdf1_async")

    def step_bdf2_async(self, nsteps, h=None):
        if h is not None:
            self.opts.h = float(h)
        self._async = None
        _abi.check(self._L.rmx_step_bdf2_async(self._batch, C.byref(self.opts), int(nsteps)), "rmx_step_bdf2_async")

    def step_history_async(self, nsteps, integrator=1, record=_abi.REC_ENERGY | _abi.REC_STATE, h=None):
        """simLoop enqueued, nothing waited for; `record` (REC_ENERGY | REC_STATE | REC_CHARTS) stays on the device until
        history_read() (after sync())."""
        if h is not None:
            self.opts.h = float(h)
        self._async = (int(nsteps), int(record))
        _abi.check(self._L.rmx_step_history_async(self._batch, C.byref(self.opts), int(nsteps), int(integrator), int(record)), "rmx_step_history_async")

    def history_read(self):
        if self._async is None:
            raise _abi.RedMaxHipError("history_read: no step_history_async record is outstanding on this batch "
                                      "(the last step call was synchronous, unrecorded, or has replaced it)")
        nsteps, record = self._async
        out, hist = _history_arrays(self.B, self.nr, self.nsph, nsteps, record)
        _abi.check(self._L.rmx_history_read(self._batch, C.byref(hist)), "rmx_history_read")
        return out

    def sync(self):
        _abi.check(self._L.rmx_sync(self._batch), "rmx_sync")
        return self._L.rmx_last_step_ms(self._batch)

    def profile_phases(self, reps=20, h=1e-2):
        """Mean cycles per wavefront of (g-eval, g+H-eval, LU solve, 2 reductions) at the current state."""
        c = np.zeros(16)
        _abi.check(self._L.rmx_profile_phases(self._batch, int(reps), float(h), _abi.dptr(c)), "rmx_profile_phases")
        d = dict(zip(("eval_g", "eval_gH", "lu", "reductions"), c[:4]))
        d["gH_stamps"] = dict(zip(("joint_T", "jump_E", "screw_phi", "xi_beta", "inertia_w", "lds_write", "suffix_scan",
                                   "subtree_read", "residual", "H_vectors", "col_write", "H_columns"), c[4:]))
        return d

    def stats_reset(self):
        _abi.check(self._L.rmx_stats_reset(self._batch), "rmx_stats_reset")

    def stats_read(self):
        out, st = _stats_arrays(self.B)
        _abi.check(self._L.rmx_stats_read(self._batch, C.byref(st)), "rmx_stats_read")
        return out

    def energy(self):
        T = np.empty(self.B)
        V = np.empty(self.B)
        _abi.check(self._L.rmx_energy(self._batch, _abi.dptr(T), _abi.dptr(V)), "rmx_energy")
        return T, V


class GroupSim:
    """The whole batch over a LIST of devices (rmx_group_*, include/redmax_hip.h): one model + batch per listed device, contiguous
    shards, every array the whole batch.  ``step`` launches all shards before it waits for the first - the multi-device simLoop a
    single host thread (MATLAB: matlab/+redmax/HipSim.m with a device vector) can drive; a device may be listed more than once."""

    def __init__(self, scene_or_desc, batch, devices=(0,), tape_forces=False):
        d = scene_or_desc.desc() if hasattr(scene_or_desc, "desc") else scene_or_desc
        self._L = _abi.lib()
        if tape_forces:      # (a group takes no force table and records no tape: the keyword cannot be honoured)
            raise _abi.RedMaxHipError("GroupSim: tape_forces is BatchSim's (rmx_model_tape_point_forces); a group has neither point "
                                      "forces nor taped rollouts")
        if d.get("point_forces"):
            raise _abi.RedMaxHipError("GroupSim: rmx_group_create has no slot for point forces (ForcePointPoint / ForceSpringDamper / "
                                      "ForceCable); use BatchSim")
        self._desc, self._keep = _abi.make_desc(d)
        gc = _abi.make_ground_contact(d, self._keep)
        dev = np.ascontiguousarray(list(devices), dtype=np.int32)
        self._g = C.c_void_p()
        _abi.check(self._L.rmx_group_create(C.byref(self._desc), C.byref(gc) if gc is not None else None, int(batch), _abi.iptr(dev),
                                            len(dev), C.byref(self._g)), "rmx_group_create")
        self.B = int(batch)
        self.nshards = self._L.rmx_group_nshards(self._g)
        m0 = self._L.rmx_group_shard_model(self._g, 0)
        self.nr, self.nsph = self._L.rmx_model_nr(m0), self._L.rmx_model_nsph(m0)
        self.shards = []
        for s in range(self.nshards):
            dv, f, c = C.c_int(), C.c_int(), C.c_int()
            _abi.check(self._L.rmx_group_shard(self._g, s, C.byref(dv), C.byref(f), C.byref(c)), "rmx_group_shard")
            self.shards.append((dv.value, f.value, c.value))
        self.opts = _abi.Opts()
        self._L.rmx_opts_default(C.byref(self.opts))
        self._async = None

    def close(self):
        if getattr(self, "_g", None):
            self._L.rmx_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _arr(self, a):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (self.B, self.nr)))

    def set_state(self, q, qdot):
        q, qdot = self._arr(q), self._arr(qdot)
        _abi.check(self._L.rmx_group_set_state(self._g, _abi.dptr(q), _abi.dptr(qdot)), "rmx_group_set_state")

    def get_state(self):
        q, qd = np.empty((self.B, self.nr)), np.empty((self.B, self.nr))
        _abi.check(self._L.rmx_group_get_state(self._g, _abi.dptr(q), _abi.dptr(qd)), "rmx_group_get_state")
        return q, qd

    GATHER_ALL = -1      # RMX_GATHER_ALL

    def gather_device(self, d_q, d_qdot, root=GATHER_ALL):
        """The final gather with device-resident destinations (rmx_group_gather_device): d_q[s], d_qdot[s] = raw device pointers
        (ints; e.g. torch tensor.data_ptr()) of [batch][nr] float64 arrays on shard s's device, None for a shard that receives nothing.
        root: a shard index, or GATHER_ALL.  RCCL (single-process clique over the group's devices) when the devices are pairwise
        distinct, device-to-device copies when a device is listed twice.  Returns how the gather travelled (rmx_group_gather_path)."""
        P = C.c_void_p * self.nshards
        pq = P(*[C.c_void_p(int(p)) if p else None for p in d_q])
        pqd = P(*[C.c_void_p(int(p)) if p else None for p in d_qdot])
        _abi.check(self._L.rmx_group_gather_device(self._g, pq, pqd, int(root)), "rmx_group_gather_device")
        return self._L.rmx_group_gather_path(self._g).decode()

    def gather(self, root=GATHER_ALL):
        """The same gather into destinations the group owns on the receiving shards' devices (rmx_group_gather)."""
        _abi.check(self._L.rmx_group_gather(self._g, int(root)), "rmx_group_gather")
        return self._L.rmx_group_gather_path(self._g).decode()

    def gathered_read(self, shard=0):
        """Host copy of shard `shard`'s gathered (q, qdot) ([batch][nr]); gathered_ptrs: its device pointers."""
        q, qd = np.empty((self.B, self.nr)), np.empty((self.B, self.nr))
        _abi.check(self._L.rmx_group_gathered_read(self._g, int(shard), _abi.dptr(q), _abi.dptr(qd)), "rmx_group_gathered_read")
        return q, qd

    def gathered_ptrs(self, shard=0):
        a, b = C.c_void_p(), C.c_void_p()
        _abi.check(self._L.rmx_group_gathered(self._g, int(shard), C.byref(a), C.byref(b)), "rmx_group_gathered")
        return a.value, b.value

    def _outputs(self, nsteps, record):
        out, st = _stats_arrays(self.B)
        rec, hist = _history_arrays(self.B, self.nr, self.nsph, nsteps, record)
        out.update(rec)
        return out, st, hist

    def step(self, nsteps, integrator=1, h=None, record=0):
        """simLoop of the whole batch (rmx_group_step); returns counters + the recorded per-step arrays + timing."""
        if h is not None:
            self.opts.h = float(h)
        out, st, hist = self._outputs(int(nsteps), int(record))
        _abi.check(self._L.rmx_group_step(self._g, C.byref(self.opts), int(nsteps), int(integrator), C.byref(st), C.byref(hist)), "rmx_group_step")
        out.update(self.timing())
        return out

    def step_async(self, nsteps, integrator=1, h=None, record=0):
        if h is not None:
            self.opts.h = float(h)
        self._async = (int(nsteps), int(record))
        _abi.check(self._L.rmx_group_step_async(self._g, C.byref(self.opts), int(nsteps), int(integrator), int(record)), "rmx_group_step_async")

    def sync(self):
        if self._async is None:
            raise _abi.RedMaxHipError("GroupSim.sync: no step_async launch is outstanding on this group")
        nsteps, record = self._async
        self._async = None
        out, st, hist = self._outputs(nsteps, record)
        _abi.check(self._L.rmx_group_sync(self._g, C.byref(st), C.byref(hist)), "rmx_group_sync")
        out.update(self.timing())
        return out

    def energy(self):
        T, V = np.empty(self.B), np.empty(self.B)
        _abi.check(self._L.rmx_group_energy(self._g, _abi.dptr(T), _abi.dptr(V)), "rmx_group_energy")
        return T, V

    def timing(self):
        """wall_ms of the last step and, per shard, kernel ms and the start / end of its launch relative to the first shard on the
        same device (rmx_group_timing)."""
        w = C.c_double()
        k, t0, t1 = np.zeros(self.nshards), np.zeros(self.nshards), np.zeros(self.nshards)
        _abi.check(self._L.rmx_group_timing(self._g, C.cast(C.byref(w), _abi._dp), _abi.dptr(k), _abi.dptr(t0), _abi.dptr(t1)), "rmx_group_timing")
        return {"wall_ms": w.value, "kernel_ms": k, "start_ms": t0, "end_ms": t1}
