"""A small batched iLQR on a quadratic cost: one problem per rollout of a BatchSim, BDF1.

The backward pass (``backward_pass``) is pure torch and runs on any device; the dynamics stay in the library: every iteration
linearises the nominal rollout with ``diff.linearize`` (rmx_rollout_tape_device + rmx_rollout_linearize_device) and runs its line
search in closed loop with ``diff.rollout_feedback`` (rmx_rollout_tape_feedback_device) - the whole batch, all steps, one launch
per trial step length.  With ``solve(backward="device")`` the backward pass leaves torch too: one launch of the library's Riccati
sweep on the tape the forward pass left (``diff.lqr_backward``, rmx_rollout_lqr_device), ``backward_pass`` staying the definition it
is checked against.  torch is imported inside the functions, as in ``diff``.

Conventions.  x = (q, qdot), 2nr entries.  Step k = 1 .. N takes x_{k-1} and the torque u_k to x_k; x_0 = (q0, qdot0) is fixed.
Arrays over the steps hold step k in row k-1.  The feedback acts on the state at the START of the step:
    u_k = ubar_k + alpha k_k + K_k (x_{k-1} - xbar_{k-1}).
Gains are returned in the usual order, K[b, k-1, i, j] = du_i/dx_j; ``diff.rollout_feedback`` wants the transpose.
"""
from __future__ import annotations

from collections import namedtuple


class QuadraticCost:
    """J_b = sum_{k=1..N} 1/2 (x_k - xg_k)' Q_k (x_k - xg_k) + 1/2 u_k' R u_k.

    Q: [N][2nr][2nr] symmetric positive semi-definite, R: [nr][nr] symmetric positive definite, xgoal: [1 or B][N][2nr] (row k-1 the
    goal for the state after step k) - float64 tensors on one device."""

    def __init__(self, Q, R, xgoal):
        if Q.dim() != 3 or Q.shape[1] != Q.shape[2]:
            raise ValueError("QuadraticCost: Q must have shape (N, 2nr, 2nr), got %r" % (tuple(Q.shape),))
        N, nx = Q.shape[0], Q.shape[1]
        if R.dim() != 2 or R.shape[0] != R.shape[1] or 2 * R.shape[0] != nx:
            raise ValueError("QuadraticCost: R must have shape (%d, %d), got %r" % (nx // 2, nx // 2, tuple(R.shape)))
        if xgoal.dim() != 3 or tuple(xgoal.shape[1:]) != (N, nx):
            raise ValueError("QuadraticCost: xgoal must have shape (1 or B, %d, %d), got %r" % (N, nx, tuple(xgoal.shape)))
        self.Q, self.R, self.xgoal = Q, R, xgoal

    def value(self, x, u):
        """J [B] of the states x [B][N][2nr] (after every step) and torques u [B][N][nr]."""
        import torch
        dx = x - self.xgoal
        return 0.5 * (torch.einsum("bki,kij,bkj->b", dx, self.Q, dx) + torch.einsum("bki,ij,bkj->b", u, self.R, u))

    def gradients(self, x, u):
        """(lx [B][N][2nr], lu [B][N][nr]) = dJ/dx_k, dJ/du_k."""
        import torch
        return torch.einsum("kij,bkj->bki", self.Q, x - self.xgoal), torch.einsum("ij,bkj->bki", self.R, u)


class TrackingCost:
    """J_b = sum_{k=1..N} 1/2 (x_k - xg_k)' Q_k (x_k - xg_k) + 1/2 u_k' R u_k + sum_t 1/2 w_t |p_t(q_{step_t}) - xtarget_t|^2:
    QuadraticCost plus point targets in task space - a point of a body brought to a world target at a step.

    sim: the BatchSim the rollouts run on; Q, R, xgoal: as QuadraticCost (Q, xgoal may be None: no joint-space state cost); terms: a
    list of dict(body, xlocal, step, wpos), wpos >= 0 (``BatchSim.adjoint_track``'s term); xtarget: [nterms][3] or [B][nterms][3] -
    float64 tensors on the sim's device.  The state part is evaluated on the device (``diff.cost_model``, rmx_rollout_cost_device):
    the value and the gradient are exact, ``model`` returns the Gauss-Newton Hessian Q_k + sum_t w_t Jp_t'Jp_t per rollout - the
    curvature of the points is dropped, so the table stays positive semi-definite.  The control part stays torch.

    Frame targets: a term may also carry wvel and wrot, adding wvel/2 |v_t - vtarget_t|^2 on the velocity of its point and
    wrot/4 |R_t - Rtarget_t|_F^2 = wrot (1 - cos theta) on the orientation of its body (``diff.cost_model`` then goes through
    rmx_rollout_cost_frames_device); vtarget: [nterms][3], Rtarget: [nterms][3][3] (R[..., r, c]), or one table per rollout; a table
    may be None where no term weighs it.  Without such a term the cost is the one above, bit for bit."""

    def __init__(self, sim, Q, R, xgoal, terms, xtarget, vtarget=None, Rtarget=None):
        if R.dim() != 2 or R.shape[0] != R.shape[1] or R.shape[0] != sim.nr:
            raise ValueError("TrackingCost: R must have shape (%d, %d), got %r" % (sim.nr, sim.nr, tuple(R.shape)))
        self.sim, self.Q, self.R, self.xgoal = sim, Q, R, xgoal
        self.terms, self.xtarget = [dict(t) for t in terms], xtarget
        self.vtarget, self.Rtarget = vtarget, Rtarget

    def _state(self, x, want):
        from . import diff
        nr = self.sim.nr
        xg = self.xgoal
        if xg is not None and xg.dim() == 3 and xg.shape[0] == 1:
            xg = xg[0]
        return diff.cost_model(self.sim, x[..., :nr], x[..., nr:], Q=self.Q, xgoal=xg, terms=self.terms, xtarget=self.xtarget, want=want,
                               vtarget=self.vtarget, Rtarget=self.Rtarget)

    def _lu(self, u):
        import torch
        return torch.einsum("ij,bkj->bki", self.R, u)

    def value(self, x, u):
        """J [B] of the states x [B][N][2nr] (after every step) and torques u [B][N][nr]."""
        import torch
        return self._state(x, ("J",))["J"] + 0.5 * torch.einsum("bki,ij,bkj->b", u, self.R, u)

    def gradients(self, x, u):
        """(lx [B][N][2nr], lu [B][N][nr]) = dJ/dx_k, dJ/du_k (exact)."""
        return self._state(x, ("lx",))["lx"], self._lu(u)

    def model(self, x, u):
        """(lx, lu, Qfull [B][N][2nr][2nr]): the gradients and the Gauss-Newton Hessian of the state cost, one table per rollout."""
        m = self._state(x, ("lx", "Q"))
        return m["lx"], self._lu(u), m["Q"]


def backward_pass(A, Bm, lx, lu, Q, R, mu=0.0):
    """The Riccati recursion of iLQR for a quadratic cost, batched: (k, K, expected).

    A [B][N][2nr][2nr], Bm [B][N][2nr][nr]: dx_k/dx_{k-1}, dx_k/du_k (``diff.linearize``); lx [B][N][2nr], lu [B][N][nr]: the cost's
    gradients at the nominal; Q [N][2nr][2nr], shared by the batch, or [B][N][2nr][2nr], one table per rollout (``TrackingCost.model``),
    R [nr][nr]: its Hessians; mu >= 0: the regulariser of Quu.  With V the cost-to-go at x_k
    (state cost of step k included; Vx_N = lx_N, Vxx_N = Q_N), for k = N .. 1:
        Qx = A' Vx        Qu = lu + B' Vx        Qxx = A' Vxx A        Qux = B' Vxx A        Quu = R + B' Vxx B + mu I
        k = -Quu^-1 Qu    K = -Quu^-1 Qux
        Vx  <- lx_{k-1} + Qx  + K' Quu0 k + K' Qu  + Qux' k          (Quu0: Quu without mu I; lx_0, Q_0: zero - x_0 is fixed)
        Vxx <- Q_{k-1}  + Qxx + K' Quu0 K + K' Qux + Qux' K
    Returns k [B][N][nr], K [B][N][nr][2nr] (K[.., i, j] = du_i/dx_j) and expected [B] = -sum_k (Qu' k + 1/2 k' Quu0 k): the decrease
    of the quadratic model of J under the full step (alpha = 1), the exact decrease where the dynamics are linear.  Works on CPU
    tensors."""
    import torch
    B, N, nx, nu = Bm.shape
    kff = torch.empty((B, N, nu), dtype=A.dtype, device=A.device)
    K = torch.empty((B, N, nu, nx), dtype=A.dtype, device=A.device)
    expected = torch.zeros(B, dtype=A.dtype, device=A.device)
    eye = torch.eye(nu, dtype=A.dtype, device=A.device)
    Vx = lx[:, N - 1]
    per = Q.dim() == 4                                                 # one table per rollout
    Vxx = Q[:, N - 1] if per else Q[N - 1].expand(B, nx, nx)
    for s in range(N - 1, -1, -1):
        Ak, Bk = A[:, s], Bm[:, s]
        BtV = Bk.transpose(1, 2) @ Vxx
        Qx = (Ak.transpose(1, 2) @ Vx.unsqueeze(-1)).squeeze(-1)
        Qu = lu[:, s] + (Bk.transpose(1, 2) @ Vx.unsqueeze(-1)).squeeze(-1)
        Qxx = Ak.transpose(1, 2) @ Vxx @ Ak
        Qux = BtV @ Ak
        Quu0 = R + BtV @ Bk
        Quu0 = 0.5 * (Quu0 + Quu0.transpose(1, 2))
        sol = torch.linalg.solve(Quu0 + mu * eye, torch.cat([Qu.unsqueeze(-1), Qux], dim=-1))
        ks, Ks = -sol[..., 0], -sol[..., 1:]
        kff[:, s], K[:, s] = ks, Ks
        Qk = (Quu0 @ ks.unsqueeze(-1)).squeeze(-1)
        expected = expected - ((Qu * ks).sum(-1) + 0.5 * (ks * Qk).sum(-1))
        KtQuu = Ks.transpose(1, 2) @ Quu0
        Vx = Qx + (KtQuu @ ks.unsqueeze(-1)).squeeze(-1) + (Ks.transpose(1, 2) @ Qu.unsqueeze(-1)).squeeze(-1) \
            + (Qux.transpose(1, 2) @ ks.unsqueeze(-1)).squeeze(-1)
        Vxx = Qxx + KtQuu @ Ks + Ks.transpose(1, 2) @ Qux + Qux.transpose(1, 2) @ Ks
        Vxx = 0.5 * (Vxx + Vxx.transpose(1, 2))
        if s > 0:
            Vx = Vx + lx[:, s - 1]
            Vxx = Vxx + (Q[:, s - 1] if per else Q[s - 1])
    return kff, K, expected


Result = namedtuple("Result", "u qtraj qdtraj cost alpha")


def solve(sim, q0, qdot0, u0, cost, iters=10, alphas=(1.0, 0.5, 0.25, 0.125, 0.0625), mu=1e-6, h=None, pscale=1.0, backward="torch", ulim=None,
          search="host"):
    """Batched iLQR: one problem per rollout of ``sim`` (a BatchSim), BDF1.  Returns (result, history).

    q0, qdot0 [B][nr], u0 [B][N][nr]: float64 tensors on the sim's device; cost: a QuadraticCost on that device, or a cost with
    ``value``, ``R`` and ``model(x, u) -> (lx, lu, Q [B][N][2nr][2nr])`` - a TrackingCost, whose Q is a Gauss-Newton table per
    rollout.  Each iteration
      1. linearises the nominal (``diff.linearize`` at the nominal torques) and runs ``backward_pass``;
      2. for each alpha in turn launches ``diff.rollout_feedback`` on the whole batch with uff = ubar + alpha_b k, the gains K per
         rollout and xref = xbar; a rollout keeps the FIRST alpha that lowers its own cost and is launched with that alpha again
         from then on (the kernel is deterministic: it returns the same bits);
      3. a rollout no alpha helps keeps its nominal: alpha = 0 with K around xbar reproduces xbar, bit for bit - the state
         differences are exact zeros -, because every nominal comes from the feedback kernel itself;
      4. where the last launch held a rejected candidate, one more launch with the final alphas follows, so that the sim's tape and
         state, and the nominal of the next iteration, belong to the accepted trajectories.
    result: u [B][N][nr] (the applied torques of the last launch), qtraj, qdtraj, cost [B], alpha [B] (the last iteration's step
    lengths, 0: no step taken).  history: [iters+1][B], the cost before the first and after every iteration - non-increasing per
    rollout.  The sim is left at the end of the returned trajectories with their open-loop tape (rollout_vjp and the others may
    follow).
    backward: "torch" (the default) is step 1 as written above.  "device" runs the backward pass as ONE launch on the tape the
    previous launch left (``diff.lqr_backward``, rmx_rollout_lqr_device): no ``diff.linearize``, no extra forward launch per
    iteration and no A_k, B_k in memory; needs nr <= 32.  A rollout whose Quu + mu I is not positive definite there gets zero gains
    and keeps alpha = 0 in that iteration.  The two paths evaluate one recursion in different summation orders: their results agree
    to rounding, not bit for bit.
    ulim=(ulo, uhi), float64 tensors [nr] on the sim's device or None each: torque limits ulo <= u <= uhi, control-limited DDP
    (Tassa, Mansard, Todorov 2014).  Every launch is then the clamped feedback rollout (u0 is clamped by the first launch itself),
    and the backward pass is ``diff.lqr_backward_box`` at ubar = the applied torques of the accepted launch; it exists on the device
    alone, so backward must be "device".  A rollout whose backward pass reports a status != 0 keeps alpha = 0 in that iteration.
    ``backward_pass`` knows no limits.
    search: "host" (the default) is steps 2 - 4 as written above.  "device" runs the whole line search of an iteration as ONE launch
    (``diff.rollout_search``, rmx_rollout_search_device): every rollout tries its alphas in turn inside the wavefront that integrates
    it, with the cost evaluated in the launch, and ends on the trajectory it keeps - no relaunch of accepted rollouts, no cost
    launches, no host round trip per alpha.  An iteration is then ``quadratic_model``, ``lqr_backward[_box]`` and one
    ``rollout_search``; it needs backward="device" and a QuadraticCost or TrackingCost (the costs the launch knows).  A rollout whose
    sweep flags it has zero gains and is passed Jbar = -inf: it ends on its nominal pass.  The two searches apply one rule in
    different summation orders of J: they may accept different alphas where a trial's J lies within rounding of Jbar."""
    import torch
    from . import diff
    if backward not in ("torch", "device"):
        raise ValueError("solve: backward must be 'torch' or 'device', got %r" % (backward,))
    if search not in ("host", "device"):
        raise ValueError("solve: search must be 'host' or 'device', got %r" % (search,))
    if search == "device" and backward != "device":
        raise ValueError("solve: search='device' needs backward='device': the search follows the Riccati sweep on the tape it leaves")
    if search == "device" and not isinstance(cost, (QuadraticCost, TrackingCost)):
        raise ValueError("solve: search='device' knows QuadraticCost and TrackingCost (the costs rmx_rollout_search evaluates), got %s"
                         % type(cost).__name__)
    if ulim is not None and backward != "device":
        raise ValueError("solve: torque limits (ulim) need backward='device': the box-constrained backward pass exists on the device alone")
    diff._check_inputs(sim, q0, qdot0, u0)
    B, N, nr = u0.shape
    has_model = hasattr(cost, "model")                                 # a cost with a Hessian of its own per rollout (TrackingCost)
    if not has_model and tuple(cost.Q.shape) != (N, 2 * nr, 2 * nr):
        raise ValueError("solve: the cost is for %d steps of %d states, the rollout has %d steps of %d" % (cost.Q.shape[0], cost.Q.shape[1], N, 2 * nr))
    x0 = torch.cat([q0, qdot0], dim=-1).unsqueeze(1)
    kw = dict(h=h, pscale=pscale, integrator=1)
    if ulim is not None:
        kw["ulim"] = ulim

    tape = [None]                                                      # sim.tape_count after the last launch

    def launch(uff, K, xref):
        qt, qdt, ua, failed = diff.rollout_feedback(sim, q0, qdot0, uff, K, xref, check=False, status=True, **kw)
        tape[0] = sim.tape_count
        x = torch.cat([qt, qdt], dim=-1)
        J = cost.value(x, ua)
        return qt, qdt, ua, x, torch.where(torch.isfinite(J) & ~failed, J, torch.full_like(J, float("inf")))      # (a failed solve: never accepted)

    def searched(ub, kff, K, xref, als, Jb):                           # search="device": one launch, the cost inside it
        qt, qdt, ua, J, al, st = diff.rollout_search(sim, q0, qdot0, ub, kff, K, xref, als, Jb, cost=cost, ulim=ulim, h=h, pscale=pscale)
        tape[0] = sim.tape_count
        J = torch.where(torch.isfinite(J) & ((st & diff._BAD_STATUS) == 0), J, torch.full_like(J, float("inf")))
        return qt, qdt, ua, torch.cat([qt, qdt], dim=-1), J, al

    if search == "device":
        qt, qdt, ubar, xbar, Jbar, _ = searched(u0.detach().contiguous(), None, None, None, (), None)
    else:
        qt, qdt, ubar, xbar, Jbar = launch(u0.detach(), None, None)
    if not torch.isfinite(Jbar).all():
        raise RuntimeError("solve: the rollout under u0 failed")
    history = [Jbar]
    alpha = torch.zeros(B, dtype=torch.float64, device=u0.device)

    def quadratic_model():                                             # (lx, lu, Q) of the cost at the nominal
        if has_model:
            return cost.model(xbar, ubar)
        return cost.gradients(xbar, ubar) + (cost.Q,)

    for _ in range(int(iters)):
        if backward == "device":
            # the last launch held the accepted trajectories only (points 2 and 4): its open-loop tape under ubar IS the nominal's
            if sim.tape_count != tape[0]:
                raise RuntimeError("the tape of this rollout has been replaced")
            lx, lu, Qk = quadratic_model()
            if ulim is not None:
                kff, Kabi, _, st, _ = diff.lqr_backward_box(sim, lx, lu, Qk, cost.R, ubar, ulim, mu)
                notpd = st != 0
            else:
                kff, Kabi, _, notpd = diff.lqr_backward(sim, lx, lu, Qk, cost.R, mu)
        else:
            _, _, A, Bm = diff.linearize(sim, q0, qdot0, ubar, **{k: v for k, v in kw.items() if k not in ("integrator", "ulim")})
            lx, lu, Qk = quadratic_model()
            kff, K, _ = backward_pass(A, Bm, lx, lu, Qk, cost.R, mu)
            Kabi = K.transpose(-1, -2).contiguous()
            notpd = None
        xref = torch.cat([x0, xbar[:, :-1]], dim=1).contiguous()      # the nominal state at the START of every step
        if search == "device":
            # a flagged rollout has zero gains: nothing can beat -inf, so it ends on its nominal pass (which reproduces xbar)
            bar = Jbar if notpd is None else torch.where(notpd, torch.full_like(Jbar, float("-inf")), Jbar)
            qt, qdt, ubar, xbar, Jbar, alpha = searched(ubar, kff, Kabi, xref, alphas, bar)
            history.append(Jbar)
            continue
        alpha = torch.zeros(B, dtype=torch.float64, device=u0.device)
        accepted = torch.zeros(B, dtype=torch.bool, device=u0.device)
        clean = False                                                  # does the last launch hold accepted trajectories only?
        for al in alphas:
            trial = torch.where(accepted, alpha, torch.full_like(alpha, float(al)))
            out = launch(ubar + trial[:, None, None] * kff, Kabi, xref)
            better = ~accepted & (out[4] < Jbar)
            if notpd is not None:
                better = better & ~notpd                               # (zero gains: no step to take)
            alpha = torch.where(better, trial, alpha)
            accepted = accepted | better
            clean = bool(accepted.all())
            if clean:
                break
        if not clean:
            out = launch(ubar + alpha[:, None, None] * kff, Kabi, xref)
        qt, qdt, ubar, xbar, Jbar = out
        history.append(Jbar)
    return Result(ubar, qt, qdt, Jbar, alpha), torch.stack(history)
