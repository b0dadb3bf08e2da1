"""The box-constrained Riccati sweep of rmx_rollout_lqr_box (include/redmax_hip.h) in numpy: the definition the kernel is checked
against.  Control-limited DDP (Tassa, Mansard, Todorov 2014): at every step the feed-forward term solves

    min  g'x + 1/2 x'H x      lo <= x <= hi          (H = Quu0 + mu I, g = Qu, lo = ulo - ubar_k, hi = uhi - ubar_k)

by projected Newton steps with an Armijo search along the projected arc (``box_qp``), the feedback rows of the torques on a bound
are zero, and the value recursion keeps proto_lqr_backward's formulas with the constrained k, K.  ``dtype``: longdouble (the
reference) or float64 (the reference's own float64 evaluation, whose error sets the bound of the GPU test).
"""
import numpy as np

import proto_lqr_backward as P

LD = P.LD
ARMIJO, SHRINK, MIN_STEP, MAX_ITER = 0.1, 0.6, 1e-20, 64      # the published constants of the box-QP; the default cap


def _ldl_solve(A, rhs, dtype):
    """proto_lqr_backward.ldl_solve in ``dtype``: (x, ok), LDL' without pivoting, ok False where a pivot is not > 0."""
    A = np.array(A, dtype=dtype)
    x = np.array(rhs, dtype=dtype)
    n = A.shape[0]
    for k in range(n):
        piv = A[k, k]
        if not piv > 0:
            return None, False
        for j in range(k + 1, n):
            A[j:, j] -= A[j:, k] * (A[j, k] / piv)
    for i in range(n):
        x[i] = (x[i] - A[i, :i] @ x[:i]) / A[i, i]
    for i in range(n - 2, -1, -1):
        x[i] = x[i] - (A[i + 1:, i] @ x[i + 1:]) / A[i, i]
    return x, True


def box_qp(H, g, lo, hi, max_iter=MAX_ITER, dtype=LD):
    """(x, c, status, iters): the minimiser, the clamped set (bool [d]), 0 / 1 (a pivot of a free block not > 0) / 2 (the cap on the
    iterations was reached or the line search ran out), and the iterations used.  A bound at +-inf never counts as reached."""
    H, g, lo, hi = (np.asarray(a, dtype=dtype) for a in (H, g, lo, hi))
    d = g.shape[0]
    clamp = lambda y: np.minimum(np.maximum(y, lo), hi)      # noqa: E731
    val = lambda y: g @ y + (y @ (H @ y)) / 2                 # noqa: E731
    x = clamp(np.zeros(d, dtype=dtype))
    full, prev = False, None
    c = np.zeros(d, dtype=bool)
    for it in range(1, max_iter + 1):
        grad = g + H @ x
        c = ((x == lo) & (grad > 0)) | ((x == hi) & (grad < 0))
        f = ~c
        if prev is not None and (c == prev).all() and full:
            return x, c, 0, it
        if c.all():
            return x, c, 0, it
        sol, ok = _ldl_solve(H[np.ix_(f, f)], -(g[f] + H[np.ix_(f, c)] @ x[c]), dtype)
        if not ok:
            return x, c, 1, it
        xn = x.copy()
        xn[f] = sol
        s = xn - x
        sg = s @ grad
        if not sg < 0:
            return x, c, 0, it
        step, vold = dtype(1), val(x)
        while (val(clamp(x + step * s)) - vold) / (step * sg) < ARMIJO:
            step = step * dtype(SHRINK)
            if step < MIN_STEP:
                return x, c, 2, it
        trial = x + step * s
        xt = clamp(trial)
        full = bool(step == 1 and (xt == trial).all())
        x, prev = xt, c
    return x, c, 2, max_iter


def box_step(H, Qu, Qux, lo, hi, max_iter=MAX_ITER, dtype=LD):
    """(k, K, c, status, iters) of one step: the outputs depend on the final set c alone - k_c = x_c, K_c = 0,
    [k_f, K_f] = -H_ff^-1 [Qu_f + H_fc k_c, Qux_f] by one final solve, k_f then clamped into the box."""
    H, Qu, Qux, lo, hi = (np.asarray(a, dtype=dtype) for a in (H, Qu, Qux, lo, hi))
    d, nx = Qux.shape
    x, c, status, iters = box_qp(H, Qu, lo, hi, max_iter, dtype)
    if status:
        return None, None, c, status, iters
    f = ~c
    k, K = np.zeros(d, dtype=dtype), np.zeros((d, nx), dtype=dtype)
    k[c] = x[c]
    if f.any():
        sol, ok = _ldl_solve(H[np.ix_(f, f)], np.concatenate([(Qu[f] + H[np.ix_(f, c)] @ k[c])[:, None], Qux[f]], axis=1), dtype)
        if not ok:
            return None, None, c, 1, iters
        k[f] = np.minimum(np.maximum(-sol[:, 0], lo[f]), hi[f])
        K[f] = -sol[:, 1:]
    return k, K, c, 0, iters


def backward_pass_box(A, Bm, lx, lu, Q, R, ubar, ulo=None, uhi=None, mu=0.0, max_iter=MAX_ITER, dtype=LD):
    """One rollout, proto_lqr_backward.backward_pass_ext's arguments and ubar [N][nr], ulo, uhi [nr] or None.  Returns a dict: kff
    [N][nr], K [N][nr][2nr], expected, status, clamped [N] (bit i: DOF i on a bound), and per step the set ``c`` [N][nr], the
    iterations ``iters`` [N], ``Qu`` [N][nr] and ``H`` [N][nr][nr] (for the KKT margins).  A flagged rollout: zeros, expected 0."""
    A, Bm, lx, lu, Q, R, ubar = (np.asarray(a, dtype=dtype) for a in (A, Bm, lx, lu, Q, R, ubar))
    N, nx, nu = Bm.shape
    ulo = np.full(nu, -np.inf, dtype=dtype) if ulo is None else np.asarray(ulo, dtype=dtype)
    uhi = np.full(nu, np.inf, dtype=dtype) if uhi is None else np.asarray(uhi, dtype=dtype)
    out = dict(kff=np.zeros((N, nu), dtype=dtype), K=np.zeros((N, nu, nx), dtype=dtype), expected=dtype(0), status=0,
               clamped=np.zeros(N, dtype=np.uint32), c=np.zeros((N, nu), dtype=bool), iters=np.zeros(N, dtype=int),
               Qu=np.zeros((N, nu), dtype=dtype), H=np.zeros((N, nu, nu), dtype=dtype))
    Vx, Vxx = lx[N - 1], Q[N - 1]
    for s in range(N - 1, -1, -1):
        Ak, Bk = A[s], Bm[s]
        Qx, Qu = Ak.T @ Vx, lu[s] + Bk.T @ Vx
        Qxx, Qux = Ak.T @ Vxx @ Ak, Bk.T @ Vxx @ Ak
        Quu0 = R + Bk.T @ Vxx @ Bk
        Quu0 = (Quu0 + Quu0.T) / 2
        H = Quu0 + dtype(mu) * np.eye(nu, dtype=dtype)
        ks, Ks, c, status, iters = box_step(H, Qu, Qux, ulo - ubar[s], uhi - ubar[s], max_iter, dtype)
        out["iters"][s] = iters
        if status:
            for name in ("kff", "K", "clamped", "c"):
                out[name][...] = 0
            out["expected"], out["status"] = dtype(0), status
            return out
        out["kff"][s], out["K"][s], out["c"][s], out["Qu"][s], out["H"][s] = ks, Ks, c, Qu, H
        out["clamped"][s] = sum(1 << i for i in range(nu) if c[i])
        out["expected"] = out["expected"] - (Qu @ ks + (ks @ (Quu0 @ ks)) / 2)
        Vx = Qx + Ks.T @ (Quu0 @ ks) + Ks.T @ Qu + Qux.T @ ks
        Vxx = Qxx + Ks.T @ Quu0 @ Ks + Ks.T @ Qux + Qux.T @ Ks
        Vxx = (Vxx + Vxx.T) / 2
        if s > 0:
            Vx, Vxx = Vx + lx[s - 1], Vxx + Q[s - 1]
    return out


def margins(res, ubar, ulo, uhi):
    """The strict-complementarity margins of a (longdouble) result, the precondition of the GPU test: the smallest clamped multiplier
    |grad_i| and the smallest distance of a free DOF to its finite bounds, each relative to its scale (max |Qu| of the step; the
    range of the box or, one-sided, max |kff| of the step), over all steps.  Returns (multiplier, distance); inf where none occurs."""
    ubar = np.asarray(ubar, dtype=LD)
    N, nu = res["kff"].shape
    ulo = np.full(nu, -np.inf) if ulo is None else np.asarray(ulo, dtype=LD)
    uhi = np.full(nu, np.inf) if uhi is None else np.asarray(uhi, dtype=LD)
    mult, dist = np.inf, np.inf
    for s in range(N):
        k, c = res["kff"][s], res["c"][s]
        grad = res["Qu"][s] + res["H"][s] @ k
        gs = max(float(np.abs(res["Qu"][s]).max()), 1e-300)
        for i in range(nu):
            lo, hi = ulo[i] - ubar[s, i], uhi[i] - ubar[s, i]
            if c[i]:
                mult = min(mult, float(abs(grad[i])) / gs)
            else:
                scale = float(hi - lo) if np.isfinite(lo) and np.isfinite(hi) else max(float(np.abs(k).max()), 1e-300)
                for bnd in (lo, hi):
                    if np.isfinite(bnd):
                        dist = min(dist, float(abs(k[i] - bnd)) / scale)
    return mult, dist
