// rmx_lqr.h -- rmx_rollout_lqr (include/redmax_hip.h): the Riccati sweep of iLQR over the BDF1 tape, the recursion of
// redmax_amd.ilqr.backward_pass.  Included and instantiated from part_plain.hip alone, for the padded sizes NP <= 32.
//
// One workgroup of LQR_THREADS threads (four wavefronts) per rollout; the step index runs N .. 1 inside the kernel, and Vx, Vxx and
// every temporary of a step live in LDS, in reduced-DOF order and size (d = nr, not n).
//
// A step.  Wavefront 0 eliminates [H | M | -h D | h^2 pscale I] of slot k-1 with lin_eliminate of rmx_linearize.h as it stands (the
// same loads, the same pivot rule, the same operation order) and stores XB, XA, XU through the node-to-DOF map of lin_store into LDS:
// S = XA + XB, XB and XU are rmx_rollout_linearize's bits.  The other wavefronts wait at the barrier behind it: the elimination is
// NOT run ahead of the Riccati algebra here (it does not depend on it, so a double-buffered hand-over could overlap the two).
// Then, with X = XB, U = XU, Z = (S - I)/h - formed once, by the division the torch assembly uses, so that A_k and B_k
//     A = [ S  hX ]      B = [ U   ]
//         [ Z   X ]          [ U/h ]
// have the blocks diff.linearize assembles - and Vxx = [Vqq Vqv; Vqv' Vvv] (the two diagonal blocks are kept symmetric, the lower
// left block is never stored), Vx = (p, r):
//     W    = Vqq + (Vqv + Vqv')/h + Vvv/h^2                   Quu0 = sym(R + U' W U)             Qu = lu + U'p + (U/h)'r
//     T    = Vxx A:   T11 = Vqq S + Vqv Z     T12 = h Vqq X + Vqv X     T21 = Vqv'S + Vvv Z     T22 = h Vqv'X + Vvv X
//     Qxx  = A' T:    11: S'T11 + Z'T21       12: S'T12 + Z'T22         22: h X'T12 + X'T22                (written over Vxx)
//     Qux  = B' T:    q: U'T11 + U'T21/h      v: U'T12 + U'T22/h        Qx = (S'p + Z'r, h X'p + X'r)
//     [k, K] = -(Quu0 + mu I)^-1 [Qu, Qux]    (LDL' without pivoting; a pivot that is not > 0 flags the rollout)
//     G = Quu0 K + Qux,  g = Quu0 k + Qu      Vxx <- Q_{k-1} + sym(Qxx + K'G + Qux'K)      Vx <- lx_{k-1} + Qx + K'g + Qux'k
// The form with Z was chosen over W-only products (Qxx = P'WP - ... + Vvv/h^2 with P = [S, hX]): there the Vvv/h^2 terms cancel
// against each other, an absolute error of eps |Vvv|/h^2 next to entries of size |Vqq|.  23 products of d x d blocks per step.
// Every product is scalar FMAs on LDS operands, a 2 x 2 register tile per thread; the leading dimension NP + 1 keeps the
// transposed reads (stride NP + 1 doubles = an odd number of 8-byte banks) free of bank conflicts.
//
// LDS budget, blocks of (NP + 1) * NP doubles (8448 bytes at NP = 32), 17 of them = 143 616 bytes of the CU's 163 840 at NP = 32:
//      0..2   Vqq, Vqv, Vvv      the Riccati state; Qxx is written over it once T is formed
//      3..6   S, X, U, Z         the slot's sensitivities (Z holds XA between the elimination and the first phase)
//      7..10  T11, T12, T21, T22 T11 and T12 first hold W and W U, and after Qxx and Qux are formed G (q and v halves)
//      11,12  Quxq, Quxv
//      13,14  Kq, Kv             the right-hand sides, solved in place
//      15,16  Quu0, LDL'(Quu0 + mu I)
// and 8 vectors of NP doubles behind them (p, r, the next p, r, Qu, k, Quu0 k, g).  Nothing is reused across steps but Vxx, Vx.
//
// BOX (k_rollout_lqr<NP, true>, rmx_rollout_lqr_box): the solve of a step becomes the box QP of control-limited DDP (Tassa, Mansard,
// Todorov 2014) over lo_k = ulo - ubar_k <= x <= hi_k = uhi - ubar_k - projected Newton steps, each one LDL' of Hq = Quu0 + mu I in
// which the rows and columns of the clamped set are the identity's (selects, no compaction), with an Armijo search along the projected
// arc - and the final solve for [k, K] is the unconstrained kernel's code on the matrix masked by the final set: k_c = x_c, K_c = 0.
// With an empty set every select is the identity, so infinite bounds return rmx_rollout_lqr's bits by construction.  The set is a
// 32-bit word every thread computes from the same LDS values (nr <= 32), so the loop's control flow is uniform without a broadcast.
// 8 more vectors of NP doubles (lo, hi, x, grad, the trial point, the direction, Hq y, the right-hand column): 16 in all, 147 712
// bytes at NP = 32 with the 17 blocks.  BOX = false compiles to the kernel as it was: every addition sits under if constexpr.
#pragma once
#include "rmx_linearize.h"      /* lin_load_*, lin_eliminate; rmx_host.h: LqrArgs */

constexpr int LQR_THREADS = 256;

// C = P + s1 op(A1) B1 + s2 op(A2) B2 over d x d blocks (column-major, leading dimension LD); P null: zero, A2 null: one product.
// op = transpose under T1 / T2.  C may be P.  2 x 2 outputs per thread, the two products in accumulators of their own.
template <int LD, bool T1, bool T2>
__device__ __forceinline__ void lqr_mm2(double* C, const double* P, const double* A1, const double* B1, const double s1,
                                        const double* A2, const double* B2, const double s2, const int d, const int tid) {
    const int dt = (d + 1) >> 1;
    for (int t = tid; t < dt * dt; t += LQR_THREADS) {
        const int tj = t / dt, ti = t - tj * dt;
        const int i0 = 2 * ti, j0 = 2 * tj;
        const int i1 = i0 + 1 < d ? i0 + 1 : i0, j1 = j0 + 1 < d ? j0 + 1 : j0;      // (an odd d: the last tile repeats its row / column)
        double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
#pragma unroll 4
        for (int k = 0; k < d; ++k) {      // (unrolled: the LDS reads of four iterations in flight ahead of their FMAs)
            const double x0 = T1 ? A1[i0 * LD + k] : A1[k * LD + i0], x1 = T1 ? A1[i1 * LD + k] : A1[k * LD + i1];
            const double y0 = B1[j0 * LD + k], y1 = B1[j1 * LD + k];
            a00 = fma(x0, y0, a00); a10 = fma(x1, y0, a10); a01 = fma(x0, y1, a01); a11 = fma(x1, y1, a11);
        }
        double c00 = s1 * a00, c10 = s1 * a10, c01 = s1 * a01, c11 = s1 * a11;
        if (A2) {
            double b00 = 0.0, b01 = 0.0, b10 = 0.0, b11 = 0.0;
#pragma unroll 4
            for (int k = 0; k < d; ++k) {
                const double x0 = T2 ? A2[i0 * LD + k] : A2[k * LD + i0], x1 = T2 ? A2[i1 * LD + k] : A2[k * LD + i1];
                const double y0 = B2[j0 * LD + k], y1 = B2[j1 * LD + k];
                b00 = fma(x0, y0, b00); b10 = fma(x1, y0, b10); b01 = fma(x0, y1, b01); b11 = fma(x1, y1, b11);
            }
            c00 = fma(s2, b00, c00); c10 = fma(s2, b10, c10); c01 = fma(s2, b01, c01); c11 = fma(s2, b11, c11);
        }
        if (P) {
            c00 += P[j0 * LD + i0]; c10 += P[j0 * LD + i1]; c01 += P[j1 * LD + i0]; c11 += P[j1 * LD + i1];
        }
        C[j0 * LD + i0] = c00;
        if (i1 != i0) C[j0 * LD + i1] = c10;
        if (j1 != j0) {
            C[j1 * LD + i0] = c01;
            if (i1 != i0) C[j1 * LD + i1] = c11;
        }
    }
}

// sum_i A(i, j) x_i + s B(i, j) y_i: column j of two blocks against two vectors
template <int LD>
__device__ __forceinline__ double lqr_col2(const double* A, const double* x, const double* B, const double* y, const int j, const int d) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < d; ++i) {
        a = fma(A[j * LD + i], x[i], a);
        b = fma(B[j * LD + i], y[i], b);
    }
    return a + b;
}

// row r of one result of the elimination to its place in an LDS block: entry (r, c) to blk[idx[c] * LD + idx[r]] (lin_store's map and product)
template <int NP, int LD>
__device__ __forceinline__ void lqr_store(double* __restrict__ blk, const double (&R)[NP], const double rinv, const int* __restrict__ idx,
                                          const int n, const int ir) {
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        if (c < n) {
            const int jc = idx[c];      // (wave-uniform)
            if (jc >= 0 && ir >= 0) blk[jc * LD + ir] = R[c] * rinv;
        }
    }
}

// ---- BOX (rmx_rollout_lqr_box): the pieces of the box QP of a step.  Hq = Quu0 + mu I is read off Quu0, never stored.
template <int LD>
__device__ __forceinline__ double lqr_hq(const double* Quu, const double mu, const int i, const int j) {
    const double v = Quu[j * LD + i];
    return i == j ? v + mu : v;
}
// val(y) = Qu'y + 1/2 y'Hq y, the same bits in every thread: Hq y row by row into hx, then one sum each
template <int LD>
__device__ __forceinline__ double lqr_box_val(const double* Quu, const double mu, const double* Qu, const double* y, double* hx, const int d,
                                              const int tid) {
    __syncthreads();      // (y is written; the last sum over hx is over)
    if (tid < d) {
        double t = 0.0;
        for (int j = 0; j < d; ++j) t = fma(lqr_hq<LD>(Quu, mu, tid, j), y[j], t);
        hx[tid] = t;
    }
    __syncthreads();
    double v = 0.0;
    for (int i = 0; i < d; ++i) v = fma(y[i], Qu[i] + 0.5 * hx[i], v);
    return v;
}
// Hq_fc x_c of row i: the columns of the set alone (a free row has no diagonal term in it)
template <int LD>
__device__ __forceinline__ double lqr_box_fc(const double* Quu, const double* x, const unsigned cset, const int i, const int d) {
    double t = 0.0;
    for (int j = 0; j < d; ++j)
        if ((cset >> j) & 1u) t = fma(Quu[j * LD + i], x[j], t);
    return t;
}
// Lc = Hq with every row and column of the set replaced by the identity's - selects, so that an empty set writes Hq's bits
template <int LD>
__device__ __forceinline__ void lqr_box_mask(double* Lc, const double* Quu, const double mu, const unsigned cset, const int d, const int tid) {
    for (int e = tid; e < d * d; e += LQR_THREADS) {
        const int j = e / d, i = e - j * d, o = j * LD + i;
        const bool m = (((cset >> i) | (cset >> j)) & 1u) != 0;
        const double v = Quu[o];
        Lc[o] = m ? (i == j ? 1.0 : 0.0) : (i == j ? v + mu : v);
    }
}

template <int NP, bool BOX = false>
__global__ void __launch_bounds__(LQR_THREADS) k_rollout_lqr(const DevModel M, const LqrArgs a) {
    constexpr int LD = NP + 1, BLK = LD * NP;
    extern __shared__ double lqr_lds[];
    double* const Vqq = lqr_lds;
    double* const Vqv = Vqq + BLK;
    double* const Vvv = Vqv + BLK;
    double* const Sb = Vvv + BLK;
    double* const Xb = Sb + BLK;
    double* const Ub = Xb + BLK;
    double* const Zb = Ub + BLK;
    double* const T11 = Zb + BLK;
    double* const T12 = T11 + BLK;
    double* const T21 = T12 + BLK;
    double* const T22 = T21 + BLK;
    double* const Quq = T22 + BLK;
    double* const Quv = Quq + BLK;
    double* const Kq = Quv + BLK;
    double* const Kv = Kq + BLK;
    double* const Quu = Kv + BLK;
    double* const Lc = Quu + BLK;
    double* const vp = Lc + BLK;
    double* const vr = vp + NP;
    double* const vpn = vr + NP;
    double* const vrn = vpn + NP;
    double* const vQu = vrn + NP;
    double* const vk = vQu + NP;
    double* const vqk = vk + NP;
    double* const vg = vqk + NP;
    // BOX: the vectors of the QP (lo_k, hi_k, the iterate, its gradient, the trial point, the direction, Hq y, the right-hand column)
    double* const blo = vg + NP;
    double* const bhi = blo + NP;
    double* const bx = bhi + NP;
    double* const bgrad = bx + NP;
    double* const bxt = bgrad + NP;
    double* const bs = bxt + NP;
    double* const bhx = bs + NP;
    double* const brhs = bhx + NP;

    const int tid = threadIdx.x, n = M.n, d = M.nr, traj = blockIdx.x, N = a.nsteps;
    const int d2 = 2 * d, dd = d * d;
    const double h = a.h, rh = 1.0 / h;
    const double mu = a.mu_b ? a.mu_b[traj] : a.mu;
    const size_t nn = (size_t)n * n;
    const double* Qt = a.Q + (size_t)traj * a.q_stride;      // [N][2d * 2d], column-major
    const double* lxb = a.lx + (size_t)traj * N * d2;
    const double* lub = a.lu + (size_t)traj * N * d;
    double* kffo = a.kff + (size_t)traj * N * d;
    double* Ko = a.K + (size_t)traj * N * d2 * d;

    // Vxx_N = Q_N, Vx_N = lx_N
    {
        const double* QN = Qt + (size_t)(N - 1) * d2 * d2;
        for (int e = tid; e < dd; e += LQR_THREADS) {
            const int j = e / d, i = e - j * d;
            Vqq[j * LD + i] = QN[(size_t)j * d2 + i];
            Vqv[j * LD + i] = QN[(size_t)(d + j) * d2 + i];
            Vvv[j * LD + i] = QN[(size_t)(d + j) * d2 + d + i];
        }
        if (tid < d) {
            vp[tid] = lxb[(size_t)(N - 1) * d2 + tid];
            vr[tid] = lxb[(size_t)(N - 1) * d2 + d + tid];
        }
    }
    double expected = 0.0;      // (thread 0's)
    bool bad = false;           // (uniform over the workgroup)
    bool slow = false;          // BOX: bad because a QP ran out of iterations or of line search (status 2), not because of a pivot

#pragma unroll 1
    for (int s = N - 1; s >= 0; --s) {
        // ---- the slot's sensitivities: wavefront 0, rmx_rollout_linearize's elimination
        if (tid < 64) {
            const int lane = tid;
            const size_t at = (size_t)traj * N + s;
            const double* Hj = a.Hs + at * nn;
            const double* Mj = a.Ms + at * nn;
            const double* Dj = a.Ds + at * nn;
            const bool dof = lane < n && M.idx[lane < n ? lane : 0] >= 0;
            double Hrow[NP], RB[NP], RA[NP], RU[NP], rinv = 0.0;
            lin_load_H<NP>(Hrow, Hj, n, lane);
            lin_load_block<NP>(RB, LIN_M, 0, Mj, Dj, n, lane, dof, h, a.pscale);
            lin_load_block<NP>(RA, LIN_D, 0, Mj, Dj, n, lane, dof, h, a.pscale);
            lin_load_block<NP>(RU, LIN_U, 0, Mj, Dj, n, lane, dof, h, a.pscale);
            int r = (lane < NP) ? -1 : (NP + 1);
            lin_eliminate<NP, NP, 3>(lane, Hrow, RB, RA, RU, true, true, true, r, rinv);
            const int ir = (r >= 0 && r < n) ? M.idx[r] : -1;
            lqr_store<NP, LD>(Xb, RB, rinv, M.idx, n, ir);
            lqr_store<NP, LD>(Zb, RA, rinv, M.idx, n, ir);      // (XA; Z from it below)
            lqr_store<NP, LD>(Ub, RU, rinv, M.idx, n, ir);
        }
        __syncthreads();
        // ---- S, Z, W (into T11)
        for (int e = tid; e < dd; e += LQR_THREADS) {
            const int j = e / d, i = e - j * d, o = j * LD + i;
            const double sv = Zb[o] + Xb[o];
            Sb[o] = sv;
            Zb[o] = (sv - (i == j ? 1.0 : 0.0)) / h;
            T11[o] = Vqq[o] + (Vqv[o] + Vqv[i * LD + j]) / h + Vvv[o] / h / h;
        }
        __syncthreads();
        lqr_mm2<LD, false, false>(T12, nullptr, T11, Ub, 1.0, nullptr, nullptr, 0.0, d, tid);      // W U
        __syncthreads();
        lqr_mm2<LD, true, false>(Quu, nullptr, Ub, T12, 1.0, nullptr, nullptr, 0.0, d, tid);       // U' W U
        // Qu, Qx: three wavefronts, one vector each
        if (tid < d) {
            double u1 = 0.0, u2 = 0.0;
            for (int i = 0; i < d; ++i) {
                u1 = fma(Ub[tid * LD + i], vp[i], u1);
                u2 = fma(Ub[tid * LD + i] / h, vr[i], u2);
            }
            vQu[tid] = lub[(size_t)s * d + tid] + (u1 + u2);
        } else if (tid >= 64 && tid < 64 + d) {
            vpn[tid - 64] = lqr_col2<LD>(Sb, vp, Zb, vr, tid - 64, d);
        } else if (tid >= 128 && tid < 128 + d) {
            const int j = tid - 128;
            double x1 = 0.0, x2 = 0.0;
            for (int i = 0; i < d; ++i) {
                x1 = fma(h * Xb[j * LD + i], vp[i], x1);
                x2 = fma(Xb[j * LD + i], vr[i], x2);
            }
            vrn[j] = x1 + x2;
        }
        __syncthreads();
        // Quu0 = sym(R + U'WU), and the matrix to factorise
        for (int e = tid; e < dd; e += LQR_THREADS) {
            const int j = e / d, i = e - j * d;
            if (i <= j) {
                const double v = 0.5 * ((a.R[(size_t)j * d + i] + Quu[j * LD + i]) + (a.R[(size_t)i * d + j] + Quu[i * LD + j]));
                Quu[j * LD + i] = v;
                Quu[i * LD + j] = v;
                Lc[j * LD + i] = Lc[i * LD + j] = (i == j) ? v + mu : v;
            }
        }
        // T = Vxx A (W and W U have been read: T11, T12 are free)
        lqr_mm2<LD, false, false>(T11, nullptr, Vqq, Sb, 1.0, Vqv, Zb, 1.0, d, tid);
        lqr_mm2<LD, false, false>(T12, nullptr, Vqq, Xb, h, Vqv, Xb, 1.0, d, tid);
        lqr_mm2<LD, true, false>(T21, nullptr, Vqv, Sb, 1.0, Vvv, Zb, 1.0, d, tid);
        lqr_mm2<LD, true, false>(T22, nullptr, Vqv, Xb, h, Vvv, Xb, 1.0, d, tid);
        __syncthreads();
        // Qxx = A'T over Vxx, Qux = B'T, and the right-hand sides -[Qu, Qux]
        lqr_mm2<LD, true, true>(Vqq, nullptr, Sb, T11, 1.0, Zb, T21, 1.0, d, tid);
        lqr_mm2<LD, true, true>(Vqv, nullptr, Sb, T12, 1.0, Zb, T22, 1.0, d, tid);
        lqr_mm2<LD, true, true>(Vvv, nullptr, Xb, T12, h, Xb, T22, 1.0, d, tid);
        lqr_mm2<LD, true, true>(Quq, nullptr, Ub, T11, 1.0, Ub, T21, rh, d, tid);
        lqr_mm2<LD, true, true>(Quv, nullptr, Ub, T12, 1.0, Ub, T22, rh, d, tid);
        __syncthreads();
        for (int e = tid; e < dd; e += LQR_THREADS) {
            const int j = e / d, i = e - j * d, o = j * LD + i;
            Kq[o] = -Quq[o];
            Kv[o] = -Quv[o];
        }
        if (tid < d) vk[tid] = -vQu[tid];
        unsigned cset = 0;      // BOX: the DOFs of this step that end on a bound (uniform over the workgroup)
        if constexpr (BOX) {
            // ---- the box QP  min Qu'x + 1/2 x'Hq x,  lo <= x <= hi,  Hq = Quu0 + mu I  (projected Newton; the header's algorithm).
            // Every decision is taken by every thread from the same LDS values: the control flow is uniform without a broadcast.
            const double inf = __builtin_huge_val();
            if (tid < d) {
                const double ub = a.ubar[((size_t)traj * N + s) * d + tid];
                const double lo = a.ulo ? a.ulo[tid] - ub : -inf, hi = a.uhi ? a.uhi[tid] - ub : inf;
                blo[tid] = lo;
                bhi[tid] = hi;
                bx[tid] = 0.0 < lo ? lo : (0.0 > hi ? hi : 0.0);
            }
            const unsigned all = d >= 32 ? 0xffffffffu : ((1u << d) - 1u);
            unsigned prev = 0;
            bool have_prev = false, full = false, done = false;
            for (int it = 0; it < a.max_iter; ++it) {
                __syncthreads();      // (x of the iteration before; the first time vQu, Quu, lo, hi, x)
                if (tid < d) {
                    double t = 0.0;
                    for (int j = 0; j < d; ++j) t = fma(lqr_hq<LD>(Quu, mu, tid, j), bx[j], t);
                    bgrad[tid] = vQu[tid] + t;
                }
                __syncthreads();
                cset = 0;
                for (int i = 0; i < d; ++i) {
                    const double xi = bx[i], gi = bgrad[i];
                    if ((xi == blo[i] && gi > 0.0) || (xi == bhi[i] && gi < 0.0)) cset |= 1u << i;
                }
                if ((have_prev && cset == prev && full) || cset == all) {
                    done = true;
                    break;
                }
                // Hq with the rows and columns of the set replaced by the identity's, and -(Qu_f + Hq_fc x_c) over zeros
                lqr_box_mask<LD>(Lc, Quu, mu, cset, d, tid);
                if (tid < d) brhs[tid] = ((cset >> tid) & 1u) ? 0.0 : -(vQu[tid] + lqr_box_fc<LD>(Quu, bx, cset, tid, d));
                // LDL' as below, one right-hand column: lane i of wavefront 0 holds its row of the forward substitution
                for (int k = 0; k < d; ++k) {
                    __syncthreads();
                    const double piv = Lc[k * LD + k];
                    if (!(piv > 0.0)) {
                        bad = true;
                        break;
                    }
                    const double rp = 1.0 / piv;
                    if (tid < 64) {
                        if (tid > k && tid < d) brhs[tid] = fma(-Lc[k * LD + tid], brhs[k] * rp, brhs[tid]);
                    } else if (tid >= 128) {
                        const int u = tid - 128, i = u & 31;
                        if (i > k && i < d) {
                            const double cik = Lc[k * LD + i];
                            for (int j = k + 1 + (u >> 5); j <= i; j += 4) Lc[j * LD + i] = fma(-cik, Lc[k * LD + j] * rp, Lc[j * LD + i]);
                        }
                    }
                }
                if (bad) break;
                __syncthreads();
                // z = y / d and x = L'^-1 z in the registers of wavefront 0 (lane r its row), then the direction s = xn - x
                if (tid < 64) {
                    const int r = tid < d ? tid : 0;
                    const double pr = Lc[r * LD + r];
                    double y = brhs[r] / pr;
                    for (int i = d - 1; i > 0; --i) {
                        const double xi = __shfl(y, i);
                        if (tid < i) y = fma(-(Lc[r * LD + i] / pr), xi, y);
                    }
                    if (tid < d) bs[tid] = ((cset >> tid) & 1u) ? 0.0 : y - bx[tid];
                }
                __syncthreads();
                double sg = 0.0;
                for (int i = 0; i < d; ++i) sg = fma(bs[i], bgrad[i], sg);
                if (!(sg < 0.0)) {      // (x already minimises on this face)
                    done = true;
                    break;
                }
                const double vold = lqr_box_val<LD>(Quu, mu, vQu, bx, bhx, d, tid);
                double step = 1.0;
                for (;;) {      // Armijo on the projected arc
                    __syncthreads();      // (the trial point of the round before has been read)
                    if (tid < d) {
                        const double t = fma(step, bs[tid], bx[tid]);
                        bxt[tid] = t < blo[tid] ? blo[tid] : (t > bhi[tid] ? bhi[tid] : t);
                    }
                    const double vnew = lqr_box_val<LD>(Quu, mu, vQu, bxt, bhx, d, tid);
                    if (!((vnew - vold) / (step * sg) < 0.1)) break;
                    step *= 0.6;
                    if (step < 1e-20) {
                        bad = slow = true;
                        break;
                    }
                }
                if (bad) break;
                bool moved = false;
                for (int i = 0; i < d; ++i) moved = moved || bxt[i] != fma(step, bs[i], bx[i]);
                full = step == 1.0 && !moved;
                __syncthreads();
                if (tid < d) bx[tid] = bxt[tid];
                prev = cset;
                have_prev = true;
            }
            if (!done && !bad) bad = slow = true;      // (the cap on the iterations)
            if (bad) break;
            // the final solve is the code below on the masked matrix: k_c = x_c and K_c = 0 are written behind it, and with an empty
            // set every select here is the identity - rmx_rollout_lqr's bits
            __syncthreads();
            lqr_box_mask<LD>(Lc, Quu, mu, cset, d, tid);
            if (cset) {
                for (int e = tid; e < dd; e += LQR_THREADS) {
                    const int j = e / d, i = e - j * d, o = j * LD + i;
                    if ((cset >> i) & 1u) {
                        Kq[o] = 0.0;
                        Kv[o] = 0.0;
                    }
                }
                if (tid < d) vk[tid] = ((cset >> tid) & 1u) ? 0.0 : -(vQu[tid] + lqr_box_fc<LD>(Quu, bx, cset, tid, d));
            }
        }
        // ---- LDL' of Quu0 + mu I without pivoting, in the lower triangle of Lc: column k keeps L(i, k) d_k below its pivot d_k.
        // The forward substitution rides along: wavefronts 0 and 1 hold one right-hand column per thread (2d + 1 of them, the same
        // thread from here to the end of the solve, so the columns need no barrier of their own), wavefronts 2 and 3 update the
        // trailing block - thread u its row u & 31, every fourth column.
        double* const col = tid < d ? Kq + tid * LD : (tid < d2 ? Kv + (tid - d) * LD : vk);
        for (int k = 0; k < d; ++k) {
            __syncthreads();
            const double piv = Lc[k * LD + k];
            if (!(piv > 0.0)) {
                bad = true;
                break;
            }
            const double rp = 1.0 / piv;
            if (tid < 128) {
                if (tid <= d2) {
                    const double yk = col[k] * rp;
                    for (int i = k + 1; i < d; ++i) col[i] = fma(-Lc[k * LD + i], yk, col[i]);
                }
            } else {
                const int u = tid - 128, i = u & 31;
                if (i > k && i < d) {
                    const double cik = Lc[k * LD + i];
                    for (int j = k + 1 + (u >> 5); j <= i; j += 4) Lc[j * LD + i] = fma(-cik, Lc[k * LD + j] * rp, Lc[j * LD + i]);
                }
            }
        }
        if (bad) break;
        __syncthreads();
        // unit L below the diagonal (the pivots stay on it)
        for (int e = tid; e < dd; e += LQR_THREADS) {
            const int k = e / d, i = e - k * d;
            if (i > k) Lc[k * LD + i] = Lc[k * LD + i] / Lc[k * LD + k];
        }
        __syncthreads();
        // z = y / d, then x = L'^-1 z column by column: x_i is final once the rows above it have taken their multiples of it
        if (tid <= d2) {
            for (int i = 0; i < d; ++i) col[i] = col[i] / Lc[i * LD + i];
            for (int i = d - 1; i > 0; --i) {
                const double xi = col[i];
                for (int r = 0; r < i; ++r) col[r] = fma(-Lc[r * LD + i], xi, col[r]);
            }
        }
        __syncthreads();
        if constexpr (BOX) {      // k_c = x_c (lo or hi exactly), K_c = 0, k_f into the box; the mask of the step leaves
            if (cset) {
                for (int e = tid; e < dd; e += LQR_THREADS) {
                    const int j = e / d, i = e - j * d, o = j * LD + i;
                    if ((cset >> i) & 1u) {
                        Kq[o] = 0.0;
                        Kv[o] = 0.0;
                    }
                }
            }
            if (tid < d) {
                const double v = vk[tid];
                vk[tid] = ((cset >> tid) & 1u) ? bx[tid] : (v < blo[tid] ? blo[tid] : (v > bhi[tid] ? bhi[tid] : v));
            }
            if (tid == 0 && a.clamped) a.clamped[(size_t)traj * N + s] = cset;
            __syncthreads();
        }
        // G = Quu0 K + Qux (over T11, T12), Quu0 k and g = Quu0 k + Qu; the gains leave
        lqr_mm2<LD, false, false>(T11, Quq, Quu, Kq, 1.0, nullptr, nullptr, 0.0, d, tid);
        lqr_mm2<LD, false, false>(T12, Quv, Quu, Kv, 1.0, nullptr, nullptr, 0.0, d, tid);
        if (tid < d) {
            double q = 0.0;
            for (int j = 0; j < d; ++j) q = fma(Quu[j * LD + tid], vk[j], q);
            vqk[tid] = q;
            vg[tid] = q + vQu[tid];
            kffo[(size_t)s * d + tid] = vk[tid];
        }
        {
            double* Ks = Ko + (size_t)s * d2 * d;
            for (int e = tid; e < dd; e += LQR_THREADS) {
                const int j = e / d, i = e - j * d;
                Ks[(size_t)j * d + i] = Kq[j * LD + i];
                Ks[(size_t)(d + j) * d + i] = Kv[j * LD + i];
            }
        }
        __syncthreads();
        // Vxx = Qxx + K'G + Qux'K, Vx = Qx + K'g + Qux'k, expected
        lqr_mm2<LD, true, true>(Vqq, Vqq, Kq, T11, 1.0, Quq, Kq, 1.0, d, tid);
        lqr_mm2<LD, true, true>(Vqv, Vqv, Kq, T12, 1.0, Quq, Kv, 1.0, d, tid);
        lqr_mm2<LD, true, true>(Vvv, Vvv, Kv, T12, 1.0, Quv, Kv, 1.0, d, tid);
        if (tid < d) {
            vpn[tid] += lqr_col2<LD>(Kq, vg, Quq, vk, tid, d);
        } else if (tid >= 64 && tid < 64 + d) {
            vrn[tid - 64] += lqr_col2<LD>(Kv, vg, Quv, vk, tid - 64, d);
        }
        if (tid == 0) {
            double e1 = 0.0, e2 = 0.0;
            for (int i = 0; i < d; ++i) {
                e1 = fma(vQu[i], vk[i], e1);
                e2 = fma(vk[i], vqk[i], e2);
            }
            expected -= e1 + 0.5 * e2;
        }
        __syncthreads();
        // the diagonal blocks symmetric, then the cost of the state before this step (none for the fixed x_0)
        {
            const double* Qp = s > 0 ? Qt + (size_t)(s - 1) * d2 * d2 : nullptr;
            for (int e = tid; e < dd; e += LQR_THREADS) {
                const int j = e / d, i = e - j * d;
                if (Qp) Vqv[j * LD + i] += Qp[(size_t)(d + j) * d2 + i];
                if (i <= j) {
                    double v = 0.5 * (Vqq[j * LD + i] + Vqq[i * LD + j]);
                    double w = 0.5 * (Vvv[j * LD + i] + Vvv[i * LD + j]);
                    Vqq[j * LD + i] = Qp ? v + Qp[(size_t)j * d2 + i] : v;
                    Vqq[i * LD + j] = Qp ? v + Qp[(size_t)i * d2 + j] : v;
                    Vvv[j * LD + i] = Qp ? w + Qp[(size_t)(d + j) * d2 + d + i] : w;
                    Vvv[i * LD + j] = Qp ? w + Qp[(size_t)(d + i) * d2 + d + j] : w;
                }
            }
            if (tid < d) {
                vp[tid] = s > 0 ? vpn[tid] + lxb[(size_t)(s - 1) * d2 + tid] : vpn[tid];
                vr[tid] = s > 0 ? vrn[tid] + lxb[(size_t)(s - 1) * d2 + d + tid] : vrn[tid];
            }
        }
        // (the next step's elimination writes X, Z, U alone; the barrier behind it orders the rest)
    }
    if (bad) {      // not positive definite: the rollout takes no step - every row zero, the rows of later steps included
        for (size_t e = tid; e < (size_t)N * d; e += LQR_THREADS) kffo[e] = 0.0;
        for (size_t e = tid; e < (size_t)N * d2 * d; e += LQR_THREADS) Ko[e] = 0.0;
        if constexpr (BOX) {
            if (a.clamped)
                for (int e = tid; e < N; e += LQR_THREADS) a.clamped[(size_t)traj * N + e] = 0u;
        }
    }
    if (tid == 0) {
        if (a.expected) a.expected[traj] = bad ? 0.0 : expected;
        if constexpr (BOX) {
            if (a.status) a.status[traj] = bad ? (slow ? 2 : 1) : 0;
        } else {
            if (a.status) a.status[traj] = bad ? 1 : 0;
        }
    }
}
