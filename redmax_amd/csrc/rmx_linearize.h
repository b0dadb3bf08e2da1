// rmx_linearize.h -- rmx_rollout_linearize (include/redmax_hip.h): the forward sensitivities of every taped solve,
//     XA = dx/dqA = -eta H^-1 D      XB = dx/dqB = H^-1 M      XU = dx/du = eta^2 pscale H^-1
// from H, M, D of the slot.  Included and instantiated from part_plain.hip alone.
//
// One wavefront per (rollout, slot): unlike the two sweeps, whose steps follow one another, every slot of the tape is independent, so
// the grid is B * nslots.  Lane = node = row of [H | M | -eta D | eta^2 pscale I]; the rows are eliminated in place by Gauss-Jordan
// with partial pivoting: at pivot k every row but the pivot's takes its multiple of the pivot row, the rows that pivoted earlier
// included, so no back substitution is left and the lane that pivoted at step k holds row k of all three results (times the
// reciprocal of its pivot, applied once at the end).  The pivot rule is lu_solve_neg's (first maximum on the full double, the lowest
// lane among equals), the pivot row is broadcast with readlane_d from the wave-uniform pivot lane.  No DPP broadcast sequence.
// The pivot index is a template constant (lin_eliminate recurses over it) and every loop has constant bounds: no register array is
// indexed at run time.
//
// Registers.  Up to NP = 32 the four blocks are 4 NP doubles per lane (256 registers at NP = 32): one pass.  At NP = 64 they do not
// fit: the right-hand blocks are taken half a block per pass (H + 32 columns: 96 doubles; with a whole block the rows alone fill the
// 256 registers the vector ALU addresses and the compiler spills them), H reloaded from the tape and eliminated again each time with
// the same pivots - a run-time loop around ONE copy of the elimination.  A NULL output drops its block through a
// wave-uniform flag: the blocks never mix, so an output has the same bits whichever others are asked for.
#pragma once
#include "rmx_host.h"      /* LinArgs */

enum { LIN_M = 0, LIN_D = 1, LIN_U = 2 };

// this lane's row of NR columns (from column c0 on) of one right-hand block: M, -eta D (unconditional loads, index clamped: see
// adj_block; LIN_CHUNK of them in flight at a time, the registers of a whole block are not there to hold more) or eta^2 pscale I.
// Rows of nodes without a DOF and padding rows are zero: nothing of them reaches a result.
constexpr int LIN_CHUNK = 16;
template <int NR>
__device__ __forceinline__ void lin_load_block(double (&R)[NR], const int kind, const int c0, const double* __restrict__ Mj,
                                               const double* __restrict__ Dj, const int n, const int lane, const bool dof, const double eta,
                                               const double pscale) {
    if (kind == LIN_U) {
        const double d = eta * eta * pscale;
#pragma unroll
        for (int c = 0; c < NR; ++c) R[c] = (dof && c0 + c == lane) ? d : 0.0;
    } else {
        const double* src = (kind == LIN_M ? Mj : Dj) + (lane < n ? lane : 0);
        const double s = kind == LIN_M ? 1.0 : -eta;
        constexpr int CH = NR < LIN_CHUNK ? NR : LIN_CHUNK;
#pragma unroll
        for (int b = 0; b < NR; b += CH) {
            double v[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) v[c] = src[(size_t)(c0 + b + c < n ? c0 + b + c : 0) * n];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < CH; ++c) R[b + c] = (dof && c0 + b + c < n) ? s * v[c] : 0.0;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <int NP>
__device__ __forceinline__ void lin_load_H(double (&Hrow)[NP], const double* __restrict__ Hj, const int n, const int lane) {
    const double* src = Hj + (lane < n ? lane : 0);
    constexpr int CH = NP < LIN_CHUNK ? NP : LIN_CHUNK;
#pragma unroll
    for (int b = 0; b < NP; b += CH) {
        double v[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) v[c] = src[(size_t)(b + c < n ? b + c : 0) * n];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < CH; ++c) Hrow[b + c] = (b + c < n && lane < n) ? v[c] : ((b + c == lane) ? 1.0 : 0.0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// row -= l * (pivot row), one block: the broadcasts of a batch ahead of its FMAs, and the scheduler kept from pulling those of later
// batches forward (under max-ilp it hoists them all and spills the scalar registers they land in, 2655 of them at NP = 64)
template <int NR, int FIRST = 0>
__device__ __forceinline__ void lin_update(double (&R)[NR], const double l, const int pl) {
    constexpr int BT = 8;
#pragma unroll
    for (int c0 = FIRST; c0 < NR; c0 += BT) {
        double pv[BT];
#pragma unroll
        for (int i = 0; i < BT; ++i) pv[i] = (c0 + i < NR) ? readlane_d(R[c0 + i < NR ? c0 + i : NR - 1], pl) : 0.0;
#pragma unroll
        for (int i = 0; i < BT; ++i)
            if (c0 + i < NR) R[c0 + i] = fma(-l, pv[i], R[c0 + i]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Gauss-Jordan on [Hrow | R0 | R1 | R2] (NB of the blocks, each under its wave-uniform flag), pivots K .. NP-1: the pivot index is a
// template constant, so every register array is indexed by constants whatever the unroller's size limits decide.  pivstep: the
// pivot step of this lane's row (-1: none yet; lanes >= NP never pivot).  The row's results stay unscaled: row pivstep of H^-1 R is
// rinv_own * R.
template <int NP, int NR, int NB, int K = 0>
__device__ __forceinline__ void lin_eliminate(const int lane, double (&Hrow)[NP], double (&R0)[NR], double (&R1)[NR], double (&R2)[NR],
                                              const bool w0, const bool w1, const bool w2, int& pivstep, double& rinv_own) {
    if constexpr (K < NP) {
        const double rinv_mine = recip(Hrow[K]);
        // the pivot search of lu_solve_neg: high words of |H|, then the low words of the lanes that tie there, then the lowest lane
        const bool cand = pivstep < 0;
        const unsigned hiw = (unsigned)__double2hiint(Hrow[K]) & 0x7fffffffu, low = (unsigned)__double2loint(Hrow[K]);
        const unsigned k1 = cand ? (hiw | 0x80000000u) : 0u;
        const unsigned m1 = (NP <= 32) ? wave_umax32(k1) : wave_umax(k1);
        const bool t1 = cand && k1 == m1;
        const unsigned k2 = t1 ? low : 0u;
        const unsigned m2 = (NP <= 32) ? wave_umax32(k2) : wave_umax(k2);
        unsigned key = (t1 && low == m2) ? (64u - (unsigned)lane) : 0u;
        key = (NP <= 32) ? wave_umax32(key) : wave_umax(key);
        const int pl = (64 - (int)key) & 63;         // (wave-uniform; & 63: a lane index whatever the rows hold)
        const double rinv = readlane_d(rinv_mine, pl);
        if (lane == pl) {
            pivstep = K;
            rinv_own = rinv;
        }
        // every other row, the earlier pivot rows included (Gauss-Jordan); lanes >= NP hold zero rows
        const double l = (lane != pl) ? Hrow[K] * rinv : 0.0;
        lin_update<NP, K + 1>(Hrow, l, pl);
        if (w0) lin_update<NR>(R0, l, pl);
        if constexpr (NB > 1) {
            if (w1) lin_update<NR>(R1, l, pl);
            if (w2) lin_update<NR>(R2, l, pl);
        }
        lin_eliminate<NP, NR, NB, K + 1>(lane, Hrow, R0, R1, R2, w0, w1, w2, pivstep, rinv_own);
    }
}

// row r of one result, columns c0 .. c0 + NR - 1: entry (r, c) to out[idx[c] * nr + idx[r]]
template <int NR>
__device__ __forceinline__ void lin_store(double* __restrict__ out, const double (&R)[NR], const int c0, const double rinv,
                                          const int* __restrict__ idx, const int n, const int nr, const int ir) {
#pragma unroll
    for (int c = 0; c < NR; ++c) {
        if (c0 + c < n) {
            const int jc = idx[c0 + c];      // (wave-uniform)
            if (jc >= 0 && ir >= 0) out[(size_t)jc * nr + ir] = R[c] * rinv;
        }
    }
}

template <int NP>
__global__ void __launch_bounds__(64) k_rollout_linearize(const DevModel M, const LinArgs a) {
    const int lane = threadIdx.x, n = M.n, nr = M.nr;
    const int traj = blockIdx.x / a.nslots, slot = blockIdx.x - traj * a.nslots;
    const size_t nn = (size_t)n * n, at = (size_t)traj * a.nslots + slot;
    const double* Hj = a.Hs + at * nn;
    const double* Mj = a.Ms + at * nn;
    const double* Dj = a.Ds + at * nn;
    const size_t oo = at * (size_t)nr * nr;
    const bool dof = lane < n && M.idx[lane < n ? lane : 0] >= 0;
    // eta of the slot: h under BDF1; under BDF2 al h for the two SDIRK2 solves (slots 0 and nsteps), 2h/3 for the others
    const double al = (2.0 - sqrt(2.0)) / 2.0;
    const double eta = a.bdf2 ? ((slot == 0 || slot == a.nslots - 1) ? al * a.h : (2.0 / 3.0) * a.h) : a.h;
    double Hrow[NP], rinv;
    if constexpr (NP <= 32) {
        double RB[NP], RA[NP], RU[NP];
        const bool wB = a.XB != nullptr, wA = a.XA != nullptr, wU = a.XU != nullptr;
        lin_load_H<NP>(Hrow, Hj, n, lane);
        if (wB) lin_load_block<NP>(RB, LIN_M, 0, Mj, Dj, n, lane, dof, eta, a.pscale);
        if (wA) lin_load_block<NP>(RA, LIN_D, 0, Mj, Dj, n, lane, dof, eta, a.pscale);
        if (wU) lin_load_block<NP>(RU, LIN_U, 0, Mj, Dj, n, lane, dof, eta, a.pscale);
        int r = (lane < NP) ? -1 : (NP + 1);
        rinv = 0.0;
        lin_eliminate<NP, NP, 3>(lane, Hrow, RB, RA, RU, wB, wA, wU, r, rinv);
        const int ir = (r >= 0 && r < n) ? M.idx[r] : -1;
        if (wB) lin_store<NP>(a.XB + oo, RB, 0, rinv, M.idx, n, nr, ir);
        if (wA) lin_store<NP>(a.XA + oo, RA, 0, rinv, M.idx, n, nr, ir);
        if (wU) lin_store<NP>(a.XU + oo, RU, 0, rinv, M.idx, n, nr, ir);
    } else {
        // 33..64 nodes: H and HALF a right-hand block per pass (96 doubles per lane, inside the 256 registers the vector ALU addresses)
        constexpr int NR = NP / 2;
#pragma unroll 1
        for (int pass = 0; pass < 6; ++pass) {
            const int kind = pass >> 1, c0 = (pass & 1) * NR;
            double* out = kind == LIN_M ? a.XB : (kind == LIN_D ? a.XA : a.XU);
            if (!out) continue;
            double R[NR];
            lin_load_H<NP>(Hrow, Hj, n, lane);
            lin_load_block<NR>(R, kind, c0, Mj, Dj, n, lane, dof, eta, a.pscale);
            int r = (lane < NP) ? -1 : (NP + 1);
            rinv = 0.0;
            lin_eliminate<NP, NR, 1>(lane, Hrow, R, R, R, true, false, false, r, rinv);
            const int ir = (r >= 0 && r < n) ? M.idx[r] : -1;
            lin_store<NR>(out + oo, R, c0, rinv, M.idx, n, nr, ir);
        }
    }
}
