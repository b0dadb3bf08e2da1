// rmx_tape.h -- the arithmetic the taped-rollout family shares (rmx_rollout_tape*, _vjp*, _linearize, _jvp in redmax_hip.hip):
// where every part of a tape lies in the adjoint workspace, and where the arrays of a host form lie in their staging room.
// Pure host C++17, no HIP header: tests/test_tape_layout.py compiles it with g++ (tests/tapeplan/tape_layout_shim.cpp).
#pragma once
#include <cstddef>

namespace rmx_tape {

// every part of the workspace and every staged array starts at a 256-byte boundary
constexpr size_t round256(const size_t x) { return (x + 255) & ~(size_t)255; }

// The workspace of a tape, in the order of its parts.  H, M, D first, where every adjoint call has them; behind them the staging
// areas of the host forms - three arrays shaped as u (u, qtraj, qdtraj of the tape; gq, gqd, du of the vjp) and two of [B][nr]
// (dq0, dqd0).  The tape call reserves all of it, so that a vjp never regrows (and so loses) the tape.
// A BDF2 tape has nsteps + 1 slots per rollout: the last one holds the SDIRK2a solve.
// Behind those, what rmx_rollout_vjp_params needs: the states the tape differentiates at - q0, qdot0 ([B][nr] each) and the recorded
// trajectory (two arrays shaped as u), (2 nsteps + 2) nr doubles per rollout, kept as long as the tape (no vjp stages over them) -,
// z of every slot ([B][nslots][n], written by the ADJ_ZS backward kernels) and the staging of the five gradient arrays.
struct Layout {
    int nslots;                      // taped solves per rollout
    size_t H, M, D;                  // [B][nslots][n*n] each
    size_t stage_traj[3];            // staging shaped as u, [B][nsteps][nr]
    size_t stage_state[2];           // staging shaped as the state, [B][nr]
    size_t Q0, QD0;                  // [B][nr] the state the tape started from
    size_t QT, QDT;                  // [B][nsteps][nr] the recorded trajectory
    size_t ZS;                       // [B][nslots][n]
    size_t PG;                           // the staging of the parameter gradients:
    size_t pg_off[5], pg_bytes[5];       // stiffness, damping, qrest, inertia, grav inside part PG
    size_t bytes_hist, bytes_traj, bytes_state, bytes_zs, bytes_pg, total;
};
inline Layout layout(const int B, const int nsteps, const int integ /* 1: BDF1, 2: BDF2 */, const int n, const int nr, const int nlist) {
    Layout t{};
    t.nslots = nsteps + (integ == 2 ? 1 : 0);
    t.bytes_hist = (size_t)B * t.nslots * n * n * sizeof(double);
    t.bytes_traj = (size_t)B * nsteps * nr * sizeof(double);
    t.bytes_state = (size_t)B * nr * sizeof(double);
    t.bytes_zs = (size_t)B * t.nslots * n * sizeof(double);
    const size_t pg[5] = {t.bytes_state, t.bytes_state, t.bytes_state, (size_t)B * nlist * 6 * sizeof(double), (size_t)B * 3 * sizeof(double)};
    for (int i = 0; i < 5; ++i) {
        t.pg_off[i] = t.bytes_pg;
        t.pg_bytes[i] = pg[i];
        t.bytes_pg += round256(pg[i]);
    }
    auto part = [&t](const size_t bytes) {
        const size_t at = t.total;
        t.total += round256(bytes);
        return at;
    };
    t.H = part(t.bytes_hist); t.M = part(t.bytes_hist); t.D = part(t.bytes_hist);
    for (size_t& s : t.stage_traj) s = part(t.bytes_traj);
    for (size_t& s : t.stage_state) s = part(t.bytes_state);
    t.Q0 = part(t.bytes_state); t.QD0 = part(t.bytes_state);
    t.QT = part(t.bytes_traj); t.QDT = part(t.bytes_traj);
    t.ZS = part(t.bytes_zs);
    t.PG = part(t.bytes_pg);
    return t;
}

// The staging room of a host form: its arrays in the order they are added, each present one at a 256-byte boundary; an absent
// (null) array takes no room.
constexpr int STAGE_MAX = 24;      // (rmx_rollout_search stages 17: gains, limits, direction, cost tables, outputs)
struct StagePlan {
    int n = 0;
    size_t off[STAGE_MAX] = {}, bytes[STAGE_MAX] = {}, total = 0;
    bool present[STAGE_MAX] = {};
    int add(const size_t nbytes, const bool is_present) {
        off[n] = total;
        bytes[n] = nbytes;
        present[n] = is_present;
        if (is_present) total += round256(nbytes);
        return n++;
    }
};

}  // namespace rmx_tape
