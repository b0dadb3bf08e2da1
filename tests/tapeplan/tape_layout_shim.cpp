// C shim around rmx_tape.h for tests/test_tape_layout.py: the header compiles with plain g++.
#include "rmx_tape.h"

typedef unsigned long long u64;

// the 14 parts in the order of the workspace: offset and (unrounded) size of each; scal = {nslots, total}; pg = offset, size of the
// five parameter-gradient arrays inside part PG
extern "C" void tl_layout(int B, int nsteps, int integ, int n, int nr, int nlist, u64* off, u64* bytes, u64* scal, u64* pg_off, u64* pg_bytes) {
    const rmx_tape::Layout t = rmx_tape::layout(B, nsteps, integ, n, nr, nlist);
    const u64 o[14] = {t.H, t.M, t.D, t.stage_traj[0], t.stage_traj[1], t.stage_traj[2], t.stage_state[0], t.stage_state[1],
                       t.Q0, t.QD0, t.QT, t.QDT, t.ZS, t.PG};
    const u64 s[14] = {t.bytes_hist, t.bytes_hist, t.bytes_hist, t.bytes_traj, t.bytes_traj, t.bytes_traj, t.bytes_state, t.bytes_state,
                       t.bytes_state, t.bytes_state, t.bytes_traj, t.bytes_traj, t.bytes_zs, t.bytes_pg};
    for (int i = 0; i < 14; ++i) {
        off[i] = o[i];
        bytes[i] = s[i];
    }
    scal[0] = (u64)t.nslots;
    scal[1] = t.total;
    for (int i = 0; i < 5; ++i) {
        pg_off[i] = t.pg_off[i];
        pg_bytes[i] = t.pg_bytes[i];
    }
}

extern "C" u64 tl_round256(u64 x) { return rmx_tape::round256(x); }
extern "C" int tl_stage_max(void) { return rmx_tape::STAGE_MAX; }

// a staging plan of nitems (<= tl_stage_max()) arrays: the offset of each, and the room of the whole
extern "C" u64 tl_stage(int nitems, const u64* bytes, const int* present, u64* off) {
    rmx_tape::StagePlan p;
    for (int i = 0; i < nitems; ++i) p.add(bytes[i], present[i] != 0);
    for (int i = 0; i < nitems; ++i) off[i] = p.off[i];
    return p.total;
}
