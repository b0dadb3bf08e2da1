// C shim around rmx_select::select_rollout_lqr for tests/test_lqr_plan.py: the header compiles with plain g++.
#include "rmx_select.h"

extern "C" int lp_select(int NP, int n, int big, int nr, int* block, unsigned long long* lds_bytes) {
    rmx_select::StepTraits t;
    t.NP = NP;
    t.n = n;
    t.big = big != 0;
    const rmx_select::LqrPlan p = rmx_select::select_rollout_lqr(t, nr);
    *block = p.block;
    *lds_bytes = (unsigned long long)p.lds_bytes;
    return (int)p.kernel;
}
extern "C" int lp_max_nr() { return rmx_select::LQR_MAX_NR; }
