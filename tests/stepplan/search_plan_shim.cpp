// C entry points around select_rollout_search (redmax_amd/csrc/rmx_select.h), for tests/test_search_plan.py: plain g++, no HIP.
#include "rmx_select.h"

using namespace rmx_select;

// the plan of rmx_rollout_search for a model of padded size NP with n nodes and nr reduced DOFs: the SearchKernel as an int
// (0 Wave, 1 RefusedNr, 2 RefusedNodes), the padded size that runs and the threads per workgroup
extern "C" int sp_select(int NP, int n, int big, int nr, int* np, int* block) {
    StepTraits t;
    t.NP = NP;
    t.n = n;
    t.big = big != 0;
    const SearchPlan p = select_rollout_search(t, nr);
    *np = p.np;
    *block = p.block;
    return (int)p.kernel;
}
extern "C" const char* sp_label(void) { return label_rollout_search(); }
extern "C" int sp_max_alphas(void) { return SEARCH_MAX_ALPHAS; }
