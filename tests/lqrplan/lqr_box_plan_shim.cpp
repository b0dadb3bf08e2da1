// C shim around rmx_select::select_rollout_lqr_box for tests/test_lqr_box_plan.py: the header compiles with plain g++.
#include "rmx_select.h"

static rmx_select::StepTraits traits(int NP, int n, int big) {
    rmx_select::StepTraits t;
    t.NP = NP;
    t.n = n;
    t.big = big != 0;
    return t;
}
extern "C" int lbp_select(int NP, int n, int big, int nr, int* block, unsigned long long* lds_bytes) {
    const rmx_select::LqrPlan p = rmx_select::select_rollout_lqr_box(traits(NP, n, big), nr);
    *block = p.block;
    *lds_bytes = (unsigned long long)p.lds_bytes;
    return (int)p.kernel;
}
// the unconstrained sweep's plan for the same model: the refusals must coincide
extern "C" int lbp_select_plain(int NP, int n, int big, int nr, unsigned long long* lds_bytes) {
    const rmx_select::LqrPlan p = rmx_select::select_rollout_lqr(traits(NP, n, big), nr);
    *lds_bytes = (unsigned long long)p.lds_bytes;
    return (int)p.kernel;
}
extern "C" int lbp_vectors() { return rmx_select::LQR_BOX_VECTORS; }
extern "C" int lbp_default_max_iter() { return rmx_select::LQR_BOX_MAX_ITER; }
extern "C" const char* lbp_label() { return rmx_select::label_rollout_lqr_box(); }
extern "C" const char* lbp_label_feedback(int integ) { return rmx_select::label_rollout_feedback_box(integ); }
