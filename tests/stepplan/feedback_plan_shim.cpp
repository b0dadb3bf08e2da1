// C shim around rmx_select::select_rollout_feedback for tests/test_feedback_plan.py: the header compiles with plain g++.
#include "rmx_select.h"

extern "C" const char* fp_select(int NP, int n, int is_chain, int adj_help_max_batch, int B, int integ, int adj_help, int* kernel, int* fullchain) {
    rmx_select::StepTraits t;
    t.NP = NP;
    t.n = n;
    t.is_chain = is_chain != 0;
    t.adj_help_max_batch = adj_help_max_batch;
    rmx_select::StepKnobs k;
    k.adj_help = adj_help != 0;
    const rmx_select::AdjPlan p = rmx_select::select_rollout_feedback(t, B, integ, k);
    *kernel = (int)p.kernel;
    *fullchain = p.fullchain ? 1 : 0;
    return rmx_select::label_rollout_feedback(integ);
}
// what the open-loop taped rollout runs for the same model and batch (the plan the feedback call must NOT follow)
extern "C" int fp_select_tape(int NP, int n, int is_chain, int adj_help_max_batch, int B, int integ, int adj_help) {
    rmx_select::StepTraits t;
    t.NP = NP;
    t.n = n;
    t.is_chain = is_chain != 0;
    t.adj_help_max_batch = adj_help_max_batch;
    rmx_select::StepKnobs k;
    k.adj_help = adj_help != 0;
    return (int)rmx_select::select_rollout_tape(t, B, integ, k).kernel;
}
