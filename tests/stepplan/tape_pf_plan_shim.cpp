// C entry points around select_rollout_tape_pf (redmax_amd/csrc/rmx_select.h), for tests/test_tape_pf_plan.py: plain g++, no HIP.
#include "rmx_select.h"

using namespace rmx_select;

// the plan of a tape call on a model with point forces: the TapePfKernel as an int (0 Wave, 1 Refused); out = the padded size that
// runs, the feedback flag and the threads per workgroup; the label, or "" where the plan refuses
extern "C" const char* tp_select(int NP, int n, int is_chain, int pf, int big, int contact, int spherical, int adj_help_max_batch, int integ,
                                 int feedback, int* kernel, int* out) {
    StepTraits t;
    t.NP = NP;
    t.n = n;
    t.is_chain = is_chain != 0;
    t.point_forces = pf != 0;
    t.big = big != 0;
    t.contact = contact != 0;
    t.spherical = spherical != 0;
    t.adj_help_max_batch = adj_help_max_batch;
    const TapePfPlan p = select_rollout_tape_pf(t, integ, feedback != 0);
    *kernel = (int)p.kernel;
    out[0] = p.np;
    out[1] = p.feedback ? 1 : 0;
    out[2] = p.block;
    return p.label;
}
extern "C" const char* tp_label(int integ, int feedback) { return label_rollout_tape_pf(integ, feedback != 0); }
