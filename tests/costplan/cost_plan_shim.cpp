// C shim around rmx_select::select_rollout_cost for tests/test_cost_plan.py: the header compiles with plain g++.
#include "rmx_select.h"

extern "C" int cp_select(int NP, int n, int big, int spherical, int contact, int point_forces, int B, int nsteps, int* np, int* block,
                         unsigned long long* grid) {
    rmx_select::StepTraits t;
    t.NP = NP;
    t.n = n;
    t.big = big != 0;
    t.spherical = spherical != 0;
    t.contact = contact != 0;
    t.point_forces = point_forces != 0;
    const rmx_select::CostPlan p = rmx_select::select_rollout_cost(t, B, nsteps);
    *np = p.np;
    *block = p.block;
    *grid = (unsigned long long)p.grid;
    return (int)p.kernel;
}
extern "C" unsigned long long cp_max_grid() { return (unsigned long long)rmx_select::COST_MAX_GRID; }
