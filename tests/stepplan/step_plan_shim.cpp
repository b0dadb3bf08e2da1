// C entry points over redmax_amd/csrc/rmx_select.h for tests/test_step_plan.py (plain g++, no HIP).
#include "rmx_select.h"

using namespace rmx_select;

extern "C" {

// traits[14]: NP, n, big, point_forces, contact, spherical, is_chain, gconst, n_simd, coop_g, w2_max_batch, w2_min_batch,
// gconst_min_batch, adj_help_max_batch
static StepTraits traits_of(const int* v) {
    StepTraits t;
    t.NP = v[0]; t.n = v[1]; t.big = v[2]; t.point_forces = v[3]; t.contact = v[4]; t.spherical = v[5]; t.is_chain = v[6]; t.gconst = v[7];
    t.n_simd = v[8]; t.coop_g = v[9]; t.w2_max_batch = v[10]; t.w2_min_batch = v[11]; t.gconst_min_batch = v[12]; t.adj_help_max_batch = v[13];
    return t;
}

// out[11]: kernel, stores_ticks, parks, park_halvings, fused, contact_pass, fullchain, fulln, energy, block, full_chain32_plain
// use_env: the knobs come from the environment (knobs_from_env) instead of knobs[6] = park_halvings, coop_map, w2_runahead, pairc,
// ground_fused, adj_help
const char* sp_select_step(const int* traits, int B, int integ, int records_energy, const int* knobs, int use_env, int* out) {
    StepKnobs k;
    if (use_env) k = knobs_from_env();
    else { k.park_halvings = knobs[0]; k.coop_map = knobs[1]; k.w2_runahead = knobs[2]; k.pairc = knobs[3]; k.ground_fused = knobs[4]; k.adj_help = knobs[5]; }
    const StepTraits t = traits_of(traits);
    const StepPlan p = select_step(t, B, integ, records_energy != 0, k);
    const int v[11] = {(int)p.kernel, p.stores_ticks, p.parks, p.park_halvings, p.fused, p.contact_pass, p.fullchain, p.fulln, p.energy, p.block,
                       full_chain32_plain(t)};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
    return p.label;
}

// returns 0 help-16, 1 full-16-chain, 2 generic; *fullchain: the plan's instantiation flag
int sp_select_adjoint(const int* traits, int B, int adj_help, int* fullchain) {
    StepKnobs k;
    k.adj_help = adj_help != 0;
    const AdjPlan p = select_adjoint(traits_of(traits), B, k);
    *fullchain = p.fullchain;
    return (int)p.kernel;
}

// the knobs as the environment gives them: out[6] as knobs[6] above
void sp_knobs_from_env(int* out) {
    const StepKnobs k = knobs_from_env();
    const int v[6] = {k.park_halvings, k.coop_map, k.w2_runahead, k.pairc, k.ground_fused, k.adj_help};
    for (int i = 0; i < 6; ++i) out[i] = v[i];
}
}
