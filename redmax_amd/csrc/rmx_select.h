// rmx_select.h -- which kernel family a step / adjoint call runs: the ONE place that decides it.
// Host only and free of HIP types (tests/test_step_plan.py compiles it with plain g++): select_step() maps what the model, the
// device, the call and the environment say onto a StepPlan; launch_step (redmax_hip.hip) executes the plan through leaf launchers
// (the part_*.hip files, rmx_big.hip) that decide nothing themselves.  The table is DESIGN.md "Which kernel runs"; first match wins.
#pragma once
#include <cstdlib>

namespace rmx_select {

enum { BDF1 = 1, BDF2 = 2 };      // (INTEG_BDF1 / INTEG_BDF2 of rmx_host.h)

// What the choice depends on, from the model and its device (fixed once the model's forces are set).
struct StepTraits {
    int NP = 0, n = 0;                  // padded size (4 .. 64; anything for big) and nodes in use
    bool big = false;                   // more than 64 nodes
    bool point_forces = false, contact = false, spherical = false;      // rmx_pf.h table, ForceGroundCuboid, nsph > 0
    bool is_chain = false, gconst = false;                               // serial chain; constants staged in global memory
    int n_simd = 0;                     // SIMDs of the device
    int coop_g = 0;                     // wavefronts of a cooperative group (COOP_G of rmx_device.h, a build constant)
    int w2_max_batch = 0, w2_min_batch = 0, gconst_min_batch = 0, adj_help_max_batch = 0;      // read at model creation
};

// The per-call switches.  Tests and tools change them inside one process, so they are read at every call.
struct StepKnobs {
    int park_halvings = 24;             // RMX_PARK_HALVINGS (0: one wavefront per rollout throughout)
    int coop_map = 0;                   // RMX_COOP_MAP (measurement aid)
    bool w2_runahead = true;            // RMX_W2_RUNAHEAD
    bool pairc = true;                  // RMX_PAIRC (0: the one-point kernels for the full 32-link chain)
    int ground_fused = 1;               // RMX_GROUND_FUSED: 1 one launch, 2 the groups in a second, 0 three launches, 3 measurement aid
    bool adj_help = true;               // RMX_ADJ_HELP
};
inline int env_int(const char* name, const int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
inline StepKnobs knobs_from_env() {
    StepKnobs k;
    k.park_halvings = env_int("RMX_PARK_HALVINGS", 24);
    k.coop_map = env_int("RMX_COOP_MAP", 0);
    k.w2_runahead = env_int("RMX_W2_RUNAHEAD", 1) != 0;
    k.pairc = env_int("RMX_PAIRC", 1) != 0;
    k.ground_fused = env_int("RMX_GROUND_FUSED", 1);
    k.adj_help = env_int("RMX_ADJ_HELP", 1) != 0;
    return k;
}

// One enumerator per launch recipe (the row of the table in the comment).
enum class StepKernel {
    Big,             //  1 rmx_big.hip
    PointForces,     //  2 part_pf
    Ct,              //  3 part_ct: the lean launch, then (contact) the launch with the contact terms
    Ground32,        //  4 part_ground32: k_ground32 (fused modes 1, 2, 3)
    StepPair32,      //  4 part_ct's lean launch, then part_ground32: k_step_pair (fused mode 0)
    W2_64,           //  5 part_w2_tree64
    PairChain32,     //  6 part_pair32
    W2Chain32,       //  7 part_w2_chain32
    FullChain,       //  8 part_fullchain
    Gconst64,        //  9 part_gconst64
    FullN64,         // 10 part_fullchain
    Plain,           // 11 part_plain
};

struct StepPlan {
    StepKernel kernel = StepKernel::Plain;
    const char* label = "";             // what rmx_last_step_kernel reports
    bool stores_ticks = false;          // the kernel STORES its tick count (every other one adds: the caller zeroes the counters first)
    bool parks = false;                 // rollouts may be parked for cooperative groups: the caller sets their buffers up
    int park_halvings = 0;              // DevOpts::parkHalv
    int fused = 0;                      // StepArgs::fused, the effective RMX_GROUND_FUSED
    bool contact_pass = false;          // Ct: the launch with the contact terms follows the lean one
    bool fullchain = false, fulln = false;      // W2_64, Gconst64: the serial-chain / n == NP instantiation
    bool energy = true;                 // false: the instantiation that does not carry the last evaluation's energies (W2_64 fulln, PairChain32)
    int block = 64;                     // threads per workgroup (128: a helper wavefront, which brings its own LDS area)
};

// The full 32-link plain chain: what the two-point kernel (and its phase-timing twin) is built for.
inline bool full_chain32_plain(const StepTraits& t) {
    return !t.big && t.NP == 32 && t.is_chain && t.n == 32 && !t.contact && !t.spherical;
}

// "<PRE><NP><S1>" under BDF1, "<PRE2><NP><S2>" under BDF2, as literals
#define RMX_SEL_LABEL(NPV, P1, S1, P2, S2) \
    case NPV: return bdf1 ? P1 #NPV S1 : P2 #NPV S2;
#define RMX_SEL_LABELS(P1, S1, P2, S2)                                                                                              \
    switch (NP) {                                                                                                                   \
        RMX_SEL_LABEL(4, P1, S1, P2, S2) RMX_SEL_LABEL(8, P1, S1, P2, S2) RMX_SEL_LABEL(16, P1, S1, P2, S2)                          \
        RMX_SEL_LABEL(32, P1, S1, P2, S2) default : return bdf1 ? P1 "64" S1 : P2 "64" S2;                                           \
    }
inline const char* label_plain(const int NP, const bool bdf1) { RMX_SEL_LABELS("k_step_bdf1<", ">", "k_step_bdf2<", ">") }
inline const char* label_ct(const int NP, const bool bdf1) { RMX_SEL_LABELS("k_step_bdf1<", ",ct>", "k_step_bdf2<", ",ct>") }
inline const char* label_fullchain(const int NP, const bool bdf1) { RMX_SEL_LABELS("k_step_bdf1<", ",fullchain>", "k_step_bdf2<", ",fullchain>") }
inline const char* label_pf(const int NP, const bool bdf1) { RMX_SEL_LABELS("k_step_pf<", ",bdf1>", "k_step_pf<", ",bdf2>") }
#undef RMX_SEL_LABELS
#undef RMX_SEL_LABEL

inline StepPlan select_step(const StepTraits& t, const int B, const int integ, const bool records_energy, const StepKnobs& k) {
    StepPlan p;
    const bool bdf1 = integ == BDF1;
    const bool full = t.n == t.NP, fullchain = t.is_chain && full;
    const bool w2_fits = t.w2_max_batch > 0 && B <= t.w2_max_batch;
    auto is = [&](const StepKernel kern, const char* label) { p.kernel = kern; p.label = label; return p; };
    if (t.big) return is(StepKernel::Big, "k_big_step");                                                              // 1
    if (t.point_forces) return is(StepKernel::PointForces, label_pf(t.NP, bdf1));                                    // 2
    if (t.NP == 32 && t.contact && t.is_chain && !t.spherical) {                                                     // 4
        p.park_halvings = (t.n_simd >= t.coop_g && B >= 1) ? k.park_halvings : 0;      // (a group needs a SIMD per member)
        p.parks = p.park_halvings > 0;
        p.fused = (k.ground_fused == 1 && !p.parks) ? 2 : k.ground_fused;      // (one launch for rollouts AND groups needs groups)
        return p.fused ? is(StepKernel::Ground32, "k_ground32") : is(StepKernel::StepPair32, "k_step_pair");
    }
    if (t.contact || t.spherical) {                                                                                  // 3
        p.contact_pass = t.contact;
        return is(StepKernel::Ct, label_ct(t.NP, bdf1));
    }
    if (t.NP == 64 && w2_fits) {                                                                                     // 5
        p.fullchain = fullchain;
        p.fulln = full && !fullchain;
        p.energy = !(p.fulln && bdf1) || records_energy;
        p.block = 128;
        return is(StepKernel::W2_64, bdf1 ? "k_step_bdf1<64,w2>" : "k_step_bdf2<64,w2>");
    }
    if (full_chain32_plain(t) && bdf1 && k.pairc) {                                                                  // 6
        p.stores_ticks = true;
        p.energy = records_energy;
        return is(StepKernel::PairChain32, "k_step_bdf1_pair32");
    }
    if (full_chain32_plain(t) && bdf1 && w2_fits && B >= t.w2_min_batch) {                                           // 7
        p.block = 128;
        return is(StepKernel::W2Chain32, "k_step_bdf1<32,fullchain,w2>");
    }
    if (t.NP >= 16 && fullchain) return is(StepKernel::FullChain, label_fullchain(t.NP, bdf1));      // 8
    if (t.NP == 64 && t.gconst && t.gconst_min_batch > 0 && B >= t.gconst_min_batch) {                               // 9
        p.fulln = full;
        return is(StepKernel::Gconst64, bdf1 ? "k_step_bdf1<64,gconst>" : "k_step_bdf2<64,gconst>");
    }
    if (t.NP == 64 && full) return is(StepKernel::FullN64, bdf1 ? "k_step_bdf1<64,fulln>" : "k_step_bdf2<64,fulln>");      // 10
    return is(StepKernel::Plain, label_plain(t.NP, bdf1));                                                          // 11
}

// The adjoint pair (forward sweep + backward sweep) of trees of <= 64 nodes without contact, Euler charts or point forces.
enum class AdjKernel {
    Help16,          // part_adjhelp16: a second wavefront per rollout forms and stores M, D (batches of up to one rollout per two SIMDs)
    FullChain16,     // part_plain: the full 16-link chain
    Generic,         // part_plain
};
struct AdjPlan {
    AdjKernel kernel = AdjKernel::Generic;
    bool fullchain = false;             // Help16: the full 16-link chain's instantiation
};
inline AdjPlan select_adjoint(const StepTraits& t, const int B, const StepKnobs& k) {
    AdjPlan p;
    p.fullchain = t.NP == 16 && t.is_chain && t.n == 16;
    if (t.NP == 16 && k.adj_help && t.adj_help_max_batch > 0 && B <= t.adj_help_max_batch) p.kernel = AdjKernel::Help16;
    else if (p.fullchain) p.kernel = AdjKernel::FullChain16;
    return p;
}

// The taped rollout (rmx_rollout_tape / rmx_rollout_tape_bdf2 and the rmx_rollout_vjp that follows): BDF1 runs what the adjoint pair
// runs.  The BDF2 tape also keeps H, M, D of the SDIRK2a solve; a second hand-over in step 1 only would make the barrier counts of the
// two wavefronts depend on the step, for a saving in one solve of the rollout, so it never takes the helper-wave form.
inline AdjPlan select_rollout_tape(const StepTraits& t, const int B, const int integ, const StepKnobs& k) {
    AdjPlan p = select_adjoint(t, B, k);
    if (integ == BDF2 && p.kernel == AdjKernel::Help16) p.kernel = p.fullchain ? AdjKernel::FullChain16 : AdjKernel::Generic;
    return p;
}
inline const char* label_rollout_tape_bdf2(const AdjPlan& p) {      // what rmx_last_step_kernel reports after rmx_rollout_tape_bdf2
    return p.kernel == AdjKernel::FullChain16 ? "k_adjoint_fwd<16,bdf2,tape,fullchain>" : "k_adjoint_fwd<bdf2,tape>";
}


// The taped rollout under state feedback (rmx_rollout_tape_feedback): always the generic one-wavefront kernel of part_plain, for
// both integrators - never the helper-wave form (the feedback stage reads the registers of the wave that integrates) and never the
// full-chain instantiation (one kernel per size keeps the new code small; the stage is a few percent of a step).  The backward
// sweeps that read its tape follow select_rollout_tape: the tape's layout does not depend on the kernel that wrote it.
inline AdjPlan select_rollout_feedback(const StepTraits&, const int, const int, const StepKnobs&) { return AdjPlan{}; }
inline const char* label_rollout_feedback(const int integ) {      // what rmx_last_step_kernel reports after rmx_rollout_tape_feedback
    return integ == BDF2 ? "k_adjoint_fwd<bdf2,tape,feedback>" : "k_adjoint_fwd<bdf1,tape,feedback>";
}

// The closed-loop backward sweep (rmx_rollout_vjp_feedback with gains or a cotangent of the applied torque): always the generic
// one-wavefront kernel of part_plain (rmx_feedback_bwd.h), for both integrators and every size - the K term sits between two solves
// of the same wavefront, so there is no helper-wave form, and one kernel per size keeps the new code small.  Without gains and
// without gu the entry IS rmx_rollout_vjp and follows select_rollout_tape: label_rollout_vjp names the backward kernel that plan runs.
inline AdjPlan select_rollout_vjp_feedback(const StepTraits&, const int, const int, const StepKnobs&) { return AdjPlan{}; }
inline const char* label_rollout_vjp_feedback(const int integ) {      // what rmx_last_step_kernel reports after rmx_rollout_vjp_feedback
    return integ == BDF2 ? "k_rollout_bwd_fb<bdf2,vjp_feedback>" : "k_rollout_bwd_fb<bdf1,vjp_feedback>";
}
inline const char* label_rollout_vjp(const AdjPlan& p, const int integ) {      // ... after rmx_rollout_vjp_feedback without gains and gu
    const bool fc = p.kernel == AdjKernel::FullChain16 || (p.kernel == AdjKernel::Help16 && p.fullchain);
    if (integ == BDF2) return fc ? "k_rollout_bwd_bdf2<16,fullchain>" : "k_rollout_bwd_bdf2";
    return fc ? "k_adjoint_bwd<16,bdf1,tape,fullchain>" : "k_adjoint_bwd<bdf1,tape>";
}

// The Riccati sweep over the BDF1 tape (rmx_rollout_lqr): one workgroup of four wavefronts per rollout with Vxx and every temporary
// of a step in LDS (rmx_lqr.h: 17 blocks of (NP + 1) NP doubles and 8 vectors of NP).  That kernel exists for the padded sizes up to
// 32 - at 64 the blocks alone would be 17 * 33 280 bytes, over three times a CU's LDS -, so nr > 32 is refused, and with it a tree
// of more than 32 nodes whose reduced DOFs are fewer (its elimination runs at the padded size of its NODES).
constexpr int LQR_MAX_NR = 32, LQR_BLOCKS = 17, LQR_VECTORS = 8, LQR_BLOCK_THREADS = 256;
enum class LqrKernel {
    Lds,             // part_plain: k_rollout_lqr<NP>
    RefusedNr,       // nr > LQR_MAX_NR
    RefusedNodes,    // nr fits, the tree's padded size does not
};
struct LqrPlan {
    LqrKernel kernel = LqrKernel::Lds;
    int block = LQR_BLOCK_THREADS;      // threads per workgroup
    size_t lds_bytes = 0;               // dynamic LDS of the workgroup
};
inline size_t lqr_lds_bytes(const int NP) { return sizeof(double) * ((size_t)LQR_BLOCKS * (NP + 1) * NP + (size_t)LQR_VECTORS * NP); }
inline LqrPlan select_rollout_lqr(const StepTraits& t, const int nr) {
    LqrPlan p;
    if (nr > LQR_MAX_NR) p.kernel = LqrKernel::RefusedNr;
    else if (t.big || t.NP > LQR_MAX_NR) p.kernel = LqrKernel::RefusedNodes;
    else p.lds_bytes = lqr_lds_bytes(t.NP);
    return p;
}

// The box-constrained sweep (rmx_rollout_lqr_box): k_rollout_lqr<NP, true>, the same workgroup and blocks with the vectors of the QP
// behind them (lo, hi, x, grad, the trial point, the direction, Hq y, the right-hand column): 17 blocks and 16 vectors, 147 712 bytes
// at NP = 32 of the CU's 163 840.  The sizes it exists for, and so its refusals, are select_rollout_lqr's.
constexpr int LQR_BOX_VECTORS = LQR_VECTORS + 8, LQR_BOX_MAX_ITER = 64;      // (the default cap on the QP iterations of a step)
inline size_t lqr_box_lds_bytes(const int NP) { return sizeof(double) * ((size_t)LQR_BLOCKS * (NP + 1) * NP + (size_t)LQR_BOX_VECTORS * NP); }
inline LqrPlan select_rollout_lqr_box(const StepTraits& t, const int nr) {
    LqrPlan p = select_rollout_lqr(t, nr);
    if (p.kernel == LqrKernel::Lds) p.lds_bytes = lqr_box_lds_bytes(t.NP);
    return p;
}
inline const char* label_rollout_lqr_box() { return "k_rollout_lqr<box>"; }      // what rmx_last_step_kernel reports after rmx_rollout_lqr_box
inline const char* label_rollout_feedback_box(const int integ) {      // ... after rmx_rollout_tape_feedback_box
    return integ == BDF2 ? "k_adjoint_fwd<bdf2,tape,feedback,box>" : "k_adjoint_fwd<bdf1,tape,feedback,box>";
}

// The taped rollouts of a model with point forces (rmx_model_tape_point_forces; rmx_tape_pf.h): always the one-wavefront kernel
// k_tape_pf of part_pf's object of the model's padded size, for both integrators, open loop or under feedback (the box is the
// feedback kernel's clamp) - never the helper-wave form, the full-chain instantiation or the matrix-core store of M, D, which all
// belong to sparse H.  The backward sweeps that read its tape follow select_rollout_tape: the layout is every tape's.  The labels
// name the sweep it stands in for; the ABI refuses what has no such kernel (more than 64 nodes, contact, spherical joints) before
// a plan is asked for, and the plan says so again.
enum class TapePfKernel {
    Wave,            // part_pf: k_tape_pf<NP, INTEG, FB>
    Refused,         // no force table, or a model rmx_model_set_point_forces refuses
};
struct TapePfPlan {
    TapePfKernel kernel = TapePfKernel::Wave;
    const char* label = "";             // what rmx_last_step_kernel reports
    int np = 0;                         // the padded size that runs
    bool feedback = false;              // the instantiation with the feedback stage
    int block = 64;                     // threads per workgroup: one wavefront per rollout
};
inline const char* label_rollout_tape_pf(const int integ, const bool feedback) {
    if (feedback) return integ == BDF2 ? "k_adjoint_fwd<bdf2,tape,feedback,pf>" : "k_adjoint_fwd<bdf1,tape,feedback,pf>";
    return integ == BDF2 ? "k_adjoint_fwd<bdf2,tape,pf>" : "k_adjoint_fwd<bdf1,tape,pf>";
}
inline TapePfPlan select_rollout_tape_pf(const StepTraits& t, const int integ, const bool feedback) {
    TapePfPlan p;
    if (!t.point_forces || t.big || t.contact || t.spherical || (integ != BDF1 && integ != BDF2)) {
        p.kernel = TapePfKernel::Refused;
        return p;
    }
    p.label = label_rollout_tape_pf(integ, feedback);
    p.np = t.NP;
    p.feedback = feedback;
    return p;
}

// The line search of the device iLQR (rmx_rollout_search; rmx_search.h): one wavefront per rollout runs every trial pass and the
// nominal pass of the closed loop, with the cost inside the launch - k_rollout_search<NP> in part_plain's object of the model's
// padded size.  The search exists where the sweep that feeds it exists: the sizes, and so the refusals, are select_rollout_lqr's.
constexpr int SEARCH_MAX_ALPHAS = 16;      // (RMX_SEARCH_MAX_ALPHAS of the header)
enum class SearchKernel {
    Wave,            // part_plain: k_rollout_search<NP>
    RefusedNr,       // nr > LQR_MAX_NR
    RefusedNodes,    // nr fits, the tree's padded size does not
};
struct SearchPlan {
    SearchKernel kernel = SearchKernel::Wave;
    int np = 0;                         // the padded size that runs
    int block = 64;                     // threads per workgroup: one wavefront per rollout
};
inline SearchPlan select_rollout_search(const StepTraits& t, const int nr) {
    SearchPlan p;
    const LqrPlan l = select_rollout_lqr(t, nr);
    if (l.kernel == LqrKernel::RefusedNr) p.kernel = SearchKernel::RefusedNr;
    else if (l.kernel == LqrKernel::RefusedNodes) p.kernel = SearchKernel::RefusedNodes;
    else p.np = t.NP;
    return p;
}
inline const char* label_rollout_search() { return "k_rollout_search<bdf1,tape,feedback>"; }      // what rmx_last_step_kernel reports

// Point kinematics and the cost model along a state record (rmx_rollout_points, rmx_rollout_cost; rmx_cost.h): one wavefront per
// (rollout, step), lane = node, in part_plain's object of the model's padded size - every size has one, 64 included, and the kernel
// holds nothing in LDS.  Kinematics alone decides: spherical joints (their Euler charts are not a function of q alone) and trees of
// more than 64 nodes are refused; ground contact and point forces do not enter kinematics and are taken.
enum class CostKernel {
    Wave,                // part_plain: k_rollout_cost<NP, FRAMES>
    RefusedSpherical,
    RefusedNodes,        // more than 64 nodes
    RefusedGrid,         // batch * nsteps wavefronts exceed the grid
};
struct CostPlan {
    CostKernel kernel = CostKernel::Wave;
    int np = 0;                         // the padded size that runs
    int block = 64;                     // threads per workgroup
    size_t grid = 0;                    // workgroups: batch * nsteps
};
constexpr size_t COST_MAX_GRID = 0x7fffffff;
inline CostPlan select_rollout_cost(const StepTraits& t, const int B, const int nsteps) {
    CostPlan p;
    if (t.spherical) p.kernel = CostKernel::RefusedSpherical;
    else if (t.big || t.NP > 64) p.kernel = CostKernel::RefusedNodes;
    else if (B < 1 || nsteps < 1 || (size_t)B * (size_t)nsteps > COST_MAX_GRID) p.kernel = CostKernel::RefusedGrid;
    else {
        p.np = t.NP;
        p.grid = (size_t)B * (size_t)nsteps;
    }
    return p;
}
inline const char* label_rollout_cost() { return "k_rollout_cost"; }      // what rmx_last_step_kernel reports after the two entries
inline const char* label_rollout_frames() { return "k_rollout_frames"; }  // ... after rmx_rollout_frames / rmx_rollout_cost_frames: the same plan,
                                                                          // the FRAMES instantiation under the label it always had

}      // namespace rmx_select
