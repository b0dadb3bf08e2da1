// redmax_hip.hip -- the C ABI of include/redmax_hip.h (host side).
//
// Scene.init()-equivalent flattening of the scene listing into SoA device constants (matlab-diff/+redmax/Scene.m:59-119),
// batch state in HBM, streams/events and launch plumbing.  Kernels and their launchers: the part_*.hip files around
// rmx_kernels.h (one object per part and padded tree size, declared in rmx_host.h); device code: rmx_device.h.
// There is no CPU fallback: every entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <cstdlib>
#include <string>
#include <vector>

#include "rmx_host.h"
#include "rmx_tape.h"

// ============================================================================ host side

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return fail(RMX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)



extern "C" const char* rmx_last_error(void) { return g_err.c_str(); }
static void hist_free(rmx_batch* b);
static hipError_t set_started(rmx_batch* b, int v);

// An error already pending in this thread's HIP state when an entry point is about to launch.  If this batch still has an
// asynchronous launch of its own that nobody waited for (rmx_step_bdf1_async without rmx_sync), the error is reported as that
// launch's and nothing is launched on top of it.  Otherwise it was left behind by another user of HIP in this process: it is taken
// out of this launch's verdict (hipGetLastError clears it), but not silently - rmx_last_error() keeps the note.
static int pending_error_check(rmx_batch* b, const char* who) {
    const hipError_t prev = hipGetLastError();
    if (prev == hipSuccess) return RMX_OK;
    if (b && b->async_pending)
        return fail(RMX_E_HIP, std::string(who) + ": an earlier asynchronous launch of this batch failed: " + hipGetErrorString(prev));
    g_err = std::string(who) + ": note: a HIP error was already pending before this call (left by another user of the process): " + hipGetErrorString(prev);
    return RMX_OK;
}
extern "C" int rmx_version(void) { return RMX_VERSION; }
extern "C" int rmx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" void rmx_opts_default(rmx_opts* o) {
    if (!o) return;
    o->h = 1e-2;            // Scene.h default (Scene.m:42)
    o->tol = 1e-9;          // driverRedMaxBDF1.m:95
    o->dxMax = 1e3;         // :96
    o->iterMaxPerDof = 10;  // :97
    o->iterLsMax = 20;      // :98
    o->lu_mode = 0;
    o->compensated = 1;
    o->ls_fail_limit = 0;   // the reference: never cut the Newton loop short
}

namespace {

struct M4 {
    double a[4][4];
};
M4 eye4() {
    M4 E{};
    for (int i = 0; i < 4; ++i) E.a[i][i] = 1.0;
    return E;
}
M4 from_cm(const double* cm) {
    M4 E;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) E.a[i][j] = cm[j * 4 + i];
    return E;
}
M4 mul(const M4& A, const M4& B) {
    M4 C{};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += A.a[i][k] * B.a[k][j];
            C.a[i][j] = s;
        }
    return C;
}
M4 inv(const M4& E) {   // se3.inv (se3.m:11-16)
    M4 I = eye4();
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) I.a[i][j] = E.a[j][i];
    for (int i = 0; i < 3; ++i) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += E.a[k][i] * E.a[k][3];
        I.a[i][3] = -s;
    }
    return I;
}

// 3x3 helpers on row-major arrays
void m3mul(const double A[9], const double B[9], double C[9]) {
    double T[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
    std::memcpy(C, T, sizeof(T));
}
void m3v(const double A[9], const double x[3], double y[3]) {
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
    std::memcpy(y, t, sizeof(t));
}

}  // namespace

// Scene.init() for a listing of fixed / revolute / prismatic joints.  idx_explicit (or NULL): reduced index of every listed
// joint, given when the listing is the lowered form of a scene with multi-DOF joints (rmx_model_create below).
// The environment variables a model reads, once, when it is created (tests set them before they create it; the per-call switches
// are rmx_select.h's StepKnobs).
struct ModelEnv {
    int lds_limit;        // RMX_BIG_LDS_LIMIT: development aid (0: H of large trees stays in HBM); default: the device's limit
    bool tree_solve;      // RMX_TREE_SOLVE=0: the dense guarded solve for every tree (tests)
    int gconst_min;       // RMX_GCONST_MIN: 33..64-node trees, batches from this size on read the constants from global memory
    int w2_max, w2c_min;  // RMX_W2_MAX, RMX_W2C_MIN: the batch sizes that take two wavefronts per rollout (w2c_min: the full 32-link chain)
};
static ModelEnv model_env(const int n_simd, const int lds_limit) {
    using rmx_select::env_int;
    return ModelEnv{env_int("RMX_BIG_LDS_LIMIT", lds_limit), env_int("RMX_TREE_SOLVE", 1) != 0,
                    env_int("RMX_GCONST_MIN", n_simd > 0 ? n_simd / 2 + 1 : 513), env_int("RMX_W2_MAX", n_simd > 0 ? n_simd / 2 : 512),
                    env_int("RMX_W2C_MIN", 128)};
}

static int model_create_flat(const rmx_model_desc* d, const int* idx_explicit, const std::vector<int>* sph_first, int device,
                             rmx_model** out) {
    if (!d || !out) return fail(RMX_E_INVALID, "null argument");
    *out = nullptr;
    int ndev = rmx_device_count();
    if (ndev <= 0) return fail(RMX_E_NODEVICE, "no HIP device visible: redmax_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(RMX_E_INVALID, "device index out of range");
    const int n = d->njoints;
    if (n < 1 || n > BIG_MAXN)
        return fail(RMX_E_INVALID, "the scene needs " + std::to_string(n) + " 1-DOF nodes; the limit is " + std::to_string(BIG_MAXN) +
                                       " (up to " + std::to_string(MAXN) + ": one wavefront per tree; beyond: one workgroup per tree)");
    if (!d->parent || !d->type || !d->axis || !d->E0_pj || !d->E0_ji || !d->I_i)
        return fail(RMX_E_INVALID, "parent/type/axis/E0_pj/E0_ji/I_i are required");
    // node stride of the SoA constant arrays and rows of the ancestor table: the one-wavefront kernels (n <= 64) and the
    // one-workgroup kernels for larger trees (rmx_big.hip)
    const bool big = n > MAXN;
    const int NS = big ? BIG_MAXN : MAXN;
    const int NROUNDS = big ? BIG_MAXROUNDS : MAXROUNDS;
    // ---- validate the listing: exactly one root first, parents before children (Scene.m:66-67)
    for (int i = 0; i < n; ++i) {
        if (d->type[i] < 0 || d->type[i] > 2) return fail(RMX_E_INVALID, "unsupported joint type");
        if (i == 0 && d->parent[i] != -1) return fail(RMX_E_INVALID, "joint 0 must be the root");
        if (i > 0 && (d->parent[i] < 0 || d->parent[i] >= i)) return fail(RMX_E_INVALID, "joints must be listed parent-before-child with a single root");
    }
    // ---- reduced / maximal numbering, leaf-to-root over the LISTING (Scene.m:69-71, Joint.countDofs, Body.countDofs)
    std::vector<int> idxL(n, -1);
    int nr = 0;
    for (int i = n - 1; i >= 0; --i)
        if (d->type[i] != RMX_JOINT_FIXED) idxL[i] = idx_explicit ? idx_explicit[i] : nr, ++nr;
    // ---- depth-first order (children in listing order); identity for the reference's scenes
    std::vector<std::vector<int>> kids(n);
    for (int i = 1; i < n; ++i) kids[d->parent[i]].push_back(i);
    std::vector<int> order;   // order[k] = listing index of the k-th node in depth-first order
    order.reserve(n);
    {
        std::vector<int> stack{0};
        while (!stack.empty()) {
            int j = stack.back();
            stack.pop_back();
            order.push_back(j);
            for (int c = (int)kids[j].size() - 1; c >= 0; --c) stack.push_back(kids[j][c]);
        }
    }
    std::vector<int> pos(n);
    for (int k = 0; k < n; ++k) pos[order[k]] = k;
    std::vector<int> par(n), endv(n), depth(n);
    for (int k = 0; k < n; ++k) {
        int pl = d->parent[order[k]];
        par[k] = pl < 0 ? -1 : pos[pl];
        depth[k] = pl < 0 ? 0 : depth[par[k]] + 1;
    }
    for (int k = n - 1; k >= 0; --k) {
        endv[k] = k + 1;
        for (int c : kids[order[k]]) endv[k] = std::max(endv[k], endv[pos[c]]);
    }
    int maxdepth = 0, is_chain = 1;
    for (int k = 0; k < n; ++k) {
        maxdepth = std::max(maxdepth, depth[k]);
        if (endv[k] != n) is_chain = 0;
    }
    int rounds = 0;
    while ((1 << rounds) < maxdepth + 1) ++rounds;
    if (rounds > NROUNDS) return fail(RMX_E_INVALID, "tree too deep");

    // constants of listed joint L for joint type jtype about axis_in: Kc[36] = rows R(9),p(3) of K0,K1,K2 ; sbc[6] = A0_ij S
    auto joint_consts = [&](const int L, const int jtype, const double* axis_in, double* Kc, double* sbc) -> bool {
        const M4 E0_pj = from_cm(d->E0_pj + 16 * L);
        const M4 E0_ji = from_cm(d->E0_ji + 16 * L);
        M4 Lm = E0_pj;   // root: E_wj = E0_pj Q  (Joint.m:404-415)
        if (d->parent[L] >= 0) Lm = mul(inv(from_cm(d->E0_ji + 16 * d->parent[L])), E0_pj);   // parent body -> joint frame
        double ax[3] = {axis_in[0], axis_in[1], axis_in[2]};
        if (jtype != RMX_JOINT_FIXED) {   // JointRevolute.m:14 / JointPrismatic.m:15
            double nn = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
            if (!(nn > 0)) return false;
            for (double& v : ax) v /= nn;
        }
        double LR[9], Lp[3], RR[9], Rp[3];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) {
                LR[3 * i + j] = Lm.a[i][j];
                RR[3 * i + j] = E0_ji.a[i][j];
            }
            Lp[i] = Lm.a[i][3];
            Rp[i] = E0_ji.a[i][3];
        }
        double K0R[9], K0p[3], K1R[9] = {0}, K1p[3] = {0}, K2R[9] = {0}, K2p[3] = {0};
        if (jtype == RMX_JOINT_REVOLUTE) {
            // se3.aaToMat (se3.m:111-176) special-cases axis-aligned rotations: snap the ROTATION axis exactly
            // as those branches do, so R(q) has the same exact zeros / ones; S keeps the given axis.
            double ar[3] = {ax[0], ax[1], ax[2]};
            const double TH = 1e-9;
            if (std::fabs(ar[0]) < TH && std::fabs(ar[1]) < TH) { ar[0] = 0; ar[1] = 0; ar[2] = ar[2] < 0 ? -1.0 : 1.0; }
            else if (std::fabs(ar[1]) < TH && std::fabs(ar[2]) < TH) { ar[1] = 0; ar[2] = 0; ar[0] = ar[0] < 0 ? -1.0 : 1.0; }
            else if (std::fabs(ar[2]) < TH && std::fabs(ar[0]) < TH) { ar[2] = 0; ar[0] = 0; ar[1] = ar[1] < 0 ? -1.0 : 1.0; }
            // R(q) = a a' + cos q (I - a a') + sin q [a]
            double aat[9], Ima[9], ab[9] = {0, -ar[2], ar[1], ar[2], 0, -ar[0], -ar[1], ar[0], 0};
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    aat[3 * i + j] = ar[i] * ar[j];
                    Ima[3 * i + j] = (i == j ? 1.0 : 0.0) - ar[i] * ar[j];
                }
            double T[9], t3[3];
            m3mul(LR, aat, T); m3mul(T, RR, K0R); m3v(T, Rp, t3);
            for (int i = 0; i < 3; ++i) K0p[i] = Lp[i] + t3[i];
            m3mul(LR, ab, T); m3mul(T, RR, K1R); m3v(T, Rp, K1p);
            m3mul(LR, Ima, T); m3mul(T, RR, K2R); m3v(T, Rp, K2p);
        } else {
            double t3[3];
            m3mul(LR, RR, K0R);
            m3v(LR, Rp, t3);
            for (int i = 0; i < 3; ++i) K0p[i] = Lp[i] + t3[i];
            if (jtype == RMX_JOINT_PRISMATIC) m3v(LR, ax, K1p);   // p(q) = a q  (JointPrismatic.m:29-33)
        }
        for (int c = 0; c < 9; ++c) {
            Kc[c] = K0R[c];
            Kc[12 + c] = K1R[c];
            Kc[24 + c] = K2R[c];
        }
        for (int c = 0; c < 3; ++c) {
            Kc[9 + c] = K0p[c];
            Kc[21 + c] = K1p[c];
            Kc[33 + c] = K2p[c];
        }
        // body-frame joint screw A0_ij S  (Body.setBodyTransform Body.m:46-51, Joint.m:508): Ad(E0_ij) [w; v]
        {
            const M4 E0_ij = inv(E0_ji);
            double S[6] = {0, 0, 0, 0, 0, 0};
            if (jtype == RMX_JOINT_REVOLUTE) { S[0] = ax[0]; S[1] = ax[1]; S[2] = ax[2]; }
            if (jtype == RMX_JOINT_PRISMATIC) { S[3] = ax[0]; S[4] = ax[1]; S[5] = ax[2]; }
            double Rm[9], pm[3] = {E0_ij.a[0][3], E0_ij.a[1][3], E0_ij.a[2][3]};
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) Rm[3 * i + j] = E0_ij.a[i][j];
            double w3[3], v3[3];
            m3v(Rm, S, w3);
            m3v(Rm, S + 3, v3);
            const double cx[3] = {pm[1] * w3[2] - pm[2] * w3[1], pm[2] * w3[0] - pm[0] * w3[2], pm[0] * w3[1] - pm[1] * w3[0]};
            for (int c = 0; c < 3; ++c) {
                sbc[c] = w3[c];
                sbc[3 + c] = v3[c] + cx[c];
            }
        }
        return true;
    };
    // ---- constants per node
    std::vector<double> K(36 * NS, 0.0), sb(6 * NS, 0.0), I4(4 * NS, 0.0), prm(8 * NS, 0.0);
    std::vector<int> type(NS, 0), idx(NS, -1), endd(NS, 0), anc(NROUNDS * NS, -1);
    std::vector<unsigned long long> rel(2 * MAXN, 0ull);      // relation bit masks: trees of up to 64 nodes only
    for (int k = 0; k < n; ++k) {
        const int L = order[k];
        type[k] = d->type[L];
        idx[k] = idxL[L];
        endd[k] = endv[k];
        int a = par[k];
        // ancestor 2^r levels up
        {
            std::vector<int> chain;   // chain[t] = ancestor t+1 levels up
            for (int t = par[k]; t >= 0; t = par[t]) {
                chain.push_back(t);
                if (!big) {
                    rel[k] |= 1ull << t;            // t is a strict ancestor of k
                    rel[MAXN + t] |= 1ull << k;     // k is a strict descendant of t
                }
            }
            for (int r = 0; r < NROUNDS; ++r) {
                int lv = 1 << r;
                anc[r * NS + k] = (lv <= (int)chain.size()) ? chain[lv - 1] : -1;
            }
        }
        (void)a;
        {
            double Kc[36], sbc[6];
            if (!joint_consts(L, type[k], d->axis + 3 * L, Kc, sbc)) return fail(RMX_E_INVALID, "zero joint axis");
            for (int c = 0; c < 36; ++c) K[c * NS + k] = Kc[c];
            for (int c = 0; c < 6; ++c) sb[c * NS + k] = sbc[c];
        }
        // inertia: the reference allows a general diagonal, but mass entries must agree (Body.m:107 uses M_i(4,4))
        const double* Ii = d->I_i + 6 * L;
        I4[0 * NS + k] = Ii[0];
        I4[1 * NS + k] = Ii[1];
        I4[2 * NS + k] = Ii[2];
        I4[3 * NS + k] = Ii[3];
        if (Ii[3] != Ii[4] || Ii[3] != Ii[5]) return fail(RMX_E_INVALID, "I_i(4:6) must all equal the body mass");
        prm[0 * NS + k] = d->tau ? d->tau[L] : 0.0;
        prm[1 * NS + k] = d->stiffness ? d->stiffness[L] : 0.0;
        prm[2 * NS + k] = d->damping ? d->damping[L] : 0.0;
        prm[3 * NS + k] = d->qRest ? d->qRest[L] : 0.0;
        prm[4 * NS + k] = d->qLimL ? d->qLimL[L] : -1e8;   // Joint.m:77-80 defaults
        prm[5 * NS + k] = d->qLimU ? d->qLimU[L] : 1e8;
        prm[6 * NS + k] = d->qLimK ? d->qLimK[L] : 1e8;
        prm[7 * NS + k] = d->qLimD ? d->qLimD[L] : 0.0;
    }

    // axis variants of the spherical group nodes: chart switches (JointSpherical.reparam_) swap them into LDS on the device
    const int nsph = sph_first ? (int)sph_first->size() : 0;
    if (nsph > MAXSPH) return fail(RMX_E_INVALID, "too many spherical joints: a scene may hold at most " + std::to_string(MAXSPH) + " JointSpherical / JointFree3D joints (their Euler-chart tables are sized for that)");
    std::vector<double> sphV((size_t)nsph * 9 * SPH_ROWS + 1, 0.0);
    for (int g = 0; g < nsph; ++g)
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                const double ea[3] = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
                double* v = &sphV[((size_t)(g * 3 + k) * 3 + a) * SPH_ROWS];
                if (pos[(*sph_first)[g] + k] != pos[(*sph_first)[g]] + k) return fail(RMX_E_INVALID, "spherical group is not contiguous");
                joint_consts((*sph_first)[g] + k, RMX_JOINT_REVOLUTE, ea, v, v + 36);
            }

    rmx_model* m = new rmx_model();
    m->device = device;
    m->n = n;
    m->nr = nr;
    m->nlist = n;
    m->nm = 6 * n;
    m->idx_listing = idxL;
    m->node_of_listing = pos;
    m->NP = n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : n <= 64 ? 64 : BIG_MAXN;
    m->big = big;
    // per-node constants + the rows of the per-body ground frames (con_setup; present in every launch so that attaching a
    // ForceGroundCuboid later does not change the layout)
    m->smem_bytes = big ? 0 : sizeof(double) * ((size_t)acc_doubles(n, m->NP) + (size_t)(NCONST + NGROUND) * cstride(m->NP));
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
            m->n_simd = 4 * prop.multiProcessorCount;
            m->lds_limit = (int)prop.sharedMemPerBlock;
            // the cooperative groups' timeout, ~2 s in s_memtime ticks: on gfx950 the counter runs at the shader clock (8.9 M ticks per
            // 3.75 ms launch, tools/pairc_ticks.py), on gfx90a / gfx942 at the constant 100 MHz reference clock
            const bool shader_rate = strncmp(prop.gcnArchName, "gfx950", 6) == 0 && prop.clockRate > 0;
            m->coop_ticks = shader_rate ? 2000ull * (unsigned long long)prop.clockRate : 200000000ull;
        }
    }
    const ModelEnv env = model_env(m->n_simd, m->lds_limit);
    m->lds_limit = env.lds_limit;
    if (hipSetDevice(device) != hipSuccess) { delete m; return fail(RMX_E_HIP, "hipSetDevice failed"); }
    // the tree as the multifrontal solve of 33..64-node branching trees walks it (DevModel::tree, tree_solve64 in rmx_device.h)
    std::vector<int> tree((size_t)TREE_ROWS * NS, -1);
    int tree_dmax = 0, tree_cmax = 0;
    if (!big && n > 32 && nsph == 0) {
        std::vector<int> dep(n, 0), nch(n, 0);
        bool ok = true;
        for (int k = 0; k < n && ok; ++k) {
            dep[k] = par[k] >= 0 ? dep[par[k]] + 1 : 0;
            if (par[k] >= k) ok = false;                       // (parents first: the depth-first order the kernels rely on)
            if (dep[k] > TREE_DMAX) ok = false;
            tree_dmax = std::max(tree_dmax, dep[k]);
            if (par[k] >= 0) {
                if (nch[par[k]] >= TREE_CMAX) ok = false;
                else tree[(size_t)(1 + TREE_DMAX + nch[par[k]]++) * NS + par[k]] = k;
                tree_cmax = std::max(tree_cmax, nch[par[k]]);
            }
        }
        int roots = 0;
        for (int k = 0; k < n; ++k) roots += par[k] < 0;
        if (roots != 1) ok = false;                            // (one tree: every frontal matrix ends at the same root)
        if (ok) {
            for (int k = 0; k < n; ++k) {
                tree[k] = dep[k];
                { int lv = 1; for (int t = par[k]; t >= 0; t = par[t], ++lv) tree[(size_t)lv * NS + k] = t; }      // row lv: the ancestor lv levels up
                tree[(size_t)(1 + TREE_DMAX + TREE_CMAX) * NS + k] = par[k];
            }
        }
        if (!ok || tree_dmax < 1) tree_dmax = 0;
        if (!env.tree_solve) tree_dmax = 0;
    }
    const size_t nd = K.size() + sb.size() + I4.size() + prm.size();
    const size_t ni = type.size() + idx.size() + endd.size() + anc.size() + tree.size();
    const size_t bytes = nd * sizeof(double) + rel.size() * sizeof(unsigned long long) + ni * sizeof(int);
    hipError_t e = hipMalloc(&m->dbuf, bytes);
    if (e != hipSuccess) { delete m; return fail(RMX_E_NOMEM, std::string("hipMalloc(model): ") + hipGetErrorString(e)); }
    std::vector<char> host(bytes);
    char* hp = host.data();
    char* dp = (char*)m->dbuf;
    auto put = [&](const void* src, size_t nb) { std::memcpy(hp, src, nb); const void* dptr = dp; hp += nb; dp += nb; return dptr; };
    m->dm.n = n;
    m->dm.nr = nr;
    m->dm.stride = NS;
    m->dm.rounds = rounds;
    m->dm.is_chain = is_chain;
    m->dm.K = (const double*)put(K.data(), K.size() * sizeof(double));
    m->dm.sb = (const double*)put(sb.data(), sb.size() * sizeof(double));
    m->dm.I4 = (const double*)put(I4.data(), I4.size() * sizeof(double));
    m->dm.prm = (const double*)put(prm.data(), prm.size() * sizeof(double));
    m->dm.rel = (const unsigned long long*)put(rel.data(), rel.size() * sizeof(unsigned long long));
    m->dm.type = (const int*)put(type.data(), type.size() * sizeof(int));
    m->dm.idx = (const int*)put(idx.data(), idx.size() * sizeof(int));
    m->dm.end = (const int*)put(endd.data(), endd.size() * sizeof(int));
    m->dm.anc = (const int*)put(anc.data(), anc.size() * sizeof(int));
    m->dm.tree = (const int*)put(tree.data(), tree.size() * sizeof(int));
    m->dm.tree_dmax = tree_dmax;
    m->dm.tree_cmax = tree_cmax;
    for (int c = 0; c < 3; ++c) m->dm.grav[c] = d->grav[c];
    e = hipMemcpy(m->dbuf, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(m->dbuf); delete m; return fail(RMX_E_HIP, std::string("hipMemcpy(model): ") + hipGetErrorString(e)); }
    m->dm.nsph = nsph;
    if (nsph) {
        for (int g = 0; g < nsph; ++g) m->dm.sph_first[g] = (short)pos[(*sph_first)[g]];
        e = hipMalloc(&m->dsph, sphV.size() * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(m->dsph, sphV.data(), sphV.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(m->dbuf); if (m->dsph) (void)hipFree(m->dsph); delete m; return fail(RMX_E_HIP, "spherical variant table"); }
        m->dm.sphV = (const double*)m->dsph;
    }
    if (m->NP == 64 && nsph == 0) {
        // Trees of 33..64 nodes: a second copy of the per-node constants, staged as the kernels read them, in global memory.  Batches
        // of more than two rollouts per CU run the kernels that read it from there (33.8 KB of LDS per wavefront instead of 68.6 KB:
        // four wavefronts per CU instead of two); RMX_GCONST_MIN in the environment moves the threshold (tests, measurements).
        e = hipMalloc(&m->dgconst, sizeof(double) * (size_t)NCONST * cstride(64));
        if (e == hipSuccess) {
            launch_stage_consts_64(m, (double*)m->dgconst, nullptr);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipDeviceSynchronize();
        }
        if (e != hipSuccess) {
            std::string msg = std::string("staging the constants table: ") + hipGetErrorString(e);
            rmx_model_destroy(m);
            return fail(RMX_E_HIP, msg);
        }
        m->dm.gconst = (const double*)m->dgconst;
    }
    // the batch sizes at which rmx_select.h changes kernels (one rollout per two SIMDs = one two-wave workgroup per CU pair of SIMDs)
    if (m->NP == 64 && nsph == 0) {      // part_gconst64.hip from gconst_min_batch rollouts on, part_w2_tree64.hip up to w2_max_batch
        m->gconst_min_batch = env.gconst_min;
        m->w2_max_batch = env.w2_max;
    }
    if (m->NP == 32 && nsph == 0 && m->dm.is_chain && m->dm.n == 32) {      // the full 32-link chain (BASELINE.json configs[1]): part_w2_chain32.hip
        m->w2_max_batch = env.w2_max;
        m->w2_min_batch = env.w2c_min;
    }
    if (m->NP == 16 && !big) m->adj_help_max_batch = m->n_simd > 0 ? m->n_simd / 2 : 512;      // (one rollout per two SIMDs)
    *out = m;
    return RMX_OK;
}

// Scene.init() (Scene.m:59-119).  Multi-DOF joints whose Q(q) is a product of one-parameter motions are lowered to a chain of
// 1-DOF nodes, parent first, the last one carrying the body and the others massless (E0_ji = I, I_i = 0):
//   JointPlanar        (JointPlanar.m:24-31)          prismatic(b1) . prismatic(b2)
//   JointTranslational (JointTranslational.m:22-26)   prismatic(x) . prismatic(y) . prismatic(z)
//   JointUniversal     (JointUniversal.m:71-74)       revolute(x) . revolute(y)            R = X1(q1) Y2(q2)
//   JointFree2D        (JointFree2D.m:20-33)          prismatic(x) . prismatic(y) . revolute(z)   Q = [Rz(q3) [q1;q2;0]]
// Same world transforms, coordinates and velocities, hence the same M, f, K, D; DOF k of joint j keeps the reference's reduced
// index idxR(k) = nr + k with joints counted from the last listed to the first (Joint.countDofs, Joint.m:149-158).
extern "C" int rmx_model_create(const rmx_model_desc* d, int device, rmx_model** out) {
    if (!d || !out) return fail(RMX_E_INVALID, "null argument");
    const int n = d->njoints;
    if (n < 1 || n > BIG_MAXN) return fail(RMX_E_INVALID, "njoints must be in [1," + std::to_string(BIG_MAXN) + "]");
    if (!d->parent || !d->type || !d->axis || !d->E0_pj || !d->E0_ji || !d->I_i)
        return fail(RMX_E_INVALID, "parent/type/axis/E0_pj/E0_ji/I_i are required");
    bool composite = false;
    for (int i = 0; i < n; ++i) {
        if (d->type[i] < 0 || d->type[i] > RMX_JOINT_FREE3D) return fail(RMX_E_INVALID, "unsupported joint type");
        if (d->type[i] > RMX_JOINT_PRISMATIC) composite = true;
        if (i > 0 && (d->parent[i] < 0 || d->parent[i] >= i)) return fail(RMX_E_INVALID, "joints must be listed parent-before-child with a single root");
    }
    if (!composite && !d->qRestR) return model_create_flat(d, nullptr, nullptr, device, out);

    struct Sub { int type; double ax[3]; };
    auto subs_of = [&](int L, std::vector<Sub>& v) -> bool {
        v.clear();
        const double ex[3] = {1, 0, 0}, ey[3] = {0, 1, 0}, ez[3] = {0, 0, 1};
        auto add = [&](int t, const double* a) { v.push_back(Sub{t, {a[0], a[1], a[2]}}); };
        switch (d->type[L]) {
            case RMX_JOINT_PLANAR:
                if (d->plane) { add(RMX_JOINT_PRISMATIC, d->plane + 6 * L); add(RMX_JOINT_PRISMATIC, d->plane + 6 * L + 3); }
                else { add(RMX_JOINT_PRISMATIC, ex); add(RMX_JOINT_PRISMATIC, ey); }     // JointPlanar.m:13-15 default plane
                break;
            case RMX_JOINT_TRANSLATIONAL: add(RMX_JOINT_PRISMATIC, ex); add(RMX_JOINT_PRISMATIC, ey); add(RMX_JOINT_PRISMATIC, ez); break;
            case RMX_JOINT_UNIVERSAL: add(RMX_JOINT_REVOLUTE, ex); add(RMX_JOINT_REVOLUTE, ey); break;
            case RMX_JOINT_FREE2D: add(RMX_JOINT_PRISMATIC, ex); add(RMX_JOINT_PRISMATIC, ey); add(RMX_JOINT_REVOLUTE, ez); break;
            case RMX_JOINT_FREE3D: add(RMX_JOINT_PRISMATIC, ex); add(RMX_JOINT_PRISMATIC, ey); add(RMX_JOINT_PRISMATIC, ez);   // fallthrough
            case RMX_JOINT_SPHERICAL: add(RMX_JOINT_REVOLUTE, ex); add(RMX_JOINT_REVOLUTE, ey); add(RMX_JOINT_REVOLUTE, ez); break;   // chart XYZ
            default: add(d->type[L], d->axis + 3 * L); break;
        }
        return true;
    };
    // reference numbering of every DOF
    std::vector<int> base(n), ndof(n);
    std::vector<Sub> sv;
    int nr = 0;
    for (int L = n - 1; L >= 0; --L) {
        subs_of(L, sv);
        ndof[L] = d->type[L] == RMX_JOINT_FIXED ? 0 : (int)sv.size();
        base[L] = nr;
        nr += ndof[L];
    }
    std::vector<int> parent, type, idx, last(n), sph_first;
    std::vector<double> axis, E0_pj, E0_ji, I_i, qRest, tau, stiff, damp, qLimL, qLimU, qLimK, qLimD;
    const double I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int L = 0; L < n; ++L) {
        subs_of(L, sv);
        if (d->type[L] == RMX_JOINT_SPHERICAL || d->type[L] == RMX_JOINT_FREE3D)
            sph_first.push_back((int)type.size() + (d->type[L] == RMX_JOINT_FREE3D ? 3 : 0));
        for (size_t k = 0; k < sv.size(); ++k) {
            const bool fin = k + 1 == sv.size();
            parent.push_back(k == 0 ? (d->parent[L] < 0 ? -1 : last[d->parent[L]]) : (int)type.size() - 1);
            type.push_back(sv[k].type);
            axis.insert(axis.end(), sv[k].ax, sv[k].ax + 3);
            const double* epj = k == 0 ? d->E0_pj + 16 * L : I16;
            const double* eji = fin ? d->E0_ji + 16 * L : I16;
            E0_pj.insert(E0_pj.end(), epj, epj + 16);
            E0_ji.insert(E0_ji.end(), eji, eji + 16);
            for (int c = 0; c < 6; ++c) I_i.push_back(fin ? d->I_i[6 * L + c] : 0.0);
            const int ri = base[L] + (int)k;
            idx.push_back(sv[k].type == RMX_JOINT_FIXED ? -1 : ri);
            qRest.push_back(sv[k].type == RMX_JOINT_FIXED ? 0.0 : d->qRestR ? d->qRestR[ri] : (k == 0 && d->qRest) ? d->qRest[L] : 0.0);
            tau.push_back(d->tau ? d->tau[L] : 0.0);
            stiff.push_back(d->stiffness ? d->stiffness[L] : 0.0);
            damp.push_back(d->damping ? d->damping[L] : 0.0);
            qLimL.push_back(d->qLimL ? d->qLimL[L] : -1e8);
            qLimU.push_back(d->qLimU ? d->qLimU[L] : 1e8);
            qLimK.push_back(d->qLimK ? d->qLimK[L] : 1e8);
            qLimD.push_back(d->qLimD ? d->qLimD[L] : 0.0);
        }
        last[L] = (int)type.size() - 1;
    }
    if ((int)type.size() > BIG_MAXN)
        return fail(RMX_E_INVALID, "the scene needs " + std::to_string(type.size()) + " 1-DOF nodes after lowering its multi-DOF joints; the limit is " + std::to_string(BIG_MAXN));
    rmx_model_desc x{};
    x.njoints = (int)type.size();
    x.parent = parent.data(); x.type = type.data(); x.axis = axis.data();
    x.E0_pj = E0_pj.data(); x.E0_ji = E0_ji.data(); x.I_i = I_i.data();
    x.qRest = qRest.data(); x.tau = tau.data(); x.stiffness = stiff.data(); x.damping = damp.data();
    x.qLimL = qLimL.data(); x.qLimU = qLimU.data(); x.qLimK = qLimK.data(); x.qLimD = qLimD.data();
    for (int c = 0; c < 3; ++c) x.grav[c] = d->grav[c];
    rmx_model* m = nullptr;
    const int rc = model_create_flat(&x, idx.data(), &sph_first, device, &m);
    if (rc) return rc;
    // what the caller sees follows ITS listing: body L is the last node of joint L's chain, idxR(L) its first DOF
    std::vector<int> node_of(n), idxL(n);
    for (int L = 0; L < n; ++L) {
        node_of[L] = m->node_of_listing[last[L]];
        idxL[L] = ndof[L] ? base[L] : -1;
    }
    m->nlist = n;
    m->nm = 6 * n;
    m->node_of_listing = node_of;
    m->idx_listing = idxL;
    *out = m;
    return RMX_OK;
}

extern "C" void rmx_model_destroy(rmx_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->dbuf) (void)hipFree(m->dbuf);
    if (m->dcon) (void)hipFree(m->dcon);
    if (m->dsph) (void)hipFree(m->dsph);
    if (m->dgconst) (void)hipFree(m->dgconst);
    if (m->dpf) (void)hipFree(m->dpf);
    delete m;
}

// scene.forces{end+1} = ForceGroundCuboid(body); setTransform / setStiffness / setDamping / setFriction
// (scenesRedMax.m:303-309, ForceGroundCuboid.m:18-48) for every flagged body, each with its own ground frame and constants.
extern "C" int rmx_model_set_ground_contact(rmx_model* m, const rmx_ground_contact* gc) {
    if (!m || !gc || !gc->flags || !gc->sides) return fail(RMX_E_INVALID, "null argument");
    if (!(gc->kn >= 0) || !(gc->kt >= 0) || !(gc->mu >= 0) || !(gc->kd >= 0)) return fail(RMX_E_INVALID, "contact constants must be >= 0");
    if (m->dpf) {
        bool any_flag = false;
        for (int L = 0; L < m->nlist; ++L) any_flag = any_flag || gc->flags[L];
        if (any_flag) return fail(RMX_E_INVALID, "rmx_model_set_ground_contact: the model has point forces (rmx_model_set_point_forces); ForceGroundCuboid together with them is not supported");
    }
    HIPCHK(hipSetDevice(m->device));
    const int MAXN = m->dm.stride;        // node stride of the table: rmx::MAXN, or BIG_MAXN for the one-workgroup kernels (rmx_big.hip)
    std::vector<double> con((size_t)NCON * MAXN, 0.0);
    bool any = false;
    for (int L = 0; L < m->nlist; ++L) {
        const int k = m->node_of_listing[L];
        con[k] = gc->flags[L] ? 1.0 : 0.0;
        any = any || gc->flags[L];
        for (int c = 0; c < 3; ++c) con[(1 + c) * MAXN + k] = gc->sides[3 * L + c];
        // this body's force object: its ground frame (ng = E(1:3,3), xg = E(1:3,4): ForceGroundCuboid.m:56-57) and constants
        const M4 E = from_cm(gc->E_body ? gc->E_body + 16 * (size_t)L : gc->E);
        const double kn = gc->kn_body ? gc->kn_body[L] : gc->kn, kt = gc->kt_body ? gc->kt_body[L] : gc->kt;
        const double mu = gc->mu_body ? gc->mu_body[L] : gc->mu, kd = gc->kd_body ? gc->kd_body[L] : gc->kd;
        if (gc->flags[L] && (!(kn >= 0) || !(kt >= 0) || !(mu >= 0) || !(kd >= 0))) return fail(RMX_E_INVALID, "contact constants must be >= 0");
        for (int c = 0; c < 3; ++c) {
            con[(4 + c) * MAXN + k] = E.a[c][2];
            con[(7 + c) * MAXN + k] = E.a[c][3];
        }
        con[10 * MAXN + k] = kn;
        con[11 * MAXN + k] = kt;
        con[12 * MAXN + k] = mu;
        con[13 * MAXN + k] = kd;
    }
    // the new table is uploaded first and swapped in only on success; kernels of existing batches that may still read the
    // old one (rmx_step_*_async) are drained before it is freed
    void* fresh = nullptr;
    if (any) {
        HIPCHK(hipMalloc(&fresh, con.size() * sizeof(double)));
        const hipError_t e = hipMemcpy(fresh, con.data(), con.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(fresh); return fail(RMX_E_HIP, std::string("hipMemcpy(contact): ") + hipGetErrorString(e)); }
    }
    for (rmx_batch* bb : m->batches) {      // only this model's batches can be reading the old table: other models' streams run on
        const hipError_t es = hipStreamSynchronize(bb->stream);
        if (es != hipSuccess) {
            if (fresh) (void)hipFree(fresh);
            return fail(RMX_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(es));
        }
        bb->async_pending = false;
    }
    if (m->dcon) (void)hipFree(m->dcon);
    m->dcon = fresh;
    m->dm.con = (const double*)fresh;
    return RMX_OK;
}

// scene.forces{end+1} = ForcePointPoint / ForceSpringDamper / ForceCable (scenesRedMax.m:286-288, 332-337, 365-370): the force table of
// the kernels around rmx_pf.h.  Bodies arrive by listing index and go through node_of_listing like the contact flags.
extern "C" int rmx_model_set_point_forces(rmx_model* m, const rmx_point_force* f, int nforces) {
    if (!m || nforces < 0 || (nforces > 0 && !f)) return fail(RMX_E_INVALID, "null argument");
    if (nforces > 0) {
        if (m->big) return fail(RMX_E_INVALID, "rmx_model_set_point_forces: point forces run on the one-wavefront kernels only (models of at most " + std::to_string(rmx::MAXN) + " nodes); this one has " + std::to_string(m->n));
        if (m->dm.con) return fail(RMX_E_INVALID, "rmx_model_set_point_forces: the model has ForceGroundCuboid (rmx_model_set_ground_contact); point forces together with it are not supported");
        if (m->dm.nsph) return fail(RMX_E_INVALID, "rmx_model_set_point_forces: point forces together with JointSpherical / JointFree3D are not supported");
        if (nforces > PF_MAX_FORCES) return fail(RMX_E_INVALID, "rmx_model_set_point_forces: " + std::to_string(nforces) + " forces; the limit is RMX_PF_MAX_FORCES = " + std::to_string(PF_MAX_FORCES));
    }
    std::vector<PfTable> tab(1);
    PfTable& T = tab[0];
    memset(&T, 0, sizeof(T));
    T.nf = nforces;
    int np = 0;
    for (int i = 0; i < nforces; ++i) {
        const rmx_point_force& fi = f[i];
        const std::string who = "rmx_model_set_point_forces: force " + std::to_string(i) + ": ";
        if (fi.kind != RMX_PF_POINTPOINT && fi.kind != RMX_PF_SPRINGDAMPER && fi.kind != RMX_PF_CABLE) return fail(RMX_E_INVALID, who + "unknown kind (RMX_PF_*)");
        if (!fi.body || !fi.x) return fail(RMX_E_INVALID, who + "null body / x");
        if (fi.kind != RMX_PF_CABLE && fi.npts != 2) return fail(RMX_E_INVALID, who + "a point-point force or a spring-damper has exactly 2 points");
        if (fi.npts < 2 || fi.npts > PF_MAX_POINTS) return fail(RMX_E_INVALID, who + std::to_string(fi.npts) + " points; a force has 2 .. RMX_PF_MAX_POINTS = " + std::to_string(PF_MAX_POINTS));
        if (np + fi.npts > PF_MAX_TOTAL) return fail(RMX_E_INVALID, who + "more than RMX_PF_MAX_TOTAL = " + std::to_string(PF_MAX_TOTAL) + " points in all forces of the model");
        if (!std::isfinite(fi.stiffness) || !std::isfinite(fi.damping)) return fail(RMX_E_INVALID, who + "stiffness and damping must be finite");
        if (fi.kind != RMX_PF_POINTPOINT && !(fi.L > 0 && std::isfinite(fi.L))) return fail(RMX_E_INVALID, who + "the rest length L must be > 0 (the host computes it from the initial configuration: Force.init)");
        T.first[i] = np;
        T.kind[i] = fi.kind;
        T.ks[i] = fi.stiffness;
        T.kd[i] = fi.damping;
        T.L[i] = fi.kind == RMX_PF_POINTPOINT ? 1.0 : fi.L;
        for (int k = 0; k < fi.npts; ++k, ++np) {
            const int L = fi.body[k];
            if (L < -1 || L >= m->nlist) return fail(RMX_E_INVALID, who + "body index out of range (listing index, -1 = the world)");
            T.node[np] = L < 0 ? -1 : m->node_of_listing[L];
            for (int c = 0; c < 3; ++c) {
                if (!std::isfinite(fi.x[3 * k + c])) return fail(RMX_E_INVALID, who + "x must be finite");
                T.xl[np][c] = fi.x[3 * k + c];
            }
        }
    }
    for (int i = nforces; i <= PF_MAX_FORCES; ++i) T.first[i] = np;
    HIPCHK(hipSetDevice(m->device));
    // as rmx_model_set_ground_contact: upload first, drain this model's batches, then swap
    void* fresh = nullptr;
    if (nforces > 0) {
        HIPCHK(hipMalloc(&fresh, sizeof(PfTable)));
        const hipError_t e = hipMemcpy(fresh, &T, sizeof(PfTable), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(fresh); return fail(RMX_E_HIP, std::string("hipMemcpy(point forces): ") + hipGetErrorString(e)); }
    }
    for (rmx_batch* bb : m->batches) {
        const hipError_t es = hipStreamSynchronize(bb->stream);
        if (es != hipSuccess) {
            if (fresh) (void)hipFree(fresh);
            return fail(RMX_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(es));
        }
        bb->async_pending = false;
    }
    if (m->dpf) (void)hipFree(m->dpf);
    m->dpf = fresh;
    m->npf = nforces;
    return RMX_OK;
}
// The switch of the taped rollouts with point forces: read by adjoint_model_refusal at every tape call, nothing else happens here.
extern "C" int rmx_model_tape_point_forces(rmx_model* m, int enable) {
    if (!m) return fail(RMX_E_INVALID, "rmx_model_tape_point_forces: null argument");
    if (enable != 0 && enable != 1) return fail(RMX_E_INVALID, "rmx_model_tape_point_forces: enable must be 0 or 1");
    m->tape_pf = enable == 1;
    return RMX_OK;
}
extern "C" int rmx_model_get_tape_point_forces(const rmx_model* m) { return m ? (m->tape_pf ? 1 : 0) : RMX_E_INVALID; }
extern "C" int rmx_model_nr(const rmx_model* m) { return m ? m->nr : RMX_E_INVALID; }
extern "C" int rmx_model_nm(const rmx_model* m) { return m ? m->nm : RMX_E_INVALID; }
extern "C" int rmx_model_idxR(const rmx_model* m, int* idx) {
    if (!m || !idx) return fail(RMX_E_INVALID, "null argument");
    for (int i = 0; i < m->nlist; ++i) idx[i] = m->idx_listing[i];
    return RMX_OK;
}

// Batches that hold cooperative-group buffers (launch_step: serial chains of <= 32 nodes with ForceGroundCuboid), process-wide: the groups of
// ONE launch spin on each other through global memory and must all be resident together, so the SIMDs of a device are DIVIDED among the
// live batches that may run such a launch on it at the same time (two shards of a group on one device, asynchronous BatchSims) - each
// sized as if it owned the device, the partly resident groups of two launches could wait for each other's missing members for ever.
static std::mutex g_coop_mu;
static std::vector<rmx_batch*> g_coop_batches;
static int coop_batches_on_device(int device) {
    std::lock_guard<std::mutex> lk(g_coop_mu);
    int n = 0;
    for (const rmx_batch* b : g_coop_batches) n += (b->m->device == device) ? 1 : 0;
    return n;
}

extern "C" int rmx_batch_create(rmx_model* m, int batch, rmx_batch** out) {
    if (!m || !out || batch < 1) return fail(RMX_E_INVALID, "bad argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(m->device));
    rmx_batch* b = new rmx_batch();
    b->m = m;
    b->B = batch;
    const size_t nb = sizeof(double) * (size_t)batch * std::max(m->nr, 1);
    hipError_t e = hipSuccess;
    auto alloc = [&](void** p, size_t bytes) { if (e == hipSuccess) { e = hipMalloc(p, bytes); if (e == hipSuccess) e = hipMemset(*p, 0, bytes); } };
    alloc((void**)&b->q, nb); alloc((void**)&b->qd, nb); alloc((void**)&b->qp, nb); alloc((void**)&b->qdp, nb);
    alloc((void**)&b->tmpA, nb); alloc((void**)&b->tmpB, nb); alloc((void**)&b->tmpC, nb);
    alloc((void**)&b->started, sizeof(int));
    alloc((void**)&b->it, sizeof(int) * batch); alloc((void**)&b->ls, sizeof(int) * batch); alloc((void**)&b->status, sizeof(int) * batch);
    alloc((void**)&b->resume, sizeof(int) * batch);
    alloc((void**)&b->ticks, sizeof(unsigned long long) * batch);
    if (m->big) {      // trees of more than 64 nodes: the per-rollout workspace of the one-workgroup-per-tree kernels
        b->bigws_stride = big_ws_doubles(m);
        alloc((void**)&b->bigws, sizeof(double) * b->bigws_stride * (size_t)batch);
    }
    if (m->dm.nsph) {   // every JointSpherical starts in CHART_XYZ (JointSpherical.m:33)
        const std::vector<int> c7((size_t)batch * m->dm.nsph, 7);
        if (e == hipSuccess) e = hipMalloc((void**)&b->chart, c7.size() * sizeof(int));
        if (e == hipSuccess) e = hipMemcpy(b->chart, c7.data(), c7.size() * sizeof(int), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&b->ev0);
    if (e == hipSuccess) e = hipEventCreate(&b->ev1);
    if (e != hipSuccess) {
        std::string msg = std::string("rmx_batch_create: ") + hipGetErrorString(e);
        rmx_batch_destroy(b);
        return fail(RMX_E_HIP, msg);
    }
    m->batches.push_back(b);
    *out = b;
    return RMX_OK;
}

extern "C" void rmx_batch_destroy(rmx_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->m->device);
    b->m->batches.erase(std::remove(b->m->batches.begin(), b->m->batches.end(), b), b->m->batches.end());
    {
        std::lock_guard<std::mutex> lk(g_coop_mu);
        g_coop_batches.erase(std::remove(g_coop_batches.begin(), g_coop_batches.end(), b), g_coop_batches.end());
    }
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    hist_free(b);
    for (void* p : {(void*)b->q, (void*)b->qd, (void*)b->qp, (void*)b->qdp, (void*)b->tmpA, (void*)b->tmpB, (void*)b->tmpC,
                    (void*)b->started, (void*)b->it, (void*)b->ls, (void*)b->status, (void*)b->resume, (void*)b->park, (void*)b->xch, (void*)b->xrec, b->gargs, (void*)b->chart, (void*)b->ticks, (void*)b->bigws, b->adjws, b->costws})
        if (p) (void)hipFree(p);
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}
extern "C" int rmx_batch_size(const rmx_batch* b) { return b ? b->B : RMX_E_INVALID; }
extern "C" void* rmx_batch_stream(const rmx_batch* b) { return b ? (void*)b->stream : nullptr; }
extern "C" double rmx_last_step_ms(const rmx_batch* b) { return b ? b->last_ms : -1.0; }
extern "C" const char* rmx_last_step_kernel(const rmx_batch* b) { return (b && b->last_kernel) ? b->last_kernel : ""; }

static int copy_state(rmx_batch* b, const double* q, const double* qd, hipMemcpyKind kind, bool set) {
    if (!b) return fail(RMX_E_INVALID, "null batch");
    HIPCHK(hipSetDevice(b->m->device));
    const size_t nb = sizeof(double) * (size_t)b->B * b->m->nr;
    if (nb == 0) return RMX_OK;
    if (set) {
        if (q) HIPCHK(hipMemcpyAsync(b->q, q, nb, kind, b->stream));
        if (qd) HIPCHK(hipMemcpyAsync(b->qd, qd, nb, kind, b->stream));
        HIPCHK(set_started(b, 0));   // a new state restarts BDF2 with SDIRK2
        if (b->chart && q) {   // the new coordinates are read in CHART_XYZ (rmx_set_charts afterwards says otherwise)
            const std::vector<int> c7((size_t)b->B * b->m->dm.nsph, 7);
            HIPCHK(hipMemcpyAsync(b->chart, c7.data(), c7.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
            HIPCHK(hipStreamSynchronize(b->stream));
        }
    } else {
        if (q) HIPCHK(hipMemcpyAsync((void*)q, b->q, nb, kind, b->stream));
        if (qd) HIPCHK(hipMemcpyAsync((void*)qd, b->qd, nb, kind, b->stream));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    b->async_pending = false;      // the batch's stream has been waited for
    return RMX_OK;
}
extern "C" int rmx_model_nsph(const rmx_model* m) { return m ? m->dm.nsph : RMX_E_INVALID; }
// JointSpherical.chart of every spherical joint and trajectory (reference numbering 1..12); host [batch][nsph]
extern "C" int rmx_get_charts(rmx_batch* b, int* charts) {
    if (!b || !charts) return fail(RMX_E_INVALID, "null argument");
    if (!b->chart) return RMX_OK;
    HIPCHK(hipSetDevice(b->m->device));
    HIPCHK(hipMemcpyAsync(charts, b->chart, sizeof(int) * (size_t)b->B * b->m->dm.nsph, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return RMX_OK;
}
extern "C" int rmx_set_charts(rmx_batch* b, const int* charts) {
    if (!b || !charts) return fail(RMX_E_INVALID, "null argument");
    if (!b->chart) return RMX_OK;
    const size_t nc = (size_t)b->B * b->m->dm.nsph;
    for (size_t i = 0; i < nc; ++i)
        if (charts[i] < 1 || charts[i] > 12) return fail(RMX_E_INVALID, "charts must be in 1..12 (JointSpherical.CHART_*)");
    HIPCHK(hipSetDevice(b->m->device));
    HIPCHK(hipMemcpyAsync(b->chart, charts, sizeof(int) * nc, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return RMX_OK;
}
extern "C" int rmx_set_state(rmx_batch* b, const double* q, const double* qdot) { return copy_state(b, q, qdot, hipMemcpyHostToDevice, true); }
extern "C" int rmx_get_state(rmx_batch* b, double* q, double* qdot) { return copy_state(b, q, qdot, hipMemcpyDeviceToHost, false); }
extern "C" int rmx_set_state_device(rmx_batch* b, const double* q, const double* qdot) { return copy_state(b, q, qdot, hipMemcpyDeviceToDevice, true); }
extern "C" int rmx_get_state_device(rmx_batch* b, double* q, double* qdot) { return copy_state(b, q, qdot, hipMemcpyDeviceToDevice, false); }

#define DISPATCH_NP(NPV, FN, ...)            \
    switch (NPV) {                            \
        case 4: FN##_4(__VA_ARGS__); break;   \
        case 8: FN##_8(__VA_ARGS__); break;   \
        case 16: FN##_16(__VA_ARGS__); break; \
        case 32: FN##_32(__VA_ARGS__); break; \
        default: FN##_64(__VA_ARGS__); break; \
    }


extern "C" int rmx_eval(rmx_batch* b, const double* q, const double* qA, const double* qB, double eta, double* g, double* H) {
    if (!b || !q || !qA || !qB || !g) return fail(RMX_E_INVALID, "null argument");
    if (!(eta > 0)) return fail(RMX_E_INVALID, "eta must be positive");
    rmx_model* m = b->m;
    HIPCHK(hipSetDevice(m->device));
    if (int rc = pending_error_check(b, "rmx_eval")) return rc;
    const size_t nv = (size_t)b->B * m->nr;
    if (nv == 0) return RMX_OK;
    double *dg = nullptr, *dH = nullptr;
    HIPCHK(hipMemcpyAsync(b->tmpA, q, nv * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->tmpB, qA, nv * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->tmpC, qB, nv * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMalloc((void**)&dg, nv * sizeof(double)));
    if (H) {
        hipError_t e = hipMalloc((void**)&dH, nv * m->nr * sizeof(double));
        if (e != hipSuccess) { (void)hipFree(dg); return fail(RMX_E_NOMEM, "hipMalloc(H)"); }
        (void)hipMemsetAsync(dH, 0, nv * m->nr * sizeof(double), b->stream);
    }
    if (m->big) launch_big_eval(m, b, H != nullptr, eta, dg, dH);
    else if (m->dpf) { DISPATCH_NP(m->NP, launch_eval_pf, m, b, H != nullptr, eta, dg, dH); }      // body-to-body forces: the kernels around rmx_pf.h
    // scenes with ForceGroundCuboid or JointSpherical run the extended instantiations (CT), everything else the plain ones
    else if (m->dm.con != nullptr || m->dm.nsph > 0) { DISPATCH_NP(m->NP, launch_eval_ct, m, b, H != nullptr, eta, dg, dH); }
    else { DISPATCH_NP(m->NP, launch_eval, m, b, H != nullptr, eta, dg, dH); }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(g, dg, nv * sizeof(double), hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess && H) e = hipMemcpyAsync(H, dH, nv * m->nr * sizeof(double), hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    (void)hipFree(dg);
    if (dH) (void)hipFree(dH);
    if (e != hipSuccess) return fail(RMX_E_HIP, std::string("rmx_eval: ") + hipGetErrorString(e));
    return RMX_OK;
}

extern "C" int rmx_eval_mfd(rmx_batch* b, const double* q, const double* qdot, double* M, double* f, double* D) {
    if (!b || !q || !qdot || !M || !f || !D) return fail(RMX_E_INVALID, "null argument");
    rmx_model* m = b->m;
    if (m->dpf) return fail(RMX_E_INVALID, "rmx_eval_mfd: models with point forces (rmx_model_set_point_forces) run rmx_eval / rmx_step_bdf1/bdf2 / rmx_energy only");
    if (m->big) return rmx_compute_values(b, q, qdot, nullptr, M, f, D, nullptr, nullptr, nullptr);   // no M / D kernel of their own: from H
    HIPCHK(hipSetDevice(m->device));
    if (int rc = pending_error_check(b, "rmx_eval_mfd")) return rc;
    const size_t nv = (size_t)b->B * m->nr, nn = nv * m->nr;
    if (nv == 0) return RMX_OK;
    double* buf = nullptr;
    HIPCHK(hipMalloc((void**)&buf, (2 * nn + nv) * sizeof(double)));
    double *dM = buf, *dD = buf + nn, *df = buf + 2 * nn;
    hipError_t e = hipMemsetAsync(buf, 0, (2 * nn + nv) * sizeof(double), b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b->tmpA, q, nv * sizeof(double), hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b->tmpB, qdot, nv * sizeof(double), hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess) {
        // (con alone, not con || nsph as eval / step / energy: k_eval_mfd sets the Euler charts up itself in BOTH instantiations, CT adds only the contact terms)
        if (m->dm.con) { DISPATCH_NP(m->NP, launch_mfd_ct, m, b, dM, df, dD); }
        else { DISPATCH_NP(m->NP, launch_mfd, m, b, dM, df, dD); }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(M, dM, nn * sizeof(double), hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(D, dD, nn * sizeof(double), hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f, df, nv * sizeof(double), hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    (void)hipFree(buf);
    if (e != hipSuccess) return fail(RMX_E_HIP, std::string("rmx_eval_mfd: ") + hipGetErrorString(e));
    return RMX_OK;
}

// computeValues' full output from evaluations of H(eta; v) = M + dMdq v - eta D - eta^2 K at fixed (q, qdot): see include/redmax_hip.h
extern "C" int rmx_compute_values(rmx_batch* b, const double* q, const double* qdot, const double* v, double* M, double* f, double* D,
                                  double* K, double* dMv, double* dMdq) {
    if (!b || !q || !qdot) return fail(RMX_E_INVALID, "null argument");
    if (dMv && !v) return fail(RMX_E_INVALID, "rmx_compute_values: dMv needs v");
    rmx_model* m = b->m;
    if (m->dpf) return fail(RMX_E_INVALID, "rmx_compute_values: models with point forces (rmx_model_set_point_forces) run rmx_eval / rmx_step_bdf1/bdf2 / rmx_energy only");
    const size_t nr = (size_t)m->nr, nv = (size_t)b->B * nr, nn = nv * nr;
    if (nv == 0) return RMX_OK;
    std::vector<double> qA(nv), qB(nv), g(nv), H1(nn), Mt, Dt, ft;
    auto eval_at = [&](const double eta, const double* vv, std::vector<double>& Hout) -> int {
        for (size_t i = 0; i < nv; ++i) {
            qA[i] = q[i] - eta * qdot[i];
            qB[i] = vv ? q[i] - vv[i] : q[i];
        }
        return rmx_eval(b, q, qA.data(), qB.data(), eta, g.data(), Hout.data());
    };
    if (int rc = eval_at(1.0, nullptr, H1)) return rc;           // H1 = M - D - K ; g = -f
    if (f) for (size_t i = 0; i < nv; ++i) f[i] = -g[i];
    if (M || D || K) {
        if (!M) { Mt.resize(nn); M = Mt.data(); }
        if (!D) { Dt.resize(nn); D = Dt.data(); }
        if (!m->big) {
            ft.resize(nv);
            if (int rc = rmx_eval_mfd(b, q, qdot, M, ft.data(), D)) return rc;
            if (K) for (size_t i = 0; i < nn; ++i) K[i] = (M[i] - D[i]) - H1[i];
        } else {
            // No M / D kernel at this size: the pieces are taken apart from H(e), H(2 e), H(e / 2):
            //   3 H(e) - H(2 e) - 2 H(e / 2) = 3/2 e^2 K ;  H(e) - H(2 e) = e D + 3 e^2 K ;  M = H(e) + e D + e^2 K.
            // H(e) carries roundoff of order eps (|M| + e |D| + e^2 |K|), so a piece comes out with good RELATIVE accuracy only from a
            // triple whose e makes it as large as the others: a first triple at e = 1 gives the scales, then K is taken at
            // e_K ~ sqrt(|M| / |K|), D at e_D ~ min(|M| / |D|, e_K) and M at min(1, e_K, e_D) (powers of two: the scalings are exact; a triple
            // whose e is 1 again is not repeated).  At e = 1 alone D and K would carry an ABSOLUTE error of ~10 eps |M| per entry.
            struct Triple { double e = 0.0; std::vector<double> H, H2, Hh; };
            auto run = [&](Triple& t, const double e, const std::vector<double>* have) -> int {
                t.e = e;
                if (have) t.H = *have;
                else { t.H.resize(nn); if (int rc = eval_at(e, nullptr, t.H)) return rc; }
                t.H2.resize(nn);
                t.Hh.resize(nn);
                if (int rc = eval_at(2.0 * e, nullptr, t.H2)) return rc;
                return eval_at(0.5 * e, nullptr, t.Hh);
            };
            auto k_of = [](const Triple& t, size_t i) { return (3.0 * t.H[i] - t.H2[i] - 2.0 * t.Hh[i]) * (2.0 / 3.0) / (t.e * t.e); };
            auto d_of = [](const Triple& t, size_t i, double k) { return ((t.H[i] - t.H2[i]) - 3.0 * t.e * t.e * k) / t.e; };
            Triple t1, tK, tD;
            if (int rc = run(t1, 1.0, &H1)) return rc;
            double nM = 0.0, nD = 0.0, nK = 0.0;
            for (size_t i = 0; i < nn; ++i) {
                const double k = k_of(t1, i), d = d_of(t1, i, k), mm = H1[i] + d + k;
                nM += mm * mm; nD += d * d; nK += k * k;
            }
            auto pow2 = [](double x) { return std::ldexp(1.0, (int)std::lround(std::log2(std::min(std::max(x, 0x1p-20), 0x1p20)))); };
            const double eK = nK > 0.0 ? pow2(std::sqrt(std::sqrt(nM / nK))) : 1.0;      // (nM, nD, nK are squared norms)
            const double eD = nD > 0.0 ? std::min(pow2(std::sqrt(nM / nD)), eK) : 1.0;      // (beyond e_K the e |K| term of the roundoff grows)
            const double eM = std::min(1.0, std::min(eK, eD));
            const Triple* pK = &t1;
            if (eK != 1.0) { if (int rc = run(tK, eK, nullptr)) return rc; pK = &tK; }
            const Triple* pD = eD == 1.0 ? &t1 : (eD == eK ? pK : &tD);
            if (pD == &tD) { if (int rc = run(tD, eD, nullptr)) return rc; }
            const std::vector<double>* HM = eM == 1.0 ? &H1 : (eM == eK ? &pK->H : &pD->H);      // (eM is 1, eK or eD)
            for (size_t i = 0; i < nn; ++i) {
                const double k = k_of(*pK, i), d = d_of(*pD, i, k);
                M[i] = (*HM)[i] + eM * d + eM * eM * k;
                D[i] = d;
                if (K) K[i] = k;
            }
        }
    }
    if (dMv) {
        std::vector<double> Hv(nn);
        if (int rc = eval_at(1.0, v, Hv)) return rc;
        for (size_t i = 0; i < nn; ++i) dMv[i] = Hv[i] - H1[i];
    }
    if (dMdq) {
        std::vector<double> Hk(nn), ek(nv);
        for (size_t k = 0; k < nr; ++k) {
            for (size_t i = 0; i < nv; ++i) ek[i] = (i % nr == k) ? 1.0 : 0.0;
            if (int rc = eval_at(1.0, ek.data(), Hk)) return rc;
            for (size_t t = 0; t < (size_t)b->B; ++t)
                for (size_t i = 0; i < nr; ++i)
                    for (size_t r = 0; r < nr; ++r)      // dMdq(r, k, i) = (dMdq(:,:,i) e_k)(r) = column i of H(e_k) - H(0)
                        dMdq[t * nr * nr * nr + r + nr * (k + nr * i)] = Hk[t * nr * nr + i * nr + r] - H1[t * nr * nr + i * nr + r];
        }
    }
    return RMX_OK;
}

using rmx_select::AdjKernel;
using rmx_select::StepKernel;
// what rmx_select.h's choice of kernel depends on, from the model and its device
static rmx_select::StepTraits step_traits(const rmx_model* m) {
    rmx_select::StepTraits t;
    t.NP = m->NP; t.n = m->dm.n; t.big = m->big;
    t.point_forces = m->dpf != nullptr; t.contact = m->dm.con != nullptr; t.spherical = m->dm.nsph > 0;
    t.is_chain = m->dm.is_chain; t.gconst = m->dm.gconst != nullptr;
    t.n_simd = m->n_simd; t.coop_g = COOP_G;
    t.w2_max_batch = m->w2_max_batch; t.w2_min_batch = m->w2_min_batch;
    t.gconst_min_batch = m->gconst_min_batch; t.adj_help_max_batch = m->adj_help_max_batch;
    return t;
}

static int make_opts(const rmx_batch* b, const rmx_opts* o, DevOpts& d) {
    rmx_opts def;
    rmx_opts_default(&def);
    if (!o) o = &def;
    if (!(o->h > 0)) return fail(RMX_E_INVALID, "opts.h must be positive");
    d.h = o->h;
    d.tol = o->tol;
    d.dxMax = o->dxMax;
    d.iterMax = o->iterMaxPerDof * b->m->nr;    // iterMax = 10*length(xInit) (:97)
    d.iterLsMax = o->iterLsMax;
    d.lu_mode = o->lu_mode;
    d.comp = o->compensated ? 1.0 : 0.0;
    if (o->ls_fail_limit < 0) return fail(RMX_E_INVALID, "opts.ls_fail_limit must be >= 0");
    d.lsFailLimit = o->ls_fail_limit;
    d.parkHalv = 0;
    d.coopTicks = b->m->coop_ticks;
    return RMX_OK;
}

static int launch_step(rmx_batch* b, const rmx_opts* opts, int nsteps, int integ, bool with_stats, double* dT, double* dV,
                       double* dQ = nullptr, double* dQd = nullptr, int* dC = nullptr) {
    const rmx_model* m = b->m;
    DevOpts o;
    int rc = make_opts(b, opts, o);
    if (rc) return rc;
    StepArgs a{};
    a.B = b->B;
    a.nsteps = nsteps;
    a.q = b->q; a.qd = b->qd; a.qp = b->qp; a.qdp = b->qdp; a.started = b->started;
    a.it = with_stats ? b->it : nullptr; a.ls = b->ls; a.status = b->status;
    a.histT = dT; a.histV = dV;
    a.histQ = dQ; a.histQd = dQd; a.histC = dC;
    a.chart = b->chart;
    a.resume = b->resume;
    a.ticks = b->ticks;
    rc = pending_error_check(b, "rmx_step");
    if (rc) return rc;
    const rmx_select::StepKnobs knobs = rmx_select::knobs_from_env();
    const rmx_select::StepPlan plan = rmx_select::select_step(step_traits(m), b->B, integ, dT != nullptr, knobs);
    b->last_kernel = plan.label;
    // Park and relaunch (rmx_device.h CoopCtx): serial chains of <= 32 nodes with ForceGroundCuboid.  A rollout whose Newton solve keeps
    // running out its line searches is parked by the launch with the contact terms and finished by groups of COOP_G wavefronts that
    // evaluate the reference's trial points side by side - same decisions, same results, the launch no longer waits for one wavefront
    // walking through 20 trials 320 times.  RMX_PARK_HALVINGS=0 switches it off (one wavefront per rollout throughout).
    o.parkHalv = plan.park_halvings;
    if (plan.parks) {
        // buffers for the most groups a launch of this batch can ever hold (it alone on the device); each under its own check, so that a
        // failed allocation leaves nothing half set up for the next call
        const int cap = std::min(b->B, m->n_simd / COOP_G);
        if (!b->park) HIPCHK(hipMalloc((void**)&b->park, sizeof(int) * (2 + 4 * (size_t)b->B)));
        if (!b->xch) HIPCHK(hipMalloc((void**)&b->xch, sizeof(unsigned) * COOP_WORDS * (size_t)cap));
        if (!b->xrec) HIPCHK(hipMalloc((void**)&b->xrec, sizeof(unsigned long long) * 2 * COOP_REC * (size_t)cap));
        {
            std::lock_guard<std::mutex> lk(g_coop_mu);
            if (std::find(g_coop_batches.begin(), g_coop_batches.end(), b) == g_coop_batches.end()) g_coop_batches.push_back(b);
        }
        // the groups of this launch: all resident at once (one 512-register wavefront per SIMD) beside those of every other live batch that
        // may be stepping on this device at the same time
        b->ngroups = std::max(1, std::min(cap, (m->n_simd / COOP_G) / std::max(1, coop_batches_on_device(m->device))));
        HIPCHK(hipMemsetAsync(b->park, 0, sizeof(int) * (2 + 4 * (size_t)b->B), b->stream));
        HIPCHK(hipMemsetAsync(b->xch, 0, sizeof(unsigned) * COOP_WORDS * (size_t)b->ngroups, b->stream));
        HIPCHK(hipMemsetAsync(b->xrec, 0, sizeof(unsigned long long) * 2 * COOP_REC * (size_t)b->ngroups, b->stream));
        a.park = b->park;
        a.xch = b->xch;
        a.xrec = b->xrec;
        a.ngroups = b->ngroups;
        a.coop_map = knobs.coop_map;
    }
    a.w2_noahead = knobs.w2_runahead ? 0 : 1;
    a.pairc = knobs.pairc ? 1 : 0;
    // RMX_GROUND_FUSED: 1 (default) ONE launch for the whole call - the rollouts (free flight, then the steps with the contact terms)
    // and, behind them in dispatch order, the cooperative groups that pick the parked rollouts up as they appear: no launch
    // boundary holds a rollout back (part_ground32.hip k_ground32); 2 the groups in a second launch; 0 three launches (lean, contact
    // terms, groups); 3 measurement aid (the groups as a second launch of k_ground32)
    a.fused = plan.fused;
    if (plan.kernel == StepKernel::Ground32 && !b->gargs) HIPCHK(hipMalloc(&b->gargs, RMX_GARGS_BYTES));
    // the per-rollout tick counters: the kernels of a call ADD their share (a contact-capable call is up to three launches); the
    // headline kernel (one launch, part_pair32.hip) stores its count instead, and the fill dispatch ahead of a 0.8 ms
    // launch is saved
    if (!plan.stores_ticks) HIPCHK(hipMemsetAsync(b->ticks, 0, sizeof(unsigned long long) * b->B, b->stream));
    HIPCHK(hipEventRecord(b->ev0, b->stream));
    switch (plan.kernel) {
        case StepKernel::Big: launch_big_step(m, b, integ, o, a); break;
        case StepKernel::PointForces: DISPATCH_NP(m->NP, launch_step_pf, m, b, integ, o, a); break;
        case StepKernel::Ct: DISPATCH_NP(m->NP, launch_step_ct, m, b, integ, o, a, plan.contact_pass); break;
        case StepKernel::Ground32: launch_step_ground_32(m, b, integ, o, a); break;
        case StepKernel::StepPair32:      // free flight in the lean launch, the rest of the steps around newton_pair
            launch_step_ct_32(m, b, integ, o, a, false);
            launch_step_pair_32(m, b, integ, o, a);
            break;
        case StepKernel::W2_64: launch_step_w2_64(m, b, integ, o, a, plan.fullchain, plan.fulln, plan.energy); break;
        case StepKernel::PairChain32: launch_step_pairchain_32(m, b, o, a, plan.energy); break;
        case StepKernel::W2Chain32: launch_step_w2c_32(m, b, o, a); break;
        case StepKernel::FullChain:
            if (m->NP == 16) launch_step_fullchain_16(m, b, integ, o, a);
            else if (m->NP == 32) launch_step_fullchain_32(m, b, integ, o, a);
            else launch_step_fullchain_64(m, b, integ, o, a);
            break;
        case StepKernel::Gconst64: launch_step_gconst_64(m, b, integ, o, a, plan.fulln); break;
        case StepKernel::FullN64: launch_step_fulln_64(m, b, integ, o, a); break;
        case StepKernel::Plain: DISPATCH_NP(m->NP, launch_step_plain, m, b, integ, o, a); break;
    }
    // BDF2 keeps (q, qdot) of step k-1 in qp/qdp.  BDF1 steps do not maintain them (and, with JointSpherical, may leave q in
    // another Euler chart than qp), so a BDF1 call invalidates the multistep history: the next rmx_step_bdf2 restarts with
    // SDIRK2, as a fresh driverRedMaxBDF2 run from that state would (driverRedMaxBDF2.m:64-88).
    HIPCHK(set_started(b, integ == INTEG_BDF2 ? 1 : 0));   // BDF2: any non-zero value
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(b->ev1, b->stream));
    return RMX_OK;
}

// ---- the per-step record of a step call (Scene.saveHistory, Scene.m:134-161), in device buffers that live on the batch
static void hist_release(rmx_batch* b) { b->hist = rmx_batch::Hist{}; }      // forget the record, keep the buffers
static void hist_free(rmx_batch* b) {                                          // batch teardown
    for (void* p : {(void*)b->hpool.T, (void*)b->hpool.V, (void*)b->hpool.Q, (void*)b->hpool.Qd, (void*)b->hpool.C})
        if (p) (void)hipFree(p);
    b->hpool = rmx_batch::HistPool{};
    hist_release(b);
}
template <class T>
static hipError_t pool_grow(rmx_batch* b, T*& p, size_t& cap, size_t need, T** second = nullptr) {
    if (need <= cap) return hipSuccess;
    // growing frees the old buffer: whatever this batch still has in flight may be writing it
    hipError_t e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) return e;
    if (p) (void)hipFree(p);
    p = nullptr;
    if (second && *second) { (void)hipFree(*second); *second = nullptr; }
    cap = 0;
    e = hipMalloc((void**)&p, need * sizeof(T));
    if (e == hipSuccess && second) e = hipMalloc((void**)second, need * sizeof(T));
    if (e == hipSuccess) cap = need;
    return e;
}
static int hist_alloc(rmx_batch* b, int nsteps, int record) {
    hist_release(b);
    const rmx_model* m = b->m;
    const size_t nh = (size_t)nsteps * b->B, nq = nh * m->nr, nc = nh * (size_t)m->dm.nsph;
    hipError_t e = hipSuccess;
    if ((record & RMX_REC_ENERGY) && nh) {
        e = pool_grow(b, b->hpool.T, b->hpool.capH, nh, &b->hpool.V);
        if (e == hipSuccess) { b->hist.T = b->hpool.T; b->hist.V = b->hpool.V; }
    }
    if (e == hipSuccess && (record & RMX_REC_STATE) && nq) {
        e = pool_grow(b, b->hpool.Q, b->hpool.capQ, nq, &b->hpool.Qd);
        if (e == hipSuccess) { b->hist.Q = b->hpool.Q; b->hist.Qd = b->hpool.Qd; }
    }
    // models with spherical joints run the extended (CT) step kernels, which record the chart after every step
    if (e == hipSuccess && (record & RMX_REC_CHARTS) && nc) {
        e = pool_grow<int>(b, b->hpool.C, b->hpool.capC, nc);
        if (e == hipSuccess) b->hist.C = b->hpool.C;
    }
    if (e != hipSuccess) {
        hist_free(b);
        (void)hipGetLastError();      // the failed allocation must not be taken for a failed launch later on
        return fail(RMX_E_NOMEM, std::string("hipMalloc(per-step record): ") + hipGetErrorString(e));
    }
    b->hist.nsteps = nsteps;
    return RMX_OK;
}
// rows of `width` bytes, `rows` of them: device (dense) -> host array whose rows are `dpitch` bytes apart
static hipError_t rows_out(void* dst, size_t dpitch, const void* src, size_t width, size_t rows, hipStream_t st) {
    if (!width || !rows) return hipSuccess;
    if (dpitch == width) return hipMemcpyAsync(dst, src, width * rows, hipMemcpyDeviceToHost, st);
    return hipMemcpy2DAsync(dst, dpitch, src, width, width, rows, hipMemcpyDeviceToHost, st);
}
// Enqueue the copies of the record into host arrays laid out for `pitchB` trajectories per step, this batch's first trajectory
// being number `first` of them (pitchB = B, first = 0 for a batch on its own; a shard of an rmx_group otherwise).
static int hist_copy_out(rmx_batch* b, const rmx_history* h, size_t pitchB, size_t first) {
    if (!h) return RMX_OK;
    const rmx_model* m = b->m;
    const size_t K = (size_t)b->hist.nsteps, B = (size_t)b->B, nr = (size_t)m->nr, ns = (size_t)m->dm.nsph;
    if ((h->T == nullptr) != (h->V == nullptr)) return fail(RMX_E_INVALID, "history T and V must be given together");
    if ((h->q == nullptr) != (h->qdot == nullptr)) return fail(RMX_E_INVALID, "history q and qdot must be given together");
    if (K && B && ((h->T && !b->hist.T) || (h->q && nr && !b->hist.Q) || (h->charts && ns && !b->hist.C)))
        return fail(RMX_E_INVALID, "this part of the per-step record was not recorded by the step call (RMX_REC_*)");
    hipError_t e = hipSuccess;
    if (h->T) {
        e = rows_out(h->T + first, pitchB * 8, b->hist.T, B * 8, K, b->stream);
        if (e == hipSuccess) e = rows_out(h->V + first, pitchB * 8, b->hist.V, B * 8, K, b->stream);
    }
    if (e == hipSuccess && h->q && nr) {
        e = rows_out(h->q + first * nr, pitchB * nr * 8, b->hist.Q, B * nr * 8, K, b->stream);
        if (e == hipSuccess) e = rows_out(h->qdot + first * nr, pitchB * nr * 8, b->hist.Qd, B * nr * 8, K, b->stream);
    }
    if (e == hipSuccess && h->charts && ns) e = rows_out(h->charts + first * ns, pitchB * ns * 4, b->hist.C, B * ns * 4, K, b->stream);
    if (e != hipSuccess) return fail(RMX_E_HIP, std::string("copying the per-step record: ") + hipGetErrorString(e));
    return RMX_OK;
}
static hipError_t stats_copy_out(rmx_batch* b, const rmx_stats* st) {
    hipError_t e = hipSuccess;
    if (!st) return e;
    if (st->newton_iters) e = hipMemcpyAsync(st->newton_iters, b->it, sizeof(int) * b->B, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess && st->ls_halvings) e = hipMemcpyAsync(st->ls_halvings, b->ls, sizeof(int) * b->B, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess && st->status) e = hipMemcpyAsync(st->status, b->status, sizeof(int) * b->B, hipMemcpyDeviceToHost, b->stream);
    return e;
}
// the device flag that tells BDF2 whether (q, qdot) of step k-1 are in place: written only when its value changes (one fill dispatch
// less on the stream of every step call: ~5 us of a 0.8 ms launch at the driver's --steps 20)
static hipError_t set_started(rmx_batch* b, const int v) {
    if (b->started_host == v) return hipSuccess;
    const hipError_t e = hipMemsetAsync(b->started, v, sizeof(int), b->stream);
    b->started_host = e == hipSuccess ? v : -1;
    return e;
}
// Wait for a stream by polling (hipStreamSynchronize's wake-up costs ~10 us: 1 - 2 % of the 0.8 ms launches of configs[1] and [3]);
// after RMX_WAIT_SPIN_MS milliseconds (default 2; polling through the 5.8 / 16.6 ms launches of configs[2] / [4] gained nothing
// measurable) the host thread blocks as before.
static hipError_t wait_stream_short(hipStream_t stream) {
    static const int spin_ms = [] { const char* e = getenv("RMX_WAIT_SPIN_MS"); const int v = e ? atoi(e) : 2; return v < 0 ? 0 : v; }();
    hipError_t es = hipErrorNotReady;
    for (const auto t0 = std::chrono::steady_clock::now(); std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(spin_ms);) {
        es = hipStreamQuery(stream);
        if (es != hipErrorNotReady) break;
    }
    if (es == hipErrorNotReady) es = hipStreamSynchronize(stream);
    else (void)hipGetLastError();      // (hipStreamQuery leaves hipErrorNotReady as the thread's last error while it polls)
    return es;
}

static void take_event_time(rmx_batch* b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, b->ev0, b->ev1) == hipSuccess) b->last_ms = ms;
}
// The tail of a synchronous call, in three pieces its callers put their copies between.  The timed part: record ev0, launch, check,
// record ev1.  launch() enqueues the kernels and returns hipSuccess, or the error that kept it from launching; e is the call's
// verdict so far (nothing is enqueued behind a failure).
template <class Launch>
static hipError_t timed_launch(rmx_batch* b, hipError_t e, Launch&& launch) {
    if (e == hipSuccess) e = hipEventRecord(b->ev0, b->stream);
    if (e == hipSuccess) e = launch();
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(b->ev1, b->stream);
    return e;
}
// ... the wait: short on success; after a failure the stream is drained where arrays of the caller must outlive their copies
static hipError_t wait_or_drain(rmx_batch* b, hipError_t e, const bool drain = true) {
    if (e == hipSuccess) e = wait_stream_short(b->stream);
    else if (drain) (void)hipStreamSynchronize(b->stream);
    return e;
}
// ... and the verdict: "who: text" of a HIP error, or the kernel time of a call that went through
static int call_result(rmx_batch* b, const hipError_t e, const std::string& who) {
    if (e != hipSuccess) return fail(RMX_E_HIP, who + ": " + hipGetErrorString(e));
    take_event_time(b);
    return RMX_OK;
}

static int step_sync(rmx_batch* b, const rmx_opts* opts, int nsteps, rmx_stats* st, double* hT, double* hV, int integ,
                     double* hQ = nullptr, double* hQd = nullptr, int* hC = nullptr) {
    if (!b) return fail(RMX_E_INVALID, "null batch");
    if (nsteps < 0) return fail(RMX_E_INVALID, "nsteps < 0");
    if ((hT == nullptr) != (hV == nullptr)) return fail(RMX_E_INVALID, "hist_T and hist_V must be given together");
    if ((hQ == nullptr) != (hQd == nullptr)) return fail(RMX_E_INVALID, "history q and qdot must be given together");
    rmx_model* m = b->m;
    HIPCHK(hipSetDevice(m->device));
    if (nsteps == 0 || m->nr == 0) return RMX_OK;
    if (b->async_pending && (b->hist.T || b->hist.Q || b->hist.C))
        // a recorded *_async launch is still in flight and its record has not been read: a synchronous call would replace it
        // (include/redmax_hip.h "Asynchronous stepping": only *_async / rmx_sync / rmx_stats_reset until rmx_sync)
        return fail(RMX_E_INVALID, "a recorded asynchronous step is pending on this batch: rmx_sync / rmx_history_read first");
    int rc = hist_alloc(b, nsteps, (hT ? RMX_REC_ENERGY : 0) | (hQ ? RMX_REC_STATE : 0) | (hC ? RMX_REC_CHARTS : 0));
    if (rc) return rc;
    const bool ws = st != nullptr;
    if (ws) {
        (void)hipMemsetAsync(b->it, 0, sizeof(int) * b->B, b->stream);
        (void)hipMemsetAsync(b->ls, 0, sizeof(int) * b->B, b->stream);
        (void)hipMemsetAsync(b->status, 0, sizeof(int) * b->B, b->stream);
    }
    rc = launch_step(b, opts, nsteps, integ, ws, b->hist.T, b->hist.V, b->hist.Q, b->hist.Qd, b->hist.C);
    hipError_t e = hipSuccess;
    if (rc == RMX_OK) {
        const rmx_history h{hT, hV, hQ, hQd, hC};
        rc = hist_copy_out(b, &h, (size_t)b->B, 0);
        if (rc == RMX_OK) {
            if (ws) e = stats_copy_out(b, st);
            if (e == hipSuccess) e = wait_stream_short(b->stream);
            if (e == hipSuccess) {
                take_event_time(b);
                b->async_pending = false;      // the stream has been waited for: nothing of this batch is in flight any more
            }
        }
    }
    hist_release(b);                            // a synchronous call has delivered its record: nothing to keep (the buffers stay)
    if (rc) return rc;
    if (e != hipSuccess) return fail(RMX_E_HIP, std::string("rmx_step: ") + hipGetErrorString(e));
    return RMX_OK;
}

// Scene.saveHistory (Scene.m:134-161) for every step and trajectory: t is k*h, the rest comes back here.
extern "C" int rmx_step_history(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, rmx_stats* stats, const rmx_history* hist) {
    if (integrator != 1 && integrator != 2) return fail(RMX_E_INVALID, "integrator must be 1 (BDF1) or 2 (BDF2)");
    if (!hist) return fail(RMX_E_INVALID, "null history");
    return step_sync(b, opts, nsteps, stats, hist->T, hist->V, integrator == 1 ? INTEG_BDF1 : INTEG_BDF2, hist->q, hist->qdot, hist->charts);
}

extern "C" int rmx_step_bdf1(rmx_batch* b, const rmx_opts* opts, int nsteps, rmx_stats* stats, double* hist_T, double* hist_V) {
    return step_sync(b, opts, nsteps, stats, hist_T, hist_V, INTEG_BDF1);
}
extern "C" int rmx_step_bdf2(rmx_batch* b, const rmx_opts* opts, int nsteps, rmx_stats* stats, double* hist_T, double* hist_V) {
    return step_sync(b, opts, nsteps, stats, hist_T, hist_V, INTEG_BDF2);
}

extern "C" int rmx_step_euler(rmx_batch* b, double h, int nsteps, double* hT, double* hV) {
    if (!b) return fail(RMX_E_INVALID, "null batch");
    if (b->m->dm.con) return fail(RMX_E_INVALID, "rmx_step_euler: matlab-simple has no ForceGroundCuboid; use rmx_step_bdf1/bdf2");
    if (b->m->dm.nsph) return fail(RMX_E_INVALID, "rmx_step_euler: matlab-simple has no JointSpherical; use rmx_step_bdf1/bdf2");
    if (b->m->big) return fail(RMX_E_INVALID, "rmx_step_euler: trees of more than 64 nodes run rmx_step_bdf1/bdf2 only");
    if (b->m->dpf) return fail(RMX_E_INVALID, "rmx_step_euler: models with point forces (rmx_model_set_point_forces) run rmx_step_bdf1/bdf2 only");
    if (nsteps < 0 || !(h > 0)) return fail(RMX_E_INVALID, "bad nsteps / h");
    if ((hT == nullptr) != (hV == nullptr)) return fail(RMX_E_INVALID, "hist_T and hist_V must be given together");
    rmx_model* m = b->m;
    HIPCHK(hipSetDevice(m->device));
    if (nsteps == 0 || m->nr == 0) return RMX_OK;
    if (int rc = pending_error_check(b, "rmx_step_euler")) return rc;
    double *dT = nullptr, *dV = nullptr;
    const size_t nh = (size_t)nsteps * b->B;
    if (hT) {
        HIPCHK(hipMalloc((void**)&dT, nh * sizeof(double)));
        hipError_t e = hipMalloc((void**)&dV, nh * sizeof(double));
        if (e != hipSuccess) { (void)hipFree(dT); return fail(RMX_E_NOMEM, "hipMalloc(hist)"); }
    }
    StepArgs a{};
    a.B = b->B; a.nsteps = nsteps; a.q = b->q; a.qd = b->qd; a.histT = dT; a.histV = dV;
    hipError_t e = timed_launch(b, hipSuccess, [&] { DISPATCH_NP(m->NP, launch_euler, m, b, h, a); return hipSuccess; });
    if (e == hipSuccess) e = set_started(b, 0);
    if (e == hipSuccess && hT) {
        e = hipMemcpyAsync(hT, dT, nh * sizeof(double), hipMemcpyDeviceToHost, b->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hV, dV, nh * sizeof(double), hipMemcpyDeviceToHost, b->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e == hipSuccess) take_event_time(b);
    if (dT) (void)hipFree(dT);
    if (dV) (void)hipFree(dV);
    if (e != hipSuccess) return fail(RMX_E_HIP, std::string("rmx_step_euler: ") + hipGetErrorString(e));
    return RMX_OK;
}


// the models the adjoint path does not take (every rmx_adjoint_* entry and rmx_rollout_tape).  tape_entry: one of the four tape
// entries (rmx_rollout_tape, _tape_bdf2, _tape_feedback, _tape_feedback_box), which take a force table where the model's switch is
// on (rmx_model_tape_point_forces; rmx_tape_pf.h) - every other caller refuses it whatever the switch says
static int adjoint_model_refusal(const rmx_model* m, const bool tape_entry = false) {
    if (m->dm.con) return fail(RMX_E_INVALID, "rmx_adjoint: ground contact is outside the adjoint path (SURVEY.md 8(f))");
    if (m->dm.nsph) return fail(RMX_E_INVALID, "rmx_adjoint: spherical joints are outside the adjoint path (SURVEY.md 8(f))");
    if (m->big) return fail(RMX_E_INVALID, "rmx_adjoint: trees of more than 64 nodes are outside the adjoint path");
    if (m->dpf && !(tape_entry && m->tape_pf))
        return fail(RMX_E_INVALID, "rmx_adjoint: point forces (rmx_model_set_point_forces) are outside the adjoint path");
    return RMX_OK;
}

// the adjoint workspace of a batch: one allocation, kept between calls, that only ever grows
static hipError_t adjws_reserve(rmx_batch* b, const size_t total) {
    if (total <= b->adjws_bytes) return hipSuccess;
    void* fresh = nullptr;
    hipError_t e = hipMalloc(&fresh, total);      // the new buffer first: a failed regrow keeps the old workspace usable
    if (e != hipSuccess && b->adjws) {      // ... unless old + new do not fit side by side: then the old one has to go first
        (void)hipGetLastError();
        (void)hipStreamSynchronize(b->stream);
        (void)hipFree(b->adjws);
        b->adjws = nullptr;
        b->adjws_bytes = 0;
        e = hipMalloc(&fresh, total);
    }
    if (e == hipSuccess) {
        if (b->adjws) { (void)hipStreamSynchronize(b->stream); (void)hipFree(b->adjws); }
        b->adjws = fresh;
        b->adjws_bytes = total;
    } else {
        (void)hipGetLastError();       // an out-of-memory here must not be taken for a failed launch by the next call
    }
    return e;
}

// Executes an adjoint plan of rmx_select.h: the one switch from AdjKernel to a launcher.
static void launch_adjoint_plan(rmx_batch* b, const rmx_select::AdjPlan& plan, const int integ, const DevOpts& o, const AdjArgs& a) {
    rmx_model* m = b->m;
    switch (plan.kernel) {
        case AdjKernel::Help16: launch_adjoint_help_16(m, b, integ, o, a, plan.fullchain); break;      // (a taped rollout: BDF1 only, select_rollout_tape)
        case AdjKernel::FullChain16: launch_adjoint_fullchain_16(m, b, integ, o, a); break;
        case AdjKernel::Generic: DISPATCH_NP(m->NP, launch_adjoint, m, b, integ, o, a); break;
    }
}

// controls (rmx_adjoint_controls): p is u[B][nsteps][nr], dPdp is dPdu of the same shape or null (the forward sweep alone)
// track (rmx_adjoint_track, with controls; task is null then): the terms of the objective; xtarget is its target table, a device array
// when on_device.  The term table (rmx_track.h), the step offsets and, in the host form, the targets go into the workspace behind
// the parts it has, and dPdq holds one row per step.
static int adjoint_impl(rmx_batch* b, const rmx_opts* opts, int nsteps, const rmx_task_pointpos* task, const double* p, double* P,
                        double* dPdp, rmx_stats* stats, const int integ, const bool on_device = false, const bool controls = false,
                        const rmx_task_track* track = nullptr, const double* xtarget = nullptr) {
    if (!b || (!task && !track) || !p || !P || (!dPdp && !controls)) return fail(RMX_E_INVALID, "null argument");
    rmx_model* m = b->m;
    if (nsteps < 1) return fail(RMX_E_INVALID, "nsteps < 1");
    if (int rc = adjoint_model_refusal(m)) return rc;
    rmx_track::Plan tplan;
    if (track) {
        tplan = rmx_track::plan_terms(track->terms, track->nterms, nsteps, m->nlist, m->node_of_listing.data());
        if (!tplan.error.empty()) return fail(RMX_E_INVALID, "rmx_adjoint_track: " + tplan.error);
    } else {
        if (task->body < 0 || task->body >= m->nlist) return fail(RMX_E_INVALID, "task body out of range");
        if (task->step < 1 || task->step > nsteps) return fail(RMX_E_INVALID, "task step must be in [1, nsteps]");
    }
    HIPCHK(hipSetDevice(m->device));
    DevOpts o;
    int rc = make_opts(b, opts, o);
    if (rc) return rc;
    rc = pending_error_check(b, "rmx_adjoint");
    if (rc) return rc;
    const size_t nn = (size_t)m->n * m->n, nv = (size_t)b->B * m->nr * (controls ? (size_t)nsteps : 1);
    const size_t hist = (size_t)b->B * nsteps * nn * sizeof(double);
    if (3 * hist > ((size_t)200 << 30)) return fail(RMX_E_NOMEM, "adjoint history (H, M, D per step) would exceed 200 GiB");
    AdjArgs a{};
    a.B = b->B; a.nsteps = nsteps;
    if (track) {
        a.pscale = track->pscale; a.wreg = track->wreg;
    } else {
        a.task_step = task->step; a.task_node = m->node_of_listing[task->body];
        for (int c = 0; c < 3; ++c) { a.xl[c] = task->xlocal[c]; a.xt[c] = task->xtarget[c]; }
        a.pscale = task->pscale; a.wreg = task->wreg; a.wpos = task->wpos;
    }
    a.q = b->q; a.qd = b->qd; a.qp = b->qp; a.qdp = b->qdp; a.p = b->tmpA;
    a.it = stats ? b->it : nullptr; a.status = b->status;
    // (the constant parameters are staged in tmpA; the per-step controls, nsteps times as many, in the workspace behind the gradient)
    // one workspace per batch, kept between calls (grow-only): its parts at 256-byte boundaries, in this order
    enum { W_H, W_M, W_D, W_DPDQ, W_P, W_DPDP, W_U, W_TRK, W_TRK_BEGIN, W_XT };
    const size_t nterms = track ? (size_t)track->nterms : 0;
    const size_t nxt = nterms * 3 * ((track && track->per_rollout) ? (size_t)b->B : 1);      // doubles of the target table
    rmx_tape::StagePlan ws;
    for (int i = W_H; i <= W_D; ++i) ws.add(hist, true);
    ws.add((size_t)b->B * m->n * (track ? (size_t)nsteps : 1) * sizeof(double), true);
    ws.add((size_t)b->B * sizeof(double), true);
    ws.add((on_device && controls) ? 0 : nv * sizeof(double), true);
    ws.add((controls && !on_device) ? nv * sizeof(double) : 0, true);
    ws.add(nterms * sizeof(rmx_track::DevTerm), true);
    ws.add(track ? ((size_t)nsteps + 1) * sizeof(int) : 0, true);
    ws.add((track && !on_device) ? nxt * sizeof(double) : 0, true);
    auto part = [&](const int i) { return (void*)((char*)b->adjws + ws.off[i]); };
    b->tape_nsteps = 0;      // (the workspace is about to be rewritten: a tape of rmx_rollout_tape ends here)
    hipError_t e = adjws_reserve(b, ws.total);
    // (dPdq needs no fill: the task step lies in [1, nsteps] - checked above -, so the forward kernel writes every entry the backward
    // kernel reads; one dispatch less ahead of a 0.83 ms launch pair.  The tracking call: row k of dPdq is written and read where step k owns
    // terms, and nowhere else)
    if (e == hipSuccess && !on_device) e = hipMemcpyAsync(controls ? part(W_U) : (void*)b->tmpA, p, nv * sizeof(double), hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess && track) {
        e = hipMemcpyAsync(part(W_TRK), tplan.terms.data(), ws.bytes[W_TRK], hipMemcpyHostToDevice, b->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(part(W_TRK_BEGIN), tplan.begin.data(), ws.bytes[W_TRK_BEGIN], hipMemcpyHostToDevice, b->stream);
        if (e == hipSuccess && !on_device) e = hipMemcpyAsync(part(W_XT), xtarget, ws.bytes[W_XT], hipMemcpyHostToDevice, b->stream);
        if (e != hipSuccess) (void)hipStreamSynchronize(b->stream);      // (the plan's arrays must outlive the copies)
    }
    if (e == hipSuccess) {
        a.Hs = (double*)part(W_H); a.Ms = (double*)part(W_M); a.Ds = (double*)part(W_D);
        a.dPdq = (double*)part(W_DPDQ); a.P = (double*)part(W_P); a.dPdp = (double*)part(W_DPDP);
        if (on_device) {          // the caller's device arrays directly: nothing staged, nothing copied back
            a.p = p; a.P = P; a.dPdp = dPdp;
        }
        if (controls) {
            a.u = on_device ? p : (const double*)part(W_U);
            a.dPdu = dPdp ? a.dPdp : nullptr;
            a.p = nullptr; a.dPdp = nullptr;
        }
        if (track) {
            a.trk = (const rmx_track::DevTerm*)part(W_TRK);
            a.trk_begin = (const int*)part(W_TRK_BEGIN);
            a.trk_xt = on_device ? xtarget : (const double*)part(W_XT);
            a.trk_xt_stride = track->per_rollout ? nterms * 3 : 0;
        }
        const rmx_select::AdjPlan plan = rmx_select::select_adjoint(step_traits(m), b->B, rmx_select::knobs_from_env());
        e = timed_launch(b, e, [&] { launch_adjoint_plan(b, plan, integ, o, a); return hipSuccess; });
        // after a BDF2 rollout (q, qdot) of step k-1 are in place: rmx_step_bdf2 may continue it; a BDF1 rollout invalidates them
        if (e == hipSuccess) e = set_started(b, integ == INTEG_BDF2 ? 1 : 0);
        if (e == hipSuccess && !on_device) e = hipMemcpyAsync(P, a.P, ws.bytes[W_P], hipMemcpyDeviceToHost, b->stream);
        if (e == hipSuccess && !on_device && dPdp) e = hipMemcpyAsync(dPdp, part(W_DPDP), ws.bytes[W_DPDP], hipMemcpyDeviceToHost, b->stream);
        if (e == hipSuccess && stats) {
            if (stats->newton_iters) e = hipMemcpyAsync(stats->newton_iters, b->it, sizeof(int) * b->B, hipMemcpyDeviceToHost, b->stream);
            if (e == hipSuccess && stats->status) e = hipMemcpyAsync(stats->status, b->status, sizeof(int) * b->B, hipMemcpyDeviceToHost, b->stream);
        }
        e = wait_or_drain(b, e, track != nullptr);      // (configs[3]: a launch pair of 0.9 ms; the tracking call drains after a failure, as above)
    }
    if (e == hipErrorOutOfMemory) return fail(RMX_E_NOMEM, "rmx_adjoint: no device memory for the history (H, M, D per step and rollout)");
    return call_result(b, e, "rmx_adjoint");
}

extern "C" int rmx_adjoint_bdf1(rmx_batch* b, const rmx_opts* opts, int nsteps, const rmx_task_pointpos* task, const double* p,
                                double* P, double* dPdp, rmx_stats* stats) {
    return adjoint_impl(b, opts, nsteps, task, p, P, dPdp, stats, INTEG_BDF1);
}
extern "C" int rmx_adjoint_bdf2(rmx_batch* b, const rmx_opts* opts, int nsteps, const rmx_task_pointpos* task, const double* p,
                                double* P, double* dPdp, rmx_stats* stats) {
    return adjoint_impl(b, opts, nsteps, task, p, P, dPdp, stats, INTEG_BDF2);
}

extern "C" int rmx_adjoint_bdf1_device(rmx_batch* b, const rmx_opts* opts, int nsteps, const rmx_task_pointpos* task, const double* d_p,
                                       double* d_P, double* d_dPdp, rmx_stats* stats) {
    return adjoint_impl(b, opts, nsteps, task, d_p, d_P, d_dPdp, stats, INTEG_BDF1, true);
}
extern "C" int rmx_adjoint_bdf2_device(rmx_batch* b, const rmx_opts* opts, int nsteps, const rmx_task_pointpos* task, const double* d_p,
                                       double* d_P, double* d_dPdp, rmx_stats* stats) {
    return adjoint_impl(b, opts, nsteps, task, d_p, d_P, d_dPdp, stats, INTEG_BDF2, true);
}

extern "C" int rmx_adjoint_controls(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, const rmx_task_pointpos* task,
                                    const double* u, double* P, double* dPdu, rmx_stats* stats) {
    if (integrator != 1 && integrator != 2) return fail(RMX_E_INVALID, "rmx_adjoint_controls: integrator must be 1 (BDF1) or 2 (BDF2)");
    return adjoint_impl(b, opts, nsteps, task, u, P, dPdu, stats, integrator == 1 ? INTEG_BDF1 : INTEG_BDF2, false, true);
}
extern "C" int rmx_adjoint_controls_device(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, const rmx_task_pointpos* task,
                                           const double* d_u, double* d_P, double* d_dPdu, rmx_stats* stats) {
    if (integrator != 1 && integrator != 2) return fail(RMX_E_INVALID, "rmx_adjoint_controls: integrator must be 1 (BDF1) or 2 (BDF2)");
    return adjoint_impl(b, opts, nsteps, task, d_u, d_P, d_dPdu, stats, integrator == 1 ? INTEG_BDF1 : INTEG_BDF2, true, true);
}

// ---- The taped-rollout family.  rmx_rollout_tape* record a tape in the adjoint workspace (rmx_tape.h: the layout of its parts);
// rmx_rollout_vjp*, _linearize and _jvp read it.  Three helpers carry what the entries share: the tape as an entry sees it
// (TapeView), the arrays of a host form on the device (Staging) and the end of a call (tape_call_end, over the pieces of the tail).
static_assert(INTEG_BDF2 == 2, "rmx_tape::layout takes the integrator as 1 or 2");
static rmx_tape::Layout tape_layout(const rmx_batch* b, const int nsteps, const int integ) {
    return rmx_tape::layout(b->B, nsteps, integ, b->m->n, b->m->nr, b->m->nlist);
}
static rmx_select::AdjPlan tape_plan(const rmx_batch* b, const int integ) {      // the sweeps of the open-loop tape, forward and backward
    return rmx_select::select_rollout_tape(step_traits(b->m), b->B, integ, rmx_select::knobs_from_env());
}

// The parts of a tape's workspace, resolved, and what the tape was recorded with.
struct TapeView {
    rmx_tape::Layout t;
    double *Hs, *Ms, *Ds;                        // [B][nslots][n*n]
    double *stage_traj[3], *stage_state[2];      // the staging areas of the host forms that must not allocate
    double *q0, *qd0, *qt, *qdt, *zs, *pg[5];    // what the tape keeps for rmx_rollout_vjp_params / _vjp_feedback; the staging of the five gradients
    int integ, nslots, bdf2;
    double h, pscale;
};
static TapeView tape_resolve(const rmx_batch* b, const rmx_tape::Layout& t, const int integ, const double h, const double pscale) {
    auto at = [b](const size_t off) { return (double*)((char*)b->adjws + off); };
    TapeView v{};
    v.t = t;
    v.Hs = at(t.H); v.Ms = at(t.M); v.Ds = at(t.D);
    for (int i = 0; i < 3; ++i) v.stage_traj[i] = at(t.stage_traj[i]);
    for (int i = 0; i < 2; ++i) v.stage_state[i] = at(t.stage_state[i]);
    v.q0 = at(t.Q0); v.qd0 = at(t.QD0); v.qt = at(t.QT); v.qdt = at(t.QDT); v.zs = at(t.ZS);
    for (int i = 0; i < 5; ++i) v.pg[i] = at(t.PG + t.pg_off[i]);
    v.integ = integ; v.nslots = t.nslots; v.bdf2 = integ == INTEG_BDF2 ? 1 : 0;
    v.h = h; v.pscale = pscale;
    return v;
}
// The tape of a batch for the entry `who`, or that entry's refusal (the order of the refusals is part of the interface).
static int tape_view(rmx_batch* b, const int nsteps, const std::string& who, TapeView& v) {
    if (b->tape_nsteps < 1 || !b->adjws)
        return fail(RMX_E_INVALID, who + ": no tape (rmx_rollout_tape has not run on this batch, or a later rmx_adjoint_* call reused its workspace)");
    if (nsteps != b->tape_nsteps) return fail(RMX_E_INVALID, who + ": nsteps differs from the tape's (" + std::to_string(b->tape_nsteps) + ")");
    HIPCHK(hipSetDevice(b->m->device));
    if (int rc = pending_error_check(b, who.c_str())) return rc;
    const rmx_tape::Layout t = tape_layout(b, nsteps, b->tape_integ);
    if (t.total > b->adjws_bytes) return fail(RMX_E_INVALID, who + ": no tape (the workspace is smaller than the tape)");
    v = tape_resolve(b, t, b->tape_integ, b->tape_h, b->tape_pscale);
    return RMX_OK;
}
// what the backward sweeps over a tape share (rmx_rollout_vjp, _vjp_params, _vjp_feedback)
static AdjArgs vjp_args(const rmx_batch* b, const TapeView& v, DevOpts& o) {
    o = DevOpts{};
    o.h = v.h;
    AdjArgs a{};
    a.B = b->B; a.nsteps = b->tape_nsteps; a.pscale = v.pscale;
    a.Hs = v.Hs; a.Ms = v.Ms; a.Ds = v.Ds;
    a.tape = 2;
    return a;
}

// The arrays of a call where the kernels find them.  Device form: the caller's pointers, nothing allocated or copied.  Host form: every
// array that is given is staged on the device, copied in ahead of the launch (in) or out behind it (out) - in an area of the
// workspace that the tape call reserved (`borrowed`: the entries that must not allocate), or in an allocation of the call's own
// (allocate(): laid out by rmx_tape::StagePlan, an absent array takes no room there).
struct Staging {
    const bool on_device;
    rmx_tape::StagePlan plan;
    const void* in[rmx_tape::STAGE_MAX] = {};
    void* out[rmx_tape::STAGE_MAX] = {};
    void* at[rmx_tape::STAGE_MAX] = {};
    char* own = nullptr;
    explicit Staging(const bool on_device_) : on_device(on_device_) {}
    int add(const size_t bytes, const void* in_, void* out_, void* borrowed = nullptr) {      // both null: absent
        const int i = plan.add(bytes, in_ || out_);
        in[i] = in_;
        out[i] = out_;
        at[i] = !plan.present[i] ? nullptr : !on_device ? borrowed : in_ ? const_cast<void*>(in_) : out_;
        return i;
    }
    int allocate(const std::string& who, const char* what) {
        if (on_device) return RMX_OK;
        const hipError_t e = hipMalloc((void**)&own, plan.total ? plan.total : 256);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(RMX_E_NOMEM, who + ": no device memory for " + what); }
        if (e != hipSuccess) return fail(RMX_E_HIP, who + ": " + hipGetErrorString(e));
        for (int i = 0; i < plan.n; ++i)
            if (plan.present[i]) at[i] = own + plan.off[i];
        return RMX_OK;
    }
    double* dev(const int i) const { return (double*)at[i]; }      // null: absent
    hipError_t copy_in(const rmx_batch* b, hipError_t e) const {
        for (int i = 0; i < plan.n && !on_device; ++i)
            if (e == hipSuccess && in[i] && plan.bytes[i]) e = hipMemcpyAsync(at[i], in[i], plan.bytes[i], hipMemcpyHostToDevice, b->stream);
        return e;
    }
    hipError_t copy_out(const rmx_batch* b, hipError_t e) const {
        for (int i = 0; i < plan.n && !on_device; ++i)
            if (e == hipSuccess && out[i] && plan.bytes[i]) e = hipMemcpyAsync(out[i], at[i], plan.bytes[i], hipMemcpyDeviceToHost, b->stream);
        return e;
    }
    void release(const rmx_batch* b, const hipError_t e) {      // (after a failure copies may still be in flight)
        if (!own) return;
        if (e != hipSuccess) (void)hipStreamSynchronize(b->stream);
        (void)hipFree(own);
        own = nullptr;
    }
};
// the end of a call that read a tape: wait (after a failure: drain - the caller's arrays must outlive their copies), free, verdict
static int tape_call_end(rmx_batch* b, hipError_t e, Staging& st, const std::string& who) {
    e = wait_or_drain(b, e);
    st.release(b, e);
    return call_result(b, e, who);
}
// The feedback sweeps exist as the generic kernel alone: a plan that names another one is an error, never a silent substitute.
static hipError_t generic_only(const rmx_select::AdjPlan& plan) {
    return plan.kernel == AdjKernel::Generic ? hipSuccess : hipErrorInvalidDeviceFunction;
}

// The torque limits of rmx_rollout_tape_feedback_box / rmx_rollout_lqr_box: an entry with ulo > uhi or a NaN bound is refused, by the
// name of its DOF.  The device forms read the 2 nr doubles back for the check; nothing of the batch is touched.
static int box_refusal(const rmx_batch* b, const rmx_box* box, const bool on_device, const std::string& who) {
    const int nr = b->m->nr;
    std::vector<double> lo(nr, -HUGE_VAL), hi(nr, HUGE_VAL);
    for (int side = 0; side < 2; ++side) {
        const double* p = side ? box->uhi : box->ulo;
        double* dst = side ? hi.data() : lo.data();
        if (!p || !nr) continue;
        if (on_device) {
            HIPCHK(hipSetDevice(b->m->device));
            HIPCHK(hipMemcpy(dst, p, sizeof(double) * nr, hipMemcpyDeviceToHost));
        } else {
            std::copy(p, p + nr, dst);
        }
    }
    for (int i = 0; i < nr; ++i) {
        if (std::isnan(lo[i]) || std::isnan(hi[i])) return fail(RMX_E_INVALID, who + ": a bound of DOF " + std::to_string(i) + " is NaN");
        if (lo[i] > hi[i]) return fail(RMX_E_INVALID, who + ": ulo > uhi at DOF " + std::to_string(i));
    }
    return RMX_OK;
}

// sr (rmx_rollout_search, with fb, BDF1): what rollout_search_impl has checked and planned.  The sweep is k_rollout_search (rmx_search.h)
// in the place of the ADJ_FB kernel: the same closed loop, run once per trial step length and once more for the nominal where none
// is accepted, with the cost formed inside the launch.  Direction, cost tables and outputs join the staging of the gain tables.
struct SearchCall {
    const rmx_search* s;
    const rmx_search_cost* cost;
    const rmx_search_out* out;
    rmx_select::SearchPlan plan;
    std::vector<FrameDevTerm> dterms;      // the cost's terms as the kernel reads them (plan_frame_terms), and their step offsets
    std::vector<int> begin;
};
static hipError_t costws_reserve(rmx_batch* b, const size_t total);
static hipError_t terms_to_device(rmx_batch* b, const std::vector<FrameDevTerm>& dterms, const std::vector<int>& begin, const size_t trk_bytes,
                                  const FrameDevTerm*& trk, const int*& trk_begin);

// fb (rmx_rollout_tape_feedback): u is fb->uff, the sweep is the ADJ_FB kernel and uapp (or null) takes the applied torques.  The host
// form stages K, xref and uapp through a device allocation of its own, freed before the return; the tape's workspace is the same.
// box (rmx_rollout_tape_feedback_box, with fb): the same kernel clamps the torque into the limits, staged with the gain tables.
static int rollout_tape_impl(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const double* u, double* qtraj,
                             double* qdtraj, rmx_stats* stats, const bool on_device, const int integ = INTEG_BDF1,
                             const rmx_feedback* fb = nullptr, double* uapp = nullptr, const rmx_box* box = nullptr,
                             const SearchCall* sr = nullptr) {
    if (!b || !u) return fail(RMX_E_INVALID, "rmx_rollout_tape: null argument");
    if ((qtraj == nullptr) != (qdtraj == nullptr)) return fail(RMX_E_INVALID, "rmx_rollout_tape: qtraj and qdtraj must be given together");
    rmx_model* m = b->m;
    if (nsteps < 1) return fail(RMX_E_INVALID, "nsteps < 1");
    if (int rc = adjoint_model_refusal(m, sr == nullptr)) return rc;
    const bool with_pf = m->dpf != nullptr;      // (past the refusal: a tape entry of a model whose switch is on)
    HIPCHK(hipSetDevice(m->device));
    DevOpts o;
    int rc = make_opts(b, opts, o);
    if (rc) return rc;
    rc = pending_error_check(b, "rmx_rollout_tape");
    if (rc) return rc;
    const rmx_tape::Layout t = tape_layout(b, nsteps, integ);
    if (3 * t.bytes_hist > ((size_t)200 << 30)) return fail(RMX_E_NOMEM, "adjoint history (H, M, D per step) would exceed 200 GiB");
    if (box && (rc = box_refusal(b, box, on_device, sr ? "rmx_rollout_search" : "rmx_rollout_tape_feedback_box"))) return rc;
    enum { F_K, F_X, F_UAPP, F_ULO, F_UHI, F_KFF, F_JBAR, F_XT, F_VT, F_RT, F_QIN, F_XG, F_R, F_J, F_AL, F_TR, F_ST };
    Staging fbst(on_device);
    const size_t trk_bytes = sr ? rmx_tape::round256(sr->dterms.size() * sizeof(FrameDevTerm)) : 0;
    if (fb) {
        const size_t row = (fb->per_rollout ? (size_t)b->B : 1) * nsteps * 2 * m->nr * sizeof(double);
        fbst.add(row * m->nr, fb->K, nullptr);
        fbst.add(row, fb->xref, nullptr);
        fbst.add(t.bytes_traj, nullptr, uapp);
        fbst.add(m->nr * sizeof(double), box ? box->ulo : nullptr, nullptr);
        fbst.add(m->nr * sizeof(double), box ? box->uhi : nullptr, nullptr);
        if (sr) {
            const size_t B = (size_t)b->B, N = (size_t)nsteps, nr = (size_t)m->nr, dbl = sizeof(double);
            const rmx_state_cost* sc = sr->cost->sc;
            const rmx_frame_terms* ft = sr->cost->ft;
            const size_t tabs = ft ? (ft->per_rollout ? B : 1) * (size_t)ft->nterms : 0;
            const bool trial = sr->s->nalpha > 0;
            fbst.add(t.bytes_traj, trial ? sr->s->kff : nullptr, nullptr);
            fbst.add(B * dbl, trial ? sr->s->Jbar : nullptr, nullptr);
            fbst.add(tabs * 3 * dbl, ft ? ft->xtarget : nullptr, nullptr);
            fbst.add(tabs * 3 * dbl, ft ? ft->vtarget : nullptr, nullptr);
            fbst.add(tabs * 9 * dbl, ft ? ft->Rtarget : nullptr, nullptr);
            fbst.add((sc && sc->Q_per_rollout ? B : 1) * N * 4 * nr * nr * dbl, sc ? sc->Q : nullptr, nullptr);
            fbst.add((sc && sc->goal_per_rollout ? B : 1) * N * 2 * nr * dbl, sc ? sc->xgoal : nullptr, nullptr);
            fbst.add(nr * nr * dbl, sr->cost->R, nullptr);
            fbst.add(B * dbl, nullptr, sr->out->J);
            fbst.add(B * dbl, nullptr, sr->out->alpha);
            fbst.add(B * sizeof(int), nullptr, sr->out->trials);
            fbst.add(B * sizeof(int), nullptr, sr->out->status);
        }
        if (fbst.plan.total > 0)      // (ahead of everything that ends the present tape)
            if ((rc = fbst.allocate(sr ? "rmx_rollout_search" : "rmx_rollout_tape_feedback",
                                    sr ? "the staging of the gain tables, the direction, the cost tables and the outputs" : "the gain tables")))
                return rc;
        if (sr && !sr->dterms.empty() && costws_reserve(b, trk_bytes + sr->begin.size() * sizeof(int)) != hipSuccess) {
            fbst.release(b, hipSuccess);
            return fail(RMX_E_NOMEM, "rmx_rollout_search: no device memory for the term table");
        }
    }
    b->tape_nsteps = 0;
    hipError_t e = adjws_reserve(b, t.total);
    if (e == hipSuccess) {
        const TapeView v = tape_resolve(b, t, integ, o.h, pscale);
        enum { S_U, S_QT, S_QDT };
        Staging st(on_device);
        st.add(t.bytes_traj, u, nullptr, v.stage_traj[0]);
        st.add(t.bytes_traj, nullptr, qtraj, v.stage_traj[1]);
        st.add(t.bytes_traj, nullptr, qdtraj, v.stage_traj[2]);
        e = fbst.copy_in(b, st.copy_in(b, e));
        AdjArgs a{};
        if (fb) {
            a.fbK = fbst.dev(F_K);
            a.fbx = fbst.dev(F_X);
            a.fb_stride = fb->per_rollout ? (size_t)nsteps : 0;
            a.uapp = fbst.dev(F_UAPP);
            a.ulo = fbst.dev(F_ULO);
            a.uhi = fbst.dev(F_UHI);
        }
        a.B = b->B; a.nsteps = nsteps; a.pscale = pscale;
        a.q = b->q; a.qd = b->qd; a.qp = b->qp; a.qdp = b->qdp;
        a.it = stats ? b->it : nullptr; a.status = b->status;
        a.Hs = v.Hs; a.Ms = v.Ms; a.Ds = v.Ds;
        a.u = st.dev(S_U);
        a.tape = 1;
        // the states rmx_rollout_vjp_params differentiates at stay with the tape: (q0, qdot0) is copied on the stream ahead of the sweep;
        // the trajectory is recorded by the kernel as ever - into the caller's arrays (or their staging) and copied behind the sweep,
        // or, where the caller wants no record, straight into the tape's own rows
        a.qtraj = qtraj ? st.dev(S_QT) : v.qt;
        a.qdtraj = qtraj ? st.dev(S_QDT) : v.qdt;
        if (e == hipSuccess) e = hipMemcpyAsync(v.q0, b->q, t.bytes_state, hipMemcpyDeviceToDevice, b->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(v.qd0, b->qd, t.bytes_state, hipMemcpyDeviceToDevice, b->stream);
        SearchArgs sa{};
        if (sr) {      // (a is complete: the kernel reads the closed-loop sweep's arguments as they stand)
            const rmx_state_cost* sc = sr->cost->sc;
            const rmx_frame_terms* ft = sr->cost->ft;
            const size_t N = (size_t)nsteps, nr = (size_t)m->nr;
            sa.a = a;
            sa.kff = fbst.dev(F_KFF); sa.Jbar = fbst.dev(F_JBAR);
            sa.nalpha = sr->s->nalpha;
            for (int i = 0; i < sa.nalpha; ++i) sa.alphas[i] = sr->s->alphas[i];
            sa.c.nsteps = nsteps; sa.c.nterms = ft ? ft->nterms : 0;
            sa.c.xt = fbst.dev(F_XT); sa.c.vt = fbst.dev(F_VT); sa.c.Rt = fbst.dev(F_RT);
            sa.c.Qin = fbst.dev(F_QIN); sa.c.xgoal = fbst.dev(F_XG);
            sa.c.t_stride = (ft && ft->per_rollout) ? (size_t)ft->nterms : 0;
            sa.c.q_stride = (sc && sc->Q_per_rollout) ? N * 4 * nr * nr : 0;
            sa.c.goal_stride = (sc && sc->goal_per_rollout) ? N * 2 * nr : 0;
            sa.R = fbst.dev(F_R);
            sa.J = fbst.dev(F_J); sa.alpha = fbst.dev(F_AL); sa.trials = (int*)fbst.at[F_TR]; sa.sstatus = (int*)fbst.at[F_ST];
            if (!sr->dterms.empty() && e == hipSuccess) e = terms_to_device(b, sr->dterms, sr->begin, trk_bytes, sa.c.trk, sa.c.trk_begin);
        }
        e = timed_launch(b, e, [&] {
            if (sr) {
                switch (sr->plan.np) {
                    case 4: launch_search_4(m, b, o, sa, sr->plan.block); break;
                    case 8: launch_search_8(m, b, o, sa, sr->plan.block); break;
                    case 16: launch_search_16(m, b, o, sa, sr->plan.block); break;
                    case 32: launch_search_32(m, b, o, sa, sr->plan.block); break;
                    default: return hipErrorInvalidDeviceFunction;      // (the plan admits no other size: never a silent substitute)
                }
                b->last_kernel = rmx_select::label_rollout_search();
                return hipSuccess;
            }
            if (with_pf) {      // the sweep that carries the forces into H and D (rmx_tape_pf.h), open or closed loop
                const rmx_select::TapePfPlan plan = rmx_select::select_rollout_tape_pf(step_traits(m), integ, fb != nullptr);
                if (plan.kernel != rmx_select::TapePfKernel::Wave) return hipErrorInvalidDeviceFunction;      // (never a silent substitute)
                DISPATCH_NP(plan.np, launch_tape_pf, m, b, integ, plan.feedback, o, a)
                b->last_kernel = plan.label;
                return hipSuccess;
            }
            if (fb) {
                const rmx_select::AdjPlan plan = rmx_select::select_rollout_feedback(step_traits(m), b->B, integ, rmx_select::knobs_from_env());
                if (generic_only(plan) == hipSuccess) DISPATCH_NP(m->NP, launch_rollout_feedback, m, b, integ, o, a)
                b->last_kernel = box ? rmx_select::label_rollout_feedback_box(integ) : rmx_select::label_rollout_feedback(integ);
                return generic_only(plan);
            }
            const rmx_select::AdjPlan plan = tape_plan(b, integ);
            launch_adjoint_plan(b, plan, integ, o, a);
            if (integ == INTEG_BDF2) b->last_kernel = rmx_select::label_rollout_tape_bdf2(plan);
            return hipSuccess;
        });
        // a BDF1 rollout: rmx_step_bdf2 takes its start step again; after a BDF2 rollout (q, qdot) of step k-1 are in place
        if (e == hipSuccess) e = set_started(b, integ == INTEG_BDF2 ? 1 : 0);
        if (e == hipSuccess && qtraj) {
            e = hipMemcpyAsync(v.qt, a.qtraj, t.bytes_traj, hipMemcpyDeviceToDevice, b->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(v.qdt, a.qdtraj, t.bytes_traj, hipMemcpyDeviceToDevice, b->stream);
        }
        e = fbst.copy_out(b, st.copy_out(b, e));
        if (e == hipSuccess && stats) {
            if (stats->newton_iters) e = hipMemcpyAsync(stats->newton_iters, b->it, sizeof(int) * b->B, hipMemcpyDeviceToHost, b->stream);
            if (e == hipSuccess && stats->status) e = hipMemcpyAsync(stats->status, b->status, sizeof(int) * b->B, hipMemcpyDeviceToHost, b->stream);
        }
        e = wait_or_drain(b, e);      // (u must outlive its copy)
        if (e == hipSuccess) {
            take_event_time(b);
            b->tape_nsteps = nsteps;
            b->tape_integ = integ;
            b->tape_h = o.h;
            b->tape_pscale = pscale;
            b->tape_pf = with_pf;
        }
    }
    fbst.release(b, e);
    if (e == hipErrorOutOfMemory) return fail(RMX_E_NOMEM, "rmx_rollout_tape: no device memory for the tape (H, M, D per step and rollout)");
    if (e != hipSuccess) return fail(RMX_E_HIP, std::string("rmx_rollout_tape: ") + hipGetErrorString(e));
    return RMX_OK;
}

// gq, gqd in and du, dq0, dqd0 out, as rmx_rollout_vjp and rmx_rollout_vjp_params take them: the host forms stage them in the areas
// the tape call reserved.
static void vjp_stage(Staging& st, const TapeView& v, AdjArgs& a, const double* gq, const double* gqd, double* du, double* dq0, double* dqd0) {
    a.gq = st.dev(st.add(v.t.bytes_traj, gq, nullptr, v.stage_traj[0]));
    a.gqd = st.dev(st.add(v.t.bytes_traj, gqd, nullptr, v.stage_traj[1]));
    a.dPdu = st.dev(st.add(v.t.bytes_traj, nullptr, du, v.stage_traj[2]));
    a.dq0 = st.dev(st.add(v.t.bytes_state, nullptr, dq0, v.stage_state[0]));
    a.dqd0 = st.dev(st.add(v.t.bytes_state, nullptr, dqd0, v.stage_state[1]));
}

static int rollout_vjp_impl(rmx_batch* b, int nsteps, const double* gq, const double* gqd, double* du, double* dq0, double* dqd0,
                            const bool on_device, const std::string& who = "rmx_rollout_vjp") {
    if (!b || !gq || !gqd || !du) return fail(RMX_E_INVALID, who + ": null argument");
    if ((dq0 == nullptr) != (dqd0 == nullptr)) return fail(RMX_E_INVALID, who + ": dq0 and dqd0 must be given together");
    TapeView v;
    if (int rc = tape_view(b, nsteps, who, v)) return rc;
    DevOpts o;
    AdjArgs a = vjp_args(b, v, o);
    Staging st(on_device);
    vjp_stage(st, v, a, gq, gqd, du, dq0, dqd0);
    hipError_t e = st.copy_in(b, hipSuccess);
    e = timed_launch(b, e, [&] {
        launch_adjoint_plan(b, tape_plan(b, v.integ), v.integ, o, a);      // (the backward sweep of the integrator that recorded the tape)
        return hipSuccess;
    });
    return tape_call_end(b, st.copy_out(b, e), st, who);
}

// rmx_rollout_vjp_feedback: the closed-loop backward sweep (rmx_feedback_bwd.h).  Without gains and without gu it IS rmx_rollout_vjp
// (the same launch, the same bits).  Otherwise one launch of k_rollout_bwd_fb; the host form stages the cotangents, K, xref and the
// outputs through a device allocation of its own, made ahead of anything else and freed before the return: the tape's workspace
// neither grows nor is written.
static int rollout_vjp_feedback_impl(rmx_batch* b, int nsteps, const rmx_feedback* fb, const double* gq, const double* gqd, const double* gu,
                                     const rmx_feedback_grads* out, const bool on_device) {
    const std::string who = "rmx_rollout_vjp_feedback";
    if (!b || !fb || !gq || !gqd || !out) return fail(RMX_E_INVALID, who + ": null argument");
    if (!out->duff && !out->dK && !out->dxref && !out->dq0) return fail(RMX_E_INVALID, who + ": all outputs are null");
    if ((out->dq0 == nullptr) != (out->dqd0 == nullptr)) return fail(RMX_E_INVALID, who + ": dq0 and dqd0 must be given together");
    if (fb->per_rollout != 0 && fb->per_rollout != 1) return fail(RMX_E_INVALID, who + ": per_rollout must be 0 or 1");
    if (!fb->K && (out->dK || out->dxref)) return fail(RMX_E_INVALID, who + ": no gains (K is null): dK and dxref cannot be formed");
    TapeView v;
    if (int rc = tape_view(b, nsteps, who, v)) return rc;
    rmx_model* m = b->m;
    if (!fb->K && !gu) {      // rmx_rollout_vjp itself; a duff nobody asked for goes to a scratch array of the call's own
        double* du = out->duff;
        std::vector<double> hdu;
        if (!du && !on_device) {
            hdu.resize((size_t)b->B * nsteps * m->nr);
            du = hdu.data();
        } else if (!du && hipMalloc((void**)&du, v.t.bytes_traj ? v.t.bytes_traj : 256) != hipSuccess) {
            (void)hipGetLastError();
            return fail(RMX_E_NOMEM, who + ": no device memory for the staging");
        }
        const int rc = rollout_vjp_impl(b, nsteps, gq, gqd, du, out->dq0, out->dqd0, on_device, who);
        if (!out->duff && on_device) (void)hipFree(du);
        if (rc == RMX_OK) b->last_kernel = rmx_select::label_rollout_vjp(tape_plan(b, v.integ), v.integ);      // (the plan just executed: the selection is pure)
        return rc;
    }
    const size_t nr = m->nr, row = 2 * nr * sizeof(double);
    const size_t fb_tables = (fb->per_rollout ? (size_t)b->B : 1) * nsteps, rows = (size_t)b->B * nsteps;
    enum { S_GQ, S_GQD, S_GU, S_K, S_X, S_DUFF, S_DK, S_DX, S_DQ0, S_DQD0 };      // the inputs, then the outputs
    Staging st(on_device);
    st.add(v.t.bytes_traj, gq, nullptr);
    st.add(v.t.bytes_traj, gqd, nullptr);
    st.add(v.t.bytes_traj, gu, nullptr);
    st.add(fb_tables * row * nr, fb->K, nullptr);
    st.add(fb_tables * row, fb->K ? fb->xref : nullptr, nullptr);
    st.add(v.t.bytes_traj, nullptr, out->duff);
    st.add(rows * row * nr, nullptr, out->dK);
    st.add(rows * row, nullptr, out->dxref);
    st.add(v.t.bytes_state, nullptr, out->dq0);
    st.add(v.t.bytes_state, nullptr, out->dqd0);
    if (int rc = st.allocate(who, "the staging")) return rc;
    DevOpts o;
    AdjArgs a = vjp_args(b, v, o);
    a.gq = st.dev(S_GQ); a.gqd = st.dev(S_GQD); a.gu = st.dev(S_GU);
    a.fbK = st.dev(S_K); a.fbx = st.dev(S_X);
    a.fb_stride = fb->per_rollout ? (size_t)nsteps : 0;
    a.dPdu = st.dev(S_DUFF); a.dK = st.dev(S_DK); a.dxref = st.dev(S_DX); a.dq0 = st.dev(S_DQ0); a.dqd0 = st.dev(S_DQD0);
    a.fq0 = v.q0; a.fqd0 = v.qd0; a.fqt = v.qt; a.fqdt = v.qdt;
    hipError_t e = st.copy_in(b, hipSuccess);
    e = timed_launch(b, e, [&] {
        const rmx_select::AdjPlan plan = rmx_select::select_rollout_vjp_feedback(step_traits(m), b->B, v.integ, rmx_select::knobs_from_env());
        if (generic_only(plan) == hipSuccess) DISPATCH_NP(m->NP, launch_vjp_feedback, m, b, v.integ, o, a)
        return generic_only(plan);
    });
    const int rc = tape_call_end(b, st.copy_out(b, e), st, who);
    if (rc == RMX_OK) b->last_kernel = rmx_select::label_rollout_vjp_feedback(v.integ);
    return rc;
}

// the listing index of the body each node carries, -1: none (ParamArgs::lst, ParamRhsArgs::lst)
static void listing_of_nodes(const rmx_model* m, short (&lst)[MAXN]) {
    for (int i = 0; i < MAXN; ++i) lst[i] = -1;
    for (int L = 0; L < m->nlist; ++L) {
        const int k = m->node_of_listing[L];
        if (k >= 0 && k < MAXN) lst[k] = (short)L;
    }
}

// what k_rollout_param_grad reads (rmx_rollout_vjp_params, rmx_rollout_vjp_forces): the tape's states and z, the five outputs where
// the kernel finds them, the listing index of the body each node carries
static ParamArgs param_args(const rmx_model* m, const TapeView& v, const int nsteps, double* const* dev) {
    ParamArgs pa{};
    pa.nsteps = nsteps; pa.nslots = v.nslots; pa.bdf2 = v.bdf2;
    pa.njoints = m->nlist; pa.h = v.h;
    pa.q0 = v.q0; pa.qd0 = v.qd0; pa.qt = v.qt; pa.qdt = v.qdt;
    pa.zs = v.zs;
    pa.stiffness = dev[0]; pa.damping = dev[1]; pa.qrest = dev[2]; pa.inertia = dev[3]; pa.grav = dev[4];
    listing_of_nodes(m, pa.lst);
    return pa;
}

// rmx_rollout_vjp_params: rmx_rollout_vjp's sweep in the instantiation that also stores z of every slot, then the contraction of
// rmx_params.h over the slots with the states the tape kept.  Everything it stages lies in parts the tape call reserved.
static int rollout_vjp_params_impl(rmx_batch* b, int nsteps, const double* gq, const double* gqd, double* du, double* dq0, double* dqd0,
                                   const rmx_param_grads* out, const bool on_device) {
    const std::string who = "rmx_rollout_vjp_params";
    if (!b || !gq || !gqd || !du || !out) return fail(RMX_E_INVALID, who + ": null argument");
    if ((dq0 == nullptr) != (dqd0 == nullptr)) return fail(RMX_E_INVALID, who + ": dq0 and dqd0 must be given together");
    double* const grads[5] = {out->stiffness, out->damping, out->qrest, out->inertia, out->grav};
    if (!grads[0] && !grads[1] && !grads[2] && !grads[3] && !grads[4]) return fail(RMX_E_INVALID, who + ": all outputs are null");
    TapeView v;
    if (int rc = tape_view(b, nsteps, who, v)) return rc;
    if (b->tape_pf)
        return fail(RMX_E_INVALID, who + ": the tape carries point forces (rmx_model_tape_point_forces); the parameters' contraction does not cover them");
    rmx_model* m = b->m;
    DevOpts o;
    AdjArgs a = vjp_args(b, v, o);
    Staging st(on_device);
    vjp_stage(st, v, a, gq, gqd, du, dq0, dqd0);
    double* dev[5];
    for (int i = 0; i < 5; ++i) dev[i] = st.dev(st.add(v.t.pg_bytes[i], nullptr, grads[i], v.pg[i]));
    a.zs = v.zs;
    const ParamArgs pa = param_args(m, v, nsteps, dev);
    hipError_t e = st.copy_in(b, hipSuccess);
    e = timed_launch(b, e, [&] {
        DISPATCH_NP(m->NP, launch_vjp_zs, m, b, v.integ, o, a, tape_plan(b, v.integ).fullchain);
        const hipError_t el = hipGetLastError();
        if (el == hipSuccess) DISPATCH_NP(m->NP, launch_param_grad, m, b, pa);
        return el;
    });
    return tape_call_end(b, st.copy_out(b, e), st, who);
}

// rmx_rollout_vjp_forces: rmx_rollout_vjp_params on a tape that carries point forces.  The sweep that stores z and the contraction of
// rmx_params.h run unchanged (dg/dtheta of the joint, inertia and gravity parameters does not involve the forces); the contraction of
// rmx_force_params.h forms the rows of the force constants from the same z.  The five model arrays stage where rmx_rollout_vjp_params
// stages them; the three force arrays through an allocation of the call's own, as rmx_rollout_linearize's outputs do.
static int rollout_vjp_forces_impl(rmx_batch* b, int nsteps, const double* gq, const double* gqd, double* du, double* dq0, double* dqd0,
                                   const rmx_param_grads* model, const rmx_force_grads* forces, const bool on_device) {
    const std::string who = "rmx_rollout_vjp_forces";
    if (!b || !gq || !gqd || !du) return fail(RMX_E_INVALID, who + ": null argument");
    if ((dq0 == nullptr) != (dqd0 == nullptr)) return fail(RMX_E_INVALID, who + ": dq0 and dqd0 must be given together");
    double* const grads[5] = {model ? model->stiffness : nullptr, model ? model->damping : nullptr, model ? model->qrest : nullptr,
                              model ? model->inertia : nullptr, model ? model->grav : nullptr};
    double* const fgrads[3] = {forces ? forces->stiffness : nullptr, forces ? forces->damping : nullptr, forces ? forces->L : nullptr};
    const bool want_model = grads[0] || grads[1] || grads[2] || grads[3] || grads[4];
    const bool want_forces = fgrads[0] || fgrads[1] || fgrads[2];
    if (!want_model && !want_forces) return fail(RMX_E_INVALID, who + ": all outputs are null");
    TapeView v;
    if (int rc = tape_view(b, nsteps, who, v)) return rc;
    rmx_model* m = b->m;
    if (!b->tape_pf)
        return fail(RMX_E_INVALID, who + ": the tape carries no point forces (rmx_model_tape_point_forces); rmx_rollout_vjp_params is the call for it");
    if (!m->dpf) return fail(RMX_E_INVALID, who + ": the model's force table has been removed since the tape was recorded");
    DevOpts o;
    AdjArgs a = vjp_args(b, v, o);
    Staging st(on_device), fst(on_device);
    vjp_stage(st, v, a, gq, gqd, du, dq0, dqd0);
    double *dev[5], *fdev[3];
    for (int i = 0; i < 5; ++i) dev[i] = st.dev(st.add(v.t.pg_bytes[i], nullptr, grads[i], v.pg[i]));
    const size_t fbytes = (size_t)b->B * m->npf * sizeof(double);
    for (int i = 0; i < 3; ++i) fst.add(fbytes, nullptr, fgrads[i]);
    if (int rc = fst.allocate(who, "the staging of the force gradients")) return rc;
    for (int i = 0; i < 3; ++i) fdev[i] = fst.dev(i);
    a.zs = v.zs;
    const ParamArgs pa = param_args(m, v, nsteps, dev);
    ForceArgs fa{};
    fa.nsteps = nsteps; fa.nslots = v.nslots; fa.bdf2 = v.bdf2; fa.h = v.h;
    fa.q0 = v.q0; fa.qd0 = v.qd0; fa.qt = v.qt; fa.qdt = v.qdt;
    fa.zs = a.zs;
    fa.stiffness = fdev[0]; fa.damping = fdev[1]; fa.L = fdev[2];
    hipError_t e = st.copy_in(b, hipSuccess);
    e = timed_launch(b, e, [&] {
        DISPATCH_NP(m->NP, launch_vjp_zs, m, b, v.integ, o, a, tape_plan(b, v.integ).fullchain);
        hipError_t el = hipGetLastError();
        if (el == hipSuccess && want_model) {
            DISPATCH_NP(m->NP, launch_param_grad, m, b, pa);
            el = hipGetLastError();
        }
        if (el == hipSuccess && want_forces) DISPATCH_NP(m->NP, launch_force_grad, m, b, fa);
        return el;
    });
    e = wait_or_drain(b, fst.copy_out(b, st.copy_out(b, e)));
    st.release(b, e);
    fst.release(b, e);
    return call_result(b, e, who);
}

// rmx_rollout_linearize: XA, XB, XU of every slot of the tape, one kernel over B * nslots wavefronts (rmx_linearize.h).  The host form
// stages through an allocation of its own: the adjoint workspace holds the tape, a regrow would lose it, and tapes that are never
// linearised do not pay for three more histories.
static int rollout_linearize_impl(rmx_batch* b, int nsteps, double* XA, double* XB, double* XU, const bool on_device) {
    const std::string who = "rmx_rollout_linearize";
    if (!b) return fail(RMX_E_INVALID, who + ": null batch");
    if (!XA && !XB && !XU) return fail(RMX_E_INVALID, who + ": all outputs are null");
    TapeView v;
    if (int rc = tape_view(b, nsteps, who, v)) return rc;
    rmx_model* m = b->m;
    LinArgs a{};
    a.nslots = v.nslots; a.bdf2 = v.bdf2; a.h = v.h; a.pscale = v.pscale;
    a.Hs = v.Hs; a.Ms = v.Ms; a.Ds = v.Ds;
    if ((size_t)b->B * a.nslots > (size_t)0x7fffffff) return fail(RMX_E_INVALID, who + ": batch * slots exceeds the grid");
    const size_t bytes = (size_t)b->B * a.nslots * m->nr * m->nr * sizeof(double);
    enum { S_XA, S_XB, S_XU };
    Staging st(on_device);
    st.add(bytes, nullptr, XA);
    st.add(bytes, nullptr, XB);
    st.add(bytes, nullptr, XU);
    if (int rc = st.allocate(who, "the staging of the outputs")) return rc;
    a.XA = st.dev(S_XA); a.XB = st.dev(S_XB); a.XU = st.dev(S_XU);
    if (!bytes) {      // (no reduced DOF: nothing to compute, and no kernel time to take)
        st.release(b, hipSuccess);
        return RMX_OK;
    }
    const hipError_t e = timed_launch(b, hipSuccess, [&] { DISPATCH_NP(m->NP, launch_linearize, m, b, a); return hipSuccess; });
    return tape_call_end(b, st.copy_out(b, e), st, who);
}

// rmx_rollout_jvp: the forward sweep over the tape, one kernel over B * ceil(ntan / JVP_TW) wavefronts (rmx_jvp.h).  The host form
// stages through an allocation of its own, as rmx_rollout_linearize does: the staging areas of the tape's workspace are shaped for one
// direction, and a regrow would lose the tape.
static int rollout_jvp_impl(rmx_batch* b, int nsteps, int ntan, const double* tu, const double* tq0, const double* tqd0, double* tq,
                            double* tqd, const bool on_device) {
    const std::string who = "rmx_rollout_jvp";
    if (!b || !tq || !tqd) return fail(RMX_E_INVALID, who + ": null argument");
    if (ntan < 1) return fail(RMX_E_INVALID, who + ": ntan < 1");
    if (!tu && !tq0 && !tqd0) return fail(RMX_E_INVALID, who + ": all tangents are null");
    TapeView v;
    if (int rc = tape_view(b, nsteps, who, v)) return rc;
    rmx_model* m = b->m;
    JvpArgs a{};
    a.nsteps = nsteps; a.nslots = v.nslots; a.bdf2 = v.bdf2;
    a.ntan = ntan;
    a.nchunks = (ntan + JVP_CHUNK - 1) / JVP_CHUNK;
    a.h = v.h; a.pscale = v.pscale;
    a.Hs = v.Hs; a.Ms = v.Ms; a.Ds = v.Ds;
    if ((size_t)b->B * a.nchunks > (size_t)0x7fffffff) return fail(RMX_E_INVALID, who + ": batch * chunks of directions exceeds the grid");
    const size_t bytes_traj = ntan * v.t.bytes_traj, bytes_state = ntan * v.t.bytes_state;
    enum { S_TQ, S_TQD, S_TU, S_TQ0, S_TQD0 };      // the outputs first
    Staging st(on_device);
    st.add(bytes_traj, nullptr, tq);
    st.add(bytes_traj, nullptr, tqd);
    st.add(bytes_traj, tu, nullptr);
    st.add(bytes_state, tq0, nullptr);
    st.add(bytes_state, tqd0, nullptr);
    if (int rc = st.allocate(who, "the staging of the tangents")) return rc;
    a.tu = st.dev(S_TU); a.tq0 = st.dev(S_TQ0); a.tqd0 = st.dev(S_TQD0);
    a.tq = st.dev(S_TQ); a.tqd = st.dev(S_TQD);
    if (!bytes_traj) {      // (no reduced DOF: nothing to compute, and no kernel time to take)
        st.release(b, hipSuccess);
        return RMX_OK;
    }
    hipError_t e = st.copy_in(b, hipSuccess);
    e = timed_launch(b, e, [&] { DISPATCH_NP(m->NP, launch_jvp, m, b, a); return hipSuccess; });
    return tape_call_end(b, st.copy_out(b, e), st, who);
}

// rmx_rollout_jvp_params: rmx_rollout_jvp's sweep with the parameter term on the right of every slot (rmx_jvp_params.h): one kernel over
// B * nslots wavefronts forms r = (dg/dtheta) ttheta, the sweep's RHS instantiation subtracts it.  r and, in the host form, the tangent
// arrays live in an allocation of the call's own, freed before it returns; the tape's workspace does not grow.
static int rollout_jvp_params_impl(rmx_batch* b, int nsteps, int ntan, const rmx_param_tangents* tp, const double* tu, const double* tq0,
                                   const double* tqd0, double* tq, double* tqd, const bool on_device) {
    const std::string who = "rmx_rollout_jvp_params";
    if (!b || !tp || !tq || !tqd) return fail(RMX_E_INVALID, who + ": null argument");
    if (ntan < 1) return fail(RMX_E_INVALID, who + ": ntan < 1");
    const double* const tans[5] = {tp->stiffness, tp->damping, tp->qrest, tp->inertia, tp->grav};
    if (!tans[0] && !tans[1] && !tans[2] && !tans[3] && !tans[4])
        return fail(RMX_E_INVALID, who + ": all parameter tangents are null; rmx_rollout_jvp is the call for it");
    TapeView v;
    if (int rc = tape_view(b, nsteps, who, v)) return rc;
    rmx_model* m = b->m;
    JvpArgs a{};
    a.nsteps = nsteps; a.nslots = v.nslots; a.bdf2 = v.bdf2;
    a.ntan = ntan;
    a.nchunks = (ntan + JVP_CHUNK - 1) / JVP_CHUNK;
    a.h = v.h; a.pscale = v.pscale;
    a.Hs = v.Hs; a.Ms = v.Ms; a.Ds = v.Ds;
    if ((size_t)b->B * a.nchunks > (size_t)0x7fffffff) return fail(RMX_E_INVALID, who + ": batch * chunks of directions exceeds the grid");
    if ((size_t)b->B * a.nslots > (size_t)0x7fffffff) return fail(RMX_E_INVALID, who + ": batch * slots exceeds the grid");
    const size_t bytes_traj = ntan * v.t.bytes_traj, bytes_state = ntan * v.t.bytes_state;
    const size_t bytes_r = (size_t)b->B * ntan * a.nslots * m->n * sizeof(double);
    enum { S_TQ, S_TQD, S_TU, S_TQ0, S_TQD0, S_TP };      // the outputs first, the five parameter tangents last
    Staging st(on_device);
    st.add(bytes_traj, nullptr, tq);
    st.add(bytes_traj, nullptr, tqd);
    st.add(bytes_traj, tu, nullptr);
    st.add(bytes_state, tq0, nullptr);
    st.add(bytes_state, tqd0, nullptr);
    for (int i = 0; i < 5; ++i) st.add(ntan * v.t.pg_bytes[i], tans[i], nullptr);
    if (!bytes_traj) return RMX_OK;      // (no reduced DOF: nothing to compute, and no kernel time to take)
    if (int rc = st.allocate(who, "the staging of the tangents")) return rc;
    double* d_r = nullptr;      // r is the call's own in both forms: the scratch between the two launches, never copied
    if (hipMalloc((void**)&d_r, bytes_r) != hipSuccess) {
        (void)hipGetLastError();
        st.release(b, hipSuccess);
        return fail(RMX_E_NOMEM, who + ": no device memory for the parameter term of every slot");
    }
    a.tu = st.dev(S_TU); a.tq0 = st.dev(S_TQ0); a.tqd0 = st.dev(S_TQD0);
    a.tq = st.dev(S_TQ); a.tqd = st.dev(S_TQD);
    a.r = d_r;
    ParamRhsArgs p{};
    p.nsteps = nsteps; p.nslots = v.nslots; p.bdf2 = v.bdf2;
    p.njoints = m->nlist; p.ntan = ntan; p.h = v.h;
    p.q0 = v.q0; p.qd0 = v.qd0; p.qt = v.qt; p.qdt = v.qdt;
    p.stiffness = st.dev(S_TP); p.damping = st.dev(S_TP + 1); p.qrest = st.dev(S_TP + 2); p.inertia = st.dev(S_TP + 3); p.grav = st.dev(S_TP + 4);
    p.r = d_r;
    listing_of_nodes(m, p.lst);
    hipError_t e = st.copy_in(b, hipSuccess);
    e = timed_launch(b, e, [&] { DISPATCH_NP(m->NP, launch_jvp_params, m, b, p, a); return hipSuccess; });
    e = wait_or_drain(b, st.copy_out(b, e));
    st.release(b, e);
    (void)hipFree(d_r);
    return call_result(b, e, who);
}

// rmx_rollout_lqr: the Riccati sweep of iLQR over the BDF1 tape, one workgroup per rollout (rmx_lqr.h); the per-slot sensitivities
// are formed inside the sweep, nothing proportional to B N nr^2 is allocated.  The host form stages through an allocation of its
// own, as rmx_rollout_linearize does.
// boxed (rmx_rollout_lqr_box): the BOX instantiation of the same kernel; the limits, ubar and clamped join the same staging.
static int rollout_lqr_impl(rmx_batch* b, int nsteps, const rmx_lqr_cost* cost, const rmx_lqr_gains* out, const bool on_device,
                            const bool boxed = false, const rmx_box* box = nullptr, const double* ubar = nullptr, int max_iter = 0,
                            unsigned* clamped = nullptr) {
    const std::string who = boxed ? "rmx_rollout_lqr_box" : "rmx_rollout_lqr";
    if (!b || !cost || !out || !cost->lx || !cost->lu || !cost->Q || !cost->R || !out->kff || !out->K || (boxed && (!box || !ubar)))
        return fail(RMX_E_INVALID, who + ": null argument");
    if (boxed && max_iter < 0) return fail(RMX_E_INVALID, who + ": max_iter must be >= 0 (0: the default of " +
                                                              std::to_string(rmx_select::LQR_BOX_MAX_ITER) + ")");
    if (cost->per_rollout != 0 && cost->per_rollout != 1) return fail(RMX_E_INVALID, who + ": per_rollout must be 0 or 1");
    if (!(cost->mu >= 0.0) || !std::isfinite(cost->mu)) return fail(RMX_E_INVALID, who + ": mu must be finite and >= 0");
    TapeView v;
    if (int rc = tape_view(b, nsteps, who, v)) return rc;
    if (v.integ != INTEG_BDF1)
        return fail(RMX_E_INVALID, who + ": needs a BDF1 tape (the tape on this batch is BDF2: its augmented state is not built)");
    rmx_model* m = b->m;
    const rmx_select::LqrPlan plan = boxed ? rmx_select::select_rollout_lqr_box(step_traits(m), m->nr) : rmx_select::select_rollout_lqr(step_traits(m), m->nr);
    if (plan.kernel == rmx_select::LqrKernel::RefusedNr)
        return fail(RMX_E_INVALID, who + ": nr > " + std::to_string(rmx_select::LQR_MAX_NR) + " (the model has nr = " + std::to_string(m->nr) +
                                       "; the LDS-resident sweep stops at " + std::to_string(rmx_select::LQR_MAX_NR) + " reduced DOFs)");
    if (plan.kernel != rmx_select::LqrKernel::Lds)
        return fail(RMX_E_INVALID, who + ": more than " + std::to_string(rmx_select::LQR_MAX_NR) + " nodes (the model has " + std::to_string(m->n) +
                                       " for nr = " + std::to_string(m->nr) + "; the LDS-resident sweep stops there)");
    const size_t B = (size_t)b->B, N = (size_t)nsteps, nr = (size_t)m->nr, dbl = sizeof(double);
    const size_t bytes_q = (cost->per_rollout ? B : 1) * N * 4 * nr * nr * dbl;
    if (boxed)
        if (int rc = box_refusal(b, box, on_device, who)) return rc;
    enum { S_KFF, S_K, S_EXP, S_ST, S_LX, S_LU, S_Q, S_R, S_MUB, S_CL, S_ULO, S_UHI, S_UBAR };      // the outputs first (clamped: with the box)
    Staging st(on_device);
    st.add(B * N * nr * dbl, nullptr, out->kff);
    st.add(B * N * 2 * nr * nr * dbl, nullptr, out->K);
    st.add(B * dbl, nullptr, out->expected);
    st.add(B * sizeof(int), nullptr, out->status);
    st.add(B * N * 2 * nr * dbl, cost->lx, nullptr);
    st.add(B * N * nr * dbl, cost->lu, nullptr);
    st.add(bytes_q, cost->Q, nullptr);
    st.add(nr * nr * dbl, cost->R, nullptr);
    st.add(B * dbl, cost->mu_b, nullptr);
    st.add(B * N * sizeof(unsigned), nullptr, clamped);
    st.add(nr * dbl, boxed ? box->ulo : nullptr, nullptr);
    st.add(nr * dbl, boxed ? box->uhi : nullptr, nullptr);
    st.add(B * N * nr * dbl, ubar, nullptr);
    if (int rc = st.allocate(who, "the staging of the cost and the gains")) return rc;
    LqrArgs a{};
    a.nsteps = nsteps; a.h = v.h; a.pscale = v.pscale; a.mu = cost->mu;
    a.Hs = v.Hs; a.Ms = v.Ms; a.Ds = v.Ds;
    a.lx = st.dev(S_LX); a.lu = st.dev(S_LU); a.Q = st.dev(S_Q); a.R = st.dev(S_R); a.mu_b = st.dev(S_MUB);
    a.q_stride = cost->per_rollout ? N * 4 * nr * nr : 0;
    a.kff = st.dev(S_KFF); a.K = st.dev(S_K); a.expected = st.dev(S_EXP); a.status = (int*)st.at[S_ST];
    a.ulo = st.dev(S_ULO); a.uhi = st.dev(S_UHI); a.ubar = st.dev(S_UBAR); a.clamped = (unsigned*)st.at[S_CL];
    a.max_iter = max_iter > 0 ? max_iter : rmx_select::LQR_BOX_MAX_ITER;
    if (!nr) {      // (no reduced DOF: no gains to compute, and no kernel time to take)
        hipError_t e = hipSuccess;
        if (a.expected) e = hipMemsetAsync(a.expected, 0, B * dbl, b->stream);
        if (e == hipSuccess && a.status) e = hipMemsetAsync(a.status, 0, B * sizeof(int), b->stream);
        if (e == hipSuccess && a.clamped) e = hipMemsetAsync(a.clamped, 0, B * N * sizeof(unsigned), b->stream);
        return tape_call_end(b, st.copy_out(b, e), st, who);
    }
    hipError_t e = st.copy_in(b, hipSuccess);
    e = timed_launch(b, e, [&] {
        if (boxed) {
            b->last_kernel = rmx_select::label_rollout_lqr_box();
            switch (m->NP) {
                case 4: launch_lqr_box_4(m, b, a, plan.lds_bytes); break;
                case 8: launch_lqr_box_8(m, b, a, plan.lds_bytes); break;
                case 16: launch_lqr_box_16(m, b, a, plan.lds_bytes); break;
                case 32: launch_lqr_box_32(m, b, a, plan.lds_bytes); break;
                default: return hipErrorInvalidDeviceFunction;
            }
            return hipSuccess;
        }
        switch (m->NP) {
            case 4: launch_lqr_4(m, b, a, plan.lds_bytes); break;
            case 8: launch_lqr_8(m, b, a, plan.lds_bytes); break;
            case 16: launch_lqr_16(m, b, a, plan.lds_bytes); break;
            case 32: launch_lqr_32(m, b, a, plan.lds_bytes); break;
            default: return hipErrorInvalidDeviceFunction;      // (the plan admits no other size: never a silent substitute)
        }
        return hipSuccess;
    });
    return tape_call_end(b, st.copy_out(b, e), st, who);
}
extern "C" int rmx_rollout_lqr(rmx_batch* b, int nsteps, const rmx_lqr_cost* cost, const rmx_lqr_gains* out) {
    return rollout_lqr_impl(b, nsteps, cost, out, false);
}
extern "C" int rmx_rollout_lqr_device(rmx_batch* b, int nsteps, const rmx_lqr_cost* cost, const rmx_lqr_gains* out) {
    return rollout_lqr_impl(b, nsteps, cost, out, true);
}
extern "C" int rmx_rollout_lqr_box(rmx_batch* b, int nsteps, const rmx_lqr_cost* cost, const rmx_box* box, const double* ubar, int max_iter,
                                   const rmx_lqr_gains* out, unsigned* clamped) {
    return rollout_lqr_impl(b, nsteps, cost, out, false, true, box, ubar, max_iter, clamped);
}
extern "C" int rmx_rollout_lqr_box_device(rmx_batch* b, int nsteps, const rmx_lqr_cost* cost, const rmx_box* box, const double* d_ubar,
                                          int max_iter, const rmx_lqr_gains* out, unsigned* d_clamped) {
    return rollout_lqr_impl(b, nsteps, cost, out, true, true, box, d_ubar, max_iter, d_clamped);
}

// rmx_rollout_points / rmx_rollout_cost / rmx_rollout_frames / rmx_rollout_cost_frames: kinematics of body points and frames along a
// state record and the cost model the Riccati sweep takes, one wavefront per (rollout, step) (rmx_cost.h; rmx_select.h
// select_rollout_cost).  They read the model and their arguments alone: no tape is needed and none is touched.  The term table
// (rmx_track::plan_terms on the position part of every term, a host array in both forms) goes to a small device area of the batch's
// own that only grows; the host form stages every other array through an allocation of its own, as rmx_rollout_lqr does.
static hipError_t costws_reserve(rmx_batch* b, const size_t total) {
    if (total <= b->costws_bytes) return hipSuccess;
    void* fresh = nullptr;
    const hipError_t e = hipMalloc(&fresh, total);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e;
    }
    if (b->costws) { (void)hipStreamSynchronize(b->stream); (void)hipFree(b->costws); }
    b->costws = fresh;
    b->costws_bytes = total;
    return hipSuccess;
}
// The terms of a cost entry as the kernels read them - sorted by step on the nodes of the device (rmx_track::plan_terms on the position
// part), the step offsets beside them - or the entry's refusal.  weights: the entry reads the weights (the cost-model entries and
// rmx_rollout_search): each must be finite and >= 0, and one that is > 0 needs its target table.
static int plan_frame_terms(const std::string& who, const rmx_frame_terms* ft, const int nsteps, const rmx_model* m, const bool weights,
                            std::vector<FrameDevTerm>& dterms, std::vector<int>& begin) {
    if (!ft->terms) return fail(RMX_E_INVALID, who + ": null terms");
    if (ft->nterms < 1) return fail(RMX_E_INVALID, who + ": nterms < 1");
    std::vector<rmx_track_term> pos((size_t)ft->nterms);
    for (int i = 0; i < ft->nterms; ++i) {
        const rmx_frame_term& t = ft->terms[i];
        pos[(size_t)i].body = t.body;
        for (int c = 0; c < 3; ++c) pos[(size_t)i].xlocal[c] = t.xlocal[c];
        pos[(size_t)i].step = t.step;
        pos[(size_t)i].wpos = t.wpos;
    }
    rmx_track::Plan tplan = rmx_track::plan_terms(pos.data(), ft->nterms, nsteps, m->nlist, m->node_of_listing.data());
    if (!tplan.error.empty()) return fail(RMX_E_INVALID, who + ": " + tplan.error);
    for (int i = 0; i < ft->nterms && weights; ++i) {      // the weights: the cost-model entries alone read them
        const rmx_frame_term& t = ft->terms[i];
        const struct { const char* name; double w; const void* table; const char* tname; } ws[3] = {
            {"wpos", t.wpos, ft->xtarget, "xtarget"}, {"wvel", t.wvel, ft->vtarget, "vtarget"}, {"wrot", t.wrot, ft->Rtarget, "Rtarget"}};
        for (const auto& e : ws) {
            if (!(e.w >= 0.0) || !std::isfinite(e.w))
                return fail(RMX_E_INVALID, who + ": term " + std::to_string(i) + ": " + e.name +
                                               " must be finite and >= 0 (the Gauss-Newton block must stay positive semi-definite)");
            if (e.w > 0.0 && !e.table)
                return fail(RMX_E_INVALID, who + ": term " + std::to_string(i) + ": " + e.name + " > 0 needs " + e.tname + ", which is null");
        }
    }
    dterms.resize((size_t)ft->nterms);
    for (int i = 0; i < ft->nterms; ++i) {
        dterms[(size_t)i].t = tplan.terms[(size_t)i];
        dterms[(size_t)i].wvel = ft->terms[tplan.terms[(size_t)i].orig].wvel;
        dterms[(size_t)i].wrot = ft->terms[tplan.terms[(size_t)i].orig].wrot;
    }
    begin = std::move(tplan.begin);
    return RMX_OK;
}
// ... and their copy to the batch's term area (costws_reserve'd by the caller for both parts), where a finds them
static hipError_t terms_to_device(rmx_batch* b, const std::vector<FrameDevTerm>& dterms, const std::vector<int>& begin, const size_t trk_bytes,
                                  const FrameDevTerm*& trk, const int*& trk_begin) {
    trk = (const FrameDevTerm*)b->costws;
    trk_begin = (const int*)((const char*)b->costws + trk_bytes);
    hipError_t e = hipMemcpyAsync(b->costws, dterms.data(), dterms.size() * sizeof(FrameDevTerm), hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync((char*)b->costws + trk_bytes, begin.data(), begin.size() * sizeof(int), hipMemcpyHostToDevice, b->stream);
    return e;
}
struct CostTerms {      // an entry's terms as frame terms: rmx_frame_terms as it is, rmx_point_terms with wvel = wrot = 0 and no vtarget, Rtarget
    bool given = false;
    rmx_frame_terms ft{};
    std::vector<rmx_frame_term> lifted;
    explicit CostTerms(const rmx_frame_terms* f) : given(f != nullptr) {
        if (f) ft = *f;
    }
    explicit CostTerms(const rmx_point_terms* p) : given(p != nullptr) {
        if (!p) return;
        ft.nterms = p->nterms; ft.xtarget = p->xtarget; ft.per_rollout = p->per_rollout;
        lifted.resize((size_t)std::max(p->nterms, 1));      // (never empty: a null `terms` is the caller's alone)
        for (int i = 0; p->terms && i < p->nterms; ++i) {
            const rmx_track_term& t = p->terms[i];
            lifted[(size_t)i] = rmx_frame_term{t.body, {t.xlocal[0], t.xlocal[1], t.xlocal[2]}, t.step, t.wpos, 0.0, 0.0};
        }
        ft.terms = p->terms ? lifted.data() : nullptr;
    }
};
struct FrameIO {      // the arrays of the kinematics entries (rmx_rollout_points: x, gx, gq alone)
    double *x, *v, *R;
    const double *gx, *gv, *gR;
    double *gq, *gqd;
};
// The four modes: io (the kinematics entries) or sc + out (the cost-model entries), on point terms (frames false: the point
// instantiation and its label) or frame terms.  `name` is the entry's, for the messages.
static int rollout_cost_impl(const char* name, const bool frames, rmx_batch* b, int nsteps, const double* q, const double* qdot,
                             const rmx_state_cost* sc, const CostTerms& ct, const rmx_cost_model* out, const FrameIO* io, const bool on_device) {
    const bool kin = io != nullptr;
    const std::string who = name;
    const rmx_frame_terms* ft = ct.given ? &ct.ft : nullptr;
    // (rmx_rollout_points has no qdot)
    if (!b || !q || (!qdot && (frames || !kin)) || (kin ? !ft : (!out || (!sc && !ft)))) return fail(RMX_E_INVALID, who + ": null argument");
    if (!frames && !kin && ft && !ft->xtarget) return fail(RMX_E_INVALID, who + ": null argument");
    if (kin ? (!io->x && !io->v && !io->R && !io->gq && !io->gqd) : (!out->Jk && !out->lx && !out->Q))
        return fail(RMX_E_INVALID, who + ": all outputs are null");
    if (kin && io->gq && !io->gx && !io->gv && !io->gR)
        return fail(RMX_E_INVALID, who + (frames ? ": gq needs gx, gv or gR (the cotangents of the frames)" : ": gq needs gx (the cotangents of the points)"));
    if (kin && io->gqd && !io->gv) return fail(RMX_E_INVALID, who + ": gqd needs gv (the cotangents of the velocities)");
    if (ft && ft->per_rollout != 0 && ft->per_rollout != 1) return fail(RMX_E_INVALID, who + ": per_rollout must be 0 or 1");
    if (sc && ((sc->Q_per_rollout != 0 && sc->Q_per_rollout != 1) || (sc->goal_per_rollout != 0 && sc->goal_per_rollout != 1)))
        return fail(RMX_E_INVALID, who + ": Q_per_rollout and goal_per_rollout must be 0 or 1");
    if (nsteps < 1) return fail(RMX_E_INVALID, who + ": nsteps < 1");
    rmx_model* m = b->m;
    const rmx_select::CostPlan plan = rmx_select::select_rollout_cost(step_traits(m), b->B, nsteps);
    if (plan.kernel == rmx_select::CostKernel::RefusedSpherical)
        return fail(RMX_E_INVALID, "rmx_adjoint: spherical joints are outside the adjoint path (SURVEY.md 8(f))");
    if (plan.kernel == rmx_select::CostKernel::RefusedNodes)
        return fail(RMX_E_INVALID, "rmx_adjoint: trees of more than 64 nodes are outside the adjoint path");
    if (plan.kernel != rmx_select::CostKernel::Wave) return fail(RMX_E_INVALID, who + ": batch * nsteps exceeds the grid");
    std::vector<FrameDevTerm> dterms;
    std::vector<int> begin;
    if (ft)
        if (int rc = plan_frame_terms(who, ft, nsteps, m, !kin, dterms, begin)) return rc;
    HIPCHK(hipSetDevice(m->device));
    if (int rc = pending_error_check(b, who.c_str())) return rc;
    const size_t B = (size_t)b->B, N = (size_t)nsteps, nr = (size_t)m->nr, dbl = sizeof(double);
    const size_t nterms = ft ? (size_t)ft->nterms : 0, tabs = (ft && ft->per_rollout ? B : 1) * nterms;
    const size_t bytes_traj = B * N * nr * dbl, bytes_Q = N * 4 * nr * nr * dbl;
    // (each mode has eight arrays of its own after the record: the staging room holds rmx_tape::STAGE_MAX)
    enum { S_Q, S_QD, S_XT, S_VT, S_RT, S_QIN, S_XG, S_JK, S_LX, S_QOUT };
    enum { S_X = S_QD + 1, S_V, S_R, S_GX, S_GV, S_GR, S_GQ, S_GQD };
    Staging st(on_device);
    st.add(bytes_traj, q, nullptr);
    st.add(bytes_traj, qdot, nullptr);
    if (!kin) {
        st.add(tabs * 3 * dbl, ft ? ft->xtarget : nullptr, nullptr);
        st.add(tabs * 3 * dbl, ft ? ft->vtarget : nullptr, nullptr);
        st.add(tabs * 9 * dbl, ft ? ft->Rtarget : nullptr, nullptr);
        st.add((sc && sc->Q_per_rollout ? B : 1) * bytes_Q, sc ? sc->Q : nullptr, nullptr);
        st.add((sc && sc->goal_per_rollout ? B : 1) * N * 2 * nr * dbl, sc ? sc->xgoal : nullptr, nullptr);
        st.add(B * N * dbl, nullptr, out->Jk);
        st.add(B * N * 2 * nr * dbl, nullptr, out->lx);
        st.add(B * bytes_Q, nullptr, out->Q);
    } else {
        const bool pull = io->gq || io->gqd;
        st.add(B * nterms * 3 * dbl, nullptr, io->x);
        st.add(B * nterms * 3 * dbl, nullptr, io->v);
        st.add(B * nterms * 9 * dbl, nullptr, io->R);
        st.add(B * nterms * 3 * dbl, pull ? io->gx : nullptr, nullptr);
        st.add(B * nterms * 3 * dbl, pull ? io->gv : nullptr, nullptr);
        st.add(B * nterms * 9 * dbl, io->gq ? io->gR : nullptr, nullptr);
        st.add(bytes_traj, nullptr, io->gq);
        st.add(bytes_traj, nullptr, io->gqd);
    }
    if (int rc = st.allocate(who, "the staging")) return rc;
    const size_t trk_bytes = rmx_tape::round256(nterms * sizeof(FrameDevTerm)), begin_bytes = (N + 1) * sizeof(int);
    hipError_t e = ft ? costws_reserve(b, trk_bytes + begin_bytes) : hipSuccess;
    if (e == hipErrorOutOfMemory) {
        st.release(b, hipSuccess);
        return fail(RMX_E_NOMEM, who + ": no device memory for the term table");
    }
    TaskArgs a{};
    a.nsteps = nsteps; a.nterms = (int)nterms;
    a.q = st.dev(S_Q); a.qd = st.dev(S_QD);
    if (ft && e == hipSuccess) e = terms_to_device(b, dterms, begin, trk_bytes, a.trk, a.trk_begin);
    a.t_stride = (ft && ft->per_rollout) ? nterms : 0;
    a.q_stride = (sc && sc->Q_per_rollout) ? N * 4 * nr * nr : 0;
    a.goal_stride = (sc && sc->goal_per_rollout) ? N * 2 * nr : 0;
    if (!kin) {
        a.xt = st.dev(S_XT); a.vt = st.dev(S_VT); a.Rt = st.dev(S_RT);
        a.Qin = st.dev(S_QIN); a.xgoal = st.dev(S_XG);
        a.Jk = st.dev(S_JK); a.lx = st.dev(S_LX); a.Qout = st.dev(S_QOUT);
    } else {
        a.x = st.dev(S_X); a.v = st.dev(S_V); a.R = st.dev(S_R);
        a.gx = st.dev(S_GX); a.gv = st.dev(S_GV); a.gR = st.dev(S_GR);
        a.gq = st.dev(S_GQ); a.gqd = st.dev(S_GQD);
    }
    e = st.copy_in(b, e);
    e = timed_launch(b, e, [&] {
        DISPATCH_NP(plan.np, launch_cost, m, b, a, frames)
        b->last_kernel = frames ? rmx_select::label_rollout_frames() : rmx_select::label_rollout_cost();
        return hipSuccess;
    });
    return tape_call_end(b, st.copy_out(b, e), st, who);      // (the wait keeps the term arrays alive for their copies)
}
extern "C" int rmx_rollout_points(rmx_batch* b, int nsteps, const double* q, const rmx_point_terms* pts, double* x, const double* gx, double* gq) {
    const FrameIO io{x, nullptr, nullptr, gx, nullptr, nullptr, gq, nullptr};
    return rollout_cost_impl("rmx_rollout_points", false, b, nsteps, q, nullptr, nullptr, CostTerms(pts), nullptr, &io, false);
}
extern "C" int rmx_rollout_points_device(rmx_batch* b, int nsteps, const double* d_q, const rmx_point_terms* pts, double* d_x, const double* d_gx,
                                         double* d_gq) {
    const FrameIO io{d_x, nullptr, nullptr, d_gx, nullptr, nullptr, d_gq, nullptr};
    return rollout_cost_impl("rmx_rollout_points", false, b, nsteps, d_q, nullptr, nullptr, CostTerms(pts), nullptr, &io, true);
}
extern "C" int rmx_rollout_cost(rmx_batch* b, int nsteps, const double* q, const double* qdot, const rmx_state_cost* sc, const rmx_point_terms* pts,
                                const rmx_cost_model* out) {
    return rollout_cost_impl("rmx_rollout_cost", false, b, nsteps, q, qdot, sc, CostTerms(pts), out, nullptr, false);
}
extern "C" int rmx_rollout_cost_device(rmx_batch* b, int nsteps, const double* d_q, const double* d_qdot, const rmx_state_cost* sc,
                                       const rmx_point_terms* pts, const rmx_cost_model* out) {
    return rollout_cost_impl("rmx_rollout_cost", false, b, nsteps, d_q, d_qdot, sc, CostTerms(pts), out, nullptr, true);
}
extern "C" int rmx_rollout_frames(rmx_batch* b, int nsteps, const double* q, const double* qdot, const rmx_frame_terms* ft, double* x, double* v,
                                  double* R, const double* gx, const double* gv, const double* gR, double* gq, double* gqd) {
    const FrameIO io{x, v, R, gx, gv, gR, gq, gqd};
    return rollout_cost_impl("rmx_rollout_frames", true, b, nsteps, q, qdot, nullptr, CostTerms(ft), nullptr, &io, false);
}
extern "C" int rmx_rollout_frames_device(rmx_batch* b, int nsteps, const double* d_q, const double* d_qdot, const rmx_frame_terms* ft, double* d_x,
                                         double* d_v, double* d_R, const double* d_gx, const double* d_gv, const double* d_gR, double* d_gq,
                                         double* d_gqd) {
    const FrameIO io{d_x, d_v, d_R, d_gx, d_gv, d_gR, d_gq, d_gqd};
    return rollout_cost_impl("rmx_rollout_frames", true, b, nsteps, d_q, d_qdot, nullptr, CostTerms(ft), nullptr, &io, true);
}
extern "C" int rmx_rollout_cost_frames(rmx_batch* b, int nsteps, const double* q, const double* qdot, const rmx_state_cost* sc,
                                       const rmx_frame_terms* ft, const rmx_cost_model* out) {
    return rollout_cost_impl("rmx_rollout_cost_frames", true, b, nsteps, q, qdot, sc, CostTerms(ft), out, nullptr, false);
}
extern "C" int rmx_rollout_cost_frames_device(rmx_batch* b, int nsteps, const double* d_q, const double* d_qdot, const rmx_state_cost* sc,
                                              const rmx_frame_terms* ft, const rmx_cost_model* out) {
    return rollout_cost_impl("rmx_rollout_cost_frames", true, b, nsteps, d_q, d_qdot, sc, CostTerms(ft), out, nullptr, true);
}

extern "C" int rmx_rollout_tape(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const double* u, double* qtraj,
                                double* qdtraj, rmx_stats* stats) {
    return rollout_tape_impl(b, opts, nsteps, pscale, u, qtraj, qdtraj, stats, false);
}
extern "C" int rmx_rollout_tape_device(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const double* d_u, double* d_qtraj,
                                       double* d_qdtraj, rmx_stats* stats) {
    return rollout_tape_impl(b, opts, nsteps, pscale, d_u, d_qtraj, d_qdtraj, stats, true);
}
static int rollout_feedback_impl(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, double pscale, const rmx_feedback* fb,
                                 double* qtraj, double* qdtraj, double* uapp, rmx_stats* stats, const bool on_device,
                                 const rmx_box* box = nullptr, const bool boxed = false) {
    const std::string who = boxed ? "rmx_rollout_tape_feedback_box" : "rmx_rollout_tape_feedback";
    if (!b || !fb || !fb->uff || (boxed && !box)) return fail(RMX_E_INVALID, who + ": null argument");
    if (integrator != 1 && integrator != 2) return fail(RMX_E_INVALID, who + ": integrator must be 1 (BDF1) or 2 (BDF2)");
    if (fb->per_rollout != 0 && fb->per_rollout != 1) return fail(RMX_E_INVALID, who + ": per_rollout must be 0 or 1");
    return rollout_tape_impl(b, opts, nsteps, pscale, fb->uff, qtraj, qdtraj, stats, on_device, integrator == 1 ? INTEG_BDF1 : INTEG_BDF2, fb, uapp,
                             box);
}
extern "C" int rmx_rollout_tape_feedback_box(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, double pscale, const rmx_feedback* fb,
                                             const rmx_box* box, double* qtraj, double* qdtraj, double* uapp, rmx_stats* stats) {
    return rollout_feedback_impl(b, opts, nsteps, integrator, pscale, fb, qtraj, qdtraj, uapp, stats, false, box, true);
}
extern "C" int rmx_rollout_tape_feedback_box_device(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, double pscale,
                                                    const rmx_feedback* fb, const rmx_box* box, double* d_qtraj, double* d_qdtraj,
                                                    double* d_uapp, rmx_stats* stats) {
    return rollout_feedback_impl(b, opts, nsteps, integrator, pscale, fb, d_qtraj, d_qdtraj, d_uapp, stats, true, box, true);
}
extern "C" int rmx_rollout_tape_feedback(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, double pscale, const rmx_feedback* fb,
                                         double* qtraj, double* qdtraj, double* uapp, rmx_stats* stats) {
    return rollout_feedback_impl(b, opts, nsteps, integrator, pscale, fb, qtraj, qdtraj, uapp, stats, false);
}
extern "C" int rmx_rollout_tape_feedback_device(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, double pscale,
                                                const rmx_feedback* fb, double* d_qtraj, double* d_qdtraj, double* d_uapp, rmx_stats* stats) {
    return rollout_feedback_impl(b, opts, nsteps, integrator, pscale, fb, d_qtraj, d_qdtraj, d_uapp, stats, true);
}
// rmx_rollout_search: the entry's own refusals and the plan (rmx_select.h select_rollout_search), the cost's terms planned as
// rmx_rollout_cost_frames plans them; the call itself is rollout_tape_impl's, which the entry follows without decisions of its own.
static_assert(rmx_select::SEARCH_MAX_ALPHAS == RMX_SEARCH_MAX_ALPHAS, "the plan's cap on the alphas is the header's");
static int rollout_search_impl(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const rmx_feedback* fb, const rmx_box* box,
                               const rmx_search* s, const rmx_search_cost* cost, double* qtraj, double* qdtraj, double* uapp,
                               const rmx_search_out* out, rmx_stats* stats, const bool on_device) {
    const std::string who = "rmx_rollout_search";
    if (!b || !fb || !fb->uff || !s || !cost || !out || !out->J) return fail(RMX_E_INVALID, who + ": null argument");
    if (fb->per_rollout != 0 && fb->per_rollout != 1) return fail(RMX_E_INVALID, who + ": per_rollout must be 0 or 1");
    if (!cost->sc && !cost->ft && !cost->R) return fail(RMX_E_INVALID, who + ": sc, ft and R are all null (there is no cost to search on)");
    if (s->nalpha < 0 || s->nalpha > rmx_select::SEARCH_MAX_ALPHAS)
        return fail(RMX_E_INVALID, who + ": nalpha must be 0 .. " + std::to_string(rmx_select::SEARCH_MAX_ALPHAS) + " (got " + std::to_string(s->nalpha) + ")");
    if (s->nalpha > 0 && (!s->alphas || !s->kff || !s->Jbar)) return fail(RMX_E_INVALID, who + ": nalpha > 0 needs alphas, kff and Jbar");
    for (int i = 0; i < s->nalpha; ++i)
        if (!std::isfinite(s->alphas[i]) || !(s->alphas[i] > 0.0))
            return fail(RMX_E_INVALID, who + ": alpha " + std::to_string(i) + " must be finite and > 0");
    if ((qtraj == nullptr) != (qdtraj == nullptr)) return fail(RMX_E_INVALID, "rmx_rollout_tape: qtraj and qdtraj must be given together");
    if (nsteps < 1) return fail(RMX_E_INVALID, "nsteps < 1");
    rmx_model* m = b->m;
    if (int rc = adjoint_model_refusal(m)) return rc;
    SearchCall sr{s, cost, out, rmx_select::select_rollout_search(step_traits(m), m->nr), {}, {}};
    if (sr.plan.kernel == rmx_select::SearchKernel::RefusedNr)
        return fail(RMX_E_INVALID, who + ": nr > " + std::to_string(rmx_select::LQR_MAX_NR) + " (the model has nr = " + std::to_string(m->nr) +
                                       "; the LDS-resident sweep stops at " + std::to_string(rmx_select::LQR_MAX_NR) + " reduced DOFs)");
    if (sr.plan.kernel != rmx_select::SearchKernel::Wave)
        return fail(RMX_E_INVALID, who + ": more than " + std::to_string(rmx_select::LQR_MAX_NR) + " nodes (the model has " + std::to_string(m->n) +
                                       " for nr = " + std::to_string(m->nr) + "; the LDS-resident sweep stops there)");
    const rmx_state_cost* sc = cost->sc;
    if (cost->ft && cost->ft->per_rollout != 0 && cost->ft->per_rollout != 1) return fail(RMX_E_INVALID, who + ": per_rollout must be 0 or 1");
    if (sc && ((sc->Q_per_rollout != 0 && sc->Q_per_rollout != 1) || (sc->goal_per_rollout != 0 && sc->goal_per_rollout != 1)))
        return fail(RMX_E_INVALID, who + ": Q_per_rollout and goal_per_rollout must be 0 or 1");
    if (cost->ft)
        if (int rc = plan_frame_terms(who, cost->ft, nsteps, m, true, sr.dterms, sr.begin)) return rc;
    return rollout_tape_impl(b, opts, nsteps, pscale, fb->uff, qtraj, qdtraj, stats, on_device, INTEG_BDF1, fb, uapp, box, &sr);
}
extern "C" int rmx_rollout_search(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const rmx_feedback* fb, const rmx_box* box,
                                  const rmx_search* s, const rmx_search_cost* cost, double* qtraj, double* qdtraj, double* uapp,
                                  const rmx_search_out* out, rmx_stats* stats) {
    return rollout_search_impl(b, opts, nsteps, pscale, fb, box, s, cost, qtraj, qdtraj, uapp, out, stats, false);
}
extern "C" int rmx_rollout_search_device(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const rmx_feedback* fb,
                                         const rmx_box* box, const rmx_search* s, const rmx_search_cost* cost, double* d_qtraj,
                                         double* d_qdtraj, double* d_uapp, const rmx_search_out* out, rmx_stats* stats) {
    return rollout_search_impl(b, opts, nsteps, pscale, fb, box, s, cost, d_qtraj, d_qdtraj, d_uapp, out, stats, true);
}
extern "C" int rmx_rollout_tape_bdf2(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const double* u, double* qtraj,
                                     double* qdtraj, rmx_stats* stats) {
    return rollout_tape_impl(b, opts, nsteps, pscale, u, qtraj, qdtraj, stats, false, INTEG_BDF2);
}
extern "C" int rmx_rollout_tape_bdf2_device(rmx_batch* b, const rmx_opts* opts, int nsteps, double pscale, const double* d_u, double* d_qtraj,
                                            double* d_qdtraj, rmx_stats* stats) {
    return rollout_tape_impl(b, opts, nsteps, pscale, d_u, d_qtraj, d_qdtraj, stats, true, INTEG_BDF2);
}
extern "C" int rmx_rollout_vjp(rmx_batch* b, int nsteps, const double* gq, const double* gqd, double* du, double* dq0, double* dqd0) {
    return rollout_vjp_impl(b, nsteps, gq, gqd, du, dq0, dqd0, false);
}
extern "C" int rmx_rollout_vjp_device(rmx_batch* b, int nsteps, const double* d_gq, const double* d_gqd, double* d_du, double* d_dq0,
                                      double* d_dqd0) {
    return rollout_vjp_impl(b, nsteps, d_gq, d_gqd, d_du, d_dq0, d_dqd0, true);
}
extern "C" int rmx_rollout_vjp_feedback(rmx_batch* b, int nsteps, const rmx_feedback* fb, const double* gq, const double* gqd, const double* gu,
                                        const rmx_feedback_grads* out) {
    return rollout_vjp_feedback_impl(b, nsteps, fb, gq, gqd, gu, out, false);
}
extern "C" int rmx_rollout_vjp_feedback_device(rmx_batch* b, int nsteps, const rmx_feedback* fb, const double* d_gq, const double* d_gqd,
                                               const double* d_gu, const rmx_feedback_grads* out) {
    return rollout_vjp_feedback_impl(b, nsteps, fb, d_gq, d_gqd, d_gu, out, true);
}
extern "C" int rmx_rollout_vjp_params(rmx_batch* b, int nsteps, const double* gq, const double* gqd, double* du, double* dq0, double* dqd0,
                                      const rmx_param_grads* out) {
    return rollout_vjp_params_impl(b, nsteps, gq, gqd, du, dq0, dqd0, out, false);
}
extern "C" int rmx_rollout_vjp_params_device(rmx_batch* b, int nsteps, const double* d_gq, const double* d_gqd, double* d_du, double* d_dq0,
                                             double* d_dqd0, const rmx_param_grads* out) {
    return rollout_vjp_params_impl(b, nsteps, d_gq, d_gqd, d_du, d_dq0, d_dqd0, out, true);
}
extern "C" int rmx_rollout_vjp_forces(rmx_batch* b, int nsteps, const double* gq, const double* gqd, double* du, double* dq0, double* dqd0,
                                      const rmx_param_grads* model, const rmx_force_grads* forces) {
    return rollout_vjp_forces_impl(b, nsteps, gq, gqd, du, dq0, dqd0, model, forces, false);
}
extern "C" int rmx_rollout_vjp_forces_device(rmx_batch* b, int nsteps, const double* d_gq, const double* d_gqd, double* d_du, double* d_dq0,
                                             double* d_dqd0, const rmx_param_grads* model, const rmx_force_grads* forces) {
    return rollout_vjp_forces_impl(b, nsteps, d_gq, d_gqd, d_du, d_dq0, d_dqd0, model, forces, true);
}
extern "C" int rmx_rollout_linearize(rmx_batch* b, int nsteps, double* XA, double* XB, double* XU) {
    return rollout_linearize_impl(b, nsteps, XA, XB, XU, false);
}
extern "C" int rmx_rollout_linearize_device(rmx_batch* b, int nsteps, double* d_XA, double* d_XB, double* d_XU) {
    return rollout_linearize_impl(b, nsteps, d_XA, d_XB, d_XU, true);
}
extern "C" int rmx_rollout_jvp(rmx_batch* b, int nsteps, int ntan, const double* tu, const double* tq0, const double* tqd0, double* tq,
                               double* tqd) {
    return rollout_jvp_impl(b, nsteps, ntan, tu, tq0, tqd0, tq, tqd, false);
}
extern "C" int rmx_rollout_jvp_device(rmx_batch* b, int nsteps, int ntan, const double* d_tu, const double* d_tq0, const double* d_tqd0,
                                      double* d_tq, double* d_tqd) {
    return rollout_jvp_impl(b, nsteps, ntan, d_tu, d_tq0, d_tqd0, d_tq, d_tqd, true);
}
extern "C" int rmx_rollout_jvp_params(rmx_batch* b, int nsteps, int ntan, const rmx_param_tangents* tp, const double* tu, const double* tq0,
                                      const double* tqd0, double* tq, double* tqd) {
    return rollout_jvp_params_impl(b, nsteps, ntan, tp, tu, tq0, tqd0, tq, tqd, false);
}
extern "C" int rmx_rollout_jvp_params_device(rmx_batch* b, int nsteps, int ntan, const rmx_param_tangents* tp, const double* d_tu,
                                             const double* d_tq0, const double* d_tqd0, double* d_tq, double* d_tqd) {
    return rollout_jvp_params_impl(b, nsteps, ntan, tp, d_tu, d_tq0, d_tqd0, d_tq, d_tqd, true);
}

static int track_refusal(const rmx_task_track* task, const double* xtarget, int integrator) {
    if (!task) return fail(RMX_E_INVALID, "rmx_adjoint_track: null task");
    if (!task->terms) return fail(RMX_E_INVALID, "rmx_adjoint_track: null terms");
    if (!xtarget) return fail(RMX_E_INVALID, "rmx_adjoint_track: null xtarget");
    if (task->nterms < 1) return fail(RMX_E_INVALID, "rmx_adjoint_track: nterms < 1");
    if (integrator != 1 && integrator != 2) return fail(RMX_E_INVALID, "rmx_adjoint_track: integrator must be 1 (BDF1) or 2 (BDF2)");
    return RMX_OK;
}
extern "C" int rmx_adjoint_track(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, const rmx_task_track* task,
                                 const double* u, double* P, double* dPdu, rmx_stats* stats) {
    if (int rc = track_refusal(task, task ? task->xtarget : nullptr, integrator)) return rc;
    return adjoint_impl(b, opts, nsteps, nullptr, u, P, dPdu, stats, integrator == 1 ? INTEG_BDF1 : INTEG_BDF2, false, true, task, task->xtarget);
}
extern "C" int rmx_adjoint_track_device(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, const rmx_task_track* task,
                                        const double* d_xtarget, const double* d_u, double* d_P, double* d_dPdu, rmx_stats* stats) {
    if (int rc = track_refusal(task, d_xtarget, integrator)) return rc;
    return adjoint_impl(b, opts, nsteps, nullptr, d_u, d_P, d_dPdu, stats, integrator == 1 ? INTEG_BDF1 : INTEG_BDF2, true, true, task, d_xtarget);
}

// simLoop of one batch enqueued on its stream, nothing waited for (include/redmax_hip.h "Asynchronous stepping")
static int step_async(rmx_batch* b, const rmx_opts* opts, int nsteps, int integ, int record) {
    if (!b) return fail(RMX_E_INVALID, "null batch");
    if (nsteps < 0) return fail(RMX_E_INVALID, "nsteps < 0");
    if (record & ~(RMX_REC_ENERGY | RMX_REC_STATE | RMX_REC_CHARTS)) return fail(RMX_E_INVALID, "record: unknown RMX_REC_* bits");
    HIPCHK(hipSetDevice(b->m->device));
    if (b->async_pending && (b->hist.T || b->hist.Q || b->hist.C)) {
        // the launch in flight writes the record that is about to be replaced: wait for it (stacked async steps without a record
        // need no wait - the stream orders them)
        HIPCHK(hipStreamSynchronize(b->stream));
    }
    int rc = hist_alloc(b, nsteps, record);
    if (rc) return rc;
    if (nsteps == 0 || b->m->nr == 0) return RMX_OK;
    rc = launch_step(b, opts, nsteps, integ, true, b->hist.T, b->hist.V, b->hist.Q, b->hist.Qd, b->hist.C);   // counters accumulate on the device
    if (rc == RMX_OK) b->async_pending = true;      // until rmx_sync (or any synchronous call on this batch) has waited for it
    return rc;
}
extern "C" int rmx_step_bdf1_async(rmx_batch* b, const rmx_opts* opts, int nsteps) { return step_async(b, opts, nsteps, INTEG_BDF1, 0); }
extern "C" int rmx_step_bdf2_async(rmx_batch* b, const rmx_opts* opts, int nsteps) { return step_async(b, opts, nsteps, INTEG_BDF2, 0); }
extern "C" int rmx_step_history_async(rmx_batch* b, const rmx_opts* opts, int nsteps, int integrator, int record) {
    if (integrator != 1 && integrator != 2) return fail(RMX_E_INVALID, "integrator must be 1 (BDF1) or 2 (BDF2)");
    return step_async(b, opts, nsteps, integrator == 1 ? INTEG_BDF1 : INTEG_BDF2, record);
}
static int history_read(rmx_batch* b, const rmx_history* hist, size_t pitchB, size_t first) {
    if (!b || !hist) return fail(RMX_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(b->m->device));
    if (b->async_pending) {
        const int rc = rmx_sync(b);
        if (rc) return rc;
    }
    const int rc = hist_copy_out(b, hist, pitchB, first);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));
    return RMX_OK;
}
extern "C" int rmx_history_read(rmx_batch* b, const rmx_history* hist) { return history_read(b, hist, b ? (size_t)b->B : 0, 0); }
extern "C" int rmx_stats_reset(rmx_batch* b) {
    if (!b) return fail(RMX_E_INVALID, "null batch");
    HIPCHK(hipSetDevice(b->m->device));
    HIPCHK(hipMemsetAsync(b->it, 0, sizeof(int) * b->B, b->stream));
    HIPCHK(hipMemsetAsync(b->ls, 0, sizeof(int) * b->B, b->stream));
    HIPCHK(hipMemsetAsync(b->status, 0, sizeof(int) * b->B, b->stream));
    return RMX_OK;
}
extern "C" int rmx_stats_read(rmx_batch* b, rmx_stats* st) {
    if (!b || !st) return fail(RMX_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(b->m->device));
    if (st->newton_iters) HIPCHK(hipMemcpyAsync(st->newton_iters, b->it, sizeof(int) * b->B, hipMemcpyDeviceToHost, b->stream));
    if (st->ls_halvings) HIPCHK(hipMemcpyAsync(st->ls_halvings, b->ls, sizeof(int) * b->B, hipMemcpyDeviceToHost, b->stream));
    if (st->status) HIPCHK(hipMemcpyAsync(st->status, b->status, sizeof(int) * b->B, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->async_pending = false;
    return RMX_OK;
}
// How the time of the last rmx_step_* launch was spread over the rollouts: shader-clock ticks (s_memtime) every rollout's wavefront
// spent inside the kernel(s).  A launch ends with its slowest rollout; this is the per-rollout distribution behind that.
extern "C" int rmx_step_ticks(rmx_batch* b, unsigned long long* ticks) {
    if (!b || !ticks) return fail(RMX_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(b->m->device));
    HIPCHK(hipMemcpyAsync(ticks, b->ticks, sizeof(unsigned long long) * b->B, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->async_pending = false;
    return RMX_OK;
}

extern "C" int rmx_sync(rmx_batch* b) {
    if (!b) return fail(RMX_E_INVALID, "null batch");
    HIPCHK(hipSetDevice(b->m->device));
    const hipError_t es = wait_stream_short(b->stream);
    b->async_pending = false;
    if (es != hipSuccess) return fail(RMX_E_HIP, std::string("rmx_sync: the asynchronous launch failed: ") + hipGetErrorString(es));
    take_event_time(b);
    return RMX_OK;
}

extern "C" int rmx_profile_phases(rmx_batch* b, int reps, double h, double* cycles4) {
    if (!b || !cycles4 || reps < 1) return fail(RMX_E_INVALID, "bad argument");
    rmx_model* m = b->m;
    if (m->big) return fail(RMX_E_INVALID, "rmx_profile_phases: one-wavefront kernels only (trees of up to 64 nodes)");
    HIPCHK(hipSetDevice(m->device));
    if (int rc = pending_error_check(b, "rmx_profile_phases")) return rc;
    unsigned long long* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, sizeof(unsigned long long) * 16 * b->B));
    // the full 32-link chain: the stages of the kernel that runs it (part_pair32.hip); everything else: the generic device functions
    if (rmx_select::full_chain32_plain(step_traits(m))) launch_phase_pairchain_32(m, b, reps, h, d);
    else { DISPATCH_NP(m->NP, launch_phase, m, b, reps, h, d); }
    std::vector<unsigned long long> hbuf(16 * (size_t)b->B);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(hbuf.data(), d, sizeof(unsigned long long) * hbuf.size(), hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(RMX_E_HIP, std::string("rmx_profile_phases: ") + hipGetErrorString(e));
    for (int k = 0; k < 16; ++k) {   // [0..3] phase totals, [4..15] stamps inside the (g,H) evaluation
        double sum = 0;
        for (int t = 0; t < b->B; ++t) sum += (double)hbuf[16 * (size_t)t + k];
        cycles4[k] = sum / ((double)b->B * reps);
    }
    return RMX_OK;
}

extern "C" int rmx_energy(rmx_batch* b, double* T, double* V) {
    if (!b || !T || !V) return fail(RMX_E_INVALID, "null argument");
    rmx_model* m = b->m;
    HIPCHK(hipSetDevice(m->device));
    if (int rc = pending_error_check(b, "rmx_energy")) return rc;
    double *dT = nullptr, *dV = nullptr;
    HIPCHK(hipMalloc((void**)&dT, sizeof(double) * b->B));
    hipError_t e = hipMalloc((void**)&dV, sizeof(double) * b->B);
    if (e != hipSuccess) { (void)hipFree(dT); return fail(RMX_E_NOMEM, "hipMalloc(energy)"); }
    if (m->big) launch_big_energy(m, b, dT, dV);
    else if (m->dpf) { DISPATCH_NP(m->NP, launch_energy_pf, m, b, dT, dV); }
    else if (m->dm.con || m->dm.nsph) { DISPATCH_NP(m->NP, launch_energy_ct, m, b, dT, dV); }
    else { DISPATCH_NP(m->NP, launch_energy, m, b, dT, dV); }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(T, dT, sizeof(double) * b->B, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(V, dV, sizeof(double) * b->B, hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    (void)hipFree(dT);
    (void)hipFree(dV);
    if (e != hipSuccess) return fail(RMX_E_HIP, std::string("rmx_energy: ") + hipGetErrorString(e));
    return RMX_OK;
}


// ============================================================================ multi-device groups (include/redmax_hip.h, ABI 107)
#include <chrono>

// ---- RCCL, bound at run time.  libredmax_hip.so links the HIP runtime only; the one collective of the path (north_star: "RCCL over
// xGMI only for the final gather") needs librccl when a group spans several DISTINCT devices, and a host without it still simulates
// (rmx_group_gather_device then says so).  The entry points are resolved from librccl.so(.1) on first use; the types come from rccl.h.
#include <dlfcn.h>
#include <rccl/rccl.h>
namespace {
struct Rccl {
    void* lib = nullptr;
    bool tried = false;
    std::string why;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
};
Rccl g_rccl;
std::mutex g_rccl_mu;
bool rccl_load() {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.tried) return g_rccl.lib != nullptr;
    g_rccl.tried = true;
    const char* env = getenv("RMX_RCCL_LIB");
    const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* nm : names) {
        if (!nm || !*nm) continue;
        g_rccl.lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
        if (g_rccl.lib) break;
        g_rccl.why = dlerror() ? dlerror() : "dlopen failed";
    }
    if (!g_rccl.lib) return false;
    bool ok = true;
#define RMX_SYM(field, name) ok = ok && ((g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(g_rccl.lib, name))) != nullptr)
    RMX_SYM(CommInitAll, "ncclCommInitAll"); RMX_SYM(CommDestroy, "ncclCommDestroy"); RMX_SYM(GetErrorString, "ncclGetErrorString");
    RMX_SYM(AllGather, "ncclAllGather"); RMX_SYM(Broadcast, "ncclBroadcast"); RMX_SYM(Send, "ncclSend"); RMX_SYM(Recv, "ncclRecv");
    RMX_SYM(GroupStart, "ncclGroupStart"); RMX_SYM(GroupEnd, "ncclGroupEnd");
#undef RMX_SYM
    if (!ok) {
        g_rccl.why = "librccl lacks an entry point this library binds";
        dlclose(g_rccl.lib);
        g_rccl.lib = nullptr;
    }
    return ok;
}
}  // namespace

struct rmx_group {
    int B = 0, nr = 0;
    std::vector<rmx_model*> models;
    std::vector<rmx_batch*> batches;
    std::vector<int> device, first, count;
    std::chrono::steady_clock::time_point t0;
    double wall_ms = 0.0;
    bool in_flight = false;
    // rmx_group_gather_device: one RCCL communicator per shard (a single-process clique, ncclCommInitAll on the device list), created
    // at the first gather of a group whose devices are pairwise distinct; a group that lists a device twice gathers by peer copies
    std::vector<ncclComm_t> comms;
    int gather_path = 0;            // 0 not decided, 1 RCCL, 2 peer copies (a device is listed more than once, or RMX_GROUP_GATHER=copy)
    const char* last_gather = "";   // "rccl:allgather" | "rccl:broadcast" | "rccl:sendrecv" | "copy" (rmx_group_gather_path)
    std::vector<double*> gq, gqd;   // rmx_group_gather: the group's own [batch][nr] destinations, one pair per shard's device (on demand)
};

extern "C" void rmx_group_destroy(rmx_group* g) {
    if (!g) return;
    for (ncclComm_t c : g->comms)
        if (c && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c);
    for (size_t s = 0; s < g->gq.size(); ++s) {
        if (g->gq[s] || g->gqd[s]) (void)hipSetDevice(g->device[s]);
        if (g->gq[s]) (void)hipFree(g->gq[s]);
        if (g->gqd[s]) (void)hipFree(g->gqd[s]);
    }
    for (rmx_batch* b : g->batches) rmx_batch_destroy(b);
    for (rmx_model* m : g->models) rmx_model_destroy(m);
    delete g;
}

extern "C" int rmx_group_create(const rmx_model_desc* desc, const rmx_ground_contact* gc, int batch, const int* devices, int ndevices,
                                rmx_group** out) {
    if (!desc || !out) return fail(RMX_E_INVALID, "null argument");
    *out = nullptr;
    if (batch < 1) return fail(RMX_E_INVALID, "batch must be >= 1");
    if (ndevices < 1) return fail(RMX_E_INVALID, "ndevices must be >= 1");
    if (ndevices > batch) return fail(RMX_E_INVALID, "more shards than trajectories");
    rmx_group* g = new rmx_group();
    g->B = batch;
    // contiguous shards in device-list order, sizes differing by at most one (sharding.plan(..., "strong"))
    const int base = batch / ndevices, extra = batch % ndevices;
    int at = 0;
    for (int s = 0; s < ndevices; ++s) {
        const int cnt = base + (s < extra ? 1 : 0);
        rmx_model* m = nullptr;
        rmx_batch* b = nullptr;
        int rc = rmx_model_create(desc, devices ? devices[s] : s, &m);
        if (rc == RMX_OK) {
            g->models.push_back(m);
            if (gc) rc = rmx_model_set_ground_contact(m, gc);
        }
        if (rc == RMX_OK) rc = rmx_batch_create(m, cnt, &b);
        if (rc != RMX_OK) {
            const std::string msg = "rmx_group_create, shard " + std::to_string(s) + ": " + g_err;
            rmx_group_destroy(g);
            return fail(rc, msg);
        }
        g->batches.push_back(b);
        g->device.push_back(m->device);
        g->first.push_back(at);
        g->count.push_back(cnt);
        at += cnt;
    }
    g->nr = g->models[0]->nr;
    *out = g;
    return RMX_OK;
}
extern "C" int rmx_group_batch_size(const rmx_group* g) { return g ? g->B : RMX_E_INVALID; }
extern "C" int rmx_group_nshards(const rmx_group* g) { return g ? (int)g->batches.size() : RMX_E_INVALID; }
extern "C" int rmx_group_shard(const rmx_group* g, int s, int* device, int* first, int* count) {
    if (!g || s < 0 || s >= (int)g->batches.size()) return fail(RMX_E_INVALID, "rmx_group_shard: bad argument");
    if (device) *device = g->device[s];
    if (first) *first = g->first[s];
    if (count) *count = g->count[s];
    return RMX_OK;
}
extern "C" rmx_batch* rmx_group_shard_batch(rmx_group* g, int s) { return (g && s >= 0 && s < (int)g->batches.size()) ? g->batches[s] : nullptr; }
extern "C" rmx_model* rmx_group_shard_model(rmx_group* g, int s) { return (g && s >= 0 && s < (int)g->models.size()) ? g->models[s] : nullptr; }

extern "C" int rmx_group_set_state(rmx_group* g, const double* q, const double* qdot) {
    if (!g) return fail(RMX_E_INVALID, "null group");
    for (size_t s = 0; s < g->batches.size(); ++s) {
        const size_t off = (size_t)g->first[s] * g->nr;
        if (int rc = rmx_set_state(g->batches[s], q ? q + off : nullptr, qdot ? qdot + off : nullptr)) return rc;
    }
    return RMX_OK;
}
extern "C" int rmx_group_get_state(rmx_group* g, double* q, double* qdot) {
    if (!g) return fail(RMX_E_INVALID, "null group");
    for (size_t s = 0; s < g->batches.size(); ++s) {
        const size_t off = (size_t)g->first[s] * g->nr;
        if (int rc = rmx_get_state(g->batches[s], q ? q + off : nullptr, qdot ? qdot + off : nullptr)) return rc;
    }
    return RMX_OK;
}
// The final gather of the path with DEVICE-resident destinations (north_star: "RCCL over xGMI only for the final gather"; SURVEY.md
// 8(e): one collective at the end of the rollout, [B/N][nr] x 2 per shard).  d_q[s], d_qdot[s]: [batch][nr] arrays on shard s's device
// (null for a shard that receives nothing).  root_or_all = RMX_GATHER_ALL: every shard's device ends up with the whole batch
// (ncclAllGather when the shards are equal, one ncclBroadcast per shard inside a group call otherwise); a shard index: that shard's
// device alone (ncclSend / ncclRecv).  The collective is enqueued on the shards' own streams, behind their step kernels - no host
// synchronisation between the rollout and the gather -, and the call returns when every stream has drained.
static int gather_fail(rmx_group* g, ncclResult_t r, const char* what) {
    (void)g;
    return fail(RMX_E_HIP, std::string("rmx_group_gather_device: ") + what + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "RCCL error"));
}
extern "C" int rmx_group_gather_device(rmx_group* g, double* const* d_q, double* const* d_qdot, int root_or_all) {
    if (!g || !d_q || !d_qdot) return fail(RMX_E_INVALID, "null argument");
    const int S = (int)g->batches.size();
    const bool all = root_or_all == RMX_GATHER_ALL;
    if (!all && (root_or_all < 0 || root_or_all >= S)) return fail(RMX_E_INVALID, "rmx_group_gather_device: root must be a shard index or RMX_GATHER_ALL");
    for (int s = 0; s < S; ++s)
        if ((all || s == root_or_all) && (!d_q[s] || !d_qdot[s])) return fail(RMX_E_INVALID, "rmx_group_gather_device: a receiving shard has no destination");
    if (g->gather_path == 0) {
        bool dup = false;
        for (int a = 0; a < S; ++a)
            for (int c = a + 1; c < S; ++c) dup = dup || g->device[a] == g->device[c];
        const char* force = getenv("RMX_GROUP_GATHER");
        if (dup || (force && !strcmp(force, "copy"))) {
            g->gather_path = 2;       // RCCL refuses a clique that names a GPU twice: such shards exchange by (peer) copies
        } else {
            if (!rccl_load()) return fail(RMX_E_HIP, "rmx_group_gather_device: librccl could not be loaded (" + g_rccl.why + "); RMX_GROUP_GATHER=copy gathers by peer copies");
            g->comms.assign(S, nullptr);
            const ncclResult_t r = g_rccl.CommInitAll(g->comms.data(), S, g->device.data());
            if (r != ncclSuccess) { g->comms.clear(); return gather_fail(g, r, "ncclCommInitAll"); }
            g->gather_path = 1;
        }
    }
    const size_t nr = (size_t)g->nr;
    if (g->gather_path == 2) {
        g->last_gather = "copy";
        for (int src = 0; src < S; ++src) {
            rmx_batch* b = g->batches[src];
            const size_t off = (size_t)g->first[src] * nr, bytes = (size_t)g->count[src] * nr * sizeof(double);
            for (int dst = 0; dst < S; ++dst) {
                if (!(all || dst == root_or_all)) continue;
                // on the SOURCE shard's stream, behind its step kernel; the destination is idle memory of the caller's
                HIPCHK(hipSetDevice(g->device[src]));
                if (g->device[src] == g->device[dst]) {
                    HIPCHK(hipMemcpyAsync(d_q[dst] + off, b->q, bytes, hipMemcpyDeviceToDevice, b->stream));
                    HIPCHK(hipMemcpyAsync(d_qdot[dst] + off, b->qd, bytes, hipMemcpyDeviceToDevice, b->stream));
                } else {
                    HIPCHK(hipMemcpyPeerAsync(d_q[dst] + off, g->device[dst], b->q, g->device[src], bytes, b->stream));
                    HIPCHK(hipMemcpyPeerAsync(d_qdot[dst] + off, g->device[dst], b->qd, g->device[src], bytes, b->stream));
                }
            }
        }
    } else {
        bool equal = true;
        for (int s = 1; s < S; ++s) equal = equal && g->count[s] == g->count[0];
        ncclResult_t r = g_rccl.GroupStart();
        if (r != ncclSuccess) return gather_fail(g, r, "ncclGroupStart");
        if (all && equal) {
            g->last_gather = "rccl:allgather";
            const size_t cnt = (size_t)g->count[0] * nr;
            for (int s = 0; s < S && r == ncclSuccess; ++s) {
                r = g_rccl.AllGather(g->batches[s]->q, d_q[s], cnt, ncclDouble, g->comms[s], g->batches[s]->stream);
                if (r == ncclSuccess) r = g_rccl.AllGather(g->batches[s]->qd, d_qdot[s], cnt, ncclDouble, g->comms[s], g->batches[s]->stream);
            }
        } else if (all) {
            g->last_gather = "rccl:broadcast";      // shards that differ by one rollout: the all-gather as one broadcast per shard
            for (int root = 0; root < S && r == ncclSuccess; ++root) {
                const size_t off = (size_t)g->first[root] * nr, cnt = (size_t)g->count[root] * nr;
                for (int s = 0; s < S && r == ncclSuccess; ++s) {
                    r = g_rccl.Broadcast(g->batches[root]->q, d_q[s] + off, cnt, ncclDouble, root, g->comms[s], g->batches[s]->stream);
                    if (r == ncclSuccess) r = g_rccl.Broadcast(g->batches[root]->qd, d_qdot[s] + off, cnt, ncclDouble, root, g->comms[s], g->batches[s]->stream);
                }
            }
        } else {
            g->last_gather = "rccl:sendrecv";
            const int root = root_or_all;
            for (int s = 0; s < S && r == ncclSuccess; ++s) {
                const size_t off = (size_t)g->first[s] * nr, cnt = (size_t)g->count[s] * nr;
                if (s == root) {      // the root's own slice: a copy on its stream
                    if (hipSetDevice(g->device[s]) != hipSuccess ||
                        hipMemcpyAsync(d_q[root] + off, g->batches[s]->q, cnt * sizeof(double), hipMemcpyDeviceToDevice, g->batches[s]->stream) != hipSuccess ||
                        hipMemcpyAsync(d_qdot[root] + off, g->batches[s]->qd, cnt * sizeof(double), hipMemcpyDeviceToDevice, g->batches[s]->stream) != hipSuccess) {
                        (void)g_rccl.GroupEnd();
                        return fail(RMX_E_HIP, "rmx_group_gather_device: copying the root's own slice failed");
                    }
                    continue;
                }
                r = g_rccl.Send(g->batches[s]->q, cnt, ncclDouble, root, g->comms[s], g->batches[s]->stream);
                if (r == ncclSuccess) r = g_rccl.Send(g->batches[s]->qd, cnt, ncclDouble, root, g->comms[s], g->batches[s]->stream);
                if (r == ncclSuccess) r = g_rccl.Recv(d_q[root] + off, cnt, ncclDouble, s, g->comms[root], g->batches[root]->stream);
                if (r == ncclSuccess) r = g_rccl.Recv(d_qdot[root] + off, cnt, ncclDouble, s, g->comms[root], g->batches[root]->stream);
            }
        }
        const ncclResult_t re = g_rccl.GroupEnd();
        if (r != ncclSuccess) return gather_fail(g, r, g->last_gather);
        if (re != ncclSuccess) return gather_fail(g, re, "ncclGroupEnd");
    }
    for (int s = 0; s < S; ++s) {
        HIPCHK(hipSetDevice(g->device[s]));
        HIPCHK(hipStreamSynchronize(g->batches[s]->stream));
    }
    return RMX_OK;
}
extern "C" const char* rmx_group_gather_path(const rmx_group* g) { return g ? g->last_gather : ""; }
// the same gather into destinations the GROUP owns (for hosts that cannot allocate device memory themselves: the MEX gateway)
extern "C" int rmx_group_gather(rmx_group* g, int root_or_all) {
    if (!g) return fail(RMX_E_INVALID, "null group");
    const int S = (int)g->batches.size();
    if (root_or_all != RMX_GATHER_ALL && (root_or_all < 0 || root_or_all >= S)) return fail(RMX_E_INVALID, "rmx_group_gather: root must be a shard index or RMX_GATHER_ALL");
    if (g->gq.empty()) { g->gq.assign(S, nullptr); g->gqd.assign(S, nullptr); }
    const size_t bytes = (size_t)g->B * g->nr * sizeof(double);
    for (int s = 0; s < S; ++s) {
        if (!(root_or_all == RMX_GATHER_ALL || s == root_or_all)) continue;
        HIPCHK(hipSetDevice(g->device[s]));
        if (!g->gq[s]) HIPCHK(hipMalloc((void**)&g->gq[s], bytes ? bytes : 8));
        if (!g->gqd[s]) HIPCHK(hipMalloc((void**)&g->gqd[s], bytes ? bytes : 8));
    }
    return rmx_group_gather_device(g, g->gq.data(), g->gqd.data(), root_or_all);
}
extern "C" int rmx_group_gathered(rmx_group* g, int s, const double** d_q, const double** d_qdot) {
    if (!g || s < 0 || s >= (int)g->gq.size() || !g->gq[s] || !g->gqd[s]) return fail(RMX_E_INVALID, "rmx_group_gathered: shard holds no gathered state (rmx_group_gather first)");
    if (d_q) *d_q = g->gq[s];
    if (d_qdot) *d_qdot = g->gqd[s];
    return RMX_OK;
}
extern "C" int rmx_group_gathered_read(rmx_group* g, int s, double* q, double* qdot) {
    const double *dq = nullptr, *dqd = nullptr;
    if (int rc = rmx_group_gathered(g, s, &dq, &dqd)) return rc;
    const size_t bytes = (size_t)g->B * g->nr * sizeof(double);
    HIPCHK(hipSetDevice(g->device[s]));
    if (q) HIPCHK(hipMemcpy(q, dq, bytes, hipMemcpyDeviceToHost));
    if (qdot) HIPCHK(hipMemcpy(qdot, dqd, bytes, hipMemcpyDeviceToHost));
    return RMX_OK;
}

extern "C" int rmx_group_energy(rmx_group* g, double* T, double* V) {
    if (!g || !T || !V) return fail(RMX_E_INVALID, "null argument");
    for (size_t s = 0; s < g->batches.size(); ++s)
        if (int rc = rmx_energy(g->batches[s], T + g->first[s], V + g->first[s])) return rc;
    return RMX_OK;
}

// simLoop of the whole batch, first half: every shard's launch is in flight when this returns
extern "C" int rmx_group_step_async(rmx_group* g, const rmx_opts* opts, int nsteps, int integrator, int record) {
    if (!g) return fail(RMX_E_INVALID, "null group");
    if (integrator != 1 && integrator != 2) return fail(RMX_E_INVALID, "integrator must be 1 (BDF1) or 2 (BDF2)");
    for (rmx_batch* b : g->batches)
        if (int rc = rmx_stats_reset(b)) return rc;          // (enqueued on the shard's stream ahead of its launch)
    g->t0 = std::chrono::steady_clock::now();
    g->in_flight = true;
    for (rmx_batch* b : g->batches)
        if (int rc = rmx_step_history_async(b, opts, nsteps, integrator, record)) return rc;
    return RMX_OK;
}
// second half: wait for every shard, then the gather - each shard's slice of the counters and of the per-step record goes straight
// into its place in the caller's whole-batch arrays
extern "C" int rmx_group_sync(rmx_group* g, rmx_stats* stats, const rmx_history* hist) {
    if (!g) return fail(RMX_E_INVALID, "null group");
    int rc = RMX_OK;
    std::string first_err;
    for (rmx_batch* b : g->batches) {
        const int r = rmx_sync(b);          // wait for ALL of them even when one has failed: nothing may stay in flight
        if (r && !rc) { rc = r; first_err = g_err; }
    }
    if (g->in_flight) {
        g->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g->t0).count();
        g->in_flight = false;
    }
    if (rc) return fail(rc, first_err);
    for (size_t s = 0; s < g->batches.size(); ++s) {
        rmx_batch* b = g->batches[s];
        const size_t f = (size_t)g->first[s];
        if (hist && b->hist.nsteps > 0)
            if (int r = history_read(b, hist, (size_t)g->B, f)) return r;
        if (stats) {
            rmx_stats st{stats->newton_iters ? stats->newton_iters + f : nullptr, stats->ls_halvings ? stats->ls_halvings + f : nullptr,
                         stats->status ? stats->status + f : nullptr};
            if (int r = rmx_stats_read(b, &st)) return r;
        }
    }
    return RMX_OK;
}
extern "C" int rmx_group_step(rmx_group* g, const rmx_opts* opts, int nsteps, int integrator, rmx_stats* stats, const rmx_history* hist) {
    if (!g) return fail(RMX_E_INVALID, "null group");
    if (nsteps < 0) return fail(RMX_E_INVALID, "nsteps < 0");
    int record = 0;
    if (hist) {
        if ((hist->T == nullptr) != (hist->V == nullptr)) return fail(RMX_E_INVALID, "history T and V must be given together");
        if ((hist->q == nullptr) != (hist->qdot == nullptr)) return fail(RMX_E_INVALID, "history q and qdot must be given together");
        record = (hist->T ? RMX_REC_ENERGY : 0) | (hist->q ? RMX_REC_STATE : 0) | (hist->charts ? RMX_REC_CHARTS : 0);
    }
    const int rc = rmx_group_step_async(g, opts, nsteps, integrator, record);
    const int rs = rmx_group_sync(g, rc ? nullptr : stats, rc ? nullptr : hist);     // (also after a failed launch: drain what did start)
    return rc ? rc : rs;
}
extern "C" int rmx_group_timing(rmx_group* g, double* wall_ms, double* kernel_ms, double* start_ms, double* end_ms) {
    if (!g) return fail(RMX_E_INVALID, "null group");
    if (wall_ms) *wall_ms = g->wall_ms;
    for (size_t s = 0; s < g->batches.size(); ++s) {
        rmx_batch* b = g->batches[s];
        if (kernel_ms) kernel_ms[s] = b->last_ms;
        size_t ref = s;
        for (size_t r = 0; r < s; ++r)
            if (g->device[r] == g->device[s]) { ref = r; break; }
        float t0 = 0.f, t1 = (float)b->last_ms;
        if (ref != s) {
            HIPCHK(hipSetDevice(g->device[s]));
            if (hipEventElapsedTime(&t0, g->batches[ref]->ev0, b->ev0) != hipSuccess || hipEventElapsedTime(&t1, g->batches[ref]->ev0, b->ev1) != hipSuccess) {
                (void)hipGetLastError();
                t0 = 0.f; t1 = (float)b->last_ms;
            }
        }
        if (start_ms) start_ms[s] = t0;
        if (end_ms) end_ms[s] = t1;
    }
    return RMX_OK;
}
