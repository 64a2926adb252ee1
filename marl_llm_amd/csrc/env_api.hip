// env_api.hip -- the host side of the env library: the swarm_env handle's bookkeeping, lattice detection and the choice of
// the cell path, and every entry point of the C ABI (include/swarm_env.h) but the two debug ones that read the step
// kernel's own tables.  No kernel is defined or named here: the step kernel is reached through env_layout / env_launch
// (swarm_env.hip) -- on a handle created with large_swarm the two large-swarm kernels through large_launch (env_large.hip)
// instead: step_launch below is the one place that chooses --, the side kernels through their launchers (env_kernels.hip); env_types.h declares both.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "swarm_env.h"
#include "env_types.h"

using namespace swarm_internal;

namespace {

thread_local std::string g_create_error;

// sqrt(d2) <= t  <=>  d2 < cut_le(t)
double cut_le(double t) { return cut_lt(std::nextafter(t, INFINITY)); }

int npad_for(int n)
{
    int v = 8;
    while (v < n) v <<= 1;
    return v;
}

// One pass of the handle, on its stream: the step kernel's launch, or on a large_swarm handle the large-swarm kernels' --
// every pass of such a handle, at any n_agents
int step_launch(swarm_env *h, const Pass &ps)
{
    return h->cfg.large_swarm ? large_launch(h, ps) : env_launch(h, ps);
}

// Is this cell list a row-major subset of a square lattice (<= 64 x 64)?  Fills `L` (geometry only) if so.
bool detect_lattice(const double *gx, const double *gy, int n, LatEnv &L)
{
    if (n < 2) return false;
    // lattice step: the closest pair among consecutive cells (cells of one row are consecutive and one step apart)
    double l2 = INFINITY; int k0 = -1;
    for (int c = 0; c + 1 < n; ++c) {
        const double dx = gx[c + 1] - gx[c], dy = gy[c + 1] - gy[c], d2 = dx * dx + dy * dy;
        if (d2 < l2) { l2 = d2; k0 = c; }
    }
    if (!(l2 > 0) || k0 < 0) return false;
    // the row direction u is one of the (at most four) distinct unit-step directions between consecutive cells
    // (single-cell rows make consecutive cells vertical neighbours): try each until the order is row-major
    double cand[4][2]; int ncand = 0;
    for (int c = 0; c + 1 < n && ncand < 4; ++c) {
        const double dx = gx[c + 1] - gx[c], dy = gy[c + 1] - gy[c], d2 = dx * dx + dy * dy;
        if (d2 > l2 * (1.0 + 1e-6)) continue;
        bool seen = false;
        for (int q = 0; q < ncand; ++q)
            if (std::fabs(cand[q][0] - dx) + std::fabs(cand[q][1] - dy) < 1e-6 * std::sqrt(l2)) seen = true;
        if (!seen) { cand[ncand][0] = dx; cand[ncand][1] = dy; ++ncand; }
    }
    std::vector<int> ai((size_t)n), bi((size_t)n);
    double ux = 0, uy = 0, vx = 0, vy = 0;
    bool found = false;
    for (int q = 0; q < ncand && !found; ++q) {
        ux = cand[q][0]; uy = cand[q][1]; vx = -uy; vy = ux;
        for (int pass = 0; pass < 2 && !found; ++pass) {
            bool ok = true;
            for (int c = 0; c < n && ok; ++c) {
                const double rx = gx[c] - gx[0], ry = gy[c] - gy[0];
                const double a = (rx * ux + ry * uy) / l2, b = (rx * vx + ry * vy) / l2;
                const double ar = std::nearbyint(a), br = std::nearbyint(b);
                if (std::fabs(a - ar) > 1e-6 || std::fabs(b - br) > 1e-6 || std::fabs(ar) > 4096 || std::fabs(br) > 4096) ok = false;
                ai[(size_t)c] = (int)ar; bi[(size_t)c] = (int)br;
            }
            if (!ok) break;
            // row-major order: within a row the column increases, rows increase
            bool order = true, flip = false;
            for (int c = 0; c + 1 < n; ++c) {
                if (bi[(size_t)c + 1] == bi[(size_t)c]) { if (ai[(size_t)c + 1] <= ai[(size_t)c]) order = false; }
                else if (bi[(size_t)c + 1] < bi[(size_t)c]) { flip = true; order = false; }
            }
            if (order) { found = true; break; }
            if (pass == 0 && flip) { vx = -vx; vy = -vy; continue; }      // rows run the other way: mirror v
            break;
        }
    }
    if (!found) return false;
    int amin = ai[0], amax = ai[0], bmin = bi[0], bmax = bi[0];
    for (int c = 0; c < n; ++c) {
        amin = std::min(amin, ai[(size_t)c]); amax = std::max(amax, ai[(size_t)c]);
        bmin = std::min(bmin, bi[(size_t)c]); bmax = std::max(bmax, bi[(size_t)c]);
    }
    if (amax - amin + 1 > 64 || bmax - bmin + 1 > 64) return false;
    std::memset(&L, 0, sizeof(L));
    L.ncols = amax - amin + 1; L.nrows = bmax - bmin + 1;
    for (int b = 0; b < 64; ++b) L.rowstart[b] = 0;
    int prev_b = -1;
    for (int c = 0; c < n; ++c) {
        const int a = ai[(size_t)c] - amin, b = bi[(size_t)c] - bmin;
        if (b != prev_b) { if (b < prev_b) return false; L.rowstart[b] = (short)c; prev_b = b; }
        if (L.rowmask[b] & (1ull << a)) return false;
        L.rowmask[b] |= 1ull << a;
    }
    L.ox = gx[0] - (ai[0] - amin) * ux - (bi[0] - bmin) * vx;
    L.oy = gy[0] - (ai[0] - amin) * uy - (bi[0] - bmin) * vy;
    L.uxi = ux / l2; L.uyi = uy / l2; L.vxi = vx / l2; L.vyi = vy / l2;
    const double l = std::sqrt(l2);
    L.R = (float)l;                 // caller turns the step length into radii
    return true;
}

// Window rows of the row walk for a cell set with d_sen = R lattice steps; the walk serves at most 15 (d_sen < ~7.5 cells: a
// window row then has at most 17 columns -- one 32-bit word -- and a list at most 240 cells -- one byte per row count).
int window_rows(float R) { return (int)std::floor(2.0f * (R + 0.01f)) + 1; }

// Decide the cell path of the next launches and lay out its LDS.  A cell set WALKS (row-space lattice path) when it is a
// lattice subset whose own sensing window is at most 15 lattice rows (and, at 64 agent threads, whose covered window is at
// most 29: classify_cells); any other set takes the generic scan, which handles
// arbitrary cell sets.  any_walk / any_scan: some env of the batch may hold a walking / a scanning set; rmax, cmax,
// ncols_max: the maxima over the walking sets.  All walk: one lattice launch; none walks: one generic launch; both kinds:
// PATH_MIXED, two launches that share the envs out by workgroup (env_launch) -- or, with debug_flags bit 3, one generic
// launch for the whole batch.
void set_lattice_mode(swarm_env *h, bool any_walk, bool any_scan, float rmax, float cmax, int ncols_max)
{
    KP &k = h->kp;
    if (h->cfg.large_swarm) {                              // no cell path to choose: the large-swarm kernels scan every env's cells
        h->path_mode = PATH_SCAN; h->half = false; k.lattice = 0; k.path_filter = 0;
        return;
    }
    k.lat_n32 = ncols_max <= 32 ? 1 : 0;
    k.lat_rw = (int)std::ceil(rmax + 0.02f);
    k.lat_cw = (int)std::ceil(cmax + 0.02f);
    k.lat_nrs = window_rows(rmax); k.lat_nrc = window_rows(cmax);
    const bool demote = (h->cfg.debug_flags & 8) != 0;
    h->path_mode = (!any_walk || h->lattice_disabled || k.lat_nrs > 15 || (any_scan && demote)) ? PATH_SCAN : any_scan ? PATH_MIXED : PATH_WALK;
    k.lattice = h->path_mode != PATH_SCAN ? 1 : 0;
    k.path_filter = 0;                                     // (a mixed batch's launches set it in their own copies of KP)
    {   // guard band of the fp32 reward decision of the lattice path, in lattice steps (R = d_sen / l <= rmax).  Per cell the
        // model coordinate relative to the agent is off by dx: lattice fit tolerance 1.5e-6 steps, fp32 cast of the relative
        // coordinate (|.| <= 17 steps) 2.1e-6, the walk's scaled form c / R - a / R (two products of magnitude <= 17 / R with
        // a 1-ulp reciprocal, cancelling) 5e-6, margin: 1.2e-5.  As in swarm_create: psi is off by
        // dpsi <= (pi^2 / 4) (2 sqrt(2) dx / R) + 1.2e-6, |v| by n (dpsi R + dx + thr dpsi) / den, thr = 0.05 R / d_sen;
        // fp32 accumulation / division / sqrt: 4e-6 relative to d_sen, i.e. 4e-6 R / d_sen steps.  1.3x margin.
        const double dx = 1.2e-5, R = std::fmax(1.0, (double)rmax), thr = 0.05 * R / k.d_sen;
        const double dpsi_R = 2.4675 * 2.0 * std::sqrt(2.0) * dx + 1.2e-6 * R;      // dpsi * R (1.2e-6: degree-5 polynomial 6.5e-7 + the 1-ulp reciprocal scaling)
        k.rew_ga_lat = (float)(1.3 * (dpsi_R + dx + thr * dpsi_R / R));
        k.rew_gb_lat = (float)(4e-6 * R / k.d_sen);
    }
    // a small batch of small environments (N < 64) that leaves at least half of the chip's workgroup slots empty: the
    // half-occupied geometry (Geo<NPAD, true>) -- twice the workgroups, eight lanes per agent in the list phase.  It exists
    // for the lattice kernel only, and the two launches of a mixed batch must share one workgroup -> env map: all-walk only
    {
        const int epb_full = env_geometry(h->npad, false).envs;
        const long long grid_full = ((long long)h->cfg.n_env + epb_full - 1) / epb_full;
        h->half = h->path_mode == PATH_WALK && h->npad < 64 && epb_full >= 2 && !(h->cfg.debug_flags & 4) && 2 * grid_full <= (long long)h->n_cu * 6;
    }
    env_layout(k, h->npad, h->half);
}

// Re-run the observation pass on the current state with the export switched on (the step keeps the index scratch in LDS and
// writes none of it to HBM); it recomputes the same caches from the same state, so it is idempotent.  Always leaves nearest
// cell / in-shape flag / neighbours in HBM; lists: also the sensed / occupied cell lists (allocated on first use); cap_even:
// the expert's rounding of the sensed-list subsample (KP::cap_even).  Enqueued on the handle's stream, no synchronisation.
int export_pass(swarm_env *h, bool lists, bool cap_even)
{
    if (lists && !h->d_exp_occ) {
        const size_t EN = (size_t)h->cfg.n_env * h->cfg.n_agents;
        DevBuf<int> sensed, occ;
        HIP_ALLOC(h, sensed, EN * (size_t)h->kp.g_max);
        HIP_ALLOC(h, occ, EN * (size_t)h->kp.occ_max);
        h->d_exp_sensed = std::move(sensed); h->d_exp_occ = std::move(occ);
    }
    Pass ps;
    ps.export_small = true; ps.export_lists = lists; ps.cap_even = cap_even;
    return step_launch(h, ps);
}

// Classify one cell set: is it a lattice subset (and is the lattice path allowed on this handle), and does it walk?  If it
// walks L is its lattice with the step length turned into the radii R / Rc; if not L is all zero (nrows == 0), which is what
// tells the kernels of a mixed batch that the generic launch steps this env.
LatInfo classify_cells(const swarm_env *h, const double *gx, const double *gy, int n, LatEnv &L)
{
    std::memset(&L, 0, sizeof(L));
    if (h->lattice_disabled || !detect_lattice(gx, gy, n, L)) {
        std::memset(&L, 0, sizeof(L));
        return LatInfo{false, false, true, 0.0f, 0.0f, 0};
    }
    const double l = L.R;
    L.R = (float)(h->kp.d_sen / l); L.Rc = (float)((h->kp.r_avoid / 2.0) / l);
    // (64 agent threads: those lattice kernels also keep a row's covered columns as a 32-bit word from the agent's first
    // possible column, which holds a covered window of at most 29 rows -- r_avoid / 2 < 14.49 steps; see row_sel_lean)
    const bool walks = window_rows(L.R) <= 15 && !(h->npad == 64 && window_rows(L.Rc) > 29);
    const LatInfo info = {true, walks, !walks, L.R, L.Rc, L.ncols};
    if (!info.walk) std::memset(&L, 0, sizeof(L));
    return info;
}

// Choose the cell path for the cell sets [first, last) (envs, or the shapes of the set a reset draws from): are all
// lattices, does any walk, does any scan, and the largest R / Rc / column count among those that walk.  Returns that
// summary, which is what it handed to set_lattice_mode.
LatInfo lattice_summary(const LatInfo *first, const LatInfo *last)
{
    LatInfo m = {true, false, false, 0.0f, 0.0f, 0};
    for (; first != last; ++first) {
        m.ok = m.ok && first->ok; m.scan = m.scan || first->scan;
        if (!first->walk) continue;
        m.walk = true;
        m.R = std::max(m.R, first->R); m.Rc = std::max(m.Rc, first->Rc);
        m.ncols = std::max(m.ncols, first->ncols);
    }
    return m;
}

LatInfo lattice_mode_of(swarm_env *h, const LatInfo *first, const LatInfo *last)
{
    const LatInfo m = lattice_summary(first, last);
    set_lattice_mode(h, m.walk, m.scan, m.R, m.Rc, m.ncols);
    return m;
}

ShapeSet shape_set(const swarm_env *h)
{
    ShapeSet S;
    S.n_shapes = h->n_shapes; S.cells = h->d_shape_cells.get(); S.n_g = h->d_shape_ng.get(); S.l_cell = h->d_shape_l.get();
    S.c_in = h->d_shape_cin.get(); S.lat = h->d_shape_lat.get();
    return S;
}

// refresh the (x, y)-interleaved copy of the cells of envs [e0, e0 + count)
int interleave(swarm_env *h, int e0, int count)
{
    HIP_LAUNCHED(h, launch_interleave(h->stream, h->d_cells.get(), h->d_cells_xy.get(), h->kp.ng_max, e0, count));
    return SWARM_OK;
}

// Does the rule expert of this handle run k_rule_large (rule_expert.hip)?  Above k_rule's 256 agents always; on a default handle
// also with debug_flags bit 5, the in-binary stand-in that lets the two kernels be compared on the same export lists.
bool rule_tiled(const swarm_env *h)
{
    return h->cfg.n_agents > 256 || (!h->cfg.large_swarm && (h->cfg.debug_flags & 32) != 0);
}

}  // namespace

int swarm_internal::fail(swarm_env *h, int code, const std::string &msg)
{
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

int swarm_internal_env_info(const swarm_env_t *h, swarm_env_info *out)
{
    if (!h || !out) return SWARM_ERR_INVALID;
    out->device = h->device; out->n_env = h->cfg.n_env; out->n_agents = h->cfg.n_agents; out->obs_dim = h->kp.obs_dim;
    out->obs_dtype = h->cfg.obs_dtype; out->with_prior = h->cfg.with_prior != 0; out->observed = h->observed;
    out->g_max = h->kp.g_max; out->llm_action = h->cfg.llm_action != 0; out->n_shapes = h->n_shapes;
    out->large_swarm = h->cfg.large_swarm != 0;
    out->rule_tiled = rule_tiled(h);
    return SWARM_OK;
}

int swarm_internal_metrics_step(swarm_env_t *h, double *out)
{
    if (!h || !out) return SWARM_ERR_INVALID;
    if (!h->have_cells || !h->have_state) return fail(h, SWARM_ERR_STATE, "swarm_rollout_eval: cells / state not set");
    DeviceGuard g(h->device);
    HIP_LAUNCHED(h, launch_metrics_step(h->stream, h->kp, h->n_cu, out));
    return SWARM_OK;
}

int swarm_internal_expert_view(swarm_env_t *h, bool lists, swarm_expert_view *out)
{
    if (!h || !out) return SWARM_ERR_INVALID;
    if (lists) {
        if (!h->d_act64) HIP_ALLOC(h, h->d_act64, (size_t)h->cfg.n_env * h->cfg.n_agents);
        const int rc = export_pass(h, true, true);
        if (rc != SWARM_OK) return rc;
    }
    out->p = h->d_p.get(); out->dp = h->d_dp.get(); out->cells = h->d_cells.get();
    out->near_cell = h->d_near.get(); out->in_flag = h->d_inflag.get(); out->exp_sensed = h->d_exp_sensed.get();
    out->act_next = h->d_act_next.get(); out->act64 = h->d_act64.get();
    out->d_sen = h->kp.d_sen; out->r_avoid = h->kp.r_avoid;
    out->n_env = h->cfg.n_env; out->n_agents = h->cfg.n_agents; out->g_max = h->kp.g_max; out->ng_max = h->kp.ng_max;
    return SWARM_OK;
}

extern "C" {

int swarm_abi_version(void) { return SWARM_ABI_VERSION; }

void swarm_default_config(swarm_config_t *c)
{
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->n_env = 1; c->n_agents = 30; c->n_cells_max = 576;
    c->topo_nei_max = 6; c->num_obs_grid_max = 80; c->num_occupied_grid_max = 200;
    c->is_boundary = 1; c->with_self_state = 1; c->with_prior = 1;
    c->obs_dtype = SWARM_F32; c->device = -1;
    c->d_sen = 0.4; c->r_avoid = 0.15; c->size_a = 0.035;
    c->k_ball = 30; c->k_wall = 100; c->c_wall = 5; c->vel_max = 0.8; c->dt = 0.1;
    c->boundary[0] = -2.4; c->boundary[1] = 2.4; c->boundary[2] = 2.4; c->boundary[3] = -2.4;
    c->prior_gain[0] = 2.0; c->prior_gain[1] = 3.0; c->prior_gain[2] = 2.0;      // AssemblyEnv.cpp:1128-1132
    c->llm_repulsion = 1.0; c->llm_action = 0;                                   // assembly.py:895
}

const char *swarm_last_error(const swarm_env_t *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int swarm_create(const swarm_config_t *cfg, swarm_env_t **out)
{
    if (!cfg || !out) return fail(nullptr, SWARM_ERR_INVALID, "swarm_create: null argument");
    *out = nullptr;
    if (cfg->n_env < 1) return fail(nullptr, SWARM_ERR_INVALID, "n_env must be >= 1");
    if (cfg->large_swarm != 0 && cfg->large_swarm != 1) return fail(nullptr, SWARM_ERR_INVALID, "large_swarm must be 0 or 1");
    if (cfg->large_swarm) {
        if (cfg->n_agents < 1 || cfg->n_agents > 1024) return fail(nullptr, SWARM_ERR_INVALID, "n_agents must be in [1, 1024] (large_swarm)");
    } else if (cfg->n_agents < 1 || cfg->n_agents > 256) return fail(nullptr, SWARM_ERR_INVALID, "n_agents must be in [1, 256]");
    if (cfg->n_cells_max < 1 || cfg->n_cells_max > 32767) return fail(nullptr, SWARM_ERR_INVALID, "n_cells_max must be in [1, 32767]");
    if (cfg->topo_nei_max < 1 || cfg->topo_nei_max > kTopoMax) return fail(nullptr, SWARM_ERR_INVALID, "topo_nei_max must be in [1, 6]");
    if (cfg->num_obs_grid_max < 2 || cfg->num_obs_grid_max > 4096) return fail(nullptr, SWARM_ERR_INVALID, "num_obs_grid_max must be in [2, 4096]");
    if (cfg->num_occupied_grid_max < 2) return fail(nullptr, SWARM_ERR_INVALID, "num_occupied_grid_max must be >= 2");
    if (cfg->obs_dtype != SWARM_F32 && cfg->obs_dtype != SWARM_F64 && cfg->obs_dtype != SWARM_BF16) return fail(nullptr, SWARM_ERR_INVALID, "obs_dtype must be SWARM_F32, SWARM_F64 or SWARM_BF16");
    if (!(cfg->d_sen > 0) || !(cfg->r_avoid > 0) || !(cfg->dt > 0)) return fail(nullptr, SWARM_ERR_INVALID, "d_sen, r_avoid, dt must be positive");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(nullptr, SWARM_ERR_HIP, std::string("no HIP device available (") + hipGetErrorString(e) + "); this library has no CPU path");
    int dev = cfg->device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= ndev) return fail(nullptr, SWARM_ERR_INVALID, "device ordinal out of range");

    swarm_env *h = new (std::nothrow) swarm_env();
    if (!h) return fail(nullptr, SWARM_ERR_INVALID, "out of host memory");
    h->cfg = *cfg; h->device = dev;
    for (int &a : h->attr_smem) a = -1;
    h->env_lat.assign((size_t)cfg->n_env, LatInfo{false, false, true, 0.0f, 0.0f, 0});
    h->lattice_disabled = (cfg->debug_flags & 2) != 0;
    h->cells_set.assign((size_t)cfg->n_env, 0);
    h->npad = npad_for(cfg->n_agents);

    KP &k = h->kp;
    k.n_env = cfg->n_env; k.n_a = cfg->n_agents; k.ng_max = cfg->n_cells_max;
    k.topo = cfg->topo_nei_max; k.g_max = cfg->num_obs_grid_max; k.occ_max = cfg->num_occupied_grid_max;
    k.with_self = cfg->with_self_state ? 1 : 0;
    k.obs_dim = 2 * 2 * (k.topo + 1 + k.with_self) + 2 * k.g_max;               // ENV:801
    k.boundary = cfg->is_boundary ? 1 : 0; k.periodic = cfg->is_boundary ? 0 : 1;  // ENV:99-103
    k.with_prior = cfg->with_prior ? 1 : 0;
    k.pk_att = cfg->prior_gain[0]; k.pk_rep = cfg->prior_gain[1]; k.pk_ali = cfg->prior_gain[2];
    k.pk_llm = cfg->llm_repulsion; k.llm = cfg->llm_action ? 1 : 0;
    k.d_sen = cfg->d_sen; k.r_avoid = cfg->r_avoid; k.size_a = cfg->size_a;
    k.size2 = cfg->size_a + cfg->size_a;                                         // ENV:785-786
    k.k_ball = cfg->k_ball; k.k_wall = cfg->k_wall; k.c_wall = cfg->c_wall; k.vel_max = cfg->vel_max; k.dt = cfg->dt;
    k.bx0 = cfg->boundary[0]; k.by1 = cfg->boundary[1]; k.bx2 = cfg->boundary[2]; k.by3 = cfg->boundary[3];
    k.w_half = (k.bx2 - k.bx0) / 2.0; k.h_half = (k.by1 - k.by3) / 2.0;         // CPP:70-71
    k.c_sen = cut_lt(k.d_sen);                            // norm < d_sen              CPP:658,902
    k.c_near = cut_lt(k.d_sen + k.r_avoid / 2.0);         // norm < d_sen + r_avoid/2  CPP:161
    k.c_occ = cut_le(k.r_avoid / 2.0);                    // !(norm > r_avoid/2)       CPP:185
    k.c_avoid = cut_lt(k.r_avoid);                        // r_avoid > norm            CPP:482
    k.c_ball = cut_lt(k.size2);                           // d_center - sizes < 0      ENV:450-451
    k.c_close2 = std::fmin(k.c_sen, (3.0 * k.r_avoid) * (3.0 * k.r_avoid));
    k.c_close = std::fmin(k.c_sen, (1.9 * k.r_avoid) * (1.9 * k.r_avoid));   // 1.9: fewest insertion trips on the 64-agent workload (measured)
    {   // fp32 pre-filter bands.  With |coordinates| <= S, a float-converted coordinate is off by <= 2^-24 S and
        // their float difference by another 2^-24 S at most: dr = 4 * 2^-24 * S bounds each component of the fp32
        // relative position (1.33x margin).  Then |d2_32 - d2_64| <= 2 sqrt(2) |r| dr + O(2^-23 d2) <= 3 sqrt(d2) dr + 2^-21 d2.
        double S = 0.0;
        for (int q = 0; q < 4; ++q) S = std::fmax(S, std::fabs(cfg->boundary[q]));
        S = 1.5 * S + 1.0;
        const double dr = 4.0 * std::ldexp(1.0, -24) * S;
        auto band = [&](double c) { return 3.0 * std::sqrt(c) * dr + std::ldexp(1.0, -21) * c + 1e-12; };
        auto f_below = [](double v) { float f = (float)v; while ((double)f > v) f = std::nextafterf(f, -INFINITY); return f; };
        auto f_above = [](double v) { float f = (float)v; while ((double)f < v) f = std::nextafterf(f, INFINITY); return f; };
        k.csen_lo = f_below(k.c_sen - band(k.c_sen)); k.csen_hi = f_above(k.c_sen + band(k.c_sen));
        k.cocc_lo = f_below(k.c_occ - band(k.c_occ)); k.cocc_hi = f_above(k.c_occ + band(k.c_occ));
        k.coord_lim = (float)S;
        k.min_tol_a = (float)(2.0 * 3.0 * dr); k.min_tol_b = (float)(2.0 * std::ldexp(1.0, -21));
        {   // error bound of the fp32 reward sums near the 0.05 threshold, v = |sum psi r| / sum psi over n list entries:
            // each fp32 component of r is off by dx (two float conversions + the subtraction), u = |r|^2 / d_sen^2 by
            // du <= 2 sqrt(2) dx / d_sen, psi by |dpsi/du| du + the polynomial's 4e-7 with |dpsi/du| <= pi^2 / 4; hence
            // |dv| <= n (dpsi d_sen + dx + 0.05 dpsi) / den + (fp32 accumulation, division, sqrt: < 3e-6).  1.3x margin.
            const double dx = 2.1 * std::ldexp(1.0, -24) * S;
            const double dpsi = 2.4675 * (2.0 * std::sqrt(2.0) * dx / k.d_sen) + 4e-7;
            k.rew_ga = (float)(1.3 * (dpsi * k.d_sen + dx + 0.0505 * dpsi));
            k.rew_gb = 4e-6f;
        }
        k.rew_thr_k = (float)(0.05 / k.d_sen);
        k.rew_ga_lat = k.rew_gb_lat = 0.0f;
        k.force_exact = (cfg->debug_flags & 1) ? 1 : 0;
        {   // unsigned division by D = 2 (G-1) (Granlund-Montgomery round-up method, exact for every 32-bit x)
            const unsigned D = 2u * (unsigned)(k.g_max - 1);
            int l = 0;
            while ((1ull << l) < D) ++l;
            k.cap_magic = (unsigned)((((1ull << l) - D) << 32) / D + 1);
            k.cap_shift = l - 1;
            // numerators stay below 2^32: 2 (G-1) (n_cells_max-1) + (G-1)
            const unsigned long long xmax = 2ull * (k.g_max - 1) * (unsigned long long)k.ng_max + k.g_max;
            k.cap_int = (((k.g_max - 1) & 1) == 1 && xmax < (1ull << 32) && l >= 1) ? 1 : 0;
        }
        k.dbg_phase = (cfg->debug_flags >> 8) & 0xF;
        k.dbg_extra = (cfg->debug_flags >> 12) & 0xF;
    }
    if (!cfg->large_swarm) env_layout(k, h->npad, false);     // (describes the step kernel's LDS; the large-swarm kernels have their own)

    DeviceGuard g(dev);
    if (!g.ok) { delete h; return fail(nullptr, SWARM_ERR_HIP, "hipSetDevice failed"); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { delete h; return fail(nullptr, SWARM_ERR_HIP, "hipGetDeviceProperties failed"); }
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // the large-swarm observation kernel stays inside the LDS every kernel may have without asking for more
    if (cfg->large_swarm ? large_lds_bytes(k.ng_max, k.n_a) > 64 * 1024 : (size_t)k.smem_generic > 160 * 1024) {
        delete h;
        return fail(nullptr, SWARM_ERR_INVALID, "configuration needs more LDS per workgroup than the device has (reduce n_cells_max / num_obs_grid_max)");
    }
    const size_t E = (size_t)cfg->n_env, N = (size_t)cfg->n_agents;
    hipError_t a = hipSuccess;
    // count: elements of the buffer's type; fill >= 0: the byte every element of the new buffer is set to
    auto alloc = [&](auto &buf, size_t count, int fill = -1) {
        if (a == hipSuccess) a = buf.alloc(count);
        if (a == hipSuccess && fill >= 0) a = hipMemset(buf.get(), fill, count * sizeof(*buf.get()));
    };
    alloc(h->d_p, E * 2 * N); alloc(h->d_dp, E * 2 * N);
    alloc(h->d_cells, E * 2 * (size_t)k.ng_max, 0); alloc(h->d_cin, E);
    alloc(h->d_cells_xy, E * (size_t)k.ng_max, 0);
    alloc(h->d_ng, E, 0); alloc(h->d_shape_idx, E, 0xFF);
    alloc(h->d_prior, E * N * 16, 0);
    if (cfg->llm_action) alloc(h->d_act_next, E * N, 0);
    alloc(h->d_lat, E);
    alloc(h->d_nei, E * N * (size_t)k.topo, 0xFF); alloc(h->d_near, E * N, 0);
    alloc(h->d_inflag, E * N, 0); alloc(h->d_sf, E * N, 0);
    if (a == hipSuccess) a = hipEventCreate(&h->ev0);
    if (a == hipSuccess) a = hipEventCreate(&h->ev1);
    // the fills above went to the null stream, and a first kernel on a non-blocking stream is not ordered behind it: wait
    // for them here, once per handle (DESIGN.md "Stream contract")
    if (a == hipSuccess) a = hipStreamSynchronize(nullptr);
    if (a != hipSuccess) {
        std::string m = std::string("device allocation failed: ") + hipGetErrorString(a);
        swarm_destroy(h);
        return fail(nullptr, SWARM_ERR_HIP, m);
    }
    k.p = h->d_p.get(); k.dp = h->d_dp.get(); k.nei = h->d_nei.get(); k.near_cell = h->d_near.get(); k.in_flag = h->d_inflag.get(); k.sf_next = h->d_sf.get();
    k.prior_next = h->d_prior.get(); k.act_next = h->d_act_next.get();
    k.cells = h->d_cells.get(); k.cells_xy = h->d_cells_xy.get(); k.n_g = h->d_ng.get(); k.c_in = h->d_cin.get();
    k.lat = h->d_lat.get(); k.lattice = 0; k.lat_rw = k.lat_cw = 0; k.lat_nrs = k.lat_nrc = 0; k.lat_n32 = 0;
    k.c_near_hi = k.c_near * (1.0 + 1e-9);
    *out = h;
    return SWARM_OK;
}

int swarm_destroy(swarm_env_t *h)
{
    if (!h) return SWARM_OK;
    DeviceGuard g(h->device);          // the handle's buffers are freed with its device current
    (void)hipStreamSynchronize(h->stream);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->aux_stream) { (void)hipStreamSynchronize(h->aux_stream); (void)hipStreamDestroy(h->aux_stream); }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    delete h;
    return SWARM_OK;
}

int swarm_set_stream(swarm_env_t *h, void *s)
{
    if (!h) return SWARM_ERR_INVALID;
    h->stream = static_cast<hipStream_t>(s);
    return SWARM_OK;
}

int swarm_synchronize(swarm_env_t *h)
{
    if (!h) return SWARM_ERR_INVALID;
    DeviceGuard g(h->device);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWARM_OK;
}

int swarm_obs_dim(const swarm_env_t *h) { return h ? h->kp.obs_dim : -1; }

int swarm_set_cells(swarm_env_t *h, int env_begin, int count, const double *cells, const int32_t *n_g, const double *l_cell)
{
    if (!h) return SWARM_ERR_INVALID;
    if (!cells || !n_g || !l_cell) return fail(h, SWARM_ERR_INVALID, "swarm_set_cells: null argument");
    if (env_begin < 0 || count < 1 || env_begin + count > h->cfg.n_env) return fail(h, SWARM_ERR_INVALID, "swarm_set_cells: env range out of bounds");
    std::vector<double> cin((size_t)count);
    for (int k = 0; k < count; ++k) {
        if (n_g[k] < 1 || n_g[k] > h->cfg.n_cells_max) return fail(h, SWARM_ERR_INVALID, "swarm_set_cells: n_g must be in [1, n_cells_max]");
        if (!(l_cell[k] > 0)) return fail(h, SWARM_ERR_INVALID, "swarm_set_cells: l_cell must be positive");
        cin[(size_t)k] = cut_lt(std::sqrt(2) * l_cell[k] / 2);            // CPP:889
    }
    DeviceGuard g(h->device);
    const size_t row = (size_t)2 * h->kp.ng_max;
    HIP_TRY(h, hipMemcpyAsync(h->d_cells.get() + (size_t)env_begin * row, cells, (size_t)count * row * 8, hipMemcpyDefault, h->stream));
    if (int rc = interleave(h, env_begin, count)) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->d_ng.get() + env_begin, n_g, (size_t)count * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_shape_idx.get() + env_begin, 0xFF, (size_t)count * 4, h->stream));   // no longer a shape of the set
    HIP_TRY(h, hipMemcpyAsync(h->d_cin.get() + env_begin, cin.data(), (size_t)count * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));           // cin is a host temporary
    {   // lattice detection on a host copy of what was uploaded (`cells` may be a device pointer)
        std::vector<double> hc((size_t)count * row);
        HIP_TRY(h, hipMemcpy(hc.data(), h->d_cells.get() + (size_t)env_begin * row, (size_t)count * row * 8, hipMemcpyDeviceToHost));
        std::vector<LatEnv> lat((size_t)count);
        for (int k = 0; k < count; ++k) {
            const double *gx = hc.data() + (size_t)k * row, *gy = gx + h->kp.ng_max;
            h->env_lat[(size_t)(env_begin + k)] = classify_cells(h, gx, gy, n_g[k], lat[(size_t)k]);
        }
        HIP_TRY(h, hipMemcpy(h->d_lat.get() + env_begin, lat.data(), (size_t)count * sizeof(LatEnv), hipMemcpyHostToDevice));
        lattice_mode_of(h, h->env_lat.data(), h->env_lat.data() + h->env_lat.size());
    }
    for (int k = 0; k < count; ++k) h->cells_set[(size_t)(env_begin + k)] = 1;
    h->have_cells = true;
    for (char c : h->cells_set) if (!c) { h->have_cells = false; break; }
    h->observed = false;
    return SWARM_OK;
}

int swarm_set_shapes(swarm_env_t *h, int n_shapes, const double *shape_cells, const int32_t *n_g, const double *l_cell)
{
    if (!h) return SWARM_ERR_INVALID;
    if (n_shapes < 1 || !shape_cells || !n_g || !l_cell) return fail(h, SWARM_ERR_INVALID, "swarm_set_shapes: bad argument");
    const size_t row = (size_t)2 * h->kp.ng_max;
    std::vector<double> cin((size_t)n_shapes);
    std::vector<LatEnv> lat((size_t)n_shapes);
    std::vector<LatInfo> info((size_t)n_shapes);
    for (int k = 0; k < n_shapes; ++k) {
        if (n_g[k] < 1 || n_g[k] > h->cfg.n_cells_max) return fail(h, SWARM_ERR_INVALID, "swarm_set_shapes: n_g must be in [1, n_cells_max]");
        if (!(l_cell[k] > 0)) return fail(h, SWARM_ERR_INVALID, "swarm_set_shapes: l_cell must be positive");
        cin[(size_t)k] = cut_lt(std::sqrt(2) * l_cell[k] / 2);
        const double *gx = shape_cells + (size_t)k * row, *gy = gx + h->kp.ng_max;
        info[(size_t)k] = classify_cells(h, gx, gy, n_g[k], lat[(size_t)k]);
    }
    DeviceGuard g(h->device);
    // the new set is built aside and replaces the old one only when it is complete: a failure leaves the old set in force
    const size_t S = (size_t)n_shapes;
    DevBuf<double> d_cells, d_l, d_cin; DevBuf<int> d_ng; DevBuf<LatEnv> d_lat;
    HIP_ALLOC(h, d_cells, S * row); HIP_ALLOC(h, d_l, S); HIP_ALLOC(h, d_cin, S); HIP_ALLOC(h, d_ng, S); HIP_ALLOC(h, d_lat, S);
    HIP_TRY(h, hipMemcpy(d_cells.get(), shape_cells, S * row * 8, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d_l.get(), l_cell, S * 8, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d_cin.get(), cin.data(), S * 8, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d_ng.get(), n_g, S * 4, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d_lat.get(), lat.data(), S * sizeof(LatEnv), hipMemcpyHostToDevice));
    h->d_shape_cells = std::move(d_cells); h->d_shape_l = std::move(d_l); h->d_shape_cin = std::move(d_cin);
    h->d_shape_ng = std::move(d_ng); h->d_shape_lat = std::move(d_lat);
    h->n_shapes = n_shapes; h->shape_lat = std::move(info);
    return SWARM_OK;
}

int swarm_reset(swarm_env_t *h, uint64_t seed, uint64_t episode, int64_t env_offset, void *obs)
{
    if (!h) return SWARM_ERR_INVALID;
    if (h->n_shapes < 1) return fail(h, SWARM_ERR_STATE, "swarm_reset: no shape set (swarm_set_shapes)");
    DeviceGuard g(h->device);
    HIP_LAUNCHED(h, launch_reset(h->stream, h->kp, shape_set(h), seed, episode, env_offset, h->d_cells.get(), h->d_ng.get(), h->d_cin.get(), h->d_lat.get(), h->d_shape_idx.get()));
    if (int rc = interleave(h, 0, h->cfg.n_env)) return rc;
    std::fill(h->cells_set.begin(), h->cells_set.end(), 1);
    h->have_cells = h->have_state = true;
    // per-env bounds for a later partial swarm_set_cells: the shape set's summary is valid for every env (which env drew a
    // shape that walks only the device records know: a set with both kinds leaves the batch mixed)
    const LatInfo all = lattice_mode_of(h, h->shape_lat.data(), h->shape_lat.data() + h->shape_lat.size());
    std::fill(h->env_lat.begin(), h->env_lat.end(), all);
    h->observed = false;
    return swarm_observe(h, obs);
}

int swarm_reset_envs(swarm_env_t *h, uint64_t seed, const int64_t *episode, int64_t env_offset, void *obs)
{
    if (!h) return SWARM_ERR_INVALID;
    if (!episode) return fail(h, SWARM_ERR_INVALID, "swarm_reset_envs: null episode");
    if (h->n_shapes < 1) return fail(h, SWARM_ERR_STATE, "swarm_reset_envs: no shape set (swarm_set_shapes)");
    if (!h->have_state) return fail(h, SWARM_ERR_STATE, "swarm_reset_envs: state not set (a kept env needs it: swarm_set_state / swarm_reset)");
    if (!h->have_cells) return fail(h, SWARM_ERR_STATE, "swarm_reset_envs: target cells not set for every env (a kept env needs them)");
    DeviceGuard g(h->device);
    HIP_LAUNCHED(h, launch_reset_envs(h->stream, h->kp, shape_set(h), seed, reinterpret_cast<const long long *>(episode), env_offset,
                                      h->d_cells.get(), h->d_cells_xy.get(), h->d_ng.get(), h->d_cin.get(), h->d_lat.get(), h->d_shape_idx.get()));
    // which env was reset, and to which shape, only the device knows (as after swarm_select_shapes): every env's record becomes
    // what holds for its present cells AND for any shape of the set; the device records stay exact
    const LatInfo set = lattice_summary(h->shape_lat.data(), h->shape_lat.data() + h->shape_lat.size());
    for (LatInfo &i : h->env_lat) {
        const LatInfo both[2] = {i, set};
        i = lattice_summary(both, both + 2);
    }
    lattice_mode_of(h, h->env_lat.data(), h->env_lat.data() + h->env_lat.size());
    h->observed = false;
    return swarm_observe(h, obs);
}

int swarm_select_shape(swarm_env_t *h, int32_t shape_index, void *obs)
{
    if (!h) return SWARM_ERR_INVALID;
    if (h->n_shapes < 1) return fail(h, SWARM_ERR_STATE, "swarm_select_shape: no shape set (swarm_set_shapes)");
    if (shape_index < 0 || shape_index >= h->n_shapes) return fail(h, SWARM_ERR_INVALID, "swarm_select_shape: shape_index outside [0, n_shapes)");
    if (!h->have_state) return fail(h, SWARM_ERR_STATE, "swarm_select_shape: state not set (swarm_set_state / swarm_reset)");
    DeviceGuard g(h->device);
    HIP_LAUNCHED(h, launch_select_shape(h->stream, shape_set(h), (int)shape_index, h->kp.ng_max, h->cfg.n_env, h->d_cells.get(), h->d_cells_xy.get(),
                                        h->d_ng.get(), h->d_cin.get(), h->d_lat.get(), h->d_shape_idx.get()));
    // the host bookkeeping swarm_set_cells would leave for E copies of this shape
    const LatInfo *one = h->shape_lat.data() + shape_index;
    std::fill(h->cells_set.begin(), h->cells_set.end(), 1);
    std::fill(h->env_lat.begin(), h->env_lat.end(), *one);
    h->have_cells = true;
    lattice_mode_of(h, one, one + 1);
    h->observed = false;
    return swarm_observe(h, obs);
}

int swarm_select_shapes(swarm_env_t *h, const int32_t *shape_index, const double *pose, void *obs)
{
    if (!h) return SWARM_ERR_INVALID;
    if (!shape_index) return fail(h, SWARM_ERR_INVALID, "swarm_select_shapes: null shape_index");
    if (h->n_shapes < 1) return fail(h, SWARM_ERR_STATE, "swarm_select_shapes: no shape set (swarm_set_shapes)");
    if (!h->have_state) return fail(h, SWARM_ERR_STATE, "swarm_select_shapes: state not set (swarm_set_state / swarm_reset)");
    if (!h->have_cells) return fail(h, SWARM_ERR_STATE, "swarm_select_shapes: target cells not set for every env (a kept env needs them)");
    DeviceGuard g(h->device);
    HIP_LAUNCHED(h, launch_select_shapes(h->stream, shape_set(h), shape_index, pose, h->kp.ng_max, h->cfg.n_env, h->d_cells.get(), h->d_cells_xy.get(),
                                         h->d_ng.get(), h->d_cin.get(), h->d_lat.get(), h->d_shape_idx.get()));
    // which env took which shape only the device knows (as after swarm_reset): every env's record becomes what holds for its
    // present cells AND for any shape of the set; the device records stay exact, and they are what the kernels' filters read
    const LatInfo set = lattice_summary(h->shape_lat.data(), h->shape_lat.data() + h->shape_lat.size());
    for (LatInfo &i : h->env_lat) {
        const LatInfo both[2] = {i, set};
        i = lattice_summary(both, both + 2);
    }
    lattice_mode_of(h, h->env_lat.data(), h->env_lat.data() + h->env_lat.size());
    h->observed = false;
    return swarm_observe(h, obs);
}

int swarm_set_state(swarm_env_t *h, const double *p, const double *dp)
{
    if (!h) return SWARM_ERR_INVALID;
    if (!p || !dp) return fail(h, SWARM_ERR_INVALID, "swarm_set_state: null argument");
    DeviceGuard g(h->device);
    const size_t bytes = (size_t)h->cfg.n_env * 2 * h->cfg.n_agents * 8;
    HIP_TRY(h, hipMemcpyAsync(h->d_p.get(), p, bytes, hipMemcpyDefault, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_dp.get(), dp, bytes, hipMemcpyDefault, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->have_state = true;
    h->observed = false;
    return SWARM_OK;
}

int swarm_metrics(swarm_env_t *h, double *out)
{
    if (!h || !out) return SWARM_ERR_INVALID;
    if (!h->have_cells || !h->have_state) return fail(h, SWARM_ERR_STATE, "swarm_metrics: cells / state not set");
    DeviceGuard g(h->device);
    HIP_LAUNCHED(h, launch_metrics(h->stream, h->kp, out));
    return SWARM_OK;
}

int swarm_get_cells(swarm_env_t *h, double *cells, int32_t *n_g)
{
    if (!h) return SWARM_ERR_INVALID;
    DeviceGuard g(h->device);
    if (cells) HIP_TRY(h, hipMemcpyAsync(cells, h->d_cells.get(), (size_t)h->cfg.n_env * 2 * h->kp.ng_max * 8, hipMemcpyDefault, h->stream));
    if (n_g) HIP_TRY(h, hipMemcpyAsync(n_g, h->d_ng.get(), (size_t)h->cfg.n_env * 4, hipMemcpyDefault, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWARM_OK;
}

int swarm_get_shape_index(swarm_env_t *h, int32_t *shape_index)
{
    if (!h || !shape_index) return SWARM_ERR_INVALID;
    DeviceGuard g(h->device);
    HIP_TRY(h, hipMemcpyAsync(shape_index, h->d_shape_idx.get(), (size_t)h->cfg.n_env * 4, hipMemcpyDefault, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWARM_OK;
}

int swarm_get_state(swarm_env_t *h, double *p, double *dp)
{
    if (!h) return SWARM_ERR_INVALID;
    DeviceGuard g(h->device);
    const size_t bytes = (size_t)h->cfg.n_env * 2 * h->cfg.n_agents * 8;
    if (p) HIP_TRY(h, hipMemcpyAsync(p, h->d_p.get(), bytes, hipMemcpyDefault, h->stream));
    if (dp) HIP_TRY(h, hipMemcpyAsync(dp, h->d_dp.get(), bytes, hipMemcpyDefault, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWARM_OK;
}

int swarm_observe(swarm_env_t *h, void *obs)
{
    if (!h) return SWARM_ERR_INVALID;
    if (!h->have_cells) return fail(h, SWARM_ERR_STATE, "swarm_observe: target cells not set for every env (swarm_set_cells)");
    if (!h->have_state) return fail(h, SWARM_ERR_STATE, "swarm_observe: state not set (swarm_set_state)");
    DeviceGuard g(h->device);
    Pass ps;
    ps.obs = obs;
    int rc = step_launch(h, ps);
    if (rc == SWARM_OK) h->observed = true;
    return rc;
}

int swarm_step(swarm_env_t *h, const void *action, int action_dtype, void *obs, float *reward, uint8_t *done, void *a_prior)
{
    if (!h) return SWARM_ERR_INVALID;
    if (!action) {
        // agent_strategy == 'llm' (assembly.py:525-529): the action is the Python twin of the prior policy, which the
        // previous pass evaluated on this very state
        if (!h->cfg.llm_action) return fail(h, SWARM_ERR_INVALID, "swarm_step: null action (only a handle created with llm_action may pass NULL)");
        action = h->d_act_next.get(); action_dtype = SWARM_F64;
    }
    if (action_dtype != SWARM_F32 && action_dtype != SWARM_F64) return fail(h, SWARM_ERR_INVALID, "swarm_step: bad action_dtype");
    if (!h->observed) return fail(h, SWARM_ERR_STATE, "swarm_step: call swarm_observe after setting cells/state (the reference's reset() ends with _get_obs())");
    DeviceGuard g(h->device);
    return step_launch(h, Pass{true, action, action_dtype == SWARM_F64 ? ACT_F64 : 0, obs, reward, done, a_prior});
}

// (io_alloc / io_export are in no header, yet libswarmenv.so has always exported these two names; SWARM_ABI_VERSION holds
// the set of exported symbols, so they stay where a dlsym finds them)
int io_alloc(swarm_env *h)
{
    if (h->h_io_action) return SWARM_OK;
    const size_t EN = (size_t)h->cfg.n_env * h->cfg.n_agents, D = (size_t)h->kp.obs_dim;
    const size_t so = obs_elem_bytes(h->cfg.obs_dtype);
    const size_t block_bytes = (D * EN + 2 * EN + EN) * 8 + ((EN + 15) & ~size_t(15));
    // built aside and handed to the handle complete (h_io_action last, which the test above reads): a failure leaves nothing
    DevBuf<char> obs, prior, action; DevBuf<float> rew; DevBuf<uint8_t> done; DevBuf<double> block;
    DevBuf<double, true> hblock0, hblock1; DevBuf<char, true> haction;
    HIP_ALLOC(h, obs, EN * D * so); HIP_ALLOC(h, prior, EN * 2 * so); HIP_ALLOC(h, rew, EN); HIP_ALLOC(h, done, EN);
    HIP_ALLOC(h, block, block_bytes / 8); HIP_ALLOC(h, action, EN * 16);
    HIP_ALLOC(h, hblock0, block_bytes / 8); HIP_ALLOC(h, hblock1, block_bytes / 8); HIP_ALLOC(h, haction, EN * 16);
    HIP_TRY(h, hipMemset(block.get(), 0, block_bytes));
    HIP_TRY(h, hipStreamSynchronize(nullptr));             // a null-stream fill, as swarm_create's: complete before any stream uses it
    std::memset(hblock0.get(), 0, block_bytes); std::memset(hblock1.get(), 0, block_bytes);
    h->io_block_bytes = block_bytes;
    h->d_io_obs = std::move(obs); h->d_io_prior = std::move(prior); h->d_io_rew = std::move(rew); h->d_io_done = std::move(done);
    h->d_io_block = std::move(block); h->d_io_action = std::move(action);
    h->h_io_block[0] = std::move(hblock0); h->h_io_block[1] = std::move(hblock1); h->h_io_action = std::move(haction);
    return SWARM_OK;
}

int io_export(swarm_env *h, int slot, bool stepped)
{
    const long long EN = (long long)h->cfg.n_env * h->cfg.n_agents;
    const int D = h->kp.obs_dim, wp = (stepped && h->kp.with_prior) ? 1 : 0;
    const float *rew = stepped ? h->d_io_rew.get() : nullptr;
    const uint8_t *dn = stepped ? h->d_io_done.get() : nullptr;
    HIP_LAUNCHED(h, launch_export(h->stream, h->cfg.obs_dtype, h->d_io_obs.get(), rew, dn, h->d_io_prior.get(), h->d_io_block.get(), D, EN, wp));
    // obs only (reset / observe) moves the obs part; a step moves the whole block -- without with_prior in two pieces around
    // the a_prior part, which k_export did not write: the slot's a_prior array then stays as the caller left it
    const size_t obs_bytes = (size_t)D * EN * 8, pri_bytes = (size_t)2 * EN * 8;
    const size_t bytes = !stepped ? obs_bytes : wp ? h->io_block_bytes : obs_bytes;
    HIP_TRY(h, hipMemcpyAsync(h->h_io_block[slot].get(), h->d_io_block.get(), bytes, hipMemcpyDeviceToHost, h->stream));
    if (stepped && !wp) {
        const size_t off = obs_bytes + pri_bytes;
        HIP_TRY(h, hipMemcpyAsync((char *)h->h_io_block[slot].get() + off, (const char *)h->d_io_block.get() + off, h->io_block_bytes - off,
                                  hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWARM_OK;
}

int swarm_get_llm_action(swarm_env_t *h, double *action)
{
    if (!h || !action) return SWARM_ERR_INVALID;
    if (!h->d_act_next) return fail(h, SWARM_ERR_STATE, "swarm_get_llm_action: handle was not created with llm_action");
    if (!h->observed) return fail(h, SWARM_ERR_STATE, "swarm_get_llm_action: nothing observed yet");
    DeviceGuard g(h->device);
    HIP_TRY(h, hipMemcpyAsync(action, h->d_act_next.get(), (size_t)h->cfg.n_env * h->cfg.n_agents * 16, hipMemcpyDefault, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWARM_OK;
}

int swarm_host_outputs(swarm_env_t *h, int slot, swarm_host_out_t *out)
{
    if (!h || !out || slot < 0 || slot > 1) return SWARM_ERR_INVALID;
    DeviceGuard g(h->device);
    int rc = io_alloc(h);
    if (rc != SWARM_OK) return rc;
    const size_t EN = (size_t)h->cfg.n_env * h->cfg.n_agents, D = (size_t)h->kp.obs_dim;
    double *b = h->h_io_block[slot].get();
    out->obs = b; out->a_prior = b + D * EN; out->reward = b + D * EN + 2 * EN;
    out->done = reinterpret_cast<uint8_t *>(b + D * EN + 3 * EN);
    return SWARM_OK;
}

int swarm_observe_host(swarm_env_t *h, int slot)
{
    if (!h || slot < 0 || slot > 1) return SWARM_ERR_INVALID;
    DeviceGuard g(h->device);
    int rc = io_alloc(h);
    if (rc != SWARM_OK) return rc;
    rc = swarm_observe(h, h->d_io_obs.get());
    if (rc != SWARM_OK) return rc;
    return io_export(h, slot, false);
}

int swarm_step_host(swarm_env_t *h, const void *action, int action_dtype, int action_on_device, int slot)
{
    if (!h || slot < 0 || slot > 1) return SWARM_ERR_INVALID;
    if (action && action_dtype != SWARM_F32 && action_dtype != SWARM_F64) return fail(h, SWARM_ERR_INVALID, "swarm_step_host: bad action_dtype");
    if (!h->observed) return fail(h, SWARM_ERR_STATE, "swarm_step_host: call swarm_observe(_host) after setting cells/state");
    DeviceGuard g(h->device);
    int rc = io_alloc(h);
    if (rc != SWARM_OK) return rc;
    const size_t EN = (size_t)h->cfg.n_env * h->cfg.n_agents;
    const void *act = action; int mode = 0;
    if (!action) {
        if (!h->cfg.llm_action) return fail(h, SWARM_ERR_INVALID, "swarm_step_host: null action");
        act = h->d_act_next.get(); mode = ACT_F64;                             // agent-major doubles
    } else if (action_on_device) {
        mode = action_dtype == SWARM_F64 ? ACT_F64 : 0;                  // [E][N][2] device tensor, as swarm_step
    } else {
        // the reference's (2, n_a) host array: through the pinned staging buffer, read component-major by the kernel
        const size_t bytes = EN * 2 * (action_dtype == SWARM_F64 ? 8 : 4);
        std::memcpy(h->h_io_action.get(), action, bytes);
        HIP_TRY(h, hipMemcpyAsync(h->d_io_action.get(), h->h_io_action.get(), bytes, hipMemcpyHostToDevice, h->stream));
        act = h->d_io_action.get(); mode = ACT_COMPONENT_MAJOR | (action_dtype == SWARM_F64 ? ACT_F64 : 0);
    }
    rc = step_launch(h, Pass{true, act, mode, h->d_io_obs.get(), h->d_io_rew.get(), h->d_io_done.get(), h->kp.with_prior ? h->d_io_prior.get() : nullptr});
    if (rc != SWARM_OK) return rc;
    return io_export(h, slot, true);
}

int swarm_get_indices(swarm_env_t *h, int32_t *neighbor_index, int32_t *in_flags, int32_t *sensed_index, int32_t *occupied_index)
{
    if (!h) return SWARM_ERR_INVALID;
    if (!h->observed) return fail(h, SWARM_ERR_STATE, "swarm_get_indices: nothing observed yet");
    DeviceGuard g(h->device);
    const size_t EN = (size_t)h->cfg.n_env * h->cfg.n_agents;
    const int rc = export_pass(h, sensed_index || occupied_index, false);
    if (rc != SWARM_OK) return rc;
    if (sensed_index) HIP_TRY(h, hipMemcpyAsync(sensed_index, h->d_exp_sensed.get(), EN * (size_t)h->kp.g_max * 4, hipMemcpyDefault, h->stream));
    if (occupied_index) HIP_TRY(h, hipMemcpyAsync(occupied_index, h->d_exp_occ.get(), EN * (size_t)h->kp.occ_max * 4, hipMemcpyDefault, h->stream));
    if (neighbor_index) HIP_TRY(h, hipMemcpyAsync(neighbor_index, h->d_nei.get(), EN * (size_t)h->kp.topo * 4, hipMemcpyDefault, h->stream));
    if (in_flags) HIP_TRY(h, hipMemcpyAsync(in_flags, h->d_inflag.get(), EN * 4, hipMemcpyDefault, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWARM_OK;
}

int swarm_rule_action(swarm_env_t *h, double *action)
{
    if (!h || !action) return SWARM_ERR_INVALID;
    if (!h->observed) return fail(h, SWARM_ERR_STATE, "swarm_rule_action: nothing observed yet");
    if (h->kp.g_max > 128) return fail(h, SWARM_ERR_INVALID, "swarm_rule_action: num_obs_grid_max > 128 not supported");
    if (h->cfg.large_swarm && h->cfg.n_agents <= 256) return fail(h, SWARM_ERR_INVALID, "swarm_rule_action: not available on a large_swarm handle (the rule expert serves n_agents <= 256 with large_swarm = 0)");
    DeviceGuard g(h->device);
    int rc = export_pass(h, true, true);
    if (rc != SWARM_OK) return rc;
    swarm_expert_view v;
    rc = swarm_internal_expert_view(h, false, &v);
    if (rc != SWARM_OK) return rc;
    HIP_TRY(h, swarm_internal_launch_rule(v, action, nullptr, h->stream, rule_tiled(h)));       // k_rule / k_rule_large (rule_expert.hip)
    return SWARM_OK;
}

int swarm_lattice_envs(const swarm_env_t *h)
{
    if (!h) return -1;
    int n = 0;
    for (const LatInfo &i : h->env_lat) n += i.ok ? 1 : 0;
    return n;
}

int swarm_path_envs(swarm_env_t *h, int32_t *walk_envs, int32_t *scan_envs)
{
    if (!h) return SWARM_ERR_INVALID;
    if (!walk_envs || !scan_envs) return fail(h, SWARM_ERR_INVALID, "swarm_path_envs: null argument");
    if (!h->have_cells) return fail(h, SWARM_ERR_STATE, "swarm_path_envs: target cells not set for every env (swarm_set_cells)");
    DeviceGuard g(h->device);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const int E = h->cfg.n_env;
    int walk = h->path_mode == PATH_WALK ? E : 0;
    if (h->path_mode == PATH_MIXED) {
        // what the two launches' filters read: nrows of every env's device record, by workgroup of the full geometry
        std::vector<int> nrows((size_t)E);
        HIP_TRY(h, hipMemcpy2D(nrows.data(), sizeof(int), reinterpret_cast<const char *>(h->d_lat.get()) + offsetof(LatEnv, nrows), sizeof(LatEnv),
                               sizeof(int), (size_t)E, hipMemcpyDeviceToHost));
        const int epb = env_geometry(h->npad, false).envs;
        for (int e0 = 0; e0 < E; e0 += epb) {
            bool any_zero = false;
            for (int k = 0; k < epb; ++k) any_zero = any_zero || nrows[(size_t)std::min(e0 + k, E - 1)] == 0;
            if (!any_zero) walk += std::min(epb, E - e0);
        }
    }
    *walk_envs = walk; *scan_envs = E - walk;
    return SWARM_OK;
}

double swarm_step_algorithmic_bytes(const swarm_env_t *h)
{
    if (!h) return 0.0;
    // Per agent-step: action 2*4 r, state p/dp 4*8 r + 4*8 w (fp64 here), obs D*sizeof w, reward 4 + done 1 +
    // prior 2*sizeof w; per env: target cells 2*n_g_max*8 r.  (with this build's dtypes.)
    const double so = (double)obs_elem_bytes(h->cfg.obs_dtype);
    const double per_agent = 8.0 + 64.0 + h->kp.obs_dim * so + 5.0 + 2.0 * so;
    return (double)h->cfg.n_env * (h->cfg.n_agents * per_agent + 2.0 * h->kp.ng_max * 8.0);
}

int swarm_timer_start(swarm_env_t *h)
{
    if (!h) return SWARM_ERR_INVALID;
    DeviceGuard g(h->device);
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    return SWARM_OK;
}

int swarm_timer_stop(swarm_env_t *h, float *ms)
{
    if (!h || !ms) return SWARM_ERR_INVALID;
    DeviceGuard g(h->device);
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    HIP_TRY(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return SWARM_OK;
}

}  // extern "C"
