// Private to the four sources of the env library -- swarm_env.hip (the step kernel and its launch; compiled as seven units), env_large.hip
// (the large-swarm step kernels), env_kernels.hip (the side kernels) and env_api.hip (the handle and the C ABI): the
// kernel-argument types, the handle, the description of one pass (Pass: what a launch's KP is derived from) and the functions
// through which they call each other.  Not installed, not exported: the namespace has hidden visibility, so the public ABI
// (swarm_env.h) does not change.  What the OTHER translation units of libswarmenv.so may ask of an env handle is in swarm_internal.h.
#ifndef SWARM_ENV_TYPES_H
#define SWARM_ENV_TYPES_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "swarm_env.h"
#include "swarm_internal.h"

namespace swarm_internal __attribute__((visibility("hidden"))) {

constexpr int kTopoMax = 6;
constexpr int kNeiStride = 8;     // shorts per agent in the LDS neighbour list: 6 ids, [6] = collision flag
constexpr double kSentinel = 1.0e200;     // coordinates of padding cells: d2 overflows to +inf

// Per-environment description of the target cells as a subset of a (rotated) square lattice, when they are one
// (the reference tiles a silhouette image into square cells and rotates / shifts them: assembly_cfg.py:56-99,
// assembly.py:175-187).  Cell (column a, row b) sits at o + a*u + b*v and the cell index order is row-major.
struct LatEnv {
    double ox, oy;
    double uxi, uyi, vxi, vyi;    // (p - o) . (uxi, uyi) = column coordinate, (p - o) . (vxi, vyi) = row coordinate
    float R, Rc;                  // d_sen / l and (r_avoid / 2) / l in lattice steps
    int nrows, ncols;
    short rowstart[64];           // cell index of the first cell of each row
    unsigned long long rowmask[64];   // occupied columns of each row
};

// The kernel argument of every env kernel.  Field order, types and size are part of the step kernel's device code (the
// scalar loads address the fields by offset): append, never move.  cxy_stride, off_cxy and off_rres are dead -- no kernel
// reads them and the host leaves them zero; they keep their places for the fields behind them.  export_idx, export_small,
// cap_even, exp_sensed, exp_occ, stamps and path_filter are zero in the handle's KP: launch_kp sets them in a launch's copy.
struct KP {
    int n_env, n_a, ng_max, ngw, topo, g_max, occ_max, obs_dim;
    int with_self, periodic, boundary, with_prior, export_idx;
    int export_small;          // also write neighbor_index / nearest cell / in_flags to HBM (export launches only: the step itself keeps them in LDS)
    int cxy_stride;            // dead (was: double2 elements per env in LDS)
    int cxq_stride;            // floats per env in the fp32 pair layout
    int g_stride;              // int16 elements per agent row in LDS
    int off_cxy, off_sp, off_cmask, off_sbits, off_obits, off_sidx, off_snei, off_sncf, off_snear, off_pc;
    int smem_lat, smem_lat_export, smem_generic;   // dynamic LDS bytes by launch kind
    double c_sen, c_near, c_occ, c_avoid, c_ball;     // squared-distance cut-offs
    double c_close, c_close2;  // (1.9 r_avoid)^2 and (3 r_avoid)^2 capped at c_sen: pre-selection radii of the neighbour insertion (any values are exact; the second is used for N > 128)
    // fp32 pre-filter bands: d2_32 < *_lo  =>  exact test true;  d2_32 >= *_hi  =>  exact test false
    float csen_lo, csen_hi, cocc_lo, cocc_hi;
    float coord_lim;           // |coordinate| bound the bands were derived for
    float min_tol_a, min_tol_b;   // nearest-cell ambiguity tolerance: a*sqrt(d2) + b*d2
    float rew_ga, rew_gb;      // the reward is re-evaluated in fp64 when | |v| - 0.05 | <= rew_ga * n / den + rew_gb
    int force_exact;           // debug: take every exact fallback path
    int cap_int;               // G-1 odd: the cap's round(i*step) is an exact integer division by 2(G-1)
    unsigned cap_magic; int cap_shift;
    int cap_even;              // the expert's export pass: ties of round(i*step) go to even, as np.round sends them (assembly.py:564);
                               // the observation itself rounds them away from zero (std::round, CPP:223).  Ties need G-1 even.
    int dbg_phase, dbg_extra;  // diagnostics only (tools/ablate.py): run phase dbg_phase dbg_extra EXTRA times; the
                               // phases are idempotent, so results are unchanged and the extra cost is the phase's cost.
                               // (The N = 64 lattice kernels read them only in a -DSWARM_DIAG build: swarm_env.hip, DIAG.)
    int off_cxyf, off_partc, off_lat, off_cov, off_flag;
    // lattice (row-space) launches only: per-agent frame, per (window row, agent) column masks / first cell index, per-agent
    // row counts, the agent permutation of the list phase, the fp32 reward verdicts, the occupied columns (export only)
    int off_hdr, off_srow, off_pcr, off_perm, off_rres, off_orow, off_partd;
    float rew_ga_lat, rew_gb_lat;   // guard band of the fp32 reward decision in lattice steps (see swarm_create)
    float rew_thr_k;           // 0.05 / d_sen: the reward's |v| threshold in lattice steps is rew_thr_k * (d_sen / l)
    int lattice;               // this launch takes the row-space path: every env it steps has cells that are a lattice subset whose
                               // sensing window is <= 15 rows (a mixed batch's other envs go to a second, generic launch: path_filter)
    int lat_rw, lat_cw;        // row half-windows (lattice steps) for d_sen and r_avoid/2
    int lat_nrs, lat_nrc;      // rows a radius can touch: floor(2 (rho_max + margin)) + 1, for d_sen and r_avoid/2
    int lat_n32;               // every env's lattice has <= 32 columns: 32-bit row masks
    double c_near_hi;          // c_near * (1 + 1e-9): pairs in [c_near, c_near_hi) flag the exact occupied-cell path
    const LatEnv *lat;
    double d_sen, r_avoid, size_a, size2, k_ball, k_wall, c_wall, vel_max, dt;
    double bx0, by1, bx2, by3, w_half, h_half;
    double *p, *dp;
    int *nei, *near_cell, *in_flag;
    double2 *sf_next;          // [E][N]: contact-spring force on agent i in the CURRENT state = the force term of the next step
    const double *cells;       // [E][2][ng_max] (the ABI's layout)
    const double2 *cells_xy;   // [E][ng_max] (x, y) interleaved copy: one 16-byte gather per cell
    const int *n_g;
    const double *c_in;
    int *exp_sensed, *exp_occ;
    void *prior_next;          // [E][N] pairs of the handle's obs dtype: the prior policy of the next step (written by every pass)
    double pk_att, pk_rep, pk_ali;   // gains of the prior policy: attraction, repulsion, alignment (CPP:1128-1132: 2, 3, 2)
    double pk_llm;             // repulsion gain of the Python twin that drives agent_strategy == 'llm' (ENV:895: 1.0)
    int llm;                   // also evaluate that twin and leave it in act_next as the NEXT step's action (ENV:525-529)
    double2 *act_next;         // [E][N]
    long long *stamps;         // diagnostic build only (-DSWARM_STAMPS): per-block phase clocks
    int path_filter;           // 0: every workgroup runs.  The two launches of a mixed batch (env_launch): 1 = the lattice launch, a
                               // workgroup returns at once if ANY of its envs has lat[e].nrows == 0; 2 = the generic launch, a
                               // workgroup returns at once if ALL of its envs have nrows > 0 -- each env is stepped by exactly one.
                               // The host picks the filtered instantiation of the kernel by it (k_env's FILT); the kernel's own
                               // test is compiled in, by the launch kind
};
static_assert(sizeof(KP) == 632, "KP: append, never move -- and a new field changes this size on purpose");
static_assert(offsetof(KP, n_env) == 0 && offsetof(KP, dbg_phase) == 232 && offsetof(KP, lat) == 336 && offsetof(KP, p) == 464 &&
              offsetof(KP, path_filter) == 624, "KP: a field moved");

// The uploaded shape set, as the reset and shape-switch kernels read it
struct ShapeSet {
    int n_shapes;
    const double *cells;      // [S][2][ng_max], shape frame (ENV: grid_center_origins[s].T)
    const int *n_g;           // [S]
    const double *l_cell;     // [S]
    const double *c_in;       // [S] in-shape cut-off
    const LatEnv *lat;        // [S] lattice of the un-rotated shape (nrows == 0: not a lattice)
};

// The host's record of one cell set (an env's, or a shape's of the uploaded set): is it a lattice subset (ok), and does the
// row walk serve it (walk: a lattice whose OWN sensing window is <= 15 rows, on a handle with the lattice path enabled; its
// LatEnv::R / Rc / ncols are read only where walk is set)?  A set that does not walk is uploaded with an all-zero LatEnv.
// scan = !walk for one cell set.  After swarm_reset the host does not know which env drew which shape: every env then holds
// the shape set's summary, where walk / scan say that SOME shape walks / does not, and both may be set.
struct LatInfo {
    bool ok, walk, scan;
    float R, Rc;
    int ncols;
};

// The cell path of the next launches (set_lattice_mode): one lattice launch, one generic launch, or both with KP::path_filter
enum PathMode { PATH_SCAN = 0, PATH_WALK = 1, PATH_MIXED = 2 };

// Layout of a pass's action array: doubles (else floats); the reference's (2, n_a) host array with the envs side by side
// (else agent-major pairs [E][N][2])
enum ActMode { ACT_F64 = 1, ACT_COMPONENT_MAJOR = 2 };

// One step (do_step) or observation pass of a handle: its arrays, and the switches that hold for this pass alone (launch_kp)
struct Pass {
    bool do_step = false;
    const void *action = nullptr; int act_mode = 0;   // ActMode bits
    void *obs = nullptr; float *reward = nullptr; uint8_t *done = nullptr; void *a_prior = nullptr;
    bool export_small = false, cap_even = false;      // KP's fields of these names
    bool export_lists = false;                        // KP::export_idx, into the handle's export lists (allocated by the caller)
    long long *stamps = nullptr;                      // KP::stamps (diagnostic build)
};

// What the host needs to know of the step kernel's Geo<NPAD, HALF>: environments and threads per workgroup
struct GeoInfo { int envs, threads; };

// slot of one k_env instantiation of the handle's agent count in swarm_env::attr_smem
constexpr int attr_slot(size_t obs_elem, bool do_step, bool lat, bool half, bool filt)
{
    return (do_step ? 1 : 0) + (obs_elem == 8 ? 2 : obs_elem == 2 ? 4 : 0) + (lat ? 6 : 0) + (half ? 12 : 0) + (filt ? 24 : 0);
}

}  // namespace swarm_internal

struct swarm_env {
    template <class T, bool PINNED = false> using Buf = swarm_internal::DevBuf<T, PINNED>;
    swarm_config_t cfg = {};
    swarm_internal::KP kp = {};
    int device = 0, npad = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool have_cells = false, have_state = false, observed = false;
    int attr_smem[swarm_internal::attr_slot(2, true, true, true, true) + 1];   // dynamic-LDS cap raised so far, per instantiation
    bool half = false;             // the half-occupied geometry is in use (set_lattice_mode; all-walk batches only)
    int path_mode = swarm_internal::PATH_SCAN;
    // the generic launch of a mixed batch runs beside the lattice launch on this stream, forked from and joined to the
    // handle's stream by the two events; created by the first mixed launch that overlaps, destroyed by swarm_destroy
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int n_cu = 256;
    std::vector<char> cells_set;
    std::string err;
    // device buffers: owned by the handle, freed when swarm_destroy deletes it (with the handle's device current)
    Buf<double> d_p, d_dp, d_cells, d_cin;
    Buf<double2> d_cells_xy;
    Buf<swarm_internal::LatEnv> d_lat;
    // shape set for the device-side reset: replaced as a whole by a swarm_set_shapes that succeeded
    int n_shapes = 0;
    Buf<double> d_shape_cells, d_shape_l, d_shape_cin;
    Buf<int> d_shape_ng, d_shape_idx;   // d_shape_idx: [E] shape index drawn by the last swarm_reset (-1 before / after swarm_set_cells)
    Buf<swarm_internal::LatEnv> d_shape_lat;
    std::vector<swarm_internal::LatInfo> shape_lat;    // per shape of the set
    std::vector<swarm_internal::LatInfo> env_lat;      // per env; after swarm_reset: the shape set's maxima, valid for every env
    bool lattice_disabled = false;
    Buf<int> d_nei, d_near, d_inflag, d_ng;
    Buf<int> d_exp_sensed, d_exp_occ;   // the export lists (first call that asks for them): both set, or neither
    Buf<double2> d_sf;
    Buf<char> d_prior;
    Buf<double2> d_act_next;       // [E][N] the 'llm' strategy's next action (cfg.llm_action)
    Buf<double2> d_act64;          // [E][N] fp64 action scratch of swarm_rollout_expert (first expert call)
    // reference-shaped host I/O (swarm_step_host): library-owned step outputs on the device, the export block on the
    // device, two pinned host copies of it (ping-pong: the previous step's arrays stay valid for one more step), a pinned
    // staging buffer for the action.  Allocated by the first call that needs them (io_alloc): all set, or none.
    Buf<char> d_io_obs, d_io_prior, d_io_action; Buf<float> d_io_rew; Buf<uint8_t> d_io_done; Buf<double> d_io_block;
    Buf<double, true> h_io_block[2]; Buf<char, true> h_io_action;
    size_t io_block_bytes = 0;
};

namespace swarm_internal __attribute__((visibility("hidden"))) {

// records msg as the handle's last error (h == NULL: the calling thread's swarm_create error) and returns code (env_api.hip)
int fail(swarm_env *h, int code, const std::string &msg);

#define HIP_TRY_AS(h, what, call)                                                             \
    do {                                                                                       \
        hipError_t e__ = (call);                                                               \
        if (e__ != hipSuccess)                                                                 \
            return swarm_internal::fail(h, SWARM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e__)); \
    } while (0)
#define HIP_TRY(h, call) HIP_TRY_AS(h, #call, call)
// `call` is one of the launchers below, which return their launch's hipGetLastError(): the message names that
#define HIP_LAUNCHED(h, call) HIP_TRY_AS(h, "hipGetLastError()", call)
// allocate `count` elements into the DevBuf `buf`: the message names hipMalloc / hipHostMalloc and the buffer
#define HIP_ALLOC(h, buf, count) HIP_TRY_AS(h, std::string((buf).kCall) + "(" #buf ")", (buf).alloc(count))

// ---- swarm_env.hip: the step kernel
// lay out the dynamic LDS of the launches of geometry (npad, half) for k.lattice / k.ng_max / k.g_max: KP's strides, off_*, smem_*
void env_layout(KP &k, int npad, bool half);
GeoInfo env_geometry(int npad, bool half);
// The KP of one launch of `ps`: the handle's with the pass's switches applied.  filter = KP::path_filter: 0, or 1 / 2 for the
// lattice / generic launch of a mixed batch (2: with the generic LDS layout).  The result is the handle's own (a plain step
// copies nothing) or `tmp`.
const KP &launch_kp(const swarm_env *h, const Pass &ps, int filter, KP &tmp);
// enqueue the pass on the handle's current cell path, on its stream
int env_launch(swarm_env *h, const Pass &ps);
// What one launch of the step kernel takes from its caller: the kernel argument (kp->lattice chooses the kernel), the stream,
// and whether the lattice kernel runs in the half-occupied geometry
struct Launch {
    const KP *kp;
    hipStream_t st;
    bool half;
};
// One launch of the k_env instantiation of padded agent count NPAD that l and ps ask for.  swarm_env.hip is compiled once
// per agent count (its kernel units); each defines the launch_npad of its own count, and the file's host unit calls them.
template <int NPAD> int launch_npad(swarm_env *h, const Launch &l, const Pass &ps);
extern template int launch_npad<8>(swarm_env *, const Launch &, const Pass &);
extern template int launch_npad<16>(swarm_env *, const Launch &, const Pass &);
extern template int launch_npad<32>(swarm_env *, const Launch &, const Pass &);
extern template int launch_npad<64>(swarm_env *, const Launch &, const Pass &);
extern template int launch_npad<128>(swarm_env *, const Launch &, const Pass &);
extern template int launch_npad<256>(swarm_env *, const Launch &, const Pass &);

// ---- env_large.hip: the two kernels of a handle created with swarm_config_t.large_swarm (any n_agents in [1, 1024])
// dynamic LDS per workgroup of the observation kernel
int large_lds_bytes(int n_cells_max, int n_agents);
// env_launch's contract for such a handle: the move kernel (do_step) and the observation kernel, both on the handle's stream
int large_launch(swarm_env *h, const Pass &ps);

// ---- env_kernels.hip: one launcher per side kernel; each enqueues on `st` and returns the launch's hipGetLastError()
hipError_t launch_reset(hipStream_t st, const KP &kp, const ShapeSet &S, unsigned long long seed, unsigned long long episode,
                        long long env_offset, double *cells, int *n_g, double *c_in, LatEnv *lat, int *shape_idx);
// episode [E] is a device array, read when the kernel runs; an env with a negative entry is kept (nothing of it is written)
hipError_t launch_reset_envs(hipStream_t st, const KP &kp, const ShapeSet &S, unsigned long long seed, const long long *episode,
                             long long env_offset, double *cells, double2 *cells_xy, int *n_g, double *c_in, LatEnv *lat, int *shape_idx);
hipError_t launch_select_shape(hipStream_t st, const ShapeSet &S, int s, int ng_max, int n_env, double *cells, double2 *cells_xy,
                               int *n_g, double *c_in, LatEnv *lat, int *shape_idx);
// shape_index [E] and pose [E][4] (or NULL) are device arrays, read when the kernel runs
hipError_t launch_select_shapes(hipStream_t st, const ShapeSet &S, const int *shape_index, const double *pose, int ng_max, int n_env,
                                double *cells, double2 *cells_xy, int *n_g, double *c_in, LatEnv *lat, int *shape_idx);
hipError_t launch_interleave(hipStream_t st, const double *cells, double2 *cells_xy, int ng_max, int e0, int count);
hipError_t launch_metrics(hipStream_t st, const KP &kp, double *out);
hipError_t launch_metrics_step(hipStream_t st, const KP &kp, int n_cu, double *out);
// obs / prior hold the handle's obs_dtype (SWARM_F32 / SWARM_F64 / SWARM_BF16)
hipError_t launch_export(hipStream_t st, int obs_dtype, const void *obs, const float *reward, const uint8_t *done,
                         const void *prior, double *out, int D, long long EN, int with_prior);

}  // namespace swarm_internal

#endif
