// env_kernels.hip -- the env library's side kernels: batched reset, shape switch, cell interleave, the evaluation metrics
// (reference form and per-step form), the reference-shaped host export and the per-env reset.  Each sits behind a launcher
// declared in env_types.h; the host side (env_api.hip) names no kernel.  The step kernel itself is swarm_env.hip.
//
// Like the step kernel these reproduce the reference's fp64 operation order: compile with -ffp-contract=off.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "swarm_env.h"
#include "env_types.h"

using namespace swarm_internal;

namespace {

// -------------------------------------------------------------------------------------------------
// batched reset: AssemblySwarmEnv.reset(), ENV:156-219, for every environment at once.
// Counter-based generator: draw k of environment g in episode ep under `seed` is
//     u = (mix64(mix64(mix64(seed + GOLD*(ep+1)) ^ g) + GOLD*(k+1)) >> 11) * 2^-53   in [0, 1)
// (splitmix64 finaliser), so any env range can be generated on any rank without communication.  Draw slots mirror
// the reference's order: 0 shape index (:160), 1 angle (:175), 2-3 the discarded offset (:182), 4-5 offset (:184-185),
// 6 branch coin (:202), 7-8 cluster centre (:207-208), then per agent x, y (:203-208) and vx, vy (:215).
// -------------------------------------------------------------------------------------------------
__host__ __device__ inline unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ inline double reset_u01(unsigned long long key, unsigned k)
{
    return (double)(mix64(key + 0x9E3779B97F4A7C15ull * (unsigned long long)(k + 1)) >> 11) * (1.0 / 9007199254740992.0);
}

// Cell c of a shape (shape-frame rows sx, sy; ng cells) at the pose (cs, sn, off): rotate_matrix = [[c, s], [-s, c]] applied to
// the cell, then the offset (ENV:177-178,187) -- this expression, elementwise, in this order; padding cells (c >= ng) are 0.0.
// Shared by the reset and the per-env shape switch.
__device__ __forceinline__ double2 pose_cell(const double *__restrict__ sx, const double *__restrict__ sy, const int c, const int ng,
                                             const double cs, const double sn, const double offx, const double offy)
{
    double2 g; g.x = 0.0; g.y = 0.0;
    if (c < ng) { g.x = cs * sx[c] + sn * sy[c] + offx; g.y = -sn * sx[c] + cs * sy[c] + offy; }
    return g;
}

// The frame of a shape's lattice record (LatEnv's origin and inverse basis; nrows > 0) at that pose: u' = R u, v' = R v,
// o' = R o + offset.  Rows, masks and radii do not change under a rigid motion.
__device__ __forceinline__ void pose_lattice(double &ox, double &oy, double &uxi, double &uyi, double &vxi, double &vyi,
                                             const double cs, const double sn, const double offx, const double offy)
{
    // shape-frame basis from the stored inverse basis: u = uxi / |uxi|^2
    const double iu = 1.0 / (uxi * uxi + uyi * uyi), iv = 1.0 / (vxi * vxi + vyi * vyi);
    const double ux = uxi * iu, uy = uyi * iu, vx = vxi * iv, vy = vyi * iv;
    const double rux = cs * ux + sn * uy, ruy = -sn * ux + cs * uy;
    const double rvx = cs * vx + sn * vy, rvy = -sn * vx + cs * vy;
    const double rox = cs * ox + sn * oy + offx, roy = -sn * ox + cs * oy + offy;
    ox = rox; oy = roy;
    uxi = rux / iu; uyi = ruy / iu; vxi = rvx / iv; vyi = rvy / iv;
}

__global__ void __launch_bounds__(256)
k_reset(const KP P, const ShapeSet S, const unsigned long long seed, const unsigned long long episode,
        const long long env_offset, double *cells_out, int *ng_out, double *cin_out, LatEnv *lat_out, int *shape_out)
{
    const int e = blockIdx.x, tid = threadIdx.x;
    const unsigned long long key = mix64(mix64(seed + 0x9E3779B97F4A7C15ull * (episode + 1)) ^ (unsigned long long)(env_offset + e));
    const double W = P.w_half, H = P.h_half;
    int s = (int)(reset_u01(key, 0) * S.n_shapes);
    s = s >= S.n_shapes ? S.n_shapes - 1 : s;
    const double ang = M_PI * (2.0 * reset_u01(key, 1) - 1.0);
    const double cs = cos(ang), sn = sin(ang);                       // rotate_matrix = [[c, s], [-s, c]], ENV:177
    const double offx = (-W + 1) + reset_u01(key, 4) * (2 * W - 2);
    const double offy = (-H + 1) + reset_u01(key, 5) * (2 * H - 2);
    const int ng = S.n_g[s];
    const double *sx_ = S.cells + (size_t)s * 2 * P.ng_max, *sy_ = sx_ + P.ng_max;
    double *gx = cells_out + (size_t)e * 2 * P.ng_max, *gy = gx + P.ng_max;
    for (int c = tid; c < P.ng_max; c += blockDim.x) {
        const double2 g = pose_cell(sx_, sy_, c, ng, cs, sn, offx, offy);
        gx[c] = g.x; gy[c] = g.y;
    }
    if (tid == 0) {
        ng_out[e] = ng; cin_out[e] = S.c_in[s]; shape_out[e] = s;
        LatEnv L = S.lat[s];
        if (L.nrows > 0) pose_lattice(L.ox, L.oy, L.uxi, L.uyi, L.vxi, L.vyi, cs, sn, offx, offy);
        lat_out[e] = L;
    }
    // agents (ENV:202-215)
    const int N = P.n_a;
    const bool spread = (2.0 * reset_u01(key, 6) - 1.0) > 0;
    const double cx = (-W + 1) + reset_u01(key, 7) * (2 * W - 2), cy = (-H + 1) + reset_u01(key, 8) * (2 * H - 2);
    for (int i = tid; i < N; i += blockDim.x) {
        const double ux_ = reset_u01(key, 16 + i), uy_ = reset_u01(key, 16 + N + i);
        double x, y;
        if (spread) { x = -W + ux_ * (2 * W); y = -H + uy_ * (2 * H); }
        else { x = (2.0 * ux_ - 1.0) + cx; y = (2.0 * uy_ - 1.0) + cy; }
        P.p[(size_t)e * 2 * N + i] = x; P.p[(size_t)e * 2 * N + N + i] = y;
        P.dp[(size_t)e * 2 * N + i] = -0.5 + reset_u01(key, 16 + 2 * N + i);
        P.dp[(size_t)e * 2 * N + N + i] = -0.5 + reset_u01(key, 16 + 3 * N + i);
    }
}

// -------------------------------------------------------------------------------------------------
// evaluation metrics: AssemblySwarmWrapper.coverage_rate / distribution_uniformity /
// voronoi_based_uniformity, /root/reference/cus_gym/gym/wrappers/customized_envs/assembly_wrapper.py:48-128, per env.
// fp64 in numpy's operation order, including np.var's two-pass form and numpy's pairwise summation (blocks of 8
// accumulators up to 128 elements, recursive halves above), so the values are bit-identical to the Python loops.
// -------------------------------------------------------------------------------------------------
__device__ double np_pairwise_sum(const double *a, int n)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int k = 0; k < 8; ++k) r[k] = a[k];
        int i;
        for (i = 8; i < n - (n % 8); i += 8)
            for (int k = 0; k < 8; ++k) r[k] += a[i + k];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

// (np.var(v) - min(v)) / (max(v) - min(v)), assembly_wrapper.py:96-99,125-126; `tmp` holds n doubles of scratch
__device__ double np_var_metric(const double *v, double *tmp, int n)
{
    const double mean = np_pairwise_sum(v, n) / n;
    double mn = v[0], mx = v[0];
    for (int i = 0; i < n; ++i) {
        const double d = v[i] - mean;
        tmp[i] = d * d;
        mn = v[i] < mn ? v[i] : mn; mx = v[i] > mx ? v[i] : mx;
    }
    const double var = np_pairwise_sum(tmp, n) / n;
    return (var - mn) / (mx - mn);
}

__global__ void __launch_bounds__(256)
k_metrics(const KP P, double *__restrict__ out)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int N = P.n_a, e = blockIdx.x, tid = threadIdx.x;
    double *px = reinterpret_cast<double *>(smem), *py = px + N;       // [N], [N]
    double *val = py + N, *tmp = val + N;                              // [N] per-agent values, [N] scratch
    int *cnt = reinterpret_cast<int *>(tmp + N);                       // [N] Voronoi counts, then [1] coverage count
    const int ng = P.n_g[e];
    const double *gx = P.cells + (size_t)e * 2 * P.ng_max, *gy = gx + P.ng_max;
    for (int i = tid; i < N; i += blockDim.x) {
        px[i] = P.p[(size_t)e * 2 * N + i]; py[i] = P.p[(size_t)e * 2 * N + N + i];
        cnt[i] = 0;
    }
    if (tid == 0) cnt[N] = 0;
    __syncthreads();
    // coverage (assembly_wrapper.py:58-73) and Voronoi owner (:110-121) of every cell
    const double half = P.r_avoid / 2;
    for (int c = tid; c < ng; c += blockDim.x) {
        bool covered = false;
        double best = 0.0; int owner = 0;
        for (int j = 0; j < N; ++j) {
            const double dx = px[j] - gx[c], dy = py[j] - gy[c];
            const double d = sqrt(dx * dx + dy * dy);                 // np.linalg.norm(axis=0)
            covered = covered || (d < half);
            if (j == 0 || d < best) { best = d; owner = j; }          // np.argmin: first minimum
        }
        if (covered) atomicAdd(&cnt[N], 1);
        atomicAdd(&cnt[owner], 1);
    }
    // minimum non-zero distance of every agent (:85-93)
    for (int i = tid; i < N; i += blockDim.x) {
        double m = INFINITY;
        for (int j = 0; j < N; ++j) {
            const double dx = px[j] - px[i], dy = py[j] - py[i];
            const double d = sqrt(dx * dx + dy * dy);
            if (d != 0 && d < m) m = d;
        }
        val[i] = m;
    }
    __syncthreads();
    if (tid == 0) {
        out[(size_t)e * 3 + 0] = (double)cnt[N] / ng;
        out[(size_t)e * 3 + 1] = np_var_metric(val, tmp, N);
    }
    __syncthreads();
    for (int i = tid; i < N; i += blockDim.x) val[i] = (double)cnt[i];
    __syncthreads();
    if (tid == 0) out[(size_t)e * 3 + 2] = np_var_metric(val, tmp, N);
}

// -------------------------------------------------------------------------------------------------
// The per-step metrics kernel of the evaluation loop (swarm_rollout_eval): the same bits as k_metrics, which stays the
// in-repo reference, at a fraction of its work.  WPE waves per env in a 256-thread workgroup: one (four envs per workgroup)
// when the batch alone fills the chip, four (one env per workgroup, the cells and agents dealt over 256 lanes) for a small
// batch, where one wave per env would leave most SIMDs idle and the launch would be latency-bound.
//
// Where k_metrics spends its time and why the cheaper form is exact.  With s = dx*dx + dy*dy (the same fp64 expression,
// no contraction) every distance k_metrics uses is d = sqrt(s), and fp64 sqrt is correctly rounded, hence monotone:
// s_a <= s_b implies d_a <= d_b.
//   * coverage of a cell: any_j (d_j < r/2)  ==  (min_j d_j < r/2)  ==  (sqrt(min_j s_j) < r/2).  So only the minimum of
//     the squared distances is needed, and with h2 = (r/2)^2 the verdict is read off it: s_min < h2 (1 - 2^-40) means
//     sqrt(s_min) is more than 2^-42 relative (thousands of ulps) below r/2, s_min > h2 (1 + 2^-40) the same above; only
//     inside that band is the exact sqrt compared.  This minimum skips NaN, as `d < r/2` does; the argmin's running
//     minimum is seeded with agent 0 whatever it is, as np.argmin's loop in k_metrics is, so NaN states give the same bits.
//   * Voronoi owner: np.argmin over the ROUNDED norms = the lowest index j with d_j == d_min.  The scan keeps the running
//     minimum of s and the first index that reached it.  An earlier agent can share the rounded norm only if its s lies
//     within a few 2^-52 of s_min; at the last update of the minimum the previous minimum (the smallest s of all earlier
//     agents) is compared with s_new (1 + 2^-40): above it, every earlier sqrt is more than 2^-42 relative larger, so the
//     index stands; otherwise (or for s below 1e-270, where the spacing of s is coarse) the cell is redone with k_metrics'
//     own sqrt loop.  A later agent never wins a tie, in either form.
//   * minimum non-zero distance of an agent: d != 0 iff s != 0, and the minimum commutes with sqrt: one sqrt per agent.
//   * np.var: numpy's pairwise sum has eight independent accumulators per block of <= 128 elements; eight lanes run one
//     each (the same additions in the same order), the ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) tree, the tail and the
//     recursive halves above 128 elements are as in np_pairwise_sum.  Minimum and maximum do not depend on the order.
// Per (cell, agent) pair that leaves two subtractions, two multiplications, one addition and a compare in fp64; the agents'
// (x, y) are read as one 16-byte LDS broadcast.
// -------------------------------------------------------------------------------------------------
constexpr int kMsEnvs = 4;                                   // envs (= waves) per workgroup

__device__ inline double wave_get(double v, int lane) { return __shfl(v, lane); }

// np_pairwise_sum(a, n) by one whole wave (every lane calls with the same arguments and gets the same value); a in LDS
__device__ double wave_pairwise_sum(const double *a, int n, int lane)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        const int n8 = n - (n % 8);
        double r = 0.0;
        if (lane < 8) {
            r = a[lane];
            for (int i = 8 + lane; i < n8; i += 8) r += a[i];
        }
        const double r0 = wave_get(r, 0), r1 = wave_get(r, 1), r2 = wave_get(r, 2), r3 = wave_get(r, 3);
        const double r4 = wave_get(r, 4), r5 = wave_get(r, 5), r6 = wave_get(r, 6), r7 = wave_get(r, 7);
        double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (int i = n8; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    const double lo = wave_pairwise_sum(a, n2, lane);
    return lo + wave_pairwise_sum(a + n2, n - n2, lane);
}

template <int WPE>
__global__ void __launch_bounds__(64 * kMsEnvs)
k_metrics_step(const KP P, double *__restrict__ out, const int stride)
{
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int T = 64 * WPE, EPBK = kMsEnvs / WPE;         // lanes per env, envs per workgroup
    const int N = P.n_a, lane = threadIdx.x & 63, w = threadIdx.x / T, t = threadIdx.x % T;
    const bool first = (threadIdx.x >> 6) % WPE == 0;         // the env's first wave runs the np.var tails
    const int e_raw = blockIdx.x * EPBK + w;
    const bool active = e_raw < P.n_env;                     // a surplus wave does no work but meets every barrier
    const int e = active ? e_raw : P.n_env - 1;
    unsigned char *base = smem + (size_t)w * stride;
    double2 *xy = reinterpret_cast<double2 *>(base);                    // [N]
    double *val = reinterpret_cast<double *>(base + (size_t)16 * N);   // [N] per-agent values
    double *tmp = val + N;                                              // [N] scratch
    int *cnt = reinterpret_cast<int *>(tmp + N);                        // [N] Voronoi counts, then [1] coverage count
    const int ng = P.n_g[e];
    const double *gx = P.cells + (size_t)e * 2 * P.ng_max, *gy = gx + P.ng_max;
    for (int i = t; i < N; i += T) {
        double2 q; q.x = P.p[(size_t)e * 2 * N + i]; q.y = P.p[(size_t)e * 2 * N + N + i];
        xy[i] = q; cnt[i] = 0;
    }
    if (t == 0) cnt[N] = 0;
    __syncthreads();
    const double half = P.r_avoid / 2, h2 = half * half;
    const double band = 1.0 + 0x1p-40, h2_lo = h2 * (1.0 - 0x1p-40), h2_hi = h2 * band;
    int covered = 0;
    for (int c = t; c < ng; c += T) {
        const double cx = gx[c], cy = gy[c];
        double best = 0.0, cmin = INFINITY; int owner = 0; bool amb = false;
        for (int j = 0; j < N; ++j) {
            const double2 q = xy[j];
            const double dx = q.x - cx, dy = q.y - cy;
            const double s2 = dx * dx + dy * dy;
            cmin = s2 < cmin ? s2 : cmin;                     // a NaN never covers (d < r/2 is false), but it does seed argmin
            if (j == 0) { best = s2; amb = s2 < 1e-270; }
            else if (s2 < best) { amb = (best <= s2 * band) || (s2 < 1e-270); best = s2; owner = j; }
        }
        if (amb) {                                            // a tie after rounding is possible: k_metrics' own loop
            double bd = 0.0; owner = 0;
            for (int j = 0; j < N; ++j) {
                const double2 q = xy[j];
                const double dx = q.x - cx, dy = q.y - cy;
                const double d = sqrt(dx * dx + dy * dy);
                if (j == 0 || d < bd) { bd = d; owner = j; }
            }
        }
        const bool cov = cmin < h2_lo ? true : (cmin > h2_hi ? false : sqrt(cmin) < half);
        covered += cov ? 1 : 0;
        atomicAdd(&cnt[owner], 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) covered += __shfl_xor(covered, o);
    if (lane == 0) atomicAdd(&cnt[N], covered);                // an integer sum: the order does not matter
    for (int i = t; i < N; i += T) {                           // minimum non-zero distance of every agent
        const double2 a = xy[i];
        double m = INFINITY;
        for (int j = 0; j < N; ++j) {
            const double2 q = xy[j];
            const double dx = q.x - a.x, dy = q.y - a.y;
            const double s2 = dx * dx + dy * dy;
            if (s2 != 0 && s2 < m) m = s2;
        }
        val[i] = sqrt(m);
    }
    __syncthreads();
    double res[2] = {0.0, 0.0};
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {                     // np_var_metric of val, by the env's first wave
        double mean = 0.0, mn = 0.0, mx = 0.0;
        if (first) {
            mean = wave_pairwise_sum(val, N, lane) / N;
            mn = val[0]; mx = val[0];
            for (int i = lane; i < N; i += 64) {
                const double v = val[i], d = v - mean;
                tmp[i] = d * d;
                mn = v < mn ? v : mn; mx = v > mx ? v : mx;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
                mn = a < mn ? a : mn; mx = b > mx ? b : mx;
            }
        }
        __syncthreads();
        if (first) {
            const double var = wave_pairwise_sum(tmp, N, lane) / N;
            res[pass] = (var - mn) / (mx - mn);
        }
        __syncthreads();
        if (pass == 0) {
            for (int i = t; i < N; i += T) val[i] = (double)cnt[i];
            __syncthreads();
        }
    }
    if (active && first && lane == 0) {
        out[(size_t)e * 3 + 0] = (double)cnt[N] / ng;
        out[(size_t)e * 3 + 1] = res[0];
        out[(size_t)e * 3 + 2] = res[1];
    }
}


// (x, y)-interleaved copy of the target cells of envs [e0, e0 + count): the step kernel gathers cells per lane, and one
// 16-byte load per cell costs half the address-unit work of two 8-byte loads from the ABI's [2][ng_max] layout.
__global__ void __launch_bounds__(256)
k_interleave(const double *__restrict__ cells, double2 *__restrict__ out, int ng_max, int e0, int count)
{
    const size_t n = (size_t)count * ng_max;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
        const size_t e = e0 + q / ng_max, c = q % ng_max;
        double2 g; g.x = cells[e * 2 * ng_max + c]; g.y = cells[e * 2 * ng_max + ng_max + c];
        out[e * ng_max + c] = g;
    }
}

// The device-side shape switch (swarm_select_shape; eval_assembly.py:34-57 process_shape with its rotation 0 and offset 0):
// every env takes shape `s` of the uploaded set as it stands -- the whole cell row (the same doubles, padding included) into
// both cell layouts, and the per-env scalars k_reset writes.  p / dp are not touched.
__global__ void __launch_bounds__(256)
k_select_shape(const ShapeSet S, const int s, const int ng_max, double *__restrict__ cells_out, double2 *__restrict__ cells_xy,
               int *__restrict__ ng_out, double *__restrict__ cin_out, LatEnv *__restrict__ lat_out, int *__restrict__ shape_out)
{
    const int e = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;         // grid (ceil(ng_max / 256), n_env)
    if (c < ng_max) {
        double2 g; g.x = S.cells[(size_t)s * 2 * ng_max + c]; g.y = S.cells[(size_t)s * 2 * ng_max + ng_max + c];
        cells_out[(size_t)e * 2 * ng_max + c] = g.x; cells_out[(size_t)e * 2 * ng_max + ng_max + c] = g.y;
        cells_xy[(size_t)e * ng_max + c] = g;
    }
    if (c == 0) { ng_out[e] = S.n_g[s]; cin_out[e] = S.c_in[s]; shape_out[e] = s; lat_out[e] = S.lat[s]; }
}

// The per-env shape switch (swarm_select_shapes; eval_assembly.py:34-57 process_shape with its rand_angle / rand_target_offset):
// env e takes shape shape_index[e] of the uploaded set -- at the set's own pose (pose == NULL: the whole row, the same doubles,
// padding included, as k_select_shape) or at pose[e] = (c, s, off_x, off_y) (k_reset's transform of cells and lattice frame;
// no trigonometric function is evaluated here).  An index outside [0, n_shapes) keeps the env: the range is tested before the
// set is read, and nothing of that env is written.  p / dp are not touched.
constexpr int kLatWords = (int)(sizeof(LatEnv) / 8), kLatFrameWords = 6;      // LatEnv in 8-byte words; ox .. vyi come first
static_assert(sizeof(LatEnv) % 8 == 0 && kLatWords <= 256 && offsetof(LatEnv, vyi) == 8 * (kLatFrameWords - 1) &&
              offsetof(LatEnv, nrows) >= 8 * kLatFrameWords, "k_select_shapes copies LatEnv by words behind its six frame doubles");

__global__ void __launch_bounds__(256)
k_select_shapes(const ShapeSet S, const int *__restrict__ shape_index, const double *__restrict__ pose, const int ng_max,
                double *__restrict__ cells_out, double2 *__restrict__ cells_xy, int *__restrict__ ng_out,
                double *__restrict__ cin_out, LatEnv *__restrict__ lat_out, int *__restrict__ shape_out)
{
    const int e = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;         // grid (ceil(ng_max / 256), n_env)
    const int s = shape_index[e];
    if (s < 0 || s >= S.n_shapes) return;                                 // keep
    const double *sx = S.cells + (size_t)s * 2 * ng_max, *sy = sx + ng_max;
    double cs = 1.0, sn = 0.0, offx = 0.0, offy = 0.0;
    if (pose != nullptr) { cs = pose[4 * (size_t)e]; sn = pose[4 * (size_t)e + 1]; offx = pose[4 * (size_t)e + 2]; offy = pose[4 * (size_t)e + 3]; }
    if (c < ng_max) {
        double2 g;
        if (pose != nullptr) g = pose_cell(sx, sy, c, S.n_g[s], cs, sn, offx, offy);
        else { g.x = sx[c]; g.y = sy[c]; }
        cells_out[(size_t)e * 2 * ng_max + c] = g.x; cells_out[(size_t)e * 2 * ng_max + ng_max + c] = g.y;
        cells_xy[(size_t)e * ng_max + c] = g;
    }
    if (blockIdx.x != 0) return;
    // the lattice record: one word per thread; with a pose thread 0 writes the frame of a record that has one
    const LatEnv *src = S.lat + s;
    const bool framed = pose != nullptr && src->nrows > 0;
    if (c < kLatWords && !(framed && c < kLatFrameWords))
        reinterpret_cast<unsigned long long *>(lat_out + e)[c] = reinterpret_cast<const unsigned long long *>(src)[c];
    if (c == 0) {
        ng_out[e] = S.n_g[s]; cin_out[e] = S.c_in[s]; shape_out[e] = s;
        if (framed) {
            double ox = src->ox, oy = src->oy, uxi = src->uxi, uyi = src->uyi, vxi = src->vxi, vyi = src->vyi;
            pose_lattice(ox, oy, uxi, uyi, vxi, vyi, cs, sn, offx, offy);
            LatEnv *dst = lat_out + e;
            dst->ox = ox; dst->oy = oy; dst->uxi = uxi; dst->uyi = uyi; dst->vxi = vxi; dst->vyi = vyi;
        }
    }
}

// -------------------------------------------------------------------------------------------------
// The reference-shaped host outputs ("a single host-side gather of obs / reward"): the step
// leaves obs [E][N][D], reward [E][N], done [E][N], a_prior [E][N][2] on the device; the numpy API of
// AssemblySwarmEnv.step returns obs (D, n_a) / reward (1, n_a) / a_prior (2, n_a) as float64 and done (1, n_a) as bool with
// the environments side by side on the agent axis (assembly.py:487-666, 227-231, 353, 480-482).  k_export writes exactly
// that block -- widened to double, transposed -- into ONE contiguous device buffer that a single hipMemcpyAsync moves
// into pinned host memory: no per-step allocation, no host-side pass over the data.
// Block layout (doubles): obs D*EN | a_prior 2*EN | reward EN | done EN bytes.
// -------------------------------------------------------------------------------------------------
template <typename OT> __device__ __forceinline__ double wide(OT v) { return (double)v; }
template <> __device__ __forceinline__ double wide<__bf16>(__bf16 v) { return (double)(float)v; }

template <typename OT>
__global__ void __launch_bounds__(256)
k_export(const OT *__restrict__ obs, const float *__restrict__ reward, const uint8_t *__restrict__ done,
         const OT *__restrict__ prior, double *__restrict__ out, const int D, const long long EN, const int with_prior)
{
    // tile: 64 agent rows x 32 features through LDS: reads run along a row (features contiguous), writes along the agent axis
    __shared__ double tile[32][65];
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * 64;
    for (int f0 = 0; f0 < D; f0 += 32) {
        const int fw = D - f0 < 32 ? D - f0 : 32;
        {
            const int f = tid & 31;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int r = (tid >> 5) + 8 * k;
                if (f < fw && r0 + r < EN) tile[f][r] = wide<OT>(obs[(size_t)(r0 + r) * D + f0 + f]);
            }
        }
        __syncthreads();
        {
            const int r = tid & 63;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int f = (tid >> 6) + 4 * k;
                if (f < fw && r0 + r < EN) __builtin_nontemporal_store(tile[f][r], &out[(size_t)(f0 + f) * EN + r0 + r]);
            }
        }
        __syncthreads();
    }
    if (tid < 64 && r0 + tid < EN) {
        const long long a = r0 + tid;
        double *pri = out + (size_t)D * EN, *rew = pri + 2 * EN;
        uint8_t *dn = reinterpret_cast<uint8_t *>(rew + EN);
        if (with_prior) { pri[a] = wide<OT>(prior[2 * a]); pri[EN + a] = wide<OT>(prior[2 * a + 1]); }
        if (reward != nullptr) rew[a] = (double)reward[a];
        if (done != nullptr) dn[a] = done[a];
    }
}

// -------------------------------------------------------------------------------------------------
// The per-env reset (swarm_reset_envs): env e is redrawn for episode[e] >= 0 exactly as k_reset draws it for (seed, episode[e],
// env_offset + e) -- the same draw slots, expressions and order, the device cos / sin, pose_cell / pose_lattice, padding cells
// 0.0: the same bits -- and is left alone for episode[e] < 0 (keep): the block reads its entry first and returns before it
// writes anything of that env (the test is block-uniform and sits in front of everything else; the kernel has no barrier and
// no LDS).  episode is a device array, read when the kernel runs.  A reset env's cells go into both layouts here, as in
// k_select_shapes: no interleave pass follows, and a kept env's cells_xy row is neither read nor written.
// Its own text, behind every other kernel of the file, so that k_reset's device code and the other kernels' stay what they
// were.  Unlike k_reset it holds no LatEnv in registers: the record is copied by words (one per thread, as k_select_shapes
// does) and thread 0 writes the posed frame of a record that has one -- no scratch.
// -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_reset_envs(const KP P, const ShapeSet S, const unsigned long long seed, const long long *__restrict__ episode,
             const long long env_offset, double *__restrict__ cells_out, double2 *__restrict__ cells_xy, int *__restrict__ ng_out,
             double *__restrict__ cin_out, LatEnv *__restrict__ lat_out, int *__restrict__ shape_out)
{
    const int e = blockIdx.x, tid = threadIdx.x;
    const long long ep = episode[e];
    if (ep < 0) return;                                                   // keep
    const unsigned long long key = mix64(mix64(seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)ep + 1)) ^ (unsigned long long)(env_offset + e));
    const double W = P.w_half, H = P.h_half;
    int s = (int)(reset_u01(key, 0) * S.n_shapes);
    s = s >= S.n_shapes ? S.n_shapes - 1 : s;
    const double ang = M_PI * (2.0 * reset_u01(key, 1) - 1.0);
    const double cs = cos(ang), sn = sin(ang);                       // rotate_matrix = [[c, s], [-s, c]], ENV:177
    const double offx = (-W + 1) + reset_u01(key, 4) * (2 * W - 2);
    const double offy = (-H + 1) + reset_u01(key, 5) * (2 * H - 2);
    const int ng = S.n_g[s];
    const double *sx_ = S.cells + (size_t)s * 2 * P.ng_max, *sy_ = sx_ + P.ng_max;
    double *gx = cells_out + (size_t)e * 2 * P.ng_max, *gy = gx + P.ng_max;
    double2 *gxy = cells_xy + (size_t)e * P.ng_max;
    for (int c = tid; c < P.ng_max; c += blockDim.x) {
        const double2 g = pose_cell(sx_, sy_, c, ng, cs, sn, offx, offy);
        gx[c] = g.x; gy[c] = g.y; gxy[c] = g;
    }
    // the lattice record: one word per thread; thread 0 writes the frame of a record that has one (k_reset: pose_lattice iff nrows > 0)
    const LatEnv *src = S.lat + s;
    const bool framed = src->nrows > 0;
    if (tid < kLatWords && !(framed && tid < kLatFrameWords))
        reinterpret_cast<unsigned long long *>(lat_out + e)[tid] = reinterpret_cast<const unsigned long long *>(src)[tid];
    if (tid == 0) {
        ng_out[e] = ng; cin_out[e] = S.c_in[s]; shape_out[e] = s;
        if (framed) {
            double ox = src->ox, oy = src->oy, uxi = src->uxi, uyi = src->uyi, vxi = src->vxi, vyi = src->vyi;
            pose_lattice(ox, oy, uxi, uyi, vxi, vyi, cs, sn, offx, offy);
            LatEnv *dst = lat_out + e;
            dst->ox = ox; dst->oy = oy; dst->uxi = uxi; dst->uyi = uyi; dst->vxi = vxi; dst->vyi = vyi;
        }
    }
    // agents (ENV:202-215)
    const int N = P.n_a;
    const bool spread = (2.0 * reset_u01(key, 6) - 1.0) > 0;
    const double cx = (-W + 1) + reset_u01(key, 7) * (2 * W - 2), cy = (-H + 1) + reset_u01(key, 8) * (2 * H - 2);
    for (int i = tid; i < N; i += blockDim.x) {
        const double ux_ = reset_u01(key, 16 + i), uy_ = reset_u01(key, 16 + N + i);
        double x, y;
        if (spread) { x = -W + ux_ * (2 * W); y = -H + uy_ * (2 * H); }
        else { x = (2.0 * ux_ - 1.0) + cx; y = (2.0 * uy_ - 1.0) + cy; }
        P.p[(size_t)e * 2 * N + i] = x; P.p[(size_t)e * 2 * N + N + i] = y;
        P.dp[(size_t)e * 2 * N + i] = -0.5 + reset_u01(key, 16 + 2 * N + i);
        P.dp[(size_t)e * 2 * N + N + i] = -0.5 + reset_u01(key, 16 + 3 * N + i);
    }
}

}  // namespace

namespace swarm_internal {

hipError_t launch_reset(hipStream_t st, const KP &kp, const ShapeSet &S, unsigned long long seed, unsigned long long episode,
                        long long env_offset, double *cells, int *n_g, double *c_in, LatEnv *lat, int *shape_idx)
{
    hipLaunchKernelGGL(k_reset, dim3(kp.n_env), dim3(256), 0, st, kp, S, seed, episode, env_offset, cells, n_g, c_in, lat, shape_idx);
    return hipGetLastError();
}

hipError_t launch_reset_envs(hipStream_t st, const KP &kp, const ShapeSet &S, unsigned long long seed, const long long *episode,
                             long long env_offset, double *cells, double2 *cells_xy, int *n_g, double *c_in, LatEnv *lat, int *shape_idx)
{
    hipLaunchKernelGGL(k_reset_envs, dim3(kp.n_env), dim3(256), 0, st, kp, S, seed, episode, env_offset, cells, cells_xy, n_g, c_in, lat,
                       shape_idx);
    return hipGetLastError();
}

hipError_t launch_select_shape(hipStream_t st, const ShapeSet &S, int s, int ng_max, int n_env, double *cells, double2 *cells_xy,
                               int *n_g, double *c_in, LatEnv *lat, int *shape_idx)
{
    hipLaunchKernelGGL(k_select_shape, dim3((unsigned)((ng_max + 255) / 256), (unsigned)n_env), dim3(256), 0, st, S, s, ng_max,
                       cells, cells_xy, n_g, c_in, lat, shape_idx);
    return hipGetLastError();
}

hipError_t launch_select_shapes(hipStream_t st, const ShapeSet &S, const int *shape_index, const double *pose, int ng_max, int n_env,
                                double *cells, double2 *cells_xy, int *n_g, double *c_in, LatEnv *lat, int *shape_idx)
{
    hipLaunchKernelGGL(k_select_shapes, dim3((unsigned)((ng_max + 255) / 256), (unsigned)n_env), dim3(256), 0, st, S, shape_index, pose,
                       ng_max, cells, cells_xy, n_g, c_in, lat, shape_idx);
    return hipGetLastError();
}

hipError_t launch_interleave(hipStream_t st, const double *cells, double2 *cells_xy, int ng_max, int e0, int count)
{
    const size_t n = (size_t)count * ng_max;
    hipLaunchKernelGGL(k_interleave, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st,
                       cells, cells_xy, ng_max, e0, count);
    return hipGetLastError();
}

hipError_t launch_metrics(hipStream_t st, const KP &kp, double *out)
{
    const size_t smem = (size_t)kp.n_a * (4 * 8 + 4) + 16;
    hipLaunchKernelGGL(k_metrics, dim3(kp.n_env), dim3(256), smem, st, kp, out);
    return hipGetLastError();
}

hipError_t launch_metrics_step(hipStream_t st, const KP &kp, int n_cu, double *out)
{
    const int stride = (36 * kp.n_a + 4 + 15) & ~15;             // per env: xy[N], val[N], tmp[N], cnt[N + 1]
    // one wave per env needs about two waves per SIMD (4 SIMDs per CU) to hide its latencies; below that, four waves per env.
    // Above 256 agents (large_swarm handles) always four waves per env: four envs' stride would not fit a workgroup's LDS
    if (kp.n_a <= 256 && (long long)kp.n_env >= 8LL * n_cu)
        hipLaunchKernelGGL(k_metrics_step<1>, dim3((unsigned)((kp.n_env + kMsEnvs - 1) / kMsEnvs)), dim3(64 * kMsEnvs),
                           (size_t)stride * kMsEnvs, st, kp, out, stride);
    else
        hipLaunchKernelGGL(k_metrics_step<kMsEnvs>, dim3((unsigned)kp.n_env), dim3(64 * kMsEnvs), (size_t)stride, st,
                           kp, out, stride);
    return hipGetLastError();
}

hipError_t launch_export(hipStream_t st, int obs_dtype, const void *obs, const float *reward, const uint8_t *done,
                         const void *prior, double *out, int D, long long EN, int with_prior)
{
    const unsigned grid = (unsigned)((EN + 63) / 64);
    return with_obs_type(obs_dtype, [&](auto t) {
        typedef typename decltype(t)::type OT;
        hipLaunchKernelGGL(k_export<OT>, dim3(grid), dim3(256), 0, st, (const OT *)obs, reward, done, (const OT *)prior, out, D, EN, with_prior);
        return hipGetLastError();
    });
}

}  // namespace swarm_internal
