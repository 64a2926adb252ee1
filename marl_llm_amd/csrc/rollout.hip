// Device rollout loop (include/swarm_rollout.h): `steps` exploring-actor + env steps enqueued by one library call, the
// transitions written straight into a chained replay ring.  The loop itself is host code that only enqueues: per step the
// policy kernel (policy_mlp.hip) or the uniform-action kernel below, the env step (swarm_env.hip) and, optionally, the
// reward-count kernel below, all on one stream; the reward statistics are finished by one launch after the loop.
// swarm_rollout_expert is the same loop with an expert in place of the policy: the rule-based expert kernel below (after the
// env's index-export observation pass) or a copy of the env's own 'llm' action.  swarm_rollout_eval is the evaluation loop:
// the actor without noise, and per step a state trace, an optional device-side shape switch and the wrapper metrics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>

#include "swarm_internal.h"
#include "swarm_rollout.h"

namespace {

using swarm_internal::np_sum_stream;
using swarm_internal::np_clip1;
using swarm_internal::pmix64;
using swarm_internal::swarm_noise_key;

constexpr unsigned long long kUniformSalt = 0x5851F42D4C957F2Dull;    // separates the uniform stream from the policy's noise
constexpr int kThreads = 256;
constexpr int kCountPerThread = 16;                                      // rewards a thread counts (grid-stride) before the block sum
constexpr int kCountMaxBlocks = 1024;

thread_local std::string g_rollout_error;

int fail(int code, const std::string &msg, const char *who = "swarm_rollout")
{
    g_rollout_error = std::string(who) + ": " + msg;
    return code;
}

// The ring checks shared by swarm_rollout and swarm_rollout_expert; "" = fine.
std::string check_ring_shape(const swarm_env_info &ei, const swarm_ring_t *ring)
{
    char msg[256];
    if (ei.obs_dtype != SWARM_F32 && ei.obs_dtype != SWARM_BF16)
        return "the env handle's obs dtype must be SWARM_F32 or SWARM_BF16 (the ring holds no fp64 rows)";
    if (ring->obs_dtype != ei.obs_dtype) return "ring obs_dtype differs from the env handle's obs dtype";
    const long long rows = (long long)ei.n_env * ei.n_agents;
    if (ring->rows != rows) {
        std::snprintf(msg, sizeof msg, "ring rows %lld != n_env * n_agents = %lld", (long long)ring->rows, rows);
        return msg;
    }
    if (ring->obs_dim != ei.obs_dim) {
        std::snprintf(msg, sizeof msg, "ring obs_dim %d != env obs_dim %d", ring->obs_dim, ei.obs_dim);
        return msg;
    }
    return "";
}

std::string check_ring_slots(const swarm_env_info &ei, const swarm_ring_t *ring)
{
    if (!ring->obs || !ring->act || !ring->rew || !ring->done) return "null ring obs / act / rew / done";
    if (ei.with_prior && !ring->prior) return "the env handle computes a prior (with_prior): ring prior is NULL";
    if (!ei.with_prior && ring->prior) return "the env handle has no prior: ring prior must be NULL";
    if (ring->n_slots < 2) return "ring n_slots must be >= 2";
    if (ring->cur < 0 || ring->cur >= ring->n_slots) return "ring cur outside [0, n_slots)";
    return "";
}

// log-pi of a uniform action on [-1, 1]^2 (agents.py:91: -act_dim * log(2)), rounded to fp32
constexpr float kLogPiUniform = (float)(-2.0 * 0.69314718055994530942);

// The epsilon branch of agents.py:89-91 (np.random.uniform(-1, 1) per component), counter-based: formula in swarm_rollout.h.
// LOGPI: also log_pi[row] = kLogPiUniform (a template parameter: the instantiation without it compiles as before).
template <bool LOGPI>
__global__ void __launch_bounds__(kThreads) k_uniform_actions(float2 *__restrict__ act, long long rows, unsigned long long ukey,
                                                              unsigned long long row_offset, float *__restrict__ log_pi)
{
    const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (row >= rows) return;
    const unsigned long long h = pmix64(ukey ^ (row_offset + (unsigned long long)row));
    float2 a;
    a.x = (float)(unsigned)((h >> 40) & 0xFFFFFFull) * 1.1920928955078125e-07f - 1.0f;      // 2^-23
    a.y = (float)(unsigned)((h >> 16) & 0xFFFFFFull) * 1.1920928955078125e-07f - 1.0f;
    act[row] = a;
    if constexpr (LOGPI) log_pi[row] = kLogPiUniform;
}

// Number of nonzero rewards of one step, added (one 64-bit atomic per workgroup) to the zeroed counter that shares the
// storage of reward_stats[t][0].  An integer sum: the result does not depend on the order the workgroups arrive in.
__global__ void __launch_bounds__(kThreads) k_reward_count(const float *__restrict__ rew, long long n,
                                                           unsigned long long *__restrict__ count)
{
    const long long stride = (long long)gridDim.x * kThreads;
    unsigned c = 0;
    if ((reinterpret_cast<uintptr_t>(rew) & 15) == 0) {                 // 16-byte loads over the whole quads, then the tail
        const float4 *r4 = reinterpret_cast<const float4 *>(rew);
        const long long n4 = n >> 2;
        for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride) {
            const float4 v = r4[i];
            c += (v.x != 0.0f) + (v.y != 0.0f) + (v.z != 0.0f) + (v.w != 0.0f);
        }
        for (long long i = 4 * n4 + (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) c += rew[i] != 0.0f;
    } else {
        for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) c += rew[i] != 0.0f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);            // wave64 sum
    __shared__ unsigned part[kThreads / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) s += part[w];
        atomicAdd(count, s);
    }
}

// reward_stats[t] = (mean, population std) from the count in reward_stats[t][0] (rewards in {0, 1}).
__global__ void __launch_bounds__(kThreads) k_reward_stats(double *__restrict__ stats, int steps, long long n)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= steps) return;
    const unsigned long long c = reinterpret_cast<const unsigned long long *>(stats)[2 * t];
    const double nd = (double)n, cd = (double)c, m = cd / nd;
    const double a = 1.0 - m;
    stats[2 * t] = m;
    stats[2 * t + 1] = sqrt((cd * (a * a) + (nd - cd) * (m * m)) / nd);
}

// ---- expert sources of swarm_rollout_expert

constexpr int kRuleMaxAgents = 256;                                     // swarm_create's n_agents cap

// The rule-based expert (assembly.py:530-601) of every agent of one env per workgroup, for the current state: the same
// fp64 operations in the same order as swarm_env.hip's k_rule (bit-identical output), restructured for the batched
// collection loop.  The env's p / dp are staged in LDS once (k_rule reads every neighbour's from HBM twice); the
// `|r| < d_sen` neighbour test runs once per pair into a per-agent bit mask of W 64-bit words (k_rule evaluates it twice);
// the interaction sum then visits the set bits in ascending j, i.e. k_rule's order.  Writes the fp64 action (the step's
// input) and its f32 rounding (the ring's act row) in the same pass.
template <int W>
__global__ void __launch_bounds__(256) k_rule_ring(const swarm_expert_view V, double2 *__restrict__ act64, float2 *__restrict__ act32)
{
    __shared__ double s_p[2 * kRuleMaxAgents], s_v[2 * kRuleMaxAgents];
    const int N = V.n_agents, e = blockIdx.x, G = V.g_max;
    {
        const double *gp = V.p + (size_t)e * 2 * N, *gv = V.dp + (size_t)e * 2 * N;
        for (int k = threadIdx.x; k < 2 * N; k += blockDim.x) { s_p[k] = gp[k]; s_v[k] = gv[k]; }
    }
    __syncthreads();
    const double *px = s_p, *py = s_p + N, *vx = s_v, *vy = s_v + N;
    const double *gx = V.cells + (size_t)e * 2 * V.ng_max, *gy = gx + V.ng_max;
    const double d_sen = V.d_sen, r_avoid = V.r_avoid;
    const double k_1 = 1, k_2 = 15, k_3 = 17;                                  // :532
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const double xi = px[i], yi = py[i], ui = vx[i], wi = vy[i];
        const bool in_shape = V.in_flag[(size_t)e * N + i] != 0;
        double ent_x = 0.0, ent_y = 0.0;                                       // :538-541
        if (!in_shape) {
            const int bc = V.near_cell[(size_t)e * N + i];
            const double rx = gx[bc] - xi, ry = gy[bc] - yi;
            const double nr = sqrt(rx * rx + ry * ry) + 1e-8;
            ent_x = k_1 * (rx / nr) + (0.0 - ui);
            ent_y = k_1 * (ry / nr) + (0.0 - wi);
        }
        const int *sel = V.exp_sensed + ((size_t)e * N + i) * G;               // capped list, -1 padded (:561-572)
        int n = 0;
        while (n < G && sel[n] >= 0) ++n;
        double exp_x = 0.0, exp_y = 0.0;                                       // :574-584
        if (n > 0) {
            auto psi = [&](double rx, double ry) {                             // _rho_cos_dec(z, 0, d_sen) :846-850
                const double z = sqrt(rx * rx + ry * ry);
                return z < d_sen ? 0.5 * (1.0 + cos(M_PI * (z / d_sen - 0) / (1.0 - 0))) : 0.0;
            };
            const double sx = np_sum_stream(n, [&](int q) { const int c = sel[q]; const double rx = gx[c] - xi, ry = gy[c] - yi; return psi(rx, ry) * rx; });
            const double sy = np_sum_stream(n, [&](int q) { const int c = sel[q]; const double rx = gx[c] - xi, ry = gy[c] - yi; return psi(rx, ry) * ry; });
            double den = np_sum_stream(n, [&](int q) { const int c = sel[q]; return psi(gx[c] - xi, gy[c] - yi); });
            if (den == 0) den = 1e-8;
            exp_x = k_2 * sx / den; exp_y = k_2 * sy / den;
        }
        unsigned long long near[W];                                            // :587-598, neighbours j != i with |r| < d_sen
        int n_near = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            unsigned long long m = 0;
            const int jn = min(64, N - 64 * w);
            for (int b = 0; b < jn; ++b) {
                const int j = 64 * w + b;
                const double rx = px[j] - xi, ry = py[j] - yi;
                m |= (unsigned long long)(j != i && sqrt(rx * rx + ry * ry) < d_sen) << b;
            }
            near[w] = m;
            n_near += __popcll(m);
        }
        double int_x = 0.0, int_y = 0.0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            for (unsigned long long m = near[w]; m; m &= m - 1) {
                const int j = 64 * w + __ffsll((long long)m) - 1;
                const double rx = px[j] - xi, ry = py[j] - yi;
                const double nr = sqrt(rx * rx + ry * ry);
                if (nr < r_avoid) {
                    const double c = -k_3 * (r_avoid / nr - 1);
                    int_x += c * rx; int_y += c * ry;
                }
                int_x += 5 * (vx[j] - ui) / n_near; int_y += 5 * (vy[j] - wi) / n_near;
            }
        }
        const double ax = (ent_x + exp_x) + int_x, ay = (ent_y + exp_y) + int_y;
        double2 a;
        a.x = np_clip1(ax);                                                    // np.clip :601
        a.y = np_clip1(ay);
        act64[(size_t)e * N + i] = a;
        act32[(size_t)e * N + i] = make_float2((float)a.x, (float)a.y);
    }
}

// The 'llm' source: the action the step is about to apply (the env's own d_act_next, fp64) rounded to f32 into act[c].
__global__ void __launch_bounds__(kThreads) k_act_f32(const double2 *__restrict__ src, float2 *__restrict__ dst, long long rows)
{
    const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (row >= rows) return;
    const double2 a = src[row];
    dst[row] = make_float2((float)a.x, (float)a.y);
}

int launch_rule_ring(const swarm_expert_view &v, float2 *act32, hipStream_t st)
{
    const dim3 grid(v.n_env), block(v.n_agents <= 64 ? 64 : 256);          // k_rule's launch shape
    switch ((v.n_agents + 63) / 64) {
    case 1: hipLaunchKernelGGL(k_rule_ring<1>, grid, block, 0, st, v, v.act64, act32); break;
    case 2: hipLaunchKernelGGL(k_rule_ring<2>, grid, block, 0, st, v, v.act64, act32); break;
    case 3: hipLaunchKernelGGL(k_rule_ring<3>, grid, block, 0, st, v, v.act64, act32); break;
    default: hipLaunchKernelGGL(k_rule_ring<4>, grid, block, 0, st, v, v.act64, act32); break;
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

struct DeviceScope {
    int prev = -1;
    bool ok = false;
    explicit DeviceScope(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) { prev = -1; return; }
        ok = prev == dev || hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace

// swarm_rollout (want_logpi = false, log_pi = NULL) and swarm_rollout_logpi (log_pi [n_slots][rows], written per step like act).
static int rollout_impl(const char *who, bool want_logpi, swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring,
                        float *log_pi, int32_t steps, const uint8_t *uniform_steps, float noise_scale, uint64_t seed, uint64_t step0,
                        uint64_t row_offset, double *reward_stats, void *stream)
{
    // ---- validation: nothing is enqueued before all of it passed
    if (!env || !pol || !ring) return fail(SWARM_ERR_INVALID, "null env, policy or ring", who);
    if (want_logpi && !log_pi) return fail(SWARM_ERR_INVALID, "null log_pi (a [n_slots][rows] fp32 device array is required)", who);
    swarm_env_info ei;
    swarm_policy_info pi;
    if (swarm_internal_env_info(env, &ei) != SWARM_OK || swarm_internal_policy_info(pol, &pi) != SWARM_POLICY_OK)
        return fail(SWARM_ERR_INVALID, "bad handle", who);
    char msg[256];
    if (steps < 0) return fail(SWARM_ERR_INVALID, "steps < 0", who);
    if (ei.device != pi.device) {
        std::snprintf(msg, sizeof msg, "env handle on device %d, policy on device %d", ei.device, pi.device);
        return fail(SWARM_ERR_INVALID, msg, who);
    }
    if (ei.obs_dtype != SWARM_F32 && ei.obs_dtype != SWARM_BF16)
        return fail(SWARM_ERR_INVALID, "the env handle's obs dtype must be SWARM_F32 or SWARM_BF16 (the policy reads no fp64 rows)", who);
    {
        const std::string m = check_ring_shape(ei, ring);
        if (!m.empty()) return fail(SWARM_ERR_INVALID, m, who);
    }
    const long long rows = (long long)ei.n_env * ei.n_agents;
    if (pi.in_dim != ei.obs_dim) {
        std::snprintf(msg, sizeof msg, "policy in_dim %d != env obs_dim %d", pi.in_dim, ei.obs_dim);
        return fail(SWARM_ERR_INVALID, msg, who);
    }
    if (pi.act_dim != 2) return fail(SWARM_ERR_INVALID, "policy act_dim must be 2 (the env's action)", who);
    if (ei.obs_dtype == SWARM_BF16 && (pi.in_dim & 7)) return fail(SWARM_ERR_INVALID, "bf16 observation rows need obs_dim % 8 == 0", who);
    {
        const std::string m = check_ring_slots(ei, ring);
        if (!m.empty()) return fail(SWARM_ERR_INVALID, m, who);
    }
    if (!ei.observed) return fail(SWARM_ERR_STATE, "the env handle is not observed (swarm_observe / swarm_reset first)", who);
    if (steps == 0) return SWARM_OK;

    // ---- enqueue
    DeviceScope dev(ei.device);
    if (!dev.ok) return fail(SWARM_ERR_HIP, "hipSetDevice failed", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (swarm_set_stream(env, stream) != SWARM_OK) return fail(SWARM_ERR_INVALID, "swarm_set_stream failed", who);
    const bool bf16 = ei.obs_dtype == SWARM_BF16;
    const size_t obs_slot = (size_t)rows * ei.obs_dim * (bf16 ? 2 : 4), pri_slot = (size_t)rows * 2 * (bf16 ? 2 : 4);
    char *const obs = static_cast<char *>(ring->obs), *const pri = static_cast<char *>(ring->prior);
    if (reward_stats) {
        const hipError_t e = hipMemsetAsync(reward_stats, 0, (size_t)steps * 2 * sizeof(double), st);
        if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e), who);
    }
    const unsigned act_grid = (unsigned)((rows + kThreads - 1) / kThreads);
    const unsigned cnt_grid = (unsigned)std::min<long long>((rows + kThreads * kCountPerThread - 1) / (kThreads * kCountPerThread),
                                                            kCountMaxBlocks);
    for (int t = 0; t < steps; ++t) {
        const int c = (int)(((long long)ring->cur + t) % ring->n_slots), n = (c + 1) % ring->n_slots;
        float *const act = ring->act + (size_t)c * rows * 2;
        float *const lp = log_pi ? log_pi + (size_t)c * rows : nullptr;
        if (uniform_steps && uniform_steps[t]) {
            const unsigned long long ukey = pmix64(swarm_noise_key(seed, step0 + t) ^ kUniformSalt);
            if (lp)
                hipLaunchKernelGGL(k_uniform_actions<true>, dim3(act_grid), dim3(kThreads), 0, st, reinterpret_cast<float2 *>(act), rows,
                                   ukey, (unsigned long long)row_offset, lp);
            else
                hipLaunchKernelGGL(k_uniform_actions<false>, dim3(act_grid), dim3(kThreads), 0, st, reinterpret_cast<float2 *>(act), rows,
                                   ukey, (unsigned long long)row_offset, nullptr);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("k_uniform_actions: ") + hipGetErrorString(e), who);
        } else if ((lp ? swarm_policy_forward_explore_logpi(pol, obs + c * obs_slot, bf16, rows, act, lp, noise_scale, seed, step0 + t,
                                                            row_offset, stream)
                       : swarm_policy_forward_explore_at(pol, obs + c * obs_slot, bf16, rows, act, noise_scale, seed, step0 + t,
                                                         row_offset, stream)) != SWARM_POLICY_OK) {
            return fail(SWARM_ERR_HIP, swarm_policy_last_error(), who);
        }
        const int rc = swarm_step(env, act, SWARM_F32, obs + n * obs_slot, ring->rew + (size_t)c * rows, ring->done + (size_t)c * rows,
                                  pri ? pri + c * pri_slot : nullptr);
        if (rc != SWARM_OK) return fail(rc, swarm_last_error(env), who);
        if (reward_stats) {
            hipLaunchKernelGGL(k_reward_count, dim3(cnt_grid), dim3(kThreads), 0, st, ring->rew + (size_t)c * rows, rows,
                               reinterpret_cast<unsigned long long *>(reward_stats + 2 * t));
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("k_reward_count: ") + hipGetErrorString(e), who);
        }
    }
    if (reward_stats) {
        hipLaunchKernelGGL(k_reward_stats, dim3((steps + kThreads - 1) / kThreads), dim3(kThreads), 0, st, reward_stats, (int)steps, rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("k_reward_stats: ") + hipGetErrorString(e), who);
    }
    return SWARM_OK;
}

extern "C" {

const char *swarm_rollout_last_error(void) { return g_rollout_error.c_str(); }

int swarm_rollout(swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring, int32_t steps, const uint8_t *uniform_steps,
                  float noise_scale, uint64_t seed, uint64_t step0, uint64_t row_offset, double *reward_stats, void *stream)
{
    return rollout_impl("swarm_rollout", false, env, pol, ring, nullptr, steps, uniform_steps, noise_scale, seed, step0, row_offset,
                        reward_stats, stream);
}

int swarm_rollout_logpi(swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring, float *log_pi, int32_t steps,
                        const uint8_t *uniform_steps, float noise_scale, uint64_t seed, uint64_t step0, uint64_t row_offset,
                        double *reward_stats, void *stream)
{
    return rollout_impl("swarm_rollout_logpi", true, env, pol, ring, log_pi, steps, uniform_steps, noise_scale, seed, step0, row_offset,
                        reward_stats, stream);
}

int swarm_rollout_expert(swarm_env_t *env, const swarm_ring_t *ring, int32_t steps, int32_t source, double *reward_stats, void *stream)
{
    static const char *const who = "swarm_rollout_expert";
    // ---- validation: nothing is enqueued before all of it passed
    if (source != SWARM_EXPERT_RULE && source != SWARM_EXPERT_LLM)
        return fail(SWARM_ERR_INVALID, "source must be SWARM_EXPERT_RULE (0) or SWARM_EXPERT_LLM (1)", who);
    if (!env || !ring) return fail(SWARM_ERR_INVALID, "null env or ring", who);
    swarm_env_info ei;
    if (swarm_internal_env_info(env, &ei) != SWARM_OK) return fail(SWARM_ERR_INVALID, "bad handle", who);
    if (steps < 0) return fail(SWARM_ERR_INVALID, "steps < 0", who);
    {
        std::string m = check_ring_shape(ei, ring);
        if (m.empty()) m = check_ring_slots(ei, ring);
        if (!m.empty()) return fail(SWARM_ERR_INVALID, m, who);
    }
    if (ei.n_agents > kRuleMaxAgents) return fail(SWARM_ERR_INVALID, "n_agents > 256", who);
    if (source == SWARM_EXPERT_RULE && ei.g_max > 128)
        return fail(SWARM_ERR_INVALID, "the rule expert needs num_obs_grid_max <= 128 (as swarm_rule_action)", who);
    if (source == SWARM_EXPERT_LLM && !ei.llm_action)
        return fail(SWARM_ERR_INVALID, "the llm source needs a handle created with llm_action", who);
    if (!ei.observed) return fail(SWARM_ERR_STATE, "the env handle is not observed (swarm_observe / swarm_reset first)", who);
    if (steps == 0) return SWARM_OK;

    // ---- enqueue
    DeviceScope dev(ei.device);
    if (!dev.ok) return fail(SWARM_ERR_HIP, "hipSetDevice failed", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (swarm_set_stream(env, stream) != SWARM_OK) return fail(SWARM_ERR_INVALID, "swarm_set_stream failed", who);
    const long long rows = ring->rows;
    const bool bf16 = ei.obs_dtype == SWARM_BF16;
    const size_t obs_slot = (size_t)rows * ei.obs_dim * (bf16 ? 2 : 4), pri_slot = (size_t)rows * 2 * (bf16 ? 2 : 4);
    char *const obs = static_cast<char *>(ring->obs), *const pri = static_cast<char *>(ring->prior);
    if (reward_stats) {
        const hipError_t e = hipMemsetAsync(reward_stats, 0, (size_t)steps * 2 * sizeof(double), st);
        if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e), who);
    }
    const unsigned act_grid = (unsigned)((rows + kThreads - 1) / kThreads);
    const unsigned cnt_grid = (unsigned)std::min<long long>((rows + kThreads * kCountPerThread - 1) / (kThreads * kCountPerThread),
                                                            kCountMaxBlocks);
    for (int t = 0; t < steps; ++t) {
        const int c = (int)(((long long)ring->cur + t) % ring->n_slots), n = (c + 1) % ring->n_slots;
        float2 *const act = reinterpret_cast<float2 *>(ring->act + (size_t)c * rows * 2);
        swarm_expert_view v;
        int rc = swarm_internal_expert_view(env, source == SWARM_EXPERT_RULE, &v);
        if (rc != SWARM_OK) return fail(rc, swarm_last_error(env), who);
        const void *step_act = nullptr;                                  // LLM: NULL = the handle's own action
        if (source == SWARM_EXPERT_RULE) {
            const int e = launch_rule_ring(v, act, st);
            if (e) return fail(SWARM_ERR_HIP, std::string("k_rule_ring: ") + hipGetErrorString((hipError_t)e), who);
            step_act = v.act64;
        } else {
            hipLaunchKernelGGL(k_act_f32, dim3(act_grid), dim3(kThreads), 0, st, v.act_next, act, rows);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("k_act_f32: ") + hipGetErrorString(e), who);
        }
        rc = swarm_step(env, step_act, SWARM_F64, obs + n * obs_slot, ring->rew + (size_t)c * rows, ring->done + (size_t)c * rows,
                        pri ? pri + c * pri_slot : nullptr);
        if (rc != SWARM_OK) return fail(rc, swarm_last_error(env), who);
        if (reward_stats) {
            hipLaunchKernelGGL(k_reward_count, dim3(cnt_grid), dim3(kThreads), 0, st, ring->rew + (size_t)c * rows, rows,
                               reinterpret_cast<unsigned long long *>(reward_stats + 2 * t));
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("k_reward_count: ") + hipGetErrorString(e), who);
        }
    }
    if (reward_stats) {
        hipLaunchKernelGGL(k_reward_stats, dim3((steps + kThreads - 1) / kThreads), dim3(kThreads), 0, st, reward_stats, (int)steps, rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("k_reward_stats: ") + hipGetErrorString(e), who);
    }
    return SWARM_OK;
}

int swarm_rollout_eval(swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring, int32_t steps, const int32_t *switch_to,
                       const swarm_eval_out_t *out, void *stream)
{
    static const char *const who = "swarm_rollout_eval";
    // ---- validation: nothing is enqueued before all of it passed
    if (!env || !pol || !ring) return fail(SWARM_ERR_INVALID, "null env, policy or ring", who);
    swarm_env_info ei;
    swarm_policy_info pi;
    if (swarm_internal_env_info(env, &ei) != SWARM_OK || swarm_internal_policy_info(pol, &pi) != SWARM_POLICY_OK)
        return fail(SWARM_ERR_INVALID, "bad handle", who);
    char msg[256];
    if (steps < 0) return fail(SWARM_ERR_INVALID, "steps < 0", who);
    if (ei.device != pi.device) {
        std::snprintf(msg, sizeof msg, "env handle on device %d, policy on device %d", ei.device, pi.device);
        return fail(SWARM_ERR_INVALID, msg, who);
    }
    {
        std::string m = check_ring_shape(ei, ring);
        if (!m.empty()) return fail(SWARM_ERR_INVALID, m, who);
    }
    const long long rows = (long long)ei.n_env * ei.n_agents;
    if (pi.in_dim != ei.obs_dim) {
        std::snprintf(msg, sizeof msg, "policy in_dim %d != env obs_dim %d", pi.in_dim, ei.obs_dim);
        return fail(SWARM_ERR_INVALID, msg, who);
    }
    if (pi.act_dim != 2) return fail(SWARM_ERR_INVALID, "policy act_dim must be 2 (the env's action)", who);
    if (ei.obs_dtype == SWARM_BF16 && (pi.in_dim & 7)) return fail(SWARM_ERR_INVALID, "bf16 observation rows need obs_dim % 8 == 0", who);
    {
        const std::string m = check_ring_slots(ei, ring);
        if (!m.empty()) return fail(SWARM_ERR_INVALID, m, who);
    }
    const swarm_eval_out_t none = {nullptr, nullptr, nullptr, nullptr};
    const swarm_eval_out_t &o = out ? *out : none;
    if ((o.p == nullptr) != (o.dp == nullptr)) return fail(SWARM_ERR_INVALID, "the state trace needs p and dp together", who);
    bool switches = false;
    if (switch_to) {
        for (int t = 0; t < steps; ++t) {
            if (switch_to[t] < -1 || (switch_to[t] >= 0 && ei.n_shapes >= 1 && switch_to[t] >= ei.n_shapes)) {
                std::snprintf(msg, sizeof msg, "switch_to[%d] = %d outside [-1, n_shapes = %d)", t, (int)switch_to[t], ei.n_shapes);
                return fail(SWARM_ERR_INVALID, msg, who);
            }
            switches = switches || switch_to[t] >= 0;
        }
    }
    if (switches && ei.n_shapes < 1) return fail(SWARM_ERR_STATE, "switch_to needs a shape set (swarm_set_shapes)", who);
    if (!ei.observed) return fail(SWARM_ERR_STATE, "the env handle is not observed (swarm_observe / swarm_reset first)", who);
    if (steps == 0) return SWARM_OK;

    // ---- enqueue
    DeviceScope dev(ei.device);
    if (!dev.ok) return fail(SWARM_ERR_HIP, "hipSetDevice failed", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (swarm_set_stream(env, stream) != SWARM_OK) return fail(SWARM_ERR_INVALID, "swarm_set_stream failed", who);
    const bool bf16 = ei.obs_dtype == SWARM_BF16;
    const size_t obs_slot = (size_t)rows * ei.obs_dim * (bf16 ? 2 : 4), pri_slot = (size_t)rows * 2 * (bf16 ? 2 : 4);
    char *const obs = static_cast<char *>(ring->obs), *const pri = static_cast<char *>(ring->prior);
    swarm_expert_view v;                                                 // the handle's p / dp (no lists: nothing is enqueued)
    if (swarm_internal_expert_view(env, false, &v) != SWARM_OK) return fail(SWARM_ERR_INVALID, "bad handle", who);
    if (o.reward_stats) {
        const hipError_t e = hipMemsetAsync(o.reward_stats, 0, (size_t)steps * 2 * sizeof(double), st);
        if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e), who);
    }
    const size_t state_elems = (size_t)rows * 2, state_bytes = state_elems * sizeof(double);
    const unsigned cnt_grid = (unsigned)std::min<long long>((rows + kThreads * kCountPerThread - 1) / (kThreads * kCountPerThread),
                                                            kCountMaxBlocks);
    for (int t = 0; t < steps; ++t) {
        const int c = (int)(((long long)ring->cur + t) % ring->n_slots), n = (c + 1) % ring->n_slots;
        float *const act = ring->act + (size_t)c * rows * 2;
        if (o.p) {
            hipError_t e = hipMemcpyAsync(o.p + (size_t)t * state_elems, v.p, state_bytes, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(o.dp + (size_t)t * state_elems, v.dp, state_bytes, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("state trace copy: ") + hipGetErrorString(e), who);
        }
        if (switch_to && switch_to[t] >= 0) {
            const int rc = swarm_select_shape(env, switch_to[t], nullptr);
            if (rc != SWARM_OK) return fail(rc, swarm_last_error(env), who);
        }
        if (o.metrics) {
            const int rc = swarm_internal_metrics_step(env, o.metrics + (size_t)t * ei.n_env * 3);
            if (rc != SWARM_OK) return fail(rc, swarm_last_error(env), who);
        }
        if (swarm_policy_forward_explore_at(pol, obs + c * obs_slot, bf16, rows, act, 0.0f, 0, (uint64_t)t, 0, stream) != SWARM_POLICY_OK)
            return fail(SWARM_ERR_HIP, swarm_policy_last_error(), who);
        const int rc = swarm_step(env, act, SWARM_F32, obs + n * obs_slot, ring->rew + (size_t)c * rows, ring->done + (size_t)c * rows,
                                  pri ? pri + c * pri_slot : nullptr);
        if (rc != SWARM_OK) return fail(rc, swarm_last_error(env), who);
        if (o.reward_stats) {
            hipLaunchKernelGGL(k_reward_count, dim3(cnt_grid), dim3(kThreads), 0, st, ring->rew + (size_t)c * rows, rows,
                               reinterpret_cast<unsigned long long *>(o.reward_stats + 2 * t));
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("k_reward_count: ") + hipGetErrorString(e), who);
        }
    }
    if (o.reward_stats) {
        hipLaunchKernelGGL(k_reward_stats, dim3((steps + kThreads - 1) / kThreads), dim3(kThreads), 0, st, o.reward_stats, (int)steps, rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("k_reward_stats: ") + hipGetErrorString(e), who);
    }
    return SWARM_OK;
}

}  // extern "C"
