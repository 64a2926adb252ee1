// Device rollout loop (include/swarm_rollout.h): `steps` exploring-actor + env steps enqueued by one library call, the
// transitions written straight into a chained replay ring.  The loop itself is host code that only enqueues: per step the
// policy kernel (policy_mlp.hip) or the uniform-action kernel below, the env step (swarm_env.hip) and, optionally, the
// reward-count kernel below, all on one stream; the reward statistics are finished by one launch after the loop.
// swarm_rollout_explore is that loop with the exploration per env: the actor without noise, then k_explore_envs below.
// swarm_rollout_expert is the same loop with an expert in place of the policy: the rule-based expert kernel (rule_expert.hip,
// after the env's index-export observation pass) or a copy of the env's own 'llm' action.  swarm_rollout_eval is the evaluation loop:
// the actor without noise, and per step a state trace, an optional device-side shape switch and the wrapper metrics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>

#include "swarm_internal.h"
#include "swarm_rollout.h"

namespace {

using swarm_internal::DeviceGuard;
using swarm_internal::obs_elem_bytes;
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

// Per-env exploration (swarm_rollout.h "Per-env exploration"), in place on the deterministic actor's output: one thread per
// row.  Env e's coin picks the uniform action of k_uniform_actions for all of its rows; otherwise sigma[e] > 0 adds the policy
// kernel's Gaussian noise -- the Box-Muller block of policy_mlp.hip restated for act_dim 2 with the same calls (logf, sqrtf,
// sincosf) in the same order, so that a constant sigma reproduces that kernel's epilogue bit for bit -- and sigma[e] <= 0 / NaN
// leaves the action alone.  epsilon[e], sigma[e] and log_c[e] are one address per wave where n_agents is a multiple of 64.
// The first row of each env writes coin[e].  LOGPI: also log_pi[row].
struct ExploreParams {
    const float *epsilon, *sigma, *log_c;      // [E]; epsilon may be NULL, log_c is read with LOGPI only
    unsigned long long key, ckey, ukey;        // the step's noise key, and its coin and uniform-action keys
    unsigned long long row_offset, env_offset; // global row of row 0, global env of env 0
    long long rows;
    int n_agents;
};
constexpr unsigned long long kCoinSalt = 0xA0761D6478BD642Full;          // separates the coin stream from the other two

template <bool LOGPI>
__global__ void __launch_bounds__(kThreads) k_explore_envs(float2 *__restrict__ act, float *__restrict__ log_pi,
                                                           uint8_t *__restrict__ coin, const ExploreParams P)
{
    const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (row >= P.rows) return;
    // rows below 2^31 (every batch in practice): a 32-bit division
    const long long e = P.rows <= 0x7FFFFFFFll ? (long long)((unsigned)row / (unsigned)P.n_agents) : row / P.n_agents;
    const unsigned long long g = P.row_offset + (unsigned long long)row;
    const unsigned long long hc = pmix64(P.ckey ^ (P.env_offset + (unsigned long long)e));
    const float u = (float)(unsigned)(hc >> 40) * 5.9604644775390625e-08f;                              // 2^-24: [0, 1)
    const bool fire = P.epsilon != nullptr && u < P.epsilon[e];
    if (coin != nullptr && row == e * P.n_agents) coin[e] = fire ? 1 : 0;
    if (fire) {
        const unsigned long long h = pmix64(P.ukey ^ g);
        float2 a;
        a.x = (float)(unsigned)((h >> 40) & 0xFFFFFFull) * 1.1920928955078125e-07f - 1.0f;             // 2^-23
        a.y = (float)(unsigned)((h >> 16) & 0xFFFFFFull) * 1.1920928955078125e-07f - 1.0f;
        act[row] = a;
        if constexpr (LOGPI) log_pi[row] = kLogPiUniform;
        return;
    }
    const float sg = P.sigma[e];
    float lp = -0.0f;                                                       // no noise: -act_dim log(1) = -0.0
    if (sg > 0.0f) {
        const unsigned long long hk = pmix64(P.key ^ g);
        const float u1 = (float)((unsigned)(hk >> 40) + 1u) * 5.9604644775390625e-08f;                  // (0, 1]
        const float u2 = (float)((unsigned)(hk >> 16) & 0xFFFFFFu) * 5.9604644775390625e-08f;           // [0, 1)
        const float rad = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincosf(6.283185307179586f * u2, &sn, &cs);
        const float z0 = rad * cs, z1 = rad * sn;
        float2 a = act[row];
        a.x = fminf(fmaxf(a.x + sg * z0, -1.0f), 1.0f);
        a.y = fminf(fmaxf(a.y + sg * z1, -1.0f), 1.0f);
        act[row] = a;
        if constexpr (LOGPI) {                                              // -(0.5 sum_k z_k^2) - c, the sum in k order
            float s = z0 * z0;
            s = s + z1 * z1;
            lp = -(0.5f * s) - P.log_c[e];
        }
    }
    if constexpr (LOGPI) log_pi[row] = lp;
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

// ---- expert sources of swarm_rollout_expert: the rule-expert kernel (rule_expert.hip) and

// the 'llm' source: the action the step is about to apply (the env's own d_act_next, fp64) rounded to f32 into act[c].
__global__ void __launch_bounds__(kThreads) k_act_f32(const double2 *__restrict__ src, float2 *__restrict__ dst, long long rows)
{
    const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (row >= rows) return;
    const double2 a = src[row];
    dst[row] = make_float2((float)a.x, (float)a.y);
}

// ---- validation shared by the entry points: each returns SWARM_OK or fail()'s code, in the order the callers document

// The handles' infos (pol, pi: NULL for an entry point without a policy), steps and the devices.
int check_handles(const char *who, const swarm_env_t *env, int32_t steps, swarm_env_info &ei, const swarm_policy_t *pol = nullptr,
                  swarm_policy_info *pi = nullptr)
{
    if (swarm_internal_env_info(env, &ei) != SWARM_OK || (pol && swarm_internal_policy_info(pol, pi) != SWARM_POLICY_OK))
        return fail(SWARM_ERR_INVALID, "bad handle", who);
    if (steps < 0) return fail(SWARM_ERR_INVALID, "steps < 0", who);
    if (pol && ei.device != pi->device) {
        char msg[256];
        std::snprintf(msg, sizeof msg, "env handle on device %d, policy on device %d", ei.device, pi->device);
        return fail(SWARM_ERR_INVALID, msg, who);
    }
    return SWARM_OK;
}

// A policy's loop: the ring's shape, the policy's dimensions against the env's, the ring's slots.
int check_policy_ring(const char *who, const swarm_env_info &ei, const swarm_policy_info &pi, const swarm_ring_t *ring)
{
    std::string m = check_ring_shape(ei, ring);
    if (!m.empty()) return fail(SWARM_ERR_INVALID, m, who);
    if (pi.in_dim != ei.obs_dim) {
        char msg[256];
        std::snprintf(msg, sizeof msg, "policy in_dim %d != env obs_dim %d", pi.in_dim, ei.obs_dim);
        return fail(SWARM_ERR_INVALID, msg, who);
    }
    if (pi.act_dim != 2) return fail(SWARM_ERR_INVALID, "policy act_dim must be 2 (the env's action)", who);
    if (ei.obs_dtype == SWARM_BF16 && (pi.in_dim & 7)) return fail(SWARM_ERR_INVALID, "bf16 observation rows need obs_dim % 8 == 0", who);
    if (pi.route_n_env > 0) {                                               // a routed bank: the route must be this env handle's
        if (pi.route_n_env != ei.n_env || pi.route_rows_per_env != ei.n_agents) {
            char msg[256];
            std::snprintf(msg, sizeof msg, "the policy bank's route is for n_env %d x rows_per_env %d, the env handle has n_env %d x n_agents %d "
                          "(swarm_policy_bank_route)", pi.route_n_env, pi.route_rows_per_env, ei.n_env, ei.n_agents);
            return fail(SWARM_ERR_INVALID, msg, who);
        }
    } else if (ei.n_env % pi.members != 0) {                                // a bank: a member owns whole envs
        char msg[256];
        std::snprintf(msg, sizeof msg, "n_env %d is no multiple of the policy bank's members %d (a member acts for whole envs)",
                      ei.n_env, pi.members);
        return fail(SWARM_ERR_INVALID, msg, who);
    }
    m = check_ring_slots(ei, ring);
    return m.empty() ? SWARM_OK : fail(SWARM_ERR_INVALID, m, who);
}

int check_observed(const char *who, const swarm_env_info &ei)
{
    return ei.observed ? SWARM_OK : fail(SWARM_ERR_STATE, "the env handle is not observed (swarm_observe / swarm_reset first)", who);
}

int hip_check(const char *who, hipError_t e, const char *what)
{
    return e == hipSuccess ? SWARM_OK : fail(SWARM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e), who);
}

// ---- the loop shared by the entry points

// One call's context, built after validation: the device and the stream in force, and where slot t of the ring lives.
struct Loop {
    const char *const who;
    swarm_env_t *const env;
    DeviceGuard dev;
    void *const stream;                                                     // as the libraries' entry points take it
    const hipStream_t st;
    const long long rows;
    const bool bf16;
    const size_t obs_slot, pri_slot;
    char *const obs_base, *const pri_base;
    float *const act_base, *const rew_base;
    uint8_t *const done_base;
    const int cur, n_slots;
    int rc;                                                                 // SWARM_OK, or why nothing may be enqueued

    Loop(const char *who_, swarm_env_t *env_, const swarm_env_info &ei, const swarm_ring_t *ring, void *stream_)
        : who(who_), env(env_), dev(ei.device), stream(stream_), st(static_cast<hipStream_t>(stream_)), rows(ring->rows),
          bf16(ei.obs_dtype == SWARM_BF16), obs_slot((size_t)rows * ei.obs_dim * obs_elem_bytes(ei.obs_dtype)), pri_slot((size_t)rows * 2 * obs_elem_bytes(ei.obs_dtype)),
          obs_base(static_cast<char *>(ring->obs)), pri_base(static_cast<char *>(ring->prior)), act_base(ring->act), rew_base(ring->rew),
          done_base(ring->done), cur(ring->cur), n_slots(ring->n_slots), rc(SWARM_OK)
    {
        if (!dev.ok) rc = fail(SWARM_ERR_HIP, "hipSetDevice failed", who);
        else if (swarm_set_stream(env, stream) != SWARM_OK) rc = fail(SWARM_ERR_INVALID, "swarm_set_stream failed", who);
    }

    int c(int t) const { return (int)(((long long)cur + t) % n_slots); }   // the slot step t writes; its next obs goes to n(t)
    int n(int t) const { return (c(t) + 1) % n_slots; }
    float *act(int t) const { return act_base + (size_t)c(t) * rows * 2; }
    void *obs(int slot) const { return obs_base + slot * obs_slot; }
    float *rew(int t) const { return rew_base + (size_t)c(t) * rows; }
    uint8_t *done(int t) const { return done_base + (size_t)c(t) * rows; }
    void *prior(int t) const { return pri_base ? pri_base + c(t) * pri_slot : nullptr; }
    unsigned row_grid() const { return (unsigned)((rows + kThreads - 1) / kThreads); }

    int step(const void *action, int dtype, int t) const
    {
        const int r = swarm_step(env, action, dtype, obs(n(t)), rew(t), done(t), prior(t));
        return r == SWARM_OK ? SWARM_OK : fail(r, swarm_last_error(env), who);
    }
    int check(hipError_t e, const char *what) const { return hip_check(who, e, what); }
    int launched(const char *kernel) const { return check(hipGetLastError(), kernel); }
};

// reward_stats [steps][2] (DEVICE) of a loop; every member is a no-op when stats is NULL.
struct RewardStats {
    const Loop &L;
    double *const stats;
    const int steps;

    int begin() const { return stats ? L.check(hipMemsetAsync(stats, 0, (size_t)steps * 2 * sizeof(double), L.st), "hipMemsetAsync") : SWARM_OK; }
    int count(int t) const
    {
        if (!stats) return SWARM_OK;
        const unsigned grid = (unsigned)std::min<long long>((L.rows + kThreads * kCountPerThread - 1) / (kThreads * kCountPerThread),
                                                            kCountMaxBlocks);
        hipLaunchKernelGGL(k_reward_count, dim3(grid), dim3(kThreads), 0, L.st, L.rew(t), L.rows,
                           reinterpret_cast<unsigned long long *>(stats + 2 * t));
        return L.launched("k_reward_count");
    }
    int finish() const
    {
        if (!stats) return SWARM_OK;
        hipLaunchKernelGGL(k_reward_stats, dim3((steps + kThreads - 1) / kThreads), dim3(kThreads), 0, L.st, stats, steps, L.rows);
        return L.launched("k_reward_stats");
    }
};

// `steps` times: the entry point's own work for step t (`act_and_step(t)`: whatever precedes the action, the action into
// L.act(t), and L.step), then the reward count.  Enqueues only; stops at the first error.
template <class F>
int run_loop(const Loop &L, int steps, double *reward_stats, F &&act_and_step)
{
    const RewardStats rs{L, reward_stats, steps};
    int rc = rs.begin();
    for (int t = 0; rc == SWARM_OK && t < steps; ++t) {
        rc = act_and_step(t);
        if (rc == SWARM_OK) rc = rs.count(t);
    }
    return rc == SWARM_OK ? rs.finish() : rc;
}

// swarm_rollout (want_logpi = false, log_pi = NULL) and swarm_rollout_logpi (log_pi [n_slots][rows], written per step like act).
int rollout_impl(const char *who, bool want_logpi, swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring, float *log_pi,
                 int32_t steps, const uint8_t *uniform_steps, float noise_scale, uint64_t seed, uint64_t step0, uint64_t row_offset,
                 double *reward_stats, void *stream)
{
    // ---- validation: nothing is enqueued before all of it passed
    if (!env || !pol || !ring) return fail(SWARM_ERR_INVALID, "null env, policy or ring", who);
    if (want_logpi && !log_pi) return fail(SWARM_ERR_INVALID, "null log_pi (a [n_slots][rows] fp32 device array is required)", who);
    swarm_env_info ei;
    swarm_policy_info pi;
    if (int rc = check_handles(who, env, steps, ei, pol, &pi)) return rc;
    if (ei.obs_dtype != SWARM_F32 && ei.obs_dtype != SWARM_BF16)
        return fail(SWARM_ERR_INVALID, "the env handle's obs dtype must be SWARM_F32 or SWARM_BF16 (the policy reads no fp64 rows)", who);
    if (int rc = check_policy_ring(who, ei, pi, ring)) return rc;
    if (int rc = check_observed(who, ei)) return rc;
    if (steps == 0) return SWARM_OK;

    // ---- enqueue
    const Loop L(who, env, ei, ring, stream);
    if (L.rc != SWARM_OK) return L.rc;
    return run_loop(L, steps, reward_stats, [&](int t) {
        float *const act = L.act(t);
        float *const lp = log_pi ? log_pi + (size_t)L.c(t) * L.rows : nullptr;
        if (uniform_steps && uniform_steps[t]) {
            const unsigned long long ukey = pmix64(swarm_noise_key(seed, step0 + t) ^ kUniformSalt);
            if (lp)
                hipLaunchKernelGGL(k_uniform_actions<true>, dim3(L.row_grid()), dim3(kThreads), 0, L.st, reinterpret_cast<float2 *>(act),
                                   L.rows, ukey, (unsigned long long)row_offset, lp);
            else
                hipLaunchKernelGGL(k_uniform_actions<false>, dim3(L.row_grid()), dim3(kThreads), 0, L.st, reinterpret_cast<float2 *>(act),
                                   L.rows, ukey, (unsigned long long)row_offset, nullptr);
            if (int rc = L.launched("k_uniform_actions")) return rc;
        } else if ((lp ? swarm_policy_forward_explore_logpi(pol, L.obs(L.c(t)), L.bf16, L.rows, act, lp, noise_scale, seed, step0 + t,
                                                            row_offset, stream)
                       : swarm_policy_forward_explore_at(pol, L.obs(L.c(t)), L.bf16, L.rows, act, noise_scale, seed, step0 + t,
                                                         row_offset, stream)) != SWARM_POLICY_OK) {
            return fail(SWARM_ERR_HIP, swarm_policy_last_error(), who);
        }
        return L.step(act, SWARM_F32, t);
    });
}

// The pointer checks of a swarm_explore_t shared by swarm_rollout_explore and swarm_explore_envs; "" = fine.
const char *check_explore(const swarm_explore_t *ex, const float *log_pi)
{
    if (!ex || !ex->sigma) return "null ex or ex->sigma (a [E] fp32 device array of noise scales is required)";
    if (log_pi && !ex->log_c) return "log_pi is given: ex->log_c (the [E] log-pi constants) is required";
    return "";
}

// One step's k_explore_envs on `st`: rows = E * n_agents rows of act (log_pi, coin [E]: NULL = off), row_offset % n_agents == 0.
hipError_t launch_explore(float *act, float *log_pi, uint8_t *coin, long long rows, int n_agents, const swarm_explore_t *ex,
                          uint64_t seed, uint64_t step, uint64_t row_offset, hipStream_t st)
{
    if (rows == 0) return hipSuccess;
    ExploreParams P;
    P.epsilon = ex->epsilon; P.sigma = ex->sigma; P.log_c = ex->log_c;
    P.key = swarm_noise_key(seed, step);
    P.ckey = pmix64(P.key ^ kCoinSalt);
    P.ukey = pmix64(P.key ^ kUniformSalt);
    P.row_offset = row_offset; P.env_offset = row_offset / (unsigned long long)n_agents;
    P.rows = rows; P.n_agents = n_agents;
    const dim3 grid((unsigned)((rows + kThreads - 1) / kThreads));
    if (log_pi)
        hipLaunchKernelGGL(k_explore_envs<true>, grid, dim3(kThreads), 0, st, reinterpret_cast<float2 *>(act), log_pi, coin, P);
    else
        hipLaunchKernelGGL(k_explore_envs<false>, grid, dim3(kThreads), 0, st, reinterpret_cast<float2 *>(act), nullptr, coin, P);
    return hipGetLastError();
}

}  // namespace

extern "C" {

const char *swarm_rollout_last_error(void) { return g_rollout_error.c_str(); }

int swarm_rollout_explore(swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring, float *log_pi, int32_t steps,
                          const swarm_explore_t *ex, uint64_t seed, uint64_t step0, uint64_t row_offset, double *reward_stats,
                          void *stream)
{
    static const char *const who = "swarm_rollout_explore";
    // ---- validation: nothing is enqueued before all of it passed
    if (!env || !pol || !ring) return fail(SWARM_ERR_INVALID, "null env, policy or ring", who);
    if (const char *m = check_explore(ex, log_pi); *m) return fail(SWARM_ERR_INVALID, m, who);
    swarm_env_info ei;
    swarm_policy_info pi;
    if (int rc = check_handles(who, env, steps, ei, pol, &pi)) return rc;
    if (ei.obs_dtype != SWARM_F32 && ei.obs_dtype != SWARM_BF16)
        return fail(SWARM_ERR_INVALID, "the env handle's obs dtype must be SWARM_F32 or SWARM_BF16 (the policy reads no fp64 rows)", who);
    if (int rc = check_policy_ring(who, ei, pi, ring)) return rc;
    if (row_offset % (uint64_t)ei.n_agents != 0) {
        char msg[256];
        std::snprintf(msg, sizeof msg, "row_offset %llu is no multiple of n_agents %d (a coin belongs to a whole env)",
                      (unsigned long long)row_offset, ei.n_agents);
        return fail(SWARM_ERR_INVALID, msg, who);
    }
    if (int rc = check_observed(who, ei)) return rc;
    if (steps == 0) return SWARM_OK;

    // ---- enqueue
    const Loop L(who, env, ei, ring, stream);
    if (L.rc != SWARM_OK) return L.rc;
    return run_loop(L, steps, reward_stats, [&](int t) {
        float *const act = L.act(t);
        float *const lp = log_pi ? log_pi + (size_t)L.c(t) * L.rows : nullptr;
        if (swarm_policy_forward_explore_at(pol, L.obs(L.c(t)), L.bf16, L.rows, act, 0.0f, seed, step0 + t, row_offset, stream) != SWARM_POLICY_OK)
            return fail(SWARM_ERR_HIP, swarm_policy_last_error(), who);
        uint8_t *const coin = ex->coin ? ex->coin + (size_t)t * ei.n_env : nullptr;
        if (int rc = L.check(launch_explore(act, lp, coin, L.rows, ei.n_agents, ex, seed, step0 + t, row_offset, L.st), "k_explore_envs")) return rc;
        return L.step(act, SWARM_F32, t);
    });
}

int swarm_explore_envs(float *act, float *log_pi, int64_t rows, int32_t n_agents, const swarm_explore_t *ex, uint8_t *coin,
                       uint64_t seed, uint64_t step, uint64_t row_offset, void *stream)
{
    static const char *const who = "swarm_explore_envs";
    if (!act) return fail(SWARM_ERR_INVALID, "null act", who);
    if (const char *m = check_explore(ex, log_pi); *m) return fail(SWARM_ERR_INVALID, m, who);
    if (rows < 0 || n_agents < 1 || rows % n_agents != 0) {
        char msg[256];
        std::snprintf(msg, sizeof msg, "rows %lld must be >= 0 and a multiple of n_agents %d >= 1", (long long)rows, n_agents);
        return fail(SWARM_ERR_INVALID, msg, who);
    }
    if (row_offset % (uint64_t)n_agents != 0) {
        char msg[256];
        std::snprintf(msg, sizeof msg, "row_offset %llu is no multiple of n_agents %d (a coin belongs to a whole env)",
                      (unsigned long long)row_offset, n_agents);
        return fail(SWARM_ERR_INVALID, msg, who);
    }
    return hip_check(who, launch_explore(act, log_pi, coin, rows, n_agents, ex, seed, step, row_offset, static_cast<hipStream_t>(stream)),
                     "k_explore_envs");
}

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
    if (int rc = check_handles(who, env, steps, ei)) return rc;
    {
        std::string m = check_ring_shape(ei, ring);
        if (m.empty()) m = check_ring_slots(ei, ring);
        if (!m.empty()) return fail(SWARM_ERR_INVALID, m, who);
    }
    // (a large_swarm handle above 256 agents is served for both sources: k_rule_large, and act_next of the large-swarm kernels)
    if (source == SWARM_EXPERT_RULE && ei.large_swarm && ei.n_agents <= 256)
        return fail(SWARM_ERR_INVALID, "the rule expert is not available on a large_swarm handle (it serves n_agents <= 256 with large_swarm = 0)", who);
    if (source == SWARM_EXPERT_RULE && ei.g_max > 128)
        return fail(SWARM_ERR_INVALID, "the rule expert needs num_obs_grid_max <= 128 (as swarm_rule_action)", who);
    if (source == SWARM_EXPERT_LLM && !ei.llm_action)
        return fail(SWARM_ERR_INVALID, "the llm source needs a handle created with llm_action", who);
    if (int rc = check_observed(who, ei)) return rc;
    if (steps == 0) return SWARM_OK;

    // ---- enqueue
    const Loop L(who, env, ei, ring, stream);
    if (L.rc != SWARM_OK) return L.rc;
    return run_loop(L, steps, reward_stats, [&](int t) {
        swarm_expert_view v;                                             // RULE: after the index-export pass it enqueues
        const int rc = swarm_internal_expert_view(env, source == SWARM_EXPERT_RULE, &v);
        if (rc != SWARM_OK) return fail(rc, swarm_last_error(env), who);
        if (source == SWARM_EXPERT_RULE) {
            if (int e = L.check(swarm_internal_launch_rule(v, reinterpret_cast<double *>(v.act64), L.act(t), L.st, ei.rule_tiled), "k_rule")) return e;
            return L.step(v.act64, SWARM_F64, t);
        }
        hipLaunchKernelGGL(k_act_f32, dim3(L.row_grid()), dim3(kThreads), 0, L.st, v.act_next, reinterpret_cast<float2 *>(L.act(t)), L.rows);
        if (int e = L.launched("k_act_f32")) return e;
        return L.step(nullptr, SWARM_F64, t);                            // NULL = the handle's own 'llm' action
    });
}

int swarm_rollout_eval(swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring, int32_t steps, const int32_t *switch_to,
                       const swarm_eval_out_t *out, void *stream)
{
    static const char *const who = "swarm_rollout_eval";
    // ---- validation: nothing is enqueued before all of it passed
    if (!env || !pol || !ring) return fail(SWARM_ERR_INVALID, "null env, policy or ring", who);
    swarm_env_info ei;
    swarm_policy_info pi;
    if (int rc = check_handles(who, env, steps, ei, pol, &pi)) return rc;
    if (int rc = check_policy_ring(who, ei, pi, ring)) return rc;
    const swarm_eval_out_t none = {nullptr, nullptr, nullptr, nullptr};
    const swarm_eval_out_t &o = out ? *out : none;
    if ((o.p == nullptr) != (o.dp == nullptr)) return fail(SWARM_ERR_INVALID, "the state trace needs p and dp together", who);
    bool switches = false;
    if (switch_to) {
        for (int t = 0; t < steps; ++t) {
            if (switch_to[t] < -1 || (switch_to[t] >= 0 && ei.n_shapes >= 1 && switch_to[t] >= ei.n_shapes)) {
                char msg[256];
                std::snprintf(msg, sizeof msg, "switch_to[%d] = %d outside [-1, n_shapes = %d)", t, (int)switch_to[t], ei.n_shapes);
                return fail(SWARM_ERR_INVALID, msg, who);
            }
            switches = switches || switch_to[t] >= 0;
        }
    }
    if (switches && ei.n_shapes < 1) return fail(SWARM_ERR_STATE, "switch_to needs a shape set (swarm_set_shapes)", who);
    if (int rc = check_observed(who, ei)) return rc;
    if (steps == 0) return SWARM_OK;

    // ---- enqueue
    const Loop L(who, env, ei, ring, stream);
    if (L.rc != SWARM_OK) return L.rc;
    swarm_expert_view v;                                                 // the handle's p / dp (no lists: nothing is enqueued)
    if (swarm_internal_expert_view(env, false, &v) != SWARM_OK) return fail(SWARM_ERR_INVALID, "bad handle", who);
    const size_t state_elems = (size_t)L.rows * 2, state_bytes = state_elems * sizeof(double);
    return run_loop(L, steps, o.reward_stats, [&](int t) {
        if (o.p) {
            hipError_t e = hipMemcpyAsync(o.p + (size_t)t * state_elems, v.p, state_bytes, hipMemcpyDeviceToDevice, L.st);
            if (e == hipSuccess) e = hipMemcpyAsync(o.dp + (size_t)t * state_elems, v.dp, state_bytes, hipMemcpyDeviceToDevice, L.st);
            if (int rc = L.check(e, "state trace copy")) return rc;
        }
        if (switch_to && switch_to[t] >= 0) {
            const int rc = swarm_select_shape(env, switch_to[t], nullptr);
            if (rc != SWARM_OK) return fail(rc, swarm_last_error(env), who);
        }
        if (o.metrics) {
            const int rc = swarm_internal_metrics_step(env, o.metrics + (size_t)t * ei.n_env * 3);
            if (rc != SWARM_OK) return fail(rc, swarm_last_error(env), who);
        }
        if (swarm_policy_forward_explore_at(pol, L.obs(L.c(t)), L.bf16, L.rows, L.act(t), 0.0f, 0, (uint64_t)t, 0, stream) != SWARM_POLICY_OK)
            return fail(SWARM_ERR_HIP, swarm_policy_last_error(), who);
        return L.step(L.act(t), SWARM_F32, t);
    });
}

}  // extern "C"
