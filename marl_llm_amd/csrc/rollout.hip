// Device rollout loop (include/swarm_rollout.h): `steps` exploring-actor + env steps enqueued by one library call, the
// transitions written straight into a chained replay ring.  The loop itself is host code that only enqueues: per step the
// policy kernel (policy_mlp.hip) or the uniform-action kernel below, the env step (swarm_env.hip) and, optionally, the
// reward-count kernel below, all on one stream; the reward statistics are finished by one launch after the loop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>

#include "swarm_internal.h"
#include "swarm_rollout.h"

namespace {

using swarm_internal::pmix64;
using swarm_internal::swarm_noise_key;

constexpr unsigned long long kUniformSalt = 0x5851F42D4C957F2Dull;    // separates the uniform stream from the policy's noise
constexpr int kThreads = 256;
constexpr int kCountPerThread = 16;                                      // rewards a thread counts (grid-stride) before the block sum
constexpr int kCountMaxBlocks = 1024;

thread_local std::string g_rollout_error;

int fail(int code, const std::string &msg)
{
    g_rollout_error = "swarm_rollout: " + msg;
    return code;
}

// The epsilon branch of agents.py:89-91 (np.random.uniform(-1, 1) per component), counter-based: formula in swarm_rollout.h.
__global__ void __launch_bounds__(kThreads) k_uniform_actions(float2 *__restrict__ act, long long rows, unsigned long long ukey,
                                                              unsigned long long row_offset)
{
    const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (row >= rows) return;
    const unsigned long long h = pmix64(ukey ^ (row_offset + (unsigned long long)row));
    float2 a;
    a.x = (float)(unsigned)((h >> 40) & 0xFFFFFFull) * 1.1920928955078125e-07f - 1.0f;      // 2^-23
    a.y = (float)(unsigned)((h >> 16) & 0xFFFFFFull) * 1.1920928955078125e-07f - 1.0f;
    act[row] = a;
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

extern "C" {

const char *swarm_rollout_last_error(void) { return g_rollout_error.c_str(); }

int swarm_rollout(swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring, int32_t steps, const uint8_t *uniform_steps,
                  float noise_scale, uint64_t seed, uint64_t step0, uint64_t row_offset, double *reward_stats, void *stream)
{
    // ---- validation: nothing is enqueued before all of it passed
    if (!env || !pol || !ring) return fail(SWARM_ERR_INVALID, "null env, policy or ring");
    swarm_env_info ei;
    swarm_policy_info pi;
    if (swarm_internal_env_info(env, &ei) != SWARM_OK || swarm_internal_policy_info(pol, &pi) != SWARM_POLICY_OK)
        return fail(SWARM_ERR_INVALID, "bad handle");
    char msg[256];
    if (steps < 0) return fail(SWARM_ERR_INVALID, "steps < 0");
    if (ei.device != pi.device) {
        std::snprintf(msg, sizeof msg, "env handle on device %d, policy on device %d", ei.device, pi.device);
        return fail(SWARM_ERR_INVALID, msg);
    }
    if (ei.obs_dtype != SWARM_F32 && ei.obs_dtype != SWARM_BF16)
        return fail(SWARM_ERR_INVALID, "the env handle's obs dtype must be SWARM_F32 or SWARM_BF16 (the policy reads no fp64 rows)");
    if (ring->obs_dtype != ei.obs_dtype) return fail(SWARM_ERR_INVALID, "ring obs_dtype differs from the env handle's obs dtype");
    const long long rows = (long long)ei.n_env * ei.n_agents;
    if (ring->rows != rows) {
        std::snprintf(msg, sizeof msg, "ring rows %lld != n_env * n_agents = %lld", (long long)ring->rows, rows);
        return fail(SWARM_ERR_INVALID, msg);
    }
    if (ring->obs_dim != ei.obs_dim) {
        std::snprintf(msg, sizeof msg, "ring obs_dim %d != env obs_dim %d", ring->obs_dim, ei.obs_dim);
        return fail(SWARM_ERR_INVALID, msg);
    }
    if (pi.in_dim != ei.obs_dim) {
        std::snprintf(msg, sizeof msg, "policy in_dim %d != env obs_dim %d", pi.in_dim, ei.obs_dim);
        return fail(SWARM_ERR_INVALID, msg);
    }
    if (pi.act_dim != 2) return fail(SWARM_ERR_INVALID, "policy act_dim must be 2 (the env's action)");
    if (ei.obs_dtype == SWARM_BF16 && (pi.in_dim & 7)) return fail(SWARM_ERR_INVALID, "bf16 observation rows need obs_dim % 8 == 0");
    if (!ring->obs || !ring->act || !ring->rew || !ring->done) return fail(SWARM_ERR_INVALID, "null ring obs / act / rew / done");
    if (ei.with_prior && !ring->prior) return fail(SWARM_ERR_INVALID, "the env handle computes a prior (with_prior): ring prior is NULL");
    if (!ei.with_prior && ring->prior) return fail(SWARM_ERR_INVALID, "the env handle has no prior: ring prior must be NULL");
    if (ring->n_slots < 2) return fail(SWARM_ERR_INVALID, "ring n_slots must be >= 2");
    if (ring->cur < 0 || ring->cur >= ring->n_slots) return fail(SWARM_ERR_INVALID, "ring cur outside [0, n_slots)");
    if (!ei.observed) return fail(SWARM_ERR_STATE, "the env handle is not observed (swarm_observe / swarm_reset first)");
    if (steps == 0) return SWARM_OK;

    // ---- enqueue
    DeviceScope dev(ei.device);
    if (!dev.ok) return fail(SWARM_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (swarm_set_stream(env, stream) != SWARM_OK) return fail(SWARM_ERR_INVALID, "swarm_set_stream failed");
    const bool bf16 = ei.obs_dtype == SWARM_BF16;
    const size_t obs_slot = (size_t)rows * ei.obs_dim * (bf16 ? 2 : 4), pri_slot = (size_t)rows * 2 * (bf16 ? 2 : 4);
    char *const obs = static_cast<char *>(ring->obs), *const pri = static_cast<char *>(ring->prior);
    if (reward_stats) {
        const hipError_t e = hipMemsetAsync(reward_stats, 0, (size_t)steps * 2 * sizeof(double), st);
        if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
    }
    const unsigned act_grid = (unsigned)((rows + kThreads - 1) / kThreads);
    const unsigned cnt_grid = (unsigned)std::min<long long>((rows + kThreads * kCountPerThread - 1) / (kThreads * kCountPerThread),
                                                            kCountMaxBlocks);
    for (int t = 0; t < steps; ++t) {
        const int c = (int)(((long long)ring->cur + t) % ring->n_slots), n = (c + 1) % ring->n_slots;
        float *const act = ring->act + (size_t)c * rows * 2;
        if (uniform_steps && uniform_steps[t]) {
            const unsigned long long ukey = pmix64(swarm_noise_key(seed, step0 + t) ^ kUniformSalt);
            hipLaunchKernelGGL(k_uniform_actions, dim3(act_grid), dim3(kThreads), 0, st, reinterpret_cast<float2 *>(act), rows, ukey,
                               (unsigned long long)row_offset);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("k_uniform_actions: ") + hipGetErrorString(e));
        } else if (swarm_policy_forward_explore_at(pol, obs + c * obs_slot, bf16, rows, act, noise_scale, seed, step0 + t, row_offset,
                                                   stream) != SWARM_POLICY_OK) {
            return fail(SWARM_ERR_HIP, swarm_policy_last_error());
        }
        const int rc = swarm_step(env, act, SWARM_F32, obs + n * obs_slot, ring->rew + (size_t)c * rows, ring->done + (size_t)c * rows,
                                  pri ? pri + c * pri_slot : nullptr);
        if (rc != SWARM_OK) return fail(rc, swarm_last_error(env));
        if (reward_stats) {
            hipLaunchKernelGGL(k_reward_count, dim3(cnt_grid), dim3(kThreads), 0, st, ring->rew + (size_t)c * rows, rows,
                               reinterpret_cast<unsigned long long *>(reward_stats + 2 * t));
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("k_reward_count: ") + hipGetErrorString(e));
        }
    }
    if (reward_stats) {
        hipLaunchKernelGGL(k_reward_stats, dim3((steps + kThreads - 1) / kThreads), dim3(kThreads), 0, st, reward_stats, (int)steps, rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(SWARM_ERR_HIP, std::string("k_reward_stats: ") + hipGetErrorString(e));
    }
    return SWARM_OK;
}

}  // extern "C"
