// Internal interface between the translation units of libswarmenv.so: what the device rollout loop (rollout.hip) needs to
// know about the two opaque handles, and the counter-based hash every in-kernel generator is built from.  Not installed,
// not exported: the accessors have hidden visibility, so the public ABI (swarm_env.h, swarm_policy.h, swarm_rollout.h)
// does not change.
#ifndef SWARM_INTERNAL_H
#define SWARM_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "swarm_env.h"
#include "swarm_policy.h"

#define SWARM_HIDDEN __attribute__((visibility("hidden")))

namespace swarm_internal {

// splitmix64's finaliser
static __host__ __device__ inline unsigned long long pmix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// key of the exploration generators for one (seed, step); a row's hash is pmix64(key ^ global row index)
static inline unsigned long long swarm_noise_key(uint64_t seed, uint64_t step)
{
    return pmix64(pmix64(seed + 0x9E3779B97F4A7C15ull) ^ (0xD1B54A32D192ED03ull * (step + 1)));
}

}  // namespace swarm_internal

struct swarm_env_info {
    int device, n_env, n_agents, obs_dim, obs_dtype;
    bool with_prior, observed;
};
SWARM_HIDDEN int swarm_internal_env_info(const swarm_env_t *h, swarm_env_info *out);

struct swarm_policy_info {
    int device, in_dim, act_dim;
};
SWARM_HIDDEN int swarm_internal_policy_info(const swarm_policy_t *p, swarm_policy_info *out);

#endif
