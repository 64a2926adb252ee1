// Internal interface between the translation units of libswarmenv.so: what the device rollout loop (rollout.hip) needs to
// know about the two opaque handles, the rule-expert kernel's launcher (rule_expert.hip; called by env_api.hip and
// rollout.hip), the counter-based hash every in-kernel generator is built from, and the two resource owners of the host code:
// DeviceGuard (the current device) and DevBuf (one device or pinned allocation).  Not installed, not exported: the accessors
// and the owners have hidden visibility, so the public ABI (swarm_env.h, swarm_policy.h, swarm_rollout.h) does not change.
#ifndef SWARM_INTERNAL_H
#define SWARM_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
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

// np.sum of f(0..n-1) for n <= 128, values generated on the fly: numpy's pairwise summation, which below its 128-element
// block size is eight interleaved partial sums combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail
template <class F>
__device__ inline double np_sum_stream(int n, F f)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += f(i);
        return res;
    }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = f(k);
    const int n8 = n - (n % 8);
    int i;
    for (i = 8; i < n8; i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += f(i + k);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += f(i);
    return res;
}

// smallest double x with sqrt(x) >= t (IEEE sqrt is correctly rounded and monotonic), so that
// sqrt(d2) < t  <=>  d2 < x  for every d2 >= 0 (and for a NaN d2: both false).  Host code: the kernels get the cut.
inline double cut_lt(double t)
{
    if (!(t > 0)) return 0.0;
    double x = t * t;
    while (x > 0 && std::sqrt(x) >= t) x = std::nextafter(x, 0.0);
    while (std::sqrt(x) < t) x = std::nextafter(x, INFINITY);
    return x;
}

// np.clip(v, -1, 1): NaN compares false both ways and passes through (fmin / fmax would return the bound); every other
// value, -0.0 included, is what fmin(fmax(v, -1.0), 1.0) gives.
__device__ inline double np_clip1(double v) { return v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v); }

}  // namespace swarm_internal

namespace swarm_internal __attribute__((visibility("hidden"))) {

// Makes `dev` the calling thread's device and restores the previous one on exit; ok: `dev` is current.
struct DeviceGuard {
    int prev;
    bool ok;
    explicit DeviceGuard(int dev) : prev(-1), ok(false)
    {
        if (hipGetDevice(&prev) != hipSuccess) return;
        ok = (prev == dev) || hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Owner of one hipMalloc (PINNED: hipHostMalloc) allocation of T elements.  Empty until alloc() succeeds and again after a
// failed alloc() or a move out of it; the allocation is freed by the destructor, by the next alloc() (before the new one is
// made) and by a move-assignment into the buffer.  Frees go to the device that is current: owners destroy their buffers
// under a DeviceGuard.
template <class T, bool PINNED = false>
class DevBuf {
    T *p_ = nullptr;
    void release() { if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; }

public:
    static constexpr const char *kCall = PINNED ? "hipHostMalloc" : "hipMalloc";
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count)
    {
        release();
        const hipError_t e = PINNED ? hipHostMalloc((void **)&p_, count * sizeof(T), hipHostMallocDefault)
                                    : hipMalloc((void **)&p_, count * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
};

// The one switch over an obs dtype code (swarm_config_t.obs_dtype): f(TypeTag<T>{}) with T the type of an observation
// element -- double, __bf16 or float.  f returns the same type for all three.
template <class T> struct TypeTag { typedef T type; };
template <class F>
inline auto with_obs_type(int dtype, F &&f)
{
    return dtype == SWARM_F64 ? f(TypeTag<double>{}) : dtype == SWARM_BF16 ? f(TypeTag<__bf16>{}) : f(TypeTag<float>{});
}
inline size_t obs_elem_bytes(int dtype) { return with_obs_type(dtype, [](auto t) { return sizeof(typename decltype(t)::type); }); }

}  // namespace swarm_internal

struct swarm_env_info {
    int device, n_env, n_agents, obs_dim, obs_dtype, g_max, n_shapes;
    bool with_prior, observed, llm_action;
    bool large_swarm;             // created with swarm_config_t.large_swarm: stepped by env_large.hip; the expert (rule and 'llm')
                                  // serves such a handle above 256 agents only -- at 256 or fewer the default handle does
    bool rule_tiled;              // the rule expert runs k_rule_large, not k_rule: n_agents > 256, or debug_flags bit 5 on a default handle
};
SWARM_HIDDEN int swarm_internal_env_info(const swarm_env_t *h, swarm_env_info *out);

// What the rule-expert kernel and the expert sources of swarm_rollout_expert read for the CURRENT state: the fp64 state, the
// target cells, the lists the index-export observation pass leaves in HBM (nearest cell, in-shape flag, capped sensed-cell
// list), the 'llm' strategy's next action and the handle's fp64 action scratch.  All device pointers of the handle's device.
struct swarm_expert_view {
    const double *p, *dp;               // [E][2][N]
    const double *cells;                // [E][2][ng_max]
    const int *near_cell, *in_flag;     // [E][N]
    const int *exp_sensed;              // [E][N][g_max], -1 padded
    const double2 *act_next;            // [E][N]: the 'llm' action (NULL unless the handle was created with llm_action)
    double2 *act64;                     // [E][N]: fp64 action scratch (allocated by the first call with lists)
    double d_sen, r_avoid;
    int n_env, n_agents, g_max, ng_max;
};
// lists = true: allocate the list / action scratch on first use (never again) and ENQUEUE the index-export observation
// pass of swarm_rule_action on the handle's stream (no host synchronisation); false: only fill `out`.  SWARM_OK or an error
// code with the message in swarm_last_error(h).
SWARM_HIDDEN int swarm_internal_expert_view(swarm_env_t *h, bool lists, swarm_expert_view *out);

// Enqueue the rule-expert kernel (rule_expert.hip) on `st` for the lists in `v`: the fp64 action into act64 [E][N][2] (8-byte
// aligned; 16-byte aligned when act32 is given, as v.act64 is) and, act32 != NULL, its f32 rounding into act32 [E][N][2].
// The kernel is k_rule (one workgroup per env, n_agents <= 256) unless n_agents > 256 or `tiled` (swarm_env_info.rule_tiled):
// then k_rule_large, one wave per (env, 64 agents), the same arithmetic.  Returns the launch's hipGetLastError().
SWARM_HIDDEN hipError_t swarm_internal_launch_rule(const swarm_expert_view &v, double *act64, float *act32, hipStream_t st, bool tiled);

// The evaluation loop's per-step metrics launch: out[E][3] (DEVICE), bit for bit what swarm_metrics writes (k_metrics_step in
// env_kernels.hip).  Enqueued on the handle's stream; no host synchronisation.
SWARM_HIDDEN int swarm_internal_metrics_step(swarm_env_t *h, double *out);

struct swarm_policy_info {
    int device, in_dim, act_dim;
    int members;                        // 1, or the members of a bank (swarm_policy_bank_create)
    int route_n_env, route_rows_per_env;    // the route in force (swarm_policy_bank_route); 0, 0: none
};
SWARM_HIDDEN int swarm_internal_policy_info(const swarm_policy_t *p, swarm_policy_info *out);

#endif
