// Interface between policy_mlp.hip (the fused actor's C ABI, its handle and its narrow kernel) and policy_wide.hip (the wide
// geometry: in_dim <= 384, hidden <= 256).  The swarm_policy handle of policy_mlp.hip owns the packed weights of either
// geometry; a wide handle holds a Layout beside them and hands both to the functions below.  Not installed, not exported.
#ifndef SWARM_POLICY_WIDE_H
#define SWARM_POLICY_WIDE_H

#include <type_traits>
#include <vector>

#include "swarm_internal.h"

namespace swarm_wide __attribute__((visibility("hidden"))) {

constexpr int kMaxIn = 384, kMaxHidden = 256, kMaxAct = 4;

// The packed stream of one actor's shape (policy_wide.hip: Geo<MT> at run time).  One member's blob is the high stream and
// the low stream behind it, n_chunks * ch 16-byte pieces each.
struct Layout {
    int mt, kc, w, tail, ch, wout;
    int n1, n_chunks;               // layer-1 chunks, chunks of the whole stream
    int in_dim, hidden, act_dim;
};

// What a routed forward kernel (k_policy_mlp_route, k_policy_wide_route) reads of a route (swarm_policy_bank_route): the tile
// table for its rows per workgroup and env_order, both written by the routing kernel of policy_mlp.hip.
struct RouteView {
    const int4 *tiles;              // [grid]: (member, first slot, slot count, 0); surplus entries carry count 0
    const int32_t *env_order;       // the served envs, by member and ascending env inside a member
    int rows_per_env;
};
constexpr int kRouteRows = 128;     // the wide geometry's rows per workgroup (policy_wide.hip checks it)

struct ForwardArgs {
    const void *obs;
    bool in_bf16;
    long long rows;                 // > 0
    float *act, *log_pi;            // log_pi != NULL: the LOGPI instantiation
    float noise_scale, logpi_c;     // as policy_forward computes them for both geometries: the clamped scale; log-pi's constant,
                                    // 0.0f where log_pi is NULL
    unsigned long long noise_key, row_offset;
    int precision;                  // SWARM_POLICY_BF16 / SWARM_POLICY_BF16X3
    hipStream_t stream;
    bool set_smem;                  // the handle's first forward: raise the kernels' dynamic LDS limit first
    bool bank;                      // a bank handle: the BANK kernels, member m on rows [m rows / members, (m + 1) rows / members)
    int members;
    const RouteView *route;         // != NULL: a route is in force -- the ROUTE kernels on route_grid workgroups
    unsigned route_grid;
};

// true where the wide kernel serves the shape; decided without a device
bool shape_ok(int in_dim, int hidden, int act_dim);
Layout layout_of(int in_dim, int hidden, int act_dim);      // of a shape that passed shape_ok
// one member's blob from w: fc1.weight, fc1.bias, ..., fc4.bias (fp32, HOST)
std::vector<unsigned char> pack_host(const Layout &g, const float *const w[8]);
// w: the same eight arrays on the DEVICE; one packing launch on `st` into the member's blob at `dst`
void load_device(const Layout &g, void *dst, const float *const w[8], hipStream_t st);
// one launch on a.stream; `blob`: the first member's.  The caller holds the device current and asks hipGetLastError.
void forward(const Layout &g, const void *blob, const ForwardArgs &a);

// hipFuncAttributeMaxDynamicSharedMemorySize = bytes on every kernel of a table (an array, of any rank, of kernel pointers)
template <class T>
void raise_smem(const T &t, int bytes)
{
    if constexpr (std::is_array<T>::value) { for (const auto &e : t) raise_smem(e, bytes); }
    else (void)hipFuncSetAttribute(reinterpret_cast<const void *>(t), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace swarm_wide

#endif
