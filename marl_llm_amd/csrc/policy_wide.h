// Interface between policy_mlp.hip (the fused actor's C ABI and its narrow kernel) and policy_wide.hip (the wide geometry:
// in_dim <= 384, hidden <= 256).  A swarm_policy handle made by swarm_policy_create_wide owns one swarm_wide::Handle and every
// entry point of include/swarm_policy.h dispatches on it.  Not installed, not exported.
#ifndef SWARM_POLICY_WIDE_H
#define SWARM_POLICY_WIDE_H

#include <string>

#include "swarm_internal.h"

namespace swarm_wide __attribute__((visibility("hidden"))) {

constexpr int kMaxIn = 384, kMaxHidden = 256, kMaxAct = 4;

struct Handle;                      // policy_wide.hip: the packed weights on the device and their geometry

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
    float noise_scale;
    uint64_t seed, step, row_offset;
    int precision;                  // SWARM_POLICY_BF16 / SWARM_POLICY_BF16X3
    hipStream_t stream;
    bool bank;                      // a bank handle: the BANK kernels, member m on rows [m rows / members, (m + 1) rows / members)
    const RouteView *route;         // != NULL: a route is in force -- the ROUTE kernels on route_grid workgroups
    unsigned route_grid;
};

// true where the wide kernel serves the shape; decided without a device
bool shape_ok(int in_dim, int hidden, int act_dim);
// w[8 m + i]: fc1.weight, fc1.bias, ..., fc4.bias of member m (fp32, HOST), a shape that passed shape_ok; members >= 1 blobs,
// one behind the other; the caller holds `device` current.  err: the reason, without the entry point's name
int create(const float *const *w, int members, int in_dim, int hidden, int act_dim, Handle **out, std::string &err);
void destroy(Handle *h);            // under the caller's DeviceGuard
int forward(Handle *h, const ForwardArgs &a, std::string &err);
// w: the eight arrays of one member on the DEVICE; one packing launch on `st` into that member's blob
int load_device(Handle *h, int member, const float *const w[8], hipStream_t st, std::string &err);
// the first member's blob and the bytes of ONE member's
const void *blob(const Handle *h, size_t *bytes);

}  // namespace swarm_wide

#endif
