/* swarm_policy.h -- C ABI of the fused policy MLP used by the device-resident rollout.
 *
 * Replaces, for inference during rollouts, the reference's actor forward
 *   /root/reference/marl_llm/algorithm/utils/networks.py:6-44   (MLPNetwork: fc1..fc4, leaky_relu x3, tanh)
 * called from /root/reference/marl_llm/algorithm/utils/agents.py:69-96 (DDPGAgent.step) on torch.Tensor(obs).
 * One HIP kernel (bf16 MFMA, fp32 accumulate) maps the env's observation rows [rows][in_dim] (fp32, device) to actions
 * [rows][act_dim] (fp32, device); weights are given once, in torch.nn.Linear layout ([out][in] row-major, fp32, host).
 * The arithmetic is stated exactly under swarm_policy_set_precision below.  No CPU path: without a HIP device create fails.
 */
#ifndef SWARM_POLICY_H
#define SWARM_POLICY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWARM_POLICY_OK 0
#define SWARM_POLICY_ERR_INVALID 1
#define SWARM_POLICY_ERR_HIP 2

typedef struct swarm_policy swarm_policy_t;

/* w1 [hidden][in_dim], w2 / w3 [hidden][hidden], w4 [act_dim][hidden], b* the biases; all fp32 HOST pointers.
 * Supported: 4 <= in_dim <= 192 (multiple of 4), 1 <= hidden <= 191, 1 <= act_dim <= 4 (the padded hidden feature 191 at the
 * most carries the constant one of the bias column).  Shapes and pointers are checked before any device call: a rejected
 * create returns SWARM_POLICY_ERR_INVALID with a message.  device < 0: the current device. */
int  swarm_policy_create(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                         const float *w4, const float *b4, int in_dim, int hidden, int act_dim, int device, swarm_policy_t **out);
/* The same arguments, a handle that runs the WIDE geometry of the kernel (csrc/policy_wide.hip), always -- also for shapes
 * swarm_policy_create serves.  Supported: 4 <= in_dim <= 384 (multiple of 4), 1 <= hidden <= 256, 1 <= act_dim <= 4: the env's
 * rows up to num_obs_grid_max = 176 at the default topology, the reference's --hidden_dim up to 256.  Checked before any device
 * call: a rejection returns SWARM_POLICY_ERR_INVALID with a message that starts "swarm_policy_create_wide:" and names the three
 * limits.  Every call below takes such a handle; SWARM_POLICY_TPW is not read for it.  The arithmetic is the one stated under
 * swarm_policy_set_precision; only the mechanism of the biases of layers 2-4 differs (no constant-one column: hidden = 256
 * leaves no padded feature for it): the accumulators start at bf(bl), and in bf16x3 mode lo(bl) = bf(bl - bf(bl)) is added to
 * them in fp32 -- the same terms, in an order that is not part of the contract.  Its packed weights
 * (swarm_policy_read_packed) have their own layout and size. */
int  swarm_policy_create_wide(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                              const float *w4, const float *b4, int in_dim, int hidden, int act_dim, int device, swarm_policy_t **out);
void swarm_policy_destroy(swarm_policy_t *p);

/* act[rows][act_dim] = tanh(fc4(lrelu(fc3(lrelu(fc2(lrelu(fc1(obs[rows][in_dim])))))))); obs / act are DEVICE pointers, rows
 * densely packed; stream is a hipStream_t (NULL: the default stream).  Asynchronous. */
int  swarm_policy_forward(swarm_policy_t *p, const float *obs, int64_t rows, float *act, void *stream);

/* The same with bfloat16 observation rows (the env's SWARM_BF16 output, swarm_env.h): each 16-byte load is one MFMA
 * operand fragment, no conversion.  in_dim must be a multiple of 8 (16-byte aligned rows).  Identical results to
 * swarm_policy_forward on the same values held in float32. */
int  swarm_policy_forward_bf16(swarm_policy_t *p, const void *obs_bf16, int64_t rows, float *act, void *stream);

/* The rollout's exploring actor in one launch (agents.py:82-96, continuous branch): act = clamp(actor(obs) + noise_scale *
 * N(0, 1), -1, 1).  The normals come from a counter-based generator keyed by (seed, step, row_offset + row, component),
 * evaluated in the kernel's epilogue, nothing to store; noise_scale <= 0: plain forward.  row_offset is the global index of
 * the call's first row: a rank that passes the start of its shard draws exactly the noise the same rows get in one call over
 * the whole batch, and ranks that share (seed, step) draw different noise.  `act` may point anywhere on the device (e.g.
 * straight into a replay-buffer slot).  obs_is_bf16 as the two calls above.
 *
 * Gaussian noise, counter-based, for global row g = row_offset + row (arithmetic mod 2^64, pmix64 as in swarm_rollout.h):
 *   key = pmix64(pmix64(seed + 0x9E3779B97F4A7C15) ^ (0xD1B54A32D192ED03 * (step + 1)))
 *   h   = pmix64(key ^ g)
 *   for the component pairs (0, 1) and (2, 3), as far as act_dim reaches:
 *     u1 = (float)((h >> 40) + 1) * 2^-24                 in (0, 1], exact in fp32
 *     u2 = (float)((h >> 16) & 0xFFFFFF) * 2^-24         in [0, 1), exact in fp32
 *     z[k] = sqrtf(-2 logf(u1)) * cosf(t),  z[k + 1] = sqrtf(-2 logf(u1)) * sinf(t),  t = 6.283185307179586f * u2 (fp32)
 *     h = pmix64(h + 0x9E3779B97F4A7C15)                  (before the next pair)
 *   act[g][k] = clamp(tanh(pre[k]) + noise_scale * z[k], -1, 1) in fp32.
 *
 * Log-probability of the noise (swarm_policy_forward_explore_logpi; GaussianNoise.log_prob of utils/noise.py on the noise
 * before the clamp, the log_pi of agents.py:93-95), in fp32 from the same z[k], with noise_scale the fp32 value passed:
 *   c  = (float)((double)act_dim * log((double)noise_scale * sqrt(2.0 * M_PI)))     once per call, on the host, in double
 *   s  = z[0]*z[0] + z[1]*z[1] + ... + z[act_dim-1]*z[act_dim-1]                   fp32, left to right, no fused multiply-add
 *   log_pi[g] = -(0.5f * s) - c                                                     fp32
 * noise_scale <= 0 (plain forward): log_pi[g] = -0.0f, the reference's -act_dim * log(1).  The actions are the same bits
 * whether log_pi is requested or not. */
int  swarm_policy_forward_explore_at(swarm_policy_t *p, const void *obs, int obs_is_bf16, int64_t rows, float *act,
                                     float noise_scale, uint64_t seed, uint64_t step, uint64_t row_offset, void *stream);
/* The same with row_offset = 0: the noise is keyed by the call-local row index. */
int  swarm_policy_forward_explore(swarm_policy_t *p, const void *obs, int obs_is_bf16, int64_t rows, float *act,
                                  float noise_scale, uint64_t seed, uint64_t step, void *stream);
/* swarm_policy_forward_explore_at that also writes log_pi[rows] (fp32, DEVICE, required: NULL is rejected with
 * SWARM_POLICY_ERR_INVALID), the log-probability of each row's exploration noise stated above. */
int  swarm_policy_forward_explore_logpi(swarm_policy_t *p, const void *obs, int obs_is_bf16, int64_t rows, float *act, float *log_pi,
                                        float noise_scale, uint64_t seed, uint64_t step, uint64_t row_offset, void *stream);

/* Arithmetic of the forward calls, exactly (tests/helpers.py policy_model restates it in float64).  bf(v): v rounded to
 * bfloat16, nearest-even.  Products of bf16 operands are exact in fp32; every sum is accumulated in fp32, in an order that
 * is not part of the contract.
 * SWARM_POLICY_BF16 (default):
 *   layer 1:      h = bf(W1) . bf(x) + b1            b1 stays fp32 (it initialises the accumulators)
 *   layers 2-4:   h = bf(Wl) . a + bf(bl)            the bias rides in the weights' constant-one column, as bf16
 *   activation:   a = bf(fmaxf(v, 0.01f * v))        v = the fp32 sum, the product rounded in fp32
 *   output:       tanhf of the fp32 sum of layer 4   (no bf16 rounding before the tanh)
 *   Close to torch.autocast(bfloat16), not equal to it: autocast also rounds b1 and the pre-tanh sum to bf16.  About 4e-2 from
 *   the reference's fp32 actor on actions in [-1, 1].
 * SWARM_POLICY_BF16X3: every operand v (weights on the host, layer inputs and activations in the kernel) is split into
 *   hi = bf(v) and lo = bf(v - hi) (v - hi is exact in fp32); a product is Whi.xhi + Whi.xlo + Wlo.xhi (lo.lo dropped), three
 *   MFMAs, fp32 sums.  Layer 1's bias is fp32, the biases of layers 2-4 are hi + lo; bf16 observation rows have lo = 0.
 *   Within ~1e-4 of the fp32 actor (networks.py:6-44), about 1.9x the time. */
#define SWARM_POLICY_BF16   0
#define SWARM_POLICY_BF16X3 1
int  swarm_policy_set_precision(swarm_policy_t *p, int precision);

/* New weights for an existing handle, from fp32 DEVICE arrays on the handle's device (torch.nn.Linear layout, the shapes the
 * handle was created with: the learner's parameters where torch keeps them).  One launch of a packing kernel on `stream`
 * (a hipStream_t; NULL: the default stream) rewrites the handle's packed weights in place: the high bf16 parts bf(v), the low
 * parts bf(v - bf(v)), the fp32 b1, the biases of layers 2-4 in the constant-one column, the constant-one feature itself and
 * the permuted k order of layers 2-4 -- everything swarm_policy_create packs on the host.
 *   Enqueue only: no host synchronisation, no allocation, no copy of the weights through the host.
 *   Stream order: a forward or rollout enqueued on the same stream before the call uses the old weights, one enqueued after
 *     it the new ones.  The eight arrays are read when the kernel RUNS, not when the call is made: they must stay valid and
 *     hold the intended values until then (writes enqueued on the same stream before the call are seen).  Work on other
 *     streams that uses the handle or writes the arrays is the caller's to order with events.
 *   Same bytes as the host packer: for finite weights whose bf16 rounding is finite, the packed weights after the call equal,
 *     byte for byte, what swarm_policy_create builds from the same fp32 values on the host (swarm_policy_read_packed reads
 *     them).  Denormals, +-0, exact bf16 values and round-to-even ties are inside that contract: v - bf(v) is the IEEE fp32
 *     difference and is not flushed.  Non-finite weights are outside it: a weight that is Inf, or rounds to Inf, gives
 *     Inf - Inf, a NaN whose sign differs between an x86 host and the GPU (and NaN payloads are not pinned either).
 *   Validation first: a NULL handle or a NULL array returns SWARM_POLICY_ERR_INVALID with a message that starts
 *     "swarm_policy_load_device:", and nothing is enqueued; a launch error returns SWARM_POLICY_ERR_HIP.
 * The precision setting is kept.  One handle holds one set of weights: a caller who learns and rolls out on different streams
 * keeps two handles. */
int  swarm_policy_load_device(swarm_policy_t *p, const float *w1, const float *b1, const float *w2, const float *b2,
                              const float *w3, const float *b3, const float *w4, const float *b4, void *stream);

/* The handle's packed weights, exactly the bytes the kernel reads (what holds swarm_policy_load_device to the host packer, and
 * what a checkpoint of the actor as evaluated would store).  Returns their size in bytes.  host_dst != NULL and capacity >=
 * that size: copies them to host_dst on `stream` (behind the loads enqueued there) and waits for it: complete on return;
 * host_dst == NULL or a smaller capacity: nothing is copied and nothing waits -- the size alone.  A NULL handle or a
 * negative capacity returns -SWARM_POLICY_ERR_INVALID, a HIP error -SWARM_POLICY_ERR_HIP, with a message. */
int64_t swarm_policy_read_packed(swarm_policy_t *p, void *host_dst, int64_t capacity, void *stream);

/* ---- Actor bank: one handle, M actors, one launch.
 * A bank holds `members` weight sets of ONE shape (in_dim, hidden, act_dim), one precision and one geometry.  Every forward
 * call above takes a bank handle: over `rows` rows, member m evaluates the contiguous rows [m R, (m + 1) R), R = rows / members
 * -- equal, contiguous groups, the split a scalar: no table, no per-row index, nothing to upload.  rows % members != 0 is
 * rejected with SWARM_POLICY_ERR_INVALID, a message that names both numbers, and nothing enqueued.  Row r of the call gets, bit
 * for bit, what a plain handle built from member (r / R)'s arrays gives for that row (actions and log_pi): the noise is keyed
 * by row_offset + r as for a plain handle, so it does not depend on M, and log-pi's constant is one per call.  A workgroup
 * serves rows of one member only and never reads or writes a row past its member's last.
 *
 * w[8 m + i]: HOST pointers in the order fc1.weight, fc1.bias, ..., fc4.bias of member m (torch.nn.Linear layout, fp32).
 * wide = 0: the narrow geometry and swarm_policy_create's shape limits; wide = 1: the wide geometry and
 * swarm_policy_create_wide's.  1 <= members <= SWARM_POLICY_BANK_MAX; device memory is members x the single handle's packed
 * weights, and member m's slice is byte for byte what swarm_policy_create / swarm_policy_create_wide builds from the same
 * arrays.  Everything is checked before any device call; a rejection returns SWARM_POLICY_ERR_INVALID with a message that
 * starts "swarm_policy_bank_create:"; without a device: SWARM_POLICY_ERR_HIP, "no HIP device".
 * swarm_policy_set_precision applies to all members.  swarm_policy_load_device and swarm_policy_read_packed on a bank of more
 * than one member are rejected (SWARM_POLICY_ERR_INVALID, the message names the bank call below). */
#define SWARM_POLICY_BANK_MAX 256
int  swarm_policy_bank_create(const float *const *w, int members, int in_dim, int hidden, int act_dim, int wide, int device,
                              swarm_policy_t **out);
/* The members of a bank; 1 for a plain handle (0 for NULL). */
int  swarm_policy_bank_members(const swarm_policy_t *p);
/* swarm_policy_load_device for ONE member (0 <= member < members, else SWARM_POLICY_ERR_INVALID and nothing enqueued): enqueue
 * only, stream order, the same bytes as the host packer; the other members' bytes are untouched.  Messages start
 * "swarm_policy_bank_load_device:". */
int  swarm_policy_bank_load_device(swarm_policy_t *p, int member, const float *w1, const float *b1, const float *w2, const float *b2,
                                   const float *w3, const float *b3, const float *w4, const float *b4, void *stream);
/* swarm_policy_read_packed for ONE member's slice (the size returned is one member's). */
int64_t swarm_policy_bank_read_packed(swarm_policy_t *p, int member, void *host_dst, int64_t capacity, void *stream);

/* ---- Routing by env: which member acts for each env comes from a device table; groups of any size, in any order.
 * Route the bank's rows by env.  member_of_env: DEVICE int32 [n_env], read when the routing kernel RUNS (stream order, as
 * swarm_policy_bank_load_device reads its arrays).  While a route is in force, a forward call over rows == n_env * rows_per_env
 * gives row r, bit for bit (act and log_pi), what a plain handle of member member_of_env[r / rows_per_env] gives that row
 * with the same (noise_scale, seed, step, row_offset): the noise key stays row_offset + r.
 * An env whose entry is outside [0, members) is served by nobody: none of its rows is read or written.
 * member_of_env == NULL with n_env == 0 ends the route (equal contiguous groups again).
 *   Enqueue only: one launch of the routing kernel on `stream`.  The first route, and a route with a larger n_env * rows_per_env
 *     than any before, allocate the tables (and wait for `stream` before the old ones are freed); every other call allocates
 *     nothing and waits for nothing.  Ending the route enqueues nothing.
 *   Stream order: a forward enqueued on the stream before the call uses the previous table, one enqueued after it the new
 *     one; re-routing between two steps needs no host wait.  The table must stay valid and hold the intended values until
 *     the routing kernel has run (writes enqueued on the stream before the call are seen); afterwards it is not read again.
 *     Which route is "in force" for the rows check below is the host's view: the last call made.
 *   How it runs: the routing kernel gathers each member's envs -- env_order, by member and by ascending env inside a member:
 *     numpy's stable argsort of the table over the served envs -- and cuts every member's rows into whole workgroup tiles of
 *     its own; the forward kernels launch floor(rows / T) + min(members, n_env) workgroups (T rows each), an upper bound of
 *     the tiles in use that needs no read-back, and the surplus workgroups return at once.  A workgroup never reads or
 *     writes a row of another member or of an unserved env.  The outputs do not depend on env_order.
 *   Refusals, each SWARM_POLICY_ERR_INVALID with nothing enqueued, the route in force kept, and a message that starts
 *     "swarm_policy_bank_route:" -- the arguments are checked before the handle: n_env < 0; n_env > 0 with a NULL table;
 *     n_env == 0 with a table; rows_per_env < 1 when n_env > 0; n_env * rows_per_env >= 2^31; a NULL handle; a plain (non-bank)
 *     handle.  A HIP error (SWARM_POLICY_ERR_HIP: the allocation of the tables, the launch) is no refusal: it ENDS the
 *     route -- equal contiguous groups again -- because the tables may no longer describe one.
 *   Under a route a forward whose `rows` is not n_env * rows_per_env is refused (SWARM_POLICY_ERR_INVALID, the message names
 *     both numbers): there is no silent fall-back to equal groups.  The rows % members check applies only without a route.
 *   swarm_policy_set_precision, swarm_policy_bank_load_device and swarm_policy_bank_read_packed are unchanged under a route
 *     (the tables serve both precisions). */
int  swarm_policy_bank_route(swarm_policy_t *p, const int32_t *member_of_env, int32_t n_env, int32_t rows_per_env, void *stream);
/* Waits for `stream`, then: counts[members] = envs per member, *unserved = envs outside [0, members), env_order[n_env] (may be
 * NULL) = the envs in the order the kernel serves them (n_env - *unserved entries, then -1).  Returns n_env of the route in
 * force (0: none, and nothing is written or waited for), or -SWARM_POLICY_ERR_INVALID (a NULL handle, NULL counts or
 * unserved) / -SWARM_POLICY_ERR_HIP with a message that starts "swarm_policy_bank_route_read:". */
int  swarm_policy_bank_route_read(swarm_policy_t *p, int32_t *counts, int32_t *unserved, int32_t *env_order, void *stream);

const char *swarm_policy_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
