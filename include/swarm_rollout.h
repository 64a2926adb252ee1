/* swarm_rollout.h -- C ABI of the device rollout loop: K policy + env steps in one library call.
 *
 * The reference's unit of work is the episode (train_assembly.py:81-111): reset, then per step the exploring actor
 * (agents.py:82-96: an epsilon coin picks a uniform action, otherwise actor(obs) + Gaussian noise), env.step, a buffer push
 * and the step's reward mean / std.  swarm_rollout enqueues `steps` such steps on one stream and returns: no host
 * synchronisation, no allocation, no graph capture.  The transitions land in a chained replay ring (the storage of the
 * Python ChainedReplay): consecutive steps share their observation slot.
 *
 * Per step t, with c = (cur + t) % n_slots and n = (c + 1) % n_slots:
 *   - uniform_steps[t] != 0: act[c] = the uniform actions below; otherwise act[c] = the policy of swarm_policy.h on obs[c]
 *     (swarm_policy_forward_explore_at with (seed, step0 + t, row_offset));
 *   - swarm_step(env, act[c]) writes obs[n], rew[c], done[c] and prior[c];
 *   - reward_stats != NULL: reward_stats[t] = (mean, population std) of rew[c].
 * The caller advances its own `cur` by `steps` after the call.
 *
 * Uniform actions (the epsilon branch, agents.py:89-91), counter-based, for global row g = row_offset + row:
 *   key  = pmix64(pmix64(seed + 0x9E3779B97F4A7C15) ^ (0xD1B54A32D192ED03 * (step + 1)))   (the policy's noise key)
 *   ukey = pmix64(key ^ 0x5851F42D4C957F2D)
 *   h    = pmix64(ukey ^ g)
 *   act[g][k] = (float)((h >> (40 - 24 k)) & 0xFFFFFF) * 2^-23 - 1,   k = 0, 1    (uniform on [-1, 1), exact in fp32)
 * with pmix64(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 * (all arithmetic mod 2^64).
 *
 * Reward statistics: the env's rewards are in {0, 1} (swarm_env.h), so the kernel counts the ones as an integer c over the
 * step's R = E * N rows and writes, in fp64, mean m = c / R and std = sqrt((c (1 - m)^2 + (R - c) m^2) / R) -- the two
 * numbers train_assembly.py:109-110 accumulates; deterministic, the mean exact.  A reward outside {0, 1} is counted as 1 if
 * nonzero, i.e. the statistics are only meaningful for this env.
 *
 * Validation comes first: a call that is rejected (bad handle, ring or shape; see swarm_rollout) enqueues nothing.
 * Every pointer in the ring and reward_stats is a DEVICE pointer on the handles' device.
 */
#ifndef SWARM_ROLLOUT_H
#define SWARM_ROLLOUT_H

#include <stdint.h>

#include "swarm_env.h"
#include "swarm_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct swarm_ring {
    void    *obs;        /* [n_slots][rows][obs_dim] in obs_dtype (SWARM_F32 or SWARM_BF16) */
    float   *act;        /* [n_slots][rows][2] */
    float   *rew;        /* [n_slots][rows] */
    uint8_t *done;       /* [n_slots][rows] */
    void    *prior;      /* [n_slots][rows][2] in obs_dtype; NULL exactly when the env handle has no prior */
    int64_t  rows;       /* = E * N of the env handle */
    int32_t  obs_dim;    /* = swarm_obs_dim(env) = the policy's in_dim */
    int32_t  obs_dtype;  /* = the env handle's obs dtype; SWARM_F64 handles are rejected */
    int32_t  n_slots;    /* >= 2 */
    int32_t  cur;        /* slot that holds the current observation, in [0, n_slots) */
} swarm_ring_t;

/* Enqueue `steps` steps on `stream` (a hipStream_t; NULL = the default stream; the env handle is pointed at it through
 * swarm_set_stream).  uniform_steps: HOST [steps], 1 = the uniform (epsilon) branch for that step; NULL = none.
 * reward_stats: DEVICE [steps][2] doubles, NULL = off.  The env handle must be observed (swarm_observe / swarm_reset) and
 * the policy's act_dim must be 2.  Returns SWARM_OK, SWARM_ERR_INVALID / SWARM_ERR_STATE (nothing enqueued) or
 * SWARM_ERR_HIP; the message is in swarm_rollout_last_error.
 * An actor bank (swarm_policy_bank_create, swarm_policy.h) is taken by swarm_rollout, swarm_rollout_logpi, swarm_rollout_explore
 * and swarm_rollout_eval unchanged: with E envs and M members, env e acts with member e / (E / M) at every step -- the
 * bank's contiguous row groups, whole envs each.  E % M != 0 is SWARM_ERR_INVALID, found during validation (nothing enqueued),
 * with a message that starts with the entry point's name.
 * A bank under a route (swarm_policy_bank_route): env e acts with member member_of_env[e] instead.  The route must be the env
 * handle's -- n_env == E and rows_per_env == N; anything else is SWARM_ERR_INVALID, found during validation (nothing enqueued),
 * with a message that starts with the entry point's name and names the numbers -- and then E % M is not checked.  An env the
 * route leaves unserved (an entry outside [0, M)) gets no action written: its rows of act[c] (and of log_pi[c]) keep whatever
 * they held, and the env steps with those values.  The route is read at validation: re-routing takes effect between calls,
 * not inside one. */
int swarm_rollout(swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring, int32_t steps,
                  const uint8_t *uniform_steps, float noise_scale, uint64_t seed, uint64_t step0, uint64_t row_offset,
                  double *reward_stats, void *stream);

/* swarm_rollout that also records the log-probability of each exploring action (the log_pi of agents.py:78-96 that
 * train_assembly_airl.py:134-143 stores with every transition): log_pi is a DEVICE fp32 array [n_slots][rows], indexed by the
 * same slot c as act, and per step t
 *   - a policy step writes log_pi[c] as swarm_policy_forward_explore_logpi does (swarm_policy.h; -0.0f if noise_scale <= 0);
 *   - a uniform (epsilon) step writes log_pi[c][row] = (float)(-2 * ln 2), i.e. -act_dim * log(2).
 * Everything else -- the actions, the env step, the ring, reward_stats -- is bit for bit what swarm_rollout computes with the
 * same arguments.  log_pi = NULL is rejected (SWARM_ERR_INVALID); validation comes first, as in swarm_rollout. */
int swarm_rollout_logpi(swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring, float *log_pi, int32_t steps,
                        const uint8_t *uniform_steps, float noise_scale, uint64_t seed, uint64_t step0, uint64_t row_offset,
                        double *reward_stats, void *stream);

/* Expert rollouts (the reference's collect_expert_data.py: agent_strategy 'rule' or 'llm' with is_collected, the data of
 * train_assembly_airl.py).  Enqueues `steps` expert steps on `stream`; per step t, with c and n as above:
 *   - SWARM_EXPERT_RULE: the rule-based expert of assembly.py:530-601 on the current state, in fp64 (swarm_rule_action's
 *     kernel after swarm_rule_action's observation pass: its action bit for bit); the env steps with that fp64 action
 *     (SWARM_F64) and act[c] = its f32 rounding.  The
 *     trajectory is bit-identical to the eager loop `u = swarm_rule_action(); swarm_step(u, SWARM_F64)`.
 *   - SWARM_EXPERT_LLM: the env steps with action = NULL (the library's prior-policy twin; the handle must be created with
 *     llm_action) and act[c] = that applied action rounded to f32 (the `is_collected` fifth return value of the eager path).
 *   - both: swarm_step writes obs[n], rew[c], done[c] and prior[c]; reward_stats as in swarm_rollout.
 * Why f32 rows suffice: ReplayBufferExpert.sample hands its rows out through torch.Tensor, i.e. as fp32, and the step's f32
 * observation is the f32 rounding of the fp64 one (the env's parity contract), so AIRL sees the same bits as from the
 * reference's fp64 buffer.
 * Checks as swarm_rollout minus the policy's; SWARM_EXPERT_RULE also needs num_obs_grid_max <= 128 and, as swarm_rule_action,
 * refuses a large_swarm handle with n_agents <= 256 (the default handle serves those counts).  A large_swarm handle with
 * n_agents in [257, 1024] is served for both sources: RULE by k_rule_large behind the large-swarm export pass, LLM by the
 * large-swarm kernels' own act_next.
 * The first RULE call allocates the handle's fp64 action scratch and, unless swarm_rule_action or swarm_get_indices already
 * did, its list scratch (once each); later calls allocate nothing.  A rejected
 * call enqueues nothing; the message is in swarm_rollout_last_error. */
enum { SWARM_EXPERT_RULE = 0, SWARM_EXPERT_LLM = 1 };
int swarm_rollout_expert(swarm_env_t *env, const swarm_ring_t *ring, int32_t steps, int32_t source, double *reward_stats,
                         void *stream);

/* Evaluation rollouts (the reference's eval_assembly.py:119-205: the deterministic actor, the three wrapper metrics and the
 * state trace every step, target-shape switches in mid-episode).  Enqueues `steps` evaluation steps on `stream`; per step t,
 * in the script's order (:145-186), with c and n as above:
 *   1. p / dp given: p[t], dp[t] = the env's state BEFORE the step (:150-151; device-to-device copies);
 *   2. switch_to[t] >= 0: swarm_select_shape(env, switch_to[t], NULL) (:154-157).  The ring slot obs[c] is NOT rewritten: the
 *      reference's actor at a switch step sees the observation the previous env.step returned, computed against the old
 *      shape (:177-185);
 *   3. metrics given: metrics[t] = swarm_metrics of the current state against the cells now in force (:160-162);
 *   4. act[c] = the policy on obs[c] without noise (explore=False, :178: swarm_policy_forward_explore_at with noise_scale 0),
 *      at the precision the policy handle is set to;
 *   5. swarm_step writes obs[n], rew[c], done[c] and prior[c]; reward_stats[t] as in swarm_rollout.
 * Without switches, metrics and trace the ring is bit for bit what swarm_rollout writes with noise_scale 0 and no uniform
 * steps.  A two-slot ring is enough for evaluation; a long ring records the evaluation transitions.
 * switch_to: HOST [steps], -1 = keep, s >= 0 = every env switches to shape s of the uploaded set; NULL = no switch.
 * out: the optional outputs, all DEVICE pointers (NULL = all off).
 * Checks as swarm_rollout, plus: every switch_to[t] in [-1, n_shapes) (SWARM_ERR_INVALID), a shape set if any entry is >= 0
 * (SWARM_ERR_STATE), p and dp given together.  A rejected call enqueues nothing and leaves the handle as it was; the message
 * is in swarm_rollout_last_error.  No host synchronisation, no allocation, no graph capture. */
typedef struct swarm_eval_out {
    double *metrics;        /* [steps][E][3]: coverage_rate, distribution_uniformity, voronoi_based_uniformity; NULL = off */
    double *p, *dp;         /* [steps][E][2][N]: the state before step t; both or neither */
    double *reward_stats;   /* [steps][2] as swarm_rollout; NULL = off */
} swarm_eval_out_t;
int swarm_rollout_eval(swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring, int32_t steps, const int32_t *switch_to,
                       const swarm_eval_out_t *out, void *stream);

/* Per-env exploration: the epsilon coin and the noise scale of agents.py:87-96 belong to ONE env (the reference flips
 * np.random.rand() < self.epsilon per step of its env), so a batch of E envs flips E coins per step and may give every env
 * its own epsilon and noise scale (an exploration spectrum over the width of the batch).  Everything is drawn on the device,
 * counter-based, in stream order: a rollout is a function of (seed, step0, row_offset) and the arrays alone, on any rank.
 *
 * With key = swarm_noise_key(seed, step) (the policy's noise key above), n_agents N, global row g = row_offset + row,
 * env e = row / N and global env ge = row_offset / N + e:
 *
 * Coin:
 *   ckey = pmix64(key ^ 0xA0761D6478BD642F)            (its own salt: not the uniform-action salt 0x5851F42D4C957F2D)
 *   h    = pmix64(ckey ^ ge)
 *   u    = (float)(h >> 40) * 2^-24                    in [0, 1), exact in fp32
 *   coin = u < epsilon[e]                              an fp32 compare: epsilon <= 0 or NaN never fires, epsilon >= 1 always
 * Coin env: act[g] = the uniform action of global row g ("Uniform actions" above, keyed by g);
 *   log_pi[g] = (float)(-2 ln 2).
 * Other env, sigma[e] > 0: z = the normals of global row g (swarm_policy.h, "Gaussian noise");
 *   act[g][k] = clamp(a[k] + sigma[e] * z[k], -1, 1) in fp32, no fused multiply-add, a = what the deterministic actor wrote;
 *   log_pi[g] = -(0.5f * s) - log_c[e], s as in swarm_policy.h.
 * Other env, sigma[e] <= 0 or NaN: act is left as it is; log_pi[g] = -0.0f.
 *
 * log_c is an input: the scalar path forms c = (float)((double)act_dim * log((double)sigma * sqrt(2 pi))) on the host with
 * libm (swarm_policy.h), and a device log is not pinned to that; the caller computes log_c[e] with that expression from the
 * fp32 sigma[e].  With epsilon = NULL and sigma[e] = s everywhere (log_c[e] = c of s) the rollout is bit for bit
 * swarm_rollout / swarm_rollout_logpi with noise_scale = s; with epsilon[e] >= 1 everywhere it is those with every
 * uniform_steps[t] = 1.
 *
 * The arrays are read when the kernels RUN, not when the call returns: as swarm_policy_load_device and swarm_reset_envs, the
 * call only enqueues, a rewrite of the arrays enqueued on `stream` before the call is seen by it, one enqueued after it is
 * not, and the caller keeps the arrays alive and unchanged until the stream has passed the call. */
typedef struct swarm_explore {
    const float *epsilon;  /* DEVICE [E] or NULL (= 0 everywhere) */
    const float *sigma;    /* DEVICE [E], required: the noise scale of env e */
    const float *log_c;    /* DEVICE [E]: env e's log-pi constant; required exactly when log_pi is given */
    uint8_t     *coin;     /* DEVICE [steps][E] or NULL: 1 where env e took the uniform branch at step t */
} swarm_explore_t;

/* swarm_rollout (log_pi = NULL) / swarm_rollout_logpi (log_pi [n_slots][rows]) with per-env exploration.  Per step t:
 *   1. swarm_policy_forward_explore_at with noise_scale = 0 on obs[c] into act[c] (the deterministic actor);
 *   2. the exploration above applied in place to act[c] (and log_pi[c], ex->coin[t]) with (seed, step0 + t, row_offset);
 *   3. swarm_step;  4. the reward count.
 * The ring, the slots and reward_stats are as in swarm_rollout.  Validation first, nothing enqueued: everything swarm_rollout
 * checks, plus: ex and ex->sigma not NULL, ex->log_c given when log_pi is, row_offset % n_agents == 0 (a coin belongs to a
 * whole env).  The message (swarm_rollout_last_error) starts with "swarm_rollout_explore". */
int swarm_rollout_explore(swarm_env_t *env, swarm_policy_t *pol, const swarm_ring_t *ring, float *log_pi /* or NULL */,
                          int32_t steps, const swarm_explore_t *ex, uint64_t seed, uint64_t step0, uint64_t row_offset,
                          double *reward_stats, void *stream);

/* The eager twin: one step's exploration applied in place to act[rows][2] (DEVICE, on the calling thread's current device),
 * which holds the deterministic actor's output; rows = E * n_agents.  coin: DEVICE [rows / n_agents] or NULL (ex->coin is not
 * used here).  One launch on `stream`, no host synchronisation.  Rejected with SWARM_ERR_INVALID, nothing enqueued: NULL act,
 * ex or ex->sigma, log_pi without ex->log_c, rows < 0, n_agents < 1, rows or row_offset no multiple of n_agents.  The message
 * (swarm_rollout_last_error) starts with "swarm_explore_envs". */
int swarm_explore_envs(float *act, float *log_pi /* or NULL */, int64_t rows, int32_t n_agents, const swarm_explore_t *ex,
                       uint8_t *coin /* [rows / n_agents] or NULL */, uint64_t seed, uint64_t step, uint64_t row_offset,
                       void *stream);

/* Message of the last failing swarm_rollout / swarm_rollout_logpi / swarm_rollout_explore / swarm_explore_envs /
 * swarm_rollout_expert / swarm_rollout_eval on the calling thread. */
const char *swarm_rollout_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SWARM_ROLLOUT_H */
