/*
 * swarm_env.h -- C ABI of libswarmenv.so: the MI355X-native batched AssemblySwarm environment step.
 *
 * This is the drop-in boundary for the reference's env-step hot path.  The reference crosses its
 * Python -> native boundary with ctypes into libAssemblyEnv.so
 * (/root/reference/cus_gym/gym/envs/customized_envs/envs_cplus/c_lib.py:11-37), five times per step, one
 * environment at a time, from AssemblySwarmEnv.step()/_get_obs()/_get_reward()
 * (/root/reference/cus_gym/gym/envs/customized_envs/assembly.py:234-255,357-380,460-466,495-504,613-624).
 * Here the same Python host binds ONE handle-based library with ctypes; state lives in HBM and one
 * call advances E independent environments.
 *
 * Two groups of entry points:
 *
 *  (1) the batched ABI (swarm_*): opaque handle, plain pointers and sizes, int status returns.
 *      It replaces, fused into one launch per step, what the reference spreads over
 *        - AssemblySwarmEnv.step numpy glue             assembly.py:487-666 (incl. _get_dist_b2b :442-457)
 *        - _sf_b2b_all                                  AssemblyEnv.h:64-73   / AssemblyEnv.cpp:735-815
 *        - _get_dist_b2w                                AssemblyEnv.h:75-81   / AssemblyEnv.cpp:817-855
 *        - calculateActionPrior / robotPolicy           AssemblyEnv.h:98-109  / AssemblyEnv.cpp:1061-1196
 *        - _get_observation (+_get_focused, _get_target_grid_state, _make_periodic)
 *                                                       AssemblyEnv.h:13-34   / AssemblyEnv.cpp:18-351,628-732,858-908
 *        - _get_reward (+_rho_cos_dec)                  AssemblyEnv.h:35-58   / AssemblyEnv.cpp:354-626,1012-1020
 *
 *  (2) the legacy symbols (_get_observation, _get_reward, _sf_b2b_all, _get_dist_b2w,
 *      calculateActionPrior) with the reference's exact signatures and host-pointer / caller-owned
 *      buffer contract, so an unmodified assembly.py can load this library in place of
 *      libAssemblyEnv.so.  They run the same HIP kernels on a private one-environment handle.
 *
 * There is no CPU fallback anywhere in this library: without a HIP device every call fails.
 *
 * Memory contract of the batched ABI: every pointer passed to swarm_step / swarm_observe / swarm_select_shapes /
 * swarm_reset_envs / swarm_get_indices is a DEVICE pointer (hipMalloc / torch.Tensor.data_ptr()) valid on the handle's
 * device.  swarm_set_cells / swarm_set_state / swarm_get_state accept host or device pointers (hipMemcpyDefault).
 *
 * Stream contract (DESIGN.md "Stream contract"; tests/test_gpu_streams.py): all device work goes to the handle's stream
 * (swarm_set_stream; NULL = the default stream).  swarm_step, swarm_observe, swarm_reset, swarm_reset_envs, swarm_select_shape(s),
 * swarm_metrics and swarm_rule_action only enqueue: they return without waiting for the stream.  swarm_set_cells, swarm_set_state and the
 * readers swarm_get_state / _get_cells / _get_shape_index / _get_indices / _get_llm_action / _path_envs, swarm_observe_host,
 * swarm_step_host and swarm_synchronize return after the stream has run everything enqueued so far, their own work included
 * (swarm_get_indices too, although its pointers are device pointers).  swarm_set_shapes and swarm_destroy release device
 * memory and thereby wait for pending work that still reads it; work enqueued before them completes on what it was given.
 *
 * Layouts (E = n_env, N = n_agents, D = obs_dim = 4*(topo + 1 + with_self) + 2*num_obs_grid_max):
 *   p, dp            double [E][2][N]     component-major per env, exactly the reference's (2, n_a) arrays
 *   cells            double [E][2][n_cells_max]  the reference's grid_center (2, n_g), row stride n_cells_max
 *   action           float|double [E][N][2]      agent-major pairs (u_x, u_y)
 *   obs              float|double [E][N][D]      one contiguous row per agent; row content and order are the
 *                                                reference's obs column (AssemblyEnv.cpp:294-306)
 *   reward           float  [E][N]    in {0,1}
 *   done             uint8  [E][N]    always 0 (assembly.py:480-482)
 *   a_prior          float|double [E][N][2]
 *   neighbor_index   int32  [E][N][topo], in_flags int32 [E][N], sensed_index int32 [E][N][num_obs_grid_max],
 *   occupied_index   int32  [E][N][num_occupied_grid_max]   (the reference's index scratch; debug export)
 * All arithmetic that decides an index, a flag, the state update or the reward is IEEE double in the
 * reference's operation order (no FMA contraction); obs / a_prior are rounded once to obs_dtype at the store.
 */
#ifndef SWARM_ENV_H
#define SWARM_ENV_H

#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define SWARM_ABI_VERSION 5

enum { SWARM_F32 = 0, SWARM_F64 = 1, SWARM_BF16 = 2 };

enum {
    SWARM_OK = 0,
    SWARM_ERR_INVALID = 1,      /* bad argument / unsupported configuration */
    SWARM_ERR_HIP = 2,          /* a HIP runtime call failed (no device, OOM, launch failure ...) */
    SWARM_ERR_STATE = 3         /* call order violated (e.g. step before cells/state were set) */
};

typedef struct swarm_env swarm_env_t;

/* Mirrors the constants AssemblySwarmEnv hard-codes or derives (assembly.py:27-81,99-131,193-199). */
typedef struct swarm_config {
    int32_t n_env;                  /* E >= 1 */
    int32_t n_agents;               /* N in [1, 256]; with large_swarm in [1, 1024] */
    int32_t n_cells_max;            /* capacity of one env's cell list, >= every n_g, <= 32767 */
    int32_t topo_nei_max;           /* assembly.py:34   = 6 (1..6) */
    int32_t num_obs_grid_max;       /* assembly.py:128  = 80 */
    int32_t num_occupied_grid_max;  /* assembly.py:130  = 200 */
    int32_t is_boundary;            /* 1 = walls (assembly.py:99-103), 0 = periodic */
    int32_t with_self_state;        /* is_con_self_state */
    int32_t with_prior;             /* training_method == 'llm_rl': compute a_prior (assembly.py:605-624) */
    int32_t obs_dtype;              /* SWARM_F32 (product), SWARM_F64 (bit-exact parity mode) or SWARM_BF16 (obs and a_prior as
                                     * bfloat16 = the f32 value rounded to nearest-even: half the rollout's bytes, feeds the bf16
                                     * policy kernel of swarm_policy.h directly) */
    int32_t device;                 /* HIP device ordinal, -1 = current */
    int32_t debug_flags;            /* bit 0: force every exact (fp64) fallback path of the fp32 pre-filters; bit 1: disable the lattice path;
                                     * bit 2: a small batch keeps the full workgroup geometry (no half-occupied variant); bit 3: a batch
                                     * that holds both cell sets the lattice walk serves and cell sets it does not runs the generic scan
                                     * for every env (one launch) instead of one launch of each kernel; bit 4: those two launches run
                                     * one after the other on the handle's stream instead of side by side -- results are identical
                                     * with any of them; bit 5: the rule expert (swarm_rule_action, swarm_rollout_expert's rule source)
                                     * runs k_rule_large, the kernel of large_swarm handles above 256 agents, instead of k_rule -- the
                                     * same bits, and no other effect: the in-binary stand-in that lets the two kernels be compared on
                                     * the same export lists (tests/test_gpu_large_rule.py); bits 8..15: diagnostics (tools/ablate.py) -- the lattice kernels of 64 agent
                                     * threads (N in 33..64, full geometry) act on them only in a library built with -DSWARM_DIAG and
                                     * ignore them otherwise; every other kernel always acts on them */
    double d_sen;                   /* assembly.py:199  = 0.4 */
    double r_avoid;                 /* assembly.py:124 */
    double size_a;                  /* assembly.py:44   = 0.035 */
    double k_ball, k_wall, c_wall;  /* assembly.py:71-74 = 30, 100, 5 */
    double vel_max;                 /* assembly.py:52   = 0.8 */
    double dt;                      /* assembly.py:79   = 0.1 */
    double boundary[4];             /* [x_min, y_max, x_max, y_min], assembly.py:193-196 */
    double prior_gain[3];           /* prior policy gains: attraction, repulsion, alignment -- AssemblyEnv.cpp:1128-1132 = 2, 3, 2 */
    double llm_repulsion;           /* repulsion gain of the prior's Python twin robot_prior_policy, assembly.py:895 = 1.0 */
    int32_t llm_action;             /* 1: agent_strategy == 'llm' (assembly.py:525-529): every pass also evaluates that twin on
                                     * the new state; swarm_step(action = NULL) then applies it as the action */
    int32_t large_swarm;            /* 0 (default): the step kernel, n_agents <= 256.  1: n_agents in [1, 1024]; every step and
                                     * observation pass of the handle runs through the two large-swarm kernels (env_large.hip), at any
                                     * n_agents, with the same results bit for bit.  Above 256 agents such a handle has the rule expert
                                     * (swarm_rule_action, swarm_rollout_expert: k_rule_large); with n_agents <= 256 it refuses both
                                     * (the default handle serves those counts).  It reports every env as scanned (swarm_path_envs)
                                     * and accepts debug_flags, bit 5 included, without effect */
} swarm_config_t;

int  swarm_abi_version(void);
void swarm_default_config(swarm_config_t *cfg);     /* fills the reference's constants; caller sets sizes */

int  swarm_create(const swarm_config_t *cfg, swarm_env_t **out);
int  swarm_destroy(swarm_env_t *h);
/* Message of the last failing call on `h`; h == NULL: last failing swarm_create on this thread. */
const char *swarm_last_error(const swarm_env_t *h);

int  swarm_set_stream(swarm_env_t *h, void *hip_stream);   /* hipStream_t; NULL = default stream */
int  swarm_synchronize(swarm_env_t *h);
int  swarm_obs_dim(const swarm_env_t *h);

/* Target cells of envs [env_begin, env_begin+count): cells[count][2][n_cells_max] (host or device),
 * n_g[count], l_cell[count] (HOST arrays; l_cell feeds the in-shape threshold sqrt(2)*l_cell/2). */
int  swarm_set_cells(swarm_env_t *h, int env_begin, int count,
                     const double *cells, const int32_t *n_g, const double *l_cell);
int  swarm_set_state(swarm_env_t *h, const double *p, const double *dp);   /* [E][2][N], host or device */

/* Batched device-side reset (what AssemblySwarmEnv.reset() does per environment, assembly.py:156-219): a shape set
 * (HOST arrays: shape_cells[S][2][n_cells_max] in the shape frame = grid_center_origins[s].T, n_g[S], l_cell[S]) is
 * uploaded once; swarm_reset then draws, for every env, shape index, rotation, offset and the agents' positions /
 * velocities from a counter-based generator keyed by (seed, episode, env_offset + env) -- no host round trip, any
 * env range reproducible on any rank -- and runs the observation pass (obs may be NULL). */
int  swarm_set_shapes(swarm_env_t *h, int n_shapes, const double *shape_cells, const int32_t *n_g, const double *l_cell);
int  swarm_reset(swarm_env_t *h, uint64_t seed, uint64_t episode, int64_t env_offset, void *obs);
/* Per-env device-side reset: the envs named by `episode` start a new episode, the others go on.
 *   episode  DEVICE int64 [E].  ep >= 0: env e is redrawn exactly as swarm_reset(seed, ep, env_offset) draws env e -- shape index,
 *     pose, cells (both layouts, padding 0.0), n_g, in-shape cut-off, lattice record, p and dp: the same draws, expressions and
 *     order, hence the same bits.  A negative entry (-1 is the documented "keep"): nothing of env e is written.
 * One kernel on the handle's stream, one workgroup per env; then the observation pass runs over the whole batch (obs may be
 * NULL), as in swarm_select_shapes -- it is idempotent on an env that did not change.  Afterwards a reset env is, for every later
 * call, bit for bit the env of a handle that ran swarm_reset with that episode, and a kept env continues exactly as if nothing
 * had been called.
 *   Enqueue only: no host synchronisation, no allocation, no host-to-device copy.
 *   Stream order: episode is read when the kernel RUNS, not when the call is made: it must stay valid and hold the intended
 *     values until then (writes enqueued on the same stream before the call are seen).  Work on other streams that writes it is
 *     the caller's to order with events.
 *   Validation first: a NULL handle or a NULL episode returns SWARM_ERR_INVALID; no shape set, no state, or cells not set for
 *     every env (a kept env needs both) returns SWARM_ERR_STATE; the message starts "swarm_reset_envs:" and nothing is enqueued.
 * The host does not learn which env was reset: it plans the cell path for the envs' present cell sets and every shape of the set
 * together (as swarm_select_shapes does); swarm_path_envs reads the device records and stays exact.  Default and large_swarm
 * handles alike. */
int  swarm_reset_envs(swarm_env_t *h, uint64_t seed, const int64_t *episode, int64_t env_offset, void *obs);
/* Device-side shape switch (what eval_assembly.py:34-57 process_shape does in mid-episode, with its rotation 0 and offset 0):
 * every env takes shape `shape_index` of the set uploaded by swarm_set_shapes, at the set's own pose -- the env's cells are the
 * shape's cells, the same doubles.  One kernel on the handle's stream writes the cells, n_g, the in-shape cut-off, the lattice
 * record and the shape index of every env; p / dp are untouched.  Then the observation pass runs (obs may be NULL: the carried
 * prior and the neighbour caches are refreshed, no observation is written).  Afterwards the handle is bit for bit in the state
 * that swarm_set_cells with E copies of that shape followed by swarm_observe leaves (swarm_get_shape_index then reports
 * shape_index instead of -1).  No host synchronisation, no host-to-device copy, no allocation.
 * SWARM_ERR_STATE without a shape set or a state, SWARM_ERR_INVALID for an index outside [0, n_shapes): nothing is enqueued. */
int  swarm_select_shape(swarm_env_t *h, int32_t shape_index, void *obs);
/* Per-env device-side shape switch (process_shape per env, eval_assembly.py:34-57, with its rand_angle / rand_target_offset):
 * each env takes its own shape at its own pose, or keeps what it has.  The agents (p / dp) stay where they are.
 *   shape_index  DEVICE int32 [E].  s in [0, n_shapes): env e takes shape s of the set uploaded by swarm_set_shapes.  Any other
 *     value (-1 is the documented "keep"): nothing of env e is written -- its cells, n_g, in-shape cut-off, lattice record and
 *     shape index stay as they are.  The kernel tests the range before it reads the set: an out-of-range index is a kept env.
 *   pose  DEVICE double [E][4] = (c, s, off_x, off_y) per env, or NULL.  NULL: the shape's own doubles, the whole row, padding
 *     included -- with all indices equal the call is bit for bit swarm_select_shape.  Given: cell k < n_g becomes
 *         x = c*sx + s*sy + off_x,   y = -s*sx + c*sy + off_y
 *     in IEEE double, in this order, without FMA contraction (swarm_reset's expression; rotate_matrix = [[c, s], [-s, c]],
 *     assembly.py:177-178,187), cells k >= n_g become 0.0, and a lattice record's frame is moved the same way.  c and s are the
 *     caller's cos / sin of the angle: the kernel evaluates no trigonometric function, so the cells are reproducible from numpy bit
 *     for bit.  The contract is this ELEMENTWISE expression, not np.dot: np.dot(R, g) + off goes through BLAS, which contracts,
 *     and differs from it in the last bit of a good part of the values (so does swarm_reset's transform).  At the reference's
 *     live setting (angle 0, offset 0) both are the identity.
 * One kernel on the handle's stream writes, per switched env, both cell layouts, n_g, the in-shape cut-off, the lattice record
 * and the shape index; then the observation pass runs (obs may be NULL, as in swarm_select_shape).  Afterwards every output of
 * every later call is bit for bit what it is on a handle that was given those cells through swarm_set_cells + swarm_observe
 * (swarm_get_shape_index reports the indices instead of -1); a kept env continues exactly as if nothing had been called.
 *   Enqueue only: no host synchronisation, no allocation, no host-to-device copy.
 *   Stream order: the two arrays are read when the kernel RUNS, not when the call is made: they must stay valid and hold the
 *     intended values until then (writes enqueued on the same stream before the call are seen).  Work on other streams that
 *     writes the arrays is the caller's to order with events.
 *   Validation first: a NULL handle or a NULL shape_index returns SWARM_ERR_INVALID; no shape set, no state, or cells not set
 *     for every env (a kept env needs cells) returns SWARM_ERR_STATE; the message starts "swarm_select_shapes:" and nothing is
 *     enqueued.
 * The host does not learn which env took what (as after swarm_reset): it plans the cell path for the envs' present cell sets
 * and every shape of the set together; swarm_path_envs reads the device records and stays exact. */
int  swarm_select_shapes(swarm_env_t *h, const int32_t *shape_index, const double *pose, void *obs);
int  swarm_get_state(swarm_env_t *h, double *p, double *dp);
int  swarm_get_cells(swarm_env_t *h, double *cells, int32_t *n_g);        /* [E][2][n_cells_max], [E]; host or device */
/* Shape index each env drew in the last swarm_reset (assembly.py:160 `rand_shape_index`) or was given by swarm_select_shape(s),
 * [E] host or device; -1 for envs whose cells were set through swarm_set_cells.  The host needs it for l_cell / shape_frequency (assembly.py:161-163). */
int  swarm_get_shape_index(swarm_env_t *h, int32_t *shape_index);

/* Recompute observations and the obs-derived caches (neighbor_index, in_flags, nearest cell) from the
 * current state: what AssemblySwarmEnv.reset() does with its final _get_obs() (assembly.py:221).
 * Must be called after swarm_set_state / swarm_set_cells and before swarm_step.  obs may be NULL. */
int  swarm_observe(swarm_env_t *h, void *obs);

/* One AssemblySwarmEnv.step(a) for every env.  action_dtype: SWARM_F32 / SWARM_F64.
 * reward / done / a_prior may be NULL (not written). */
/* action == NULL (handles created with llm_action only): apply the 'llm' strategy's action of the current state. */
int  swarm_step(swarm_env_t *h, const void *action, int action_dtype,
                void *obs, float *reward, uint8_t *done, void *a_prior);

/* ---- reference-shaped HOST outputs: the numpy API of AssemblySwarmEnv.step / reset (assembly.py:487-666,156-223) ----
 * The reference returns obs (D, n_a) float64, reward (1, n_a) float64, done (1, n_a) bool, a_prior (2, n_a) float64
 * (assembly.py:227-231,353,480-482,612,663-666).  With E environments the agent axis is n_a = E*N, env-major.  The library
 * owns the step outputs on the device, widens / transposes them into that layout on the device and moves them with ONE
 * asynchronous copy into pinned host memory it owns: two slots (ping-pong; the arrays of the previous step stay valid while
 * the next one is taken).  swarm_host_outputs returns the four host arrays of a slot (valid until swarm_destroy);
 * a_prior is meaningful only with with_prior.  Both calls below return after the data has landed in the slot. */
typedef struct swarm_host_out {
    double  *obs;        /* (D, E*N)  row-major: obs[r * E*N + e*N + i] */
    double  *a_prior;    /* (2, E*N) */
    double  *reward;     /* (1, E*N) */
    uint8_t *done;       /* (1, E*N)  0 / 1 */
} swarm_host_out_t;
int  swarm_host_outputs(swarm_env_t *h, int slot, swarm_host_out_t *out);
/* swarm_observe + export of obs into `slot` (the tail of reset(), assembly.py:221-223). */
int  swarm_observe_host(swarm_env_t *h, int slot);
/* One step + export into `slot`.  action: action_on_device == 0: HOST array in the reference's layout (2, E*N)
 * (component-major, envs side by side), float or double; action_on_device == 1: DEVICE [E][N][2] as swarm_step;
 * NULL: the 'llm' strategy's own action (llm_action handles only). */
int  swarm_step_host(swarm_env_t *h, const void *action, int action_dtype, int action_on_device, int slot);

/* The 'llm' strategy's action for the CURRENT state (what swarm_step(action = NULL) would apply): [E][N][2] doubles, host or
 * device pointer.  llm_action handles only. */
int  swarm_get_llm_action(swarm_env_t *h, double *action);

/* Evaluation metrics of the current state, per env: out[E][3] (DEVICE pointer, double) =
 * [coverage_rate, distribution_uniformity, voronoi_based_uniformity] of
 * /root/reference/cus_gym/gym/wrappers/customized_envs/assembly_wrapper.py:48-128 (numpy semantics incl. np.var). */
int  swarm_metrics(swarm_env_t *h, double *out);

/* The reference's rule-based expert controller (agent_strategy == 'rule', assembly.py:530-601) evaluated on the CURRENT
 * state: action[E][N][2] (DEVICE pointer, double), clipped to [-1, 1]; feed it to swarm_step with SWARM_F64 to reproduce
 * a rule-mode step (with is_collected the reference returns it as the fifth element, assembly.py:663-664).  Runs the
 * observation pass with the index export switched on, then a one-thread-per-agent kernel.  fp64 in numpy's operation
 * order; np.cos differs from the device cos by a few ulp, so parity is 1e-12 absolute, not bit-exact.
 * The clip is np.clip: a NaN sum stays NaN (it is not turned into a bound).  Two agents at the same position give
 * r_avoid / 0 * 0 = NaN in both components of both; a NaN coordinate makes that agent's action NaN and removes it from
 * everybody's neighbourhood (NaN compares false), a NaN velocity makes NaN the action of every agent that has it within
 * d_sen.  Every finite state gives a finite action.  (The observation pass is memory-safe for such states: DESIGN.md,
 * "Non-finite positions in the observation pass".)
 * The n_s > num_obs_grid_max selection of the sensed cells rounds i * step as the controller does, np.round (a tie goes to
 * the even index, assembly.py:564); the observation (swarm_observe / swarm_step / swarm_get_indices) keeps std::round
 * (AssemblyEnv.cpp:223).  Ties exist only when num_obs_grid_max - 1 is even, so not for the default 80; for those caps the
 * list the expert reads differs from the one swarm_get_indices returns.
 * Periodic handles (is_boundary == 0): the controller takes no wrap, as assembly.py:530-601 takes none -- its distances to
 * agents and cells, the in-shape flag, the nearest cell and the sensed-cell list with its occupied-cell filter all use the
 * plain differences of the stored positions (the observation pass wraps only the topological-neighbour rows).
 * tests/test_gpu_rule_contract.py holds this call and swarm_rollout_expert's rule source to the numpy restatement.
 * Handles created with large_swarm: with n_agents in [257, 1024] the cap_even export pass of the large-swarm kernels, then
 * k_rule_large (rule_expert.hip: one wave per env and 64 agents, k_rule's arithmetic and operation order; on the same lists
 * the same bits as k_rule, which debug_flags bit 5 lets a default handle show) -- enqueued on the handle's stream like the
 * default handle's.  tests/test_gpu_large_rule.py holds it to the same restatement.  With n_agents <= 256 a large_swarm
 * handle is refused (SWARM_ERR_INVALID, nothing enqueued): the default handle serves n_agents <= 256. */
int  swarm_rule_action(swarm_env_t *h, double *action);

/* Index scratch of the CURRENT state (device pointers, any may be NULL).  The step keeps neighbor_index / in_flags / the
 * sensed and occupied lists in LDS and writes none of them to HBM; this call re-runs the observation pass on the current
 * state with the export switched on (it recomputes the same caches from the same state: idempotent) and copies them out. */
int  swarm_get_indices(swarm_env_t *h, int32_t *neighbor_index, int32_t *in_flags,
                       int32_t *sensed_index, int32_t *occupied_index);

/* How many environments currently have target cells that are a row-major subset of a square lattice (the reference's
 * tiled shapes always are, its seven fig PNGs included).  For such an env (any n_agents up to 256) whose own sensing window spans
 * at most 15 lattice rows, the sensed / occupied bit sets are built by a row walk over the lattice instead of the all-cells scan;
 * results are identical.  The choice is made per workgroup, not per batch (swarm_path_envs): other envs of the batch keep the
 * all-cells scan without taking the row walk from this one.  debug_flags bit 1 disables that path.  After swarm_reset the
 * answer is n_env if every shape of the set is such a lattice, else 0. */
int  swarm_lattice_envs(const swarm_env_t *h);

/* How many environments the next launch steps with the row walk (*walk_envs) and with the all-cells scan (*scan_envs); the two
 * add up to n_env.  The unit is the workgroup: with n_agents < 64 one workgroup holds 64 / npad envs (npad = n_agents rounded up
 * to a power of two, at least 8), and one env that needs the scan takes its whole workgroup to it.  A batch with envs of both
 * kinds is stepped by two launches, one of each kernel, each returning at once from the other's workgroups; a batch of one kind
 * by one launch, as is any batch with debug_flags bit 3 (all scan).  Synchronises the handle's stream and reads the envs'
 * device records: after swarm_reset only they know which env drew which shape.  SWARM_ERR_STATE before every env has cells.
 * Cost: the two launches run side by side, which pays while one of them is small; where both are large (about half the
 * workgroups each) the serial form (debug_flags bit 4) is faster, and a batch in which NO workgroup walks (N < 64 with an
 * off-lattice env in every workgroup) still pays for a lattice launch that only exits -- bit 3 is the cheaper setting there
 * ("Mixed batches"). */
int  swarm_path_envs(swarm_env_t *h, int32_t *walk_envs, int32_t *scan_envs);

/* Roofline helper: bytes one swarm_step moves by SURVEY.md section 8d's accounting IN THIS BUILD'S DTYPES (fp64 state and
 * cells); bench.py's `roofline` uses section 8d's own fp32 figure (821 B per agent-step + 8 B per cell) and reports this one
 * beside it. */
double swarm_step_algorithmic_bytes(const swarm_env_t *h);
/* Time the last N launches?  No: timing lives in the caller (HIP events on the handle's stream).
 * These two record / read HIP events on that stream so a ctypes host needs no HIP binding. */
int  swarm_timer_start(swarm_env_t *h);
int  swarm_timer_stop(swarm_env_t *h, float *elapsed_ms);   /* synchronizes on the stop event */

/* Diagnostics: the library also exports two entry points that are deliberately NOT part of this interface and are declared
 * nowhere -- tools and tests bind them by name.  swarm_debug_lds_map(npad, half, g_max, out[32]) is host-only and reports the
 * LDS map of the lattice launches (tests/test_lds_map.py); swarm_debug_stamps(...) exists only in the -DSWARM_STAMPS build
 * (tools/phase_profile.py).  Their arguments are documented at their definitions in csrc/swarm_env.hip,
 * beside the step kernel whose tables they read; every other entry point is defined in csrc/env_api.hip. */

/* ---- legacy symbols: exact reference signatures (AssemblyEnv.h:13-34,35-58,64-73,75-81,98-109) ---- */
void _get_observation(double *p_input, double *dp_input, double *heading_input, double *obs_input,
                      double *boundary_pos_input, double *grid_center_input, int *neighbor_index_input,
                      int *in_flags_input, int *sensed_index_input, int *occupied_index_input,
                      double d_sen, double r_avoid, double l_cell, double Vel_max, int topo_nei_max,
                      int num_obs_grid_max, int num_occupied_grid_max, int n_a, int n_g,
                      int obs_dim_agent, int dim, bool *condition);
void _get_reward(double *p_input, double *dp_input, double *heading_input, double *act_input,
                 double *reward_input, double *boundary_pos_input, double *grid_center_input,
                 int *neighbor_index_input, int *in_flags_input, int *sensed_index_input,
                 int *occupied_index_input, double d_sen, double r_avoid, double l_cell,
                 int topo_nei_max, int num_obs_grid_max, int num_occupied_grid_max, int n_a, int n_g,
                 int dim, bool *condition, bool *is_collide_b2b_input, bool *is_collide_b2w_input,
                 double *coefficients);
void _sf_b2b_all(double *p_input, double *sf_b2b_input, double *d_b2b_edge_input,
                 bool *is_collide_b2b_input, double *boundary_pos_input, double *d_b2b_center_input,
                 int n_a, int dim, double k_ball, bool is_periodic);
void _get_dist_b2w(double *p_input, double *r_input, double *d_b2w_input, bool *isCollision_input,
                   int dim, int n_a, double *boundary_pos);
void calculateActionPrior(double *p_input, double *dp_input, double *a_prior_input,
                          double *grid_center_input, int *neighbor_index_input, double d_sen,
                          double r_avoid, double l_cell, int topo_nei_max, int n_a, int n_g, int dim);

/* The legacy entry points return void like the reference's; after a call, its status on the calling thread: 0 = ok,
 * 1 = failed (outputs were filled with NaN, a line was written to stderr) and the reason (e.g. n_a > 256, no HIP device). */
int  swarm_legacy_status(void);
const char *swarm_legacy_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SWARM_ENV_H */
