"""Inputs of the per-env reset tests (test_reset_envs_host.py checks their conditions on the CPU, test_gpu_reset_envs.py and
test_gpu_rollout_resets.py run them): a shape set that holds lattice and off-lattice shapes together, seeds, and episode
vectors (-1 = keep) in which kept and reset envs share a step-kernel workgroup, the reset envs draw both kinds of shape and
at least two episode numbers occur.  The shape a reset draws is the generator's first draw (k_reset's slot 0), restated here
as in tests/test_gpu_reset_rollout.py, so the conditions are decided without a device."""
import numpy as np

from helpers import GOLD, mix64

OFF_LATTICE = (2,)                  # shape indices of mixed_shape_set() that are no lattice subset


def mixed_shape_set():
    """Two tiled shapes and a jittered copy of a third (shape index 2), as tests/test_gpu_mixed_paths.py builds it."""
    from marl_llm_amd.shapes import SHAPE_NAMES, synthetic_shape_set
    s = synthetic_shape_set(SHAPE_NAMES[:3])
    g = np.asarray(s["grid_coords"][2], np.float64)
    s["grid_coords"][2] = g + np.random.default_rng(12).normal(0, 0.004, g.shape)
    return s


def u01(key, k):
    return float(mix64(key + GOLD * (k + 1)) >> 11) * (1.0 / 9007199254740992.0)


def drawn_shape(seed, episode, env_id, n_shapes=3):
    key = mix64(mix64(seed + GOLD * (episode + 1)) ^ env_id)
    return min(int(u01(key, 0) * n_shapes), n_shapes - 1)


def envs_per_workgroup(n_a):
    npad = 8
    while npad < n_a:
        npad *= 2
    return 64 // npad if npad < 64 else 1


def episode_vector(n_env, phase=0):
    """Kept envs (-1) between envs that start episode 2, 5 or 7; phase shifts the pattern."""
    pattern = (-1, 2, 5, -1, 7, 2)
    return np.array([pattern[(e + phase) % len(pattern)] for e in range(n_env)], np.int64)


def conditions(seed, vector, n_a, env_offset=0):
    """What an episode vector is for, as named booleans."""
    vector = np.asarray(vector)
    epb = envs_per_workgroup(n_a)
    took = vector >= 0
    shapes = {drawn_shape(seed, int(ep), env_offset + e) for e, ep in enumerate(vector) if ep >= 0}
    groups = [took[b:b + epb] for b in range(0, len(vector), epb)]
    return {
        "kept and reset envs": bool(took.any() and not took.all()),
        "kept and reset envs inside one workgroup": epb == 1 or any(g.any() and not g.all() for g in groups),
        "two distinct shapes": len(shapes) >= 2,
        "a lattice and an off-lattice shape": bool(shapes & set(OFF_LATTICE)) and bool(shapes - set(OFF_LATTICE)),
        "two distinct episode numbers": len(set(vector[took].tolist())) >= 2,
    }


# test_gpu_reset_envs.py: (n_agents, n_env, large_swarm) -> seed; the vector is episode_vector(n_env)
EQUALITY = {(8, 17, False): 1, (30, 6, False): 1, (64, 9, False): 1, (256, 3, False): 1, (300, 3, True): 1}

# test_gpu_rollout_resets.py: (n_agents, n_env) -> seed; per-env resets at steps 3 and 6 (phases 0 and 1), whole-batch ones at 0 and 5
ROLLOUT = {(8, 16): 1, (64, 8): 1, (300, 2): 1}
ROLLOUT_STEPS = 8


def rollout_schedule(seed, n_env):
    return {0: (seed, 0), 3: (seed, episode_vector(n_env, 0)), 5: (seed, 4), 6: (seed, episode_vector(n_env, 1))}


def large_schedule(seed, n_env):
    """300 agents x 2 envs, 4 steps, one cut: env 1 starts episode 5 at step 2"""
    return {0: (seed, 0), 2: (seed, np.array([-1, 5][:n_env], np.int64))}
