"""include/swarm_rollout.h "Per-env exploration", restated in numpy: the coin of (seed, step, global env), the uniform actions
of a coin env's rows, the log-pi constants, and the composition -- which rows of a step take which branch.  The Gaussian
branch itself is not restated here (its logf / sincosf are the device's): the GPU tests take it from the scalar forward."""
import math

import numpy as np

from helpers import mix64, mix64_np, noise_key

COIN_SALT = 0xA0761D6478BD642F
UNIFORM_SALT = 0x5851F42D4C957F2D
LOG_PI_UNIFORM = np.float32(-2.0 * math.log(2.0))


def coin_hash(seed, step, ge):
    """h of the header's coin for global envs `ge` (an int or an int array): uint64."""
    ckey = mix64(noise_key(seed, step) ^ COIN_SALT)
    return mix64_np(np.uint64(ckey) ^ np.asarray(ge).astype(np.uint64))


def uniform_hash(seed, step, g):
    """h of the header's uniform action for global rows `g`: uint64."""
    ukey = mix64(noise_key(seed, step) ^ UNIFORM_SALT)
    return mix64_np(np.uint64(ukey) ^ np.asarray(g).astype(np.uint64))


def coin_uniforms(seed, step, n_env, env_offset=0):
    """u [n_env] float32 in [0, 1): (float)(h >> 40) * 2^-24, exact."""
    h = coin_hash(seed, step, np.arange(n_env, dtype=np.uint64) + np.uint64(env_offset))
    return (h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def coins(seed, step, epsilon, env_offset=0):
    """coin [E] uint8 of one step: u < epsilon[e] as an fp32 compare (NaN and <= 0 never fire, >= 1 always)."""
    eps = np.asarray(epsilon, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (coin_uniforms(seed, step, eps.shape[0], env_offset) < eps).astype(np.uint8)


def coin_table(seed, step0, steps, epsilon, env_offset=0):
    """coin [steps, E] uint8: what coin_out receives."""
    return np.stack([coins(seed, step0 + t, epsilon, env_offset) for t in range(steps)])


def uniform_actions(seed, step, rows, row_offset=0):
    """'Uniform actions' of global rows row_offset + [0, rows): [rows, 2] float32 in [-1, 1)."""
    h = uniform_hash(seed, step, np.arange(rows, dtype=np.uint64) + np.uint64(row_offset))
    out = np.empty((rows, 2), np.float32)
    for k in range(2):
        bits = (h >> np.uint64(40 - 24 * k)) & np.uint64(0xFFFFFF)
        out[:, k] = bits.astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    return out


def log_c(sigma, act_dim=2):
    """The header's expression per env: (float)((double)act_dim * log((double)sigma * sqrt(2 pi))) for an fp32 sigma > 0."""
    s = np.asarray(sigma, dtype=np.float32)
    return np.array([np.float32(act_dim * math.log(float(v) * math.sqrt(2.0 * math.pi))) if v > 0 else np.float32(0) for v in s],
                    dtype=np.float32)


COIN, NOISE, PLAIN = 0, 1, 2


def branches(seed, step, n_agents, epsilon, sigma, row_offset=0):
    """The composition of one step: (coin [E] uint8, branch [E * n_agents] of COIN / NOISE / PLAIN).  A coin env's rows take
    the uniform actions; another env's take the Gaussian noise if sigma[e] > 0 and stay as the actor wrote them otherwise."""
    assert row_offset % n_agents == 0
    sigma = np.asarray(sigma, dtype=np.float32)
    c = coins(seed, step, epsilon, row_offset // n_agents)
    with np.errstate(invalid="ignore"):
        env = np.where(c == 1, COIN, np.where(sigma > 0, NOISE, PLAIN))
    return c, np.repeat(env, n_agents)
