"""Log-probabilities of the exploring actions (the log_pi of agents.py:78-96 that AIRL subtracts from its discriminator),
host side: ChainedReplay's log-pi column and sample(is_log_pi=True), rollout(log_pi=True) on a torch module, and the C ABI
of swarm_policy_forward_explore_logpi / swarm_rollout_logpi rejecting bad calls before they reach a device."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _ring(K=4, n=6, log_pi=True):
    from marl_llm_amd.rollout import ChainedReplay
    return ChainedReplay(K, n, 3, 2, "cpu", log_pi=log_pi)


def _push(ring, step, n):
    """One step whose act[:, 0] and log-pi both encode (step, row): 1000 * step + row."""
    code = torch.arange(n, dtype=torch.float32) + 1000.0 * step
    obs = torch.full((1, n, 3), float(step)); nxt = torch.full((1, n, 3), float(step + 1))
    act = torch.stack([code, -code], -1).reshape(1, n, 2)
    ring.push(obs, act, torch.zeros(1, n), nxt, torch.zeros(1, n, dtype=torch.uint8), log_pi=(-code).reshape(1, n))


def _check_pairs(sample):
    obs, act, rew, nxt, done, pri, lp = sample
    assert lp.shape == (obs.shape[0], 1) and lp.dtype == torch.float32
    assert torch.equal(lp[:, 0], -act[:, 0])                           # same transition: same (step, row)
    assert torch.equal(obs[:, 0], torch.floor(act[:, 0] / 1000.0))    # and the obs of that step


def test_sample_returns_the_log_pi_of_the_same_transition():
    n = 6
    ring = _ring(4, n)
    for s in range(7):                                                 # wraps: only steps 3..6 remain
        _push(ring, s, n)
    g = torch.Generator().manual_seed(3)
    smp = ring.sample(512, generator=g, is_log_pi=True)
    assert len(smp) == 7
    _check_pairs(smp)
    steps = set(torch.floor(smp[1][:, 0] / 1000.0).int().tolist())
    assert steps == {3, 4, 5, 6}


def test_log_pi_across_a_sealed_chain():
    n = 5
    ring = _ring(6, n)
    for s in range(3):
        _push(ring, s, n)
    ring.new_chain(torch.full((1, n, 3), 10.0))                        # the boundary slot is sealed
    for s in range(10, 12):
        _push(ring, s, n)
    smp = ring.sample(1024, generator=torch.Generator().manual_seed(0), is_log_pi=True)
    _check_pairs(smp)
    steps = set(torch.floor(smp[1][:, 0] / 1000.0).int().tolist())
    assert steps == {0, 1, 2, 10, 11}                                  # never the sealed slot
    assert len(ring) == 5 * n


def test_default_sample_is_the_six_tuple_with_the_same_draws():
    n = 4
    a, b = _ring(3, n, log_pi=True), _ring(3, n, log_pi=False)
    for s in range(5):
        _push(a, s, n)
        code = torch.arange(n, dtype=torch.float32) + 1000.0 * s
        b.push(torch.full((1, n, 3), float(s)), torch.stack([code, -code], -1).reshape(1, n, 2), torch.zeros(1, n),
               torch.full((1, n, 3), float(s + 1)), torch.zeros(1, n, dtype=torch.uint8))
    six_a = a.sample(64, generator=torch.Generator().manual_seed(9))
    six_b = b.sample(64, generator=torch.Generator().manual_seed(9))
    seven = a.sample(64, generator=torch.Generator().manual_seed(9), is_log_pi=True)
    assert len(six_a) == 6 and len(six_b) == 6
    for x, y, z in zip(six_a, six_b, seven[:6]):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_log_pi_needs_the_column():
    ring = _ring(2, 3, log_pi=False)
    assert ring.log_pi is None
    with pytest.raises(ValueError):
        _push(ring, 0, 3)
    ring.push(torch.zeros(1, 3, 3), torch.zeros(1, 3, 2), torch.zeros(1, 3), torch.zeros(1, 3, 3), torch.zeros(1, 3))
    with pytest.raises(ValueError):
        ring.sample(4, is_log_pi=True)
    with pytest.raises(ValueError):                                    # bad shape: not one value per row
        _ring(2, 3).push(torch.zeros(1, 3, 3), torch.zeros(1, 3, 2), torch.zeros(1, 3), torch.zeros(1, 3, 3), torch.zeros(1, 3),
                         log_pi=torch.zeros(2))


class _ToyEnv:
    """A deterministic stand-in env with step_tensor (rollout()'s eager path), on the CPU."""

    def __init__(self, E, N, D):
        self.E, self.N, self.D, self.t = E, N, D, 0

    def step_tensor(self, act):
        self.t += 1
        obs = torch.full((self.E, self.N, self.D), float(self.t)) + act[..., :1]
        return obs, (act[..., 0] > 0).float(), torch.zeros(self.E, self.N), None


def _reference_log_prob(noise, scale):
    """utils/noise.py GaussianNoise.log_prob, float64."""
    act_dim = noise.shape[1]
    lp = -0.5 * ((noise / scale) ** 2).sum(axis=-1)
    lp -= act_dim * np.log(scale * np.sqrt(2 * np.pi))
    return lp


@pytest.mark.parametrize("scale", [0.125, 0.3, 1.7])
def test_rollout_records_the_torch_noise_log_pi_and_the_coin_constant(scale):
    from marl_llm_amd.rollout import LOG_PI_UNIFORM, ChainedReplay, PolicyMLP, rollout
    E, N, D, T = 2, 5, 8, 6
    torch.manual_seed(1)
    pol = PolicyMLP(D, 2, 16)
    ring = ChainedReplay(T, E * N, D, 2, "cpu", log_pi=True)
    gen = torch.Generator().manual_seed(4)
    coins = np.random.RandomState(2)
    rollout(_ToyEnv(E, N, D), pol, T, torch.zeros(E, N, D), replay=ring, noise_scale=scale, epsilon=0.4, generator=gen,
            host_rng=coins, log_pi=True)
    # replay the draws: the coins, then per policy step the module output and its normals
    coins, gen, env = np.random.RandomState(2), torch.Generator().manual_seed(4), _ToyEnv(E, N, D)
    obs = torch.zeros(E, N, D)
    n_coin = n_pol = 0
    s32 = float(np.float32(scale))
    for t in range(T):
        lp = ring.log_pi[t, :, 0]
        if coins.random() < 0.4:
            act = torch.rand((E * N, 2), generator=gen) * 2 - 1
            assert LOG_PI_UNIFORM == float(np.float32(-2 * math.log(2)))
            assert (lp == LOG_PI_UNIFORM).all()
            n_coin += 1
        else:
            a0 = pol(obs.reshape(E * N, D))
            z = torch.randn(a0.shape, generator=gen)
            act = (a0 + scale * z).clamp(-1, 1)
            zn = z.numpy()
            s = zn[:, 0] * zn[:, 0] + zn[:, 1] * zn[:, 1]                  # fp32, k order (numpy restatement)
            c = np.float32(2 * math.log(s32 * math.sqrt(2 * math.pi)))
            assert np.array_equal(lp.numpy(), -(np.float32(0.5) * s) - c)
            ref = _reference_log_prob(s32 * zn.astype(np.float64), s32)
            assert np.abs(lp.numpy() - ref).max() < 1e-4 * (1 + np.abs(ref).max())
            n_pol += 1
        assert torch.equal(ring.act[t], act)
        obs, _, _, _ = env.step_tensor(act.reshape(E, N, 2))
    assert n_coin and n_pol


def test_rollout_without_noise_records_minus_zero():
    from marl_llm_amd.rollout import ChainedReplay, PolicyMLP, rollout
    ring = ChainedReplay(2, 4, 8, 2, "cpu", log_pi=True)
    ring.log_pi.fill_(7.0)
    rollout(_ToyEnv(1, 4, 8), PolicyMLP(8, 2, 16), 2, torch.zeros(1, 4, 8), replay=ring, log_pi=True)
    lp = ring.log_pi[:2].flatten()
    assert (lp == 0).all() and torch.signbit(lp).all()


def test_rollout_log_pi_needs_a_chained_ring_with_the_column():
    from marl_llm_amd.rollout import ChainedReplay, DeviceReplay, PolicyMLP, rollout
    pol, env, obs = PolicyMLP(8, 2, 16), _ToyEnv(1, 4, 8), torch.zeros(1, 4, 8)
    for replay in (None, DeviceReplay(16, 8, 2, "cpu"), ChainedReplay(2, 4, 8, 2, "cpu")):
        with pytest.raises(ValueError):
            rollout(env, pol, 1, obs, replay=replay, log_pi=True)
    assert env.t == 0                                                  # raised before any step


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def test_new_symbols_are_bound(lib):
    from marl_llm_amd._lib import POLICY_SYMBOLS, ROLLOUT_SYMBOLS
    assert "swarm_policy_forward_explore_logpi" in POLICY_SYMBOLS and "swarm_rollout_logpi" in ROLLOUT_SYMBOLS
    f = lib.swarm_policy_forward_explore_logpi
    assert len(f.argtypes) == 11 and f.argtypes[6] is ctypes.c_float and f.argtypes[9] is ctypes.c_uint64
    g = lib.swarm_rollout_logpi
    assert len(g.argtypes) == 12 and g.argtypes[4] is ctypes.c_int32 and g.argtypes[6] is ctypes.c_float


def test_policy_logpi_rejects_bad_calls_with_a_message(lib):
    f = lib.swarm_policy_forward_explore_logpi
    fake = ctypes.c_void_p(8)                                          # never dereferenced: the argument checks come first
    assert f(fake, fake, 0, 4, fake, None, 0.1, 0, 0, 0, None) == 1    # SWARM_POLICY_ERR_INVALID
    assert b"null log_pi" in lib.swarm_policy_last_error()
    assert f(None, None, 0, 0, None, fake, 0.1, 0, 0, 0, None) == 1
    assert b"bad argument" in lib.swarm_policy_last_error()
    assert f(fake, fake, 0, -1, fake, fake, 0.1, 0, 0, 0, None) == 1   # rows < 0
    assert b"bad argument" in lib.swarm_policy_last_error()


def test_rollout_logpi_rejects_bad_calls_with_a_message(lib):
    from marl_llm_amd._lib import SwarmRing
    ring = SwarmRing()
    ring.n_slots, ring.rows = 2, 1
    tail = (1, None, 0.0, 0, 0, 0, None, None)
    fake = ctypes.c_void_p(8)
    assert lib.swarm_rollout_logpi(None, None, ctypes.byref(ring), fake, *tail) == 1
    assert lib.swarm_rollout_last_error() == b"swarm_rollout_logpi: null env, policy or ring"
    assert lib.swarm_rollout_logpi(fake, fake, ctypes.byref(ring), None, *tail) == 1
    assert lib.swarm_rollout_last_error().startswith(b"swarm_rollout_logpi: null log_pi")
    assert lib.swarm_rollout_logpi(fake, fake, None, fake, *tail) == 1
    assert b"null env, policy or ring" in lib.swarm_rollout_last_error()
