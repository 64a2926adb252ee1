"""The device rollout loop (rollout_device -> swarm_rollout, include/swarm_rollout.h): K exploring-actor + env steps per
library call.  It must compute exactly what the Python fused loop (rollout() with FusedPolicy + ChainedReplay) computes, the
epsilon branch must follow the header's generator, the noise must be keyed by the global row, the reward statistics must be
exact, episode boundaries must not corrupt the ring, and a rejected call must leave everything as it was."""
import ctypes

import numpy as np
import pytest

from helpers import mix64, mix64_np, noise_key
from helpers import shape_batch as make_batch

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def uniform_actions(seed, step, rows, row_offset=0):
    """include/swarm_rollout.h 'Uniform actions', restated: [rows, 2] float32."""
    ukey = mix64(noise_key(seed, step) ^ 0x5851F42D4C957F2D)
    g = np.arange(rows, dtype=np.uint64) + np.uint64(row_offset)
    h = mix64_np(np.uint64(ukey) ^ g)
    out = np.empty((rows, 2), np.float32)
    for k in range(2):
        bits = (h >> np.uint64(40 - 24 * k)) & np.uint64(0xFFFFFF)
        out[:, k] = bits.astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    return out


@pytest.fixture(scope="module")
def policy():
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP
    torch.manual_seed(0)
    return FusedPolicy(PolicyMLP(192, 2, 180).cuda())


RING = ("obs", "act", "rew", "done", "act_prior")


def snapshot(ring):
    return {k: getattr(ring, k).clone() for k in RING}, ring.cur, ring.count


def same_ring(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in RING) and a.cur == b.cur and a.count == b.count


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("E,N", [(12, 32), (5, 64)])
def test_device_loop_equals_the_python_fused_loop(shapes, policy, E, N, dtype):
    from marl_llm_amd.rollout import ChainedReplay, rollout, rollout_device
    K, n = 3, E * N
    out = []
    for device_loop in (False, True):
        sb = make_batch(shapes, E, N, dtype)
        obs = sb.reset(seed=5)
        ring = ChainedReplay(K, n, sb.obs_dim, 2, sb.device, obs_dtype=dtype)
        if device_loop:                       # 7 > n_slots: the ring wraps; the second call continues the chain
            obs, _ = rollout_device(sb, policy, 4, obs=obs, replay=ring, noise_scale=0.1, seed=11, step0=100)
            obs, _ = rollout_device(sb, policy, 3, obs=obs, replay=ring, noise_scale=0.1, seed=11, step0=104)
        else:
            obs, _ = rollout(sb, policy, 7, obs, replay=ring, noise_scale=0.1, seed=11, step0=100)
        torch.cuda.synchronize()
        out.append((ring, obs.clone(), [x.clone() for x in sb.get_state()]))
        sb.close()
    (a, oa, sa), (b, ob, sbs) = out
    assert same_ring(a, b) and a.count == K
    assert torch.equal(oa, ob) and all(torch.equal(x, y) for x, y in zip(sa, sbs))
    assert torch.equal(b.obs[b.cur], ob.reshape(n, -1))


def test_epsilon_branch_follows_the_header_and_a_mirror_loop(shapes, policy):
    from marl_llm_amd.rollout import ChainedReplay, rollout_device
    E, N, steps, eps, seed, step0 = 6, 32, 8, 0.3, 21, 40
    n = E * N
    coins = [c < eps for c in np.random.RandomState(7).random_sample(steps)]
    assert any(coins) and not all(coins)
    sb = make_batch(shapes, E, N)
    obs = sb.reset(seed=9)
    ring = ChainedReplay(steps, n, sb.obs_dim, 2, sb.device)
    rng = np.random.RandomState(7)
    obs, _ = rollout_device(sb, policy, steps, obs=obs, replay=ring, noise_scale=0.2, epsilon=eps, host_rng=rng, seed=seed,
                            step0=step0, track_reward=False)
    ref = np.random.RandomState(7)
    ref.random_sample(steps)
    assert rng.random_sample() == ref.random_sample()          # exactly `steps` draws, like rollout()
    # mirror: FusedPolicy on policy steps, the restated uniform actions on coin steps, SwarmBatch.step
    mb = make_batch(shapes, E, N)
    o = mb.reset(seed=9)
    for t in range(steps):
        if coins[t]:
            act = torch.from_numpy(uniform_actions(seed, step0 + t, n)).to(mb.device)
            assert torch.equal(ring.act[t], act), t
        else:
            act = policy(o.reshape(n, -1), noise_scale=0.2, seed=seed, step=step0 + t)
        assert torch.equal(ring.obs[t], o.reshape(n, -1)) and torch.equal(ring.act[t], act), t
        o, rew, done, pri = mb.step(act.view(E, N, 2))
        assert torch.equal(ring.rew[t].view(E, N), rew) and torch.equal(ring.act_prior[t].view(E, N, 2), pri), t
    assert torch.equal(obs, o)
    assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), mb.get_state()))
    u = ring.act[[t for t in range(steps) if coins[t]]]
    assert u.min() >= -1 and u.max() < 1
    sb.close(); mb.close()


def test_row_offset_keys_the_noise_by_global_row(policy):
    lib, rows, D = policy.lib, 1000, 192
    torch.manual_seed(3)
    x = torch.randn(rows, D, device=policy.device)
    stream = torch.cuda.current_stream(policy.device).cuda_stream

    def at(xs, off, scale=0.3):
        y = torch.empty((xs.shape[0], 2), device=policy.device)
        assert lib.swarm_policy_forward_explore_at(policy.handle, xs.data_ptr(), 0, xs.shape[0], y.data_ptr(), scale, 5, 9, off,
                                                   stream) == 0
        return y

    full = at(x, 0)
    halves = torch.cat([at(x[: rows // 2], 0), at(x[rows // 2:], rows // 2)])
    assert torch.equal(full, halves)
    assert torch.equal(full, policy(x, noise_scale=0.3, seed=5, step=9))        # swarm_policy_forward_explore = offset 0
    shifted = at(x, 12345)
    assert not torch.equal(full, shifted) and (full != shifted).float().mean() > 0.5
    assert torch.equal(at(x, 12345, 0.0), at(x, 0, 0.0))                        # no noise: the offset is irrelevant


@pytest.mark.parametrize("E,N", [(48, 64), (5, 31)])
def test_reward_stats_are_exact_and_deterministic(shapes, policy, E, N):
    from marl_llm_amd.rollout import ChainedReplay, rollout, rollout_device
    steps, n = 6, E * N
    runs = []
    for _ in range(2):
        sb = make_batch(shapes, E, N)
        obs = sb.reset(seed=4)
        ring = ChainedReplay(steps, n, sb.obs_dim, 2, sb.device)
        _, st = rollout_device(sb, policy, steps, obs=obs, replay=ring, noise_scale=0.3, seed=2)
        runs.append((ring, st.cpu().numpy()))
        sb.close()
    (ring, st), (_, st2) = runs
    assert st.shape == (steps, 2) and st.dtype == np.float64
    assert np.array_equal(st, st2)
    for t in range(steps):
        r = ring.rew[t].double().flatten()
        assert st[t, 0] == r.sum().item() / r.numel()                          # count / rows, correctly rounded
        ref = np.std(r.cpu().numpy())
        assert abs(st[t, 1] - ref) <= 1e-12 * max(ref, 1e-300)
    sb = make_batch(shapes, E, N)
    obs = sb.reset(seed=4)
    _, rews = rollout(sb, policy, steps, obs, replay=ChainedReplay(steps, n, sb.obs_dim, 2, sb.device), noise_scale=0.3, seed=2)
    np.testing.assert_allclose(rews.cpu().numpy(), st[:, 0], rtol=0, atol=1e-6)
    sb.close()


def test_episode_boundary_keeps_the_last_transition(shapes, policy):
    from marl_llm_amd.rollout import ChainedReplay, DeviceReplay, rollout_device
    E, N, K = 6, 32, 12
    n = E * N
    sb = make_batch(shapes, E, N)
    ring = ChainedReplay(K, n, sb.obs_dim, 2, sb.device)
    rollout_device(sb, policy, 5, reset=(3, 0), replay=ring, noise_scale=0.1, seed=1)
    rollout_device(sb, policy, 4, reset=(3, 1), replay=ring, noise_scale=0.1, seed=1, step0=5)
    # the same trajectory through push()
    mb = make_batch(shapes, E, N)
    flat = DeviceReplay(9 * n, sb.obs_dim, 2, sb.device)
    t = 0
    for ep, k in ((0, 5), (1, 4)):
        o = mb.reset(3, ep).clone()
        for _ in range(k):
            a = policy(o.reshape(n, -1), noise_scale=0.1, seed=1, step=t).view(E, N, 2)
            nx, r, d, p = mb.step(a)
            flat.push(o, a, r, nx, d, p)
            o, t = nx.clone(), t + 1
    assert ring.cur == 10 and ring.count == 10 and len(ring) == 9 * n      # slot 5 sealed
    for k, slot in enumerate([0, 1, 2, 3, 4, 6, 7, 8, 9]):
        s = slice(k * n, (k + 1) * n)
        assert torch.equal(ring.obs[slot], flat.obs[s]) and torch.equal(ring.obs[slot + 1], flat.next_obs[s]), k
        assert torch.equal(ring.act[slot], flat.act[s]) and torch.equal(ring.rew[slot], flat.rew[s]), k
        assert torch.equal(ring.act_prior[slot], flat.act_prior[s]), k
    assert not torch.equal(ring.obs[5], ring.obs[6])          # episode 1's true last next_obs, not episode 2's reset obs
    # sampled (obs, next_obs) pairs are always transitions of the trajectory
    pairs = {(a.tobytes(), b.tobytes()) for a, b in zip(flat.obs.cpu().numpy(), flat.next_obs.cpu().numpy())}
    g = torch.Generator(device=sb.device).manual_seed(0)
    o, a, r, no, d, pr = ring.sample(10000, generator=g)
    o, no = o.cpu().numpy(), no.cpu().numpy()
    assert all((x.tobytes(), y.tobytes()) in pairs for x, y in zip(o, no))
    # a fresh obs tensor without reset= seals and copies as well
    fresh = sb.reset(3, 2)
    sealed_before = ring.obs[ring.cur].clone()
    start = ring.cur
    obs, _ = rollout_device(sb, policy, 2, obs=fresh, replay=ring, noise_scale=0.1, seed=1, step0=9)
    assert ring.cur == (start + 3) % ring.S
    assert torch.equal(ring.obs[start], sealed_before) and torch.equal(ring.obs[(start + 1) % ring.S], fresh.reshape(n, -1))
    assert len(ring) == 10 * n                                # 12 slots behind cur, two of them sealed
    sb.close(); mb.close()


def test_rejected_calls_enqueue_nothing(shapes, policy):
    from marl_llm_amd import _lib
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.rollout import ChainedReplay, FusedPolicy, PolicyMLP, rollout_device
    from marl_llm_amd.shapes import r_avoid_for
    E, N = 4, 32
    n = E * N
    sb = make_batch(shapes, E, N)
    obs = sb.reset(seed=1)

    def rejected(env, pol, ring, obs, match):
        before, cur, count = snapshot(ring)
        with pytest.raises(_lib.SwarmError, match=match):
            rollout_device(env, pol, 3, obs=obs, replay=ring, noise_scale=0.1)
        torch.cuda.synchronize()
        assert all(torch.equal(getattr(ring, k), v) for k, v in before.items()) and (ring.cur, ring.count) == (cur, count)

    rejected(sb, policy, ChainedReplay(2, n + 1, sb.obs_dim, 2, sb.device), obs, "ring rows")
    torch.manual_seed(0)
    rejected(sb, FusedPolicy(PolicyMLP(96, 2, 180).cuda()), ChainedReplay(2, n, sb.obs_dim, 2, sb.device), obs, "policy in_dim")
    rejected(sb, policy, ChainedReplay(0, n, sb.obs_dim, 2, sb.device), obs, "n_slots")
    sb64 = make_batch(shapes, E, N, torch.float64)
    o64 = sb64.reset(seed=1)
    rejected(sb64, policy, ChainedReplay(2, n, sb.obs_dim, 2, sb.device, obs_dtype=torch.float64), o64, "obs dtype")
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    fresh = SwarmBatch(n_env=E, n_agents=N, n_cells_max=ng_max, r_avoid=r_avoid_for(N, shapes))       # never observed
    rejected(fresh, policy, ChainedReplay(2, n, sb.obs_dim, 2, sb.device), torch.zeros_like(obs), "not observed")
    # a ring without prior on a with_prior handle (the Python layer always passes it, so through the C ABI)
    ring = ChainedReplay(2, n, sb.obs_dim, 2, sb.device)
    before, _, _ = snapshot(ring)
    r = _lib.SwarmRing(ring.obs.data_ptr(), ring.act.data_ptr(), ring.rew.data_ptr(), ring.done.data_ptr(), None, n, sb.obs_dim,
                       _lib.F32, ring.S, 0)
    lib = policy.lib
    rc = lib.swarm_rollout(sb.handle, policy.handle, ctypes.byref(r), 3, None, 0.1, 0, 0, 0, None,
                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 1 and b"ring prior is NULL" in lib.swarm_rollout_last_error()
    assert all(torch.equal(getattr(ring, k), v) for k, v in before.items())
    # the env still works after all of that
    _, st = rollout_device(sb, policy, 2, obs=obs, noise_scale=0.1)
    assert st.shape == (2, 2)
    for b in (sb, sb64, fresh):
        b.close()


def test_assembly_env_metrics_follow_the_device_loop(shapes, policy):
    from marl_llm_amd.env import AssemblySwarmEnv, make_args
    from marl_llm_amd.rollout import rollout_device
    env = AssemblySwarmEnv(n_envs=4, obs_dtype="float32", rng="device", seed=77)
    env.__reinit__(make_args(n_a=16, results_file=shapes))
    obs = env.reset_tensor()
    m0 = env.metrics_tensor().clone()
    obs, st = rollout_device(env, policy, 5, obs=obs, noise_scale=0.5, seed=3)
    m1 = env.metrics_tensor()
    fresh = env._backend().metrics()
    assert torch.equal(m1, fresh) and not torch.equal(m1, m0)
    assert abs(env.simulation_time - 5 * env.dt) < 1e-12 and obs.shape == (4, 16, 192)
    env.close()
