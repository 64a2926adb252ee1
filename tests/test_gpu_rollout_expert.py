"""Expert rollouts on the device (rollout_expert -> swarm_rollout_expert, include/swarm_rollout.h) and their export
(save_expert_data).  The fused loop must compute, bit for bit, what the eager loop `u = rule_action(); step(u)` (or the
'llm' loop `step(None)`) computes; the rule expert must stay within test_gpu_rule.py's tolerance of the numpy
restatement; chains, reward statistics, rejections and the reference-shaped AssemblySwarmEnv path are covered."""
import numpy as np
import pytest

from helpers import shape_batch as make_batch

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-12                 # test_gpu_rule.py
RING = ("obs", "act", "rew", "done", "act_prior")


def ring_for(sb, K):
    from marl_llm_amd.rollout import ChainedReplay
    return ChainedReplay(K, sb.n_env * sb.n_agents, sb.obs_dim, 2, sb.device, obs_dtype=sb.obs_dtype)


def eager_matches(shapes, E, N, dtype, K, ring, source="rule", seed=11, episode=0, **kw):
    """Drive a twin batch eagerly from the same reset and compare every step with the ring's slots 0..K (bitwise)."""
    sb = make_batch(shapes, E, N, dtype, **kw)
    obs = sb.reset(seed, episode)
    assert torch.equal(ring.obs[0].view_as(obs), obs)
    n = E * N
    for t in range(K):
        if source == "rule":
            u = sb.rule_action()
            obs, rew, done, pri = sb.step(u)
        else:
            u = sb.llm_action()
            obs, rew, done, pri = sb.step(None)
        assert torch.equal(ring.act[t], u.float().view(n, 2)), t
        assert torch.equal(ring.obs[t + 1], obs.view(n, -1)), t
        assert torch.equal(ring.rew[t], rew.view(n, 1)), t
        assert torch.equal(ring.done[t], done.view(n, 1)), t
        if pri is not None:
            assert torch.equal(ring.act_prior[t], pri.view(n, 2)), t
    return sb


CONFIGS = [(30, 16, {}), (64, 64, {}), (64, 64, {"debug_flags": 2}), (128, 8, {}), (256, 4, {})]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,E,kw", CONFIGS, ids=["30x16", "64x64", "64x64_generic", "128x8", "256x4"])
def test_fused_rule_equals_eager_loop(shapes, N, E, kw, dtype):
    from marl_llm_amd.rollout import rollout_expert
    K = 50
    sb = make_batch(shapes, E, N, dtype, **kw)
    if kw.get("debug_flags", 0) & 2:
        sb.reset(11, 0)
        assert sb.lattice_envs() == 0
    ring = ring_for(sb, K)
    obs, stats = rollout_expert(sb, K, replay=ring, reset=(11, 0))
    assert ring.cur == K and obs.data_ptr() == ring.obs[K].data_ptr()
    twin = eager_matches(shapes, E, N, dtype, K, ring, **kw)
    for a, b in zip(sb.get_state(), twin.get_state()):
        assert torch.equal(a, b)
    # reward statistics: (mean, population std) of every step's rewards
    r = ring.rew[:K, :, 0].double()
    assert torch.equal(stats[:, 0], r.sum(1) / r.shape[1])
    assert torch.allclose(stats[:, 1], r.std(1, unbiased=False), rtol=1e-12, atol=0)


def test_rule_expert_matches_the_oracle_teacher_forced(shapes):
    """At steps 0, K/2 and K-1 of a fused run (three chained calls), the numpy restatement on the GPU's state agrees with
    the eager fp64 action within 1e-12, and the ring's f32 row is that action's rounding."""
    from marl_llm_amd.rollout import rollout_expert
    from oracle.oracle_py import rule_action
    E, N, K = 16, 30, 50
    sb, twin = make_batch(shapes, E, N), make_batch(shapes, E, N)
    ring = ring_for(sb, K)
    rollout_expert(sb, 0, replay=ring, reset=(7, 3))
    twin.reset(7, 3)
    cells, n_g = sb.get_cells()
    l_cell = np.asarray(shapes["l_cell"], np.float64)[sb.get_shape_index()]
    envs = np.random.default_rng(0).choice(E, 8, replace=False)
    done = 0
    for t_check in (0, K // 2, K - 1):
        if t_check > done:
            rollout_expert(sb, t_check - done, replay=ring)
            for _ in range(t_check - done):
                twin.step(twin.rule_action())
            done = t_check
        p, dp = [x.cpu().numpy() for x in sb.get_state()]
        for a, b in zip(sb.get_state(), twin.get_state()):
            assert torch.equal(a, b)
        u = twin.rule_action().cpu().numpy()
        rollout_expert(sb, 1, replay=ring)
        twin.step(twin.rule_action())
        done += 1
        act = ring.act[t_check].view(E, N, 2).cpu().numpy()
        assert np.array_equal(act, u.astype(np.float32))
        for e in envs:
            want = rule_action(p[e], dp[e], np.ascontiguousarray(cells[e][:, : n_g[e]]), float(l_cell[e]), sb_r_avoid(sb))
            assert np.abs(u[e].T - want).max() <= TOL, (t_check, e)


def sb_r_avoid(sb):
    return float(sb.cfg.r_avoid)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_llm_source_equals_eager_loop(shapes, dtype):
    from marl_llm_amd.rollout import rollout_expert
    E, N, K = 16, 30, 50
    sb = make_batch(shapes, E, N, dtype, llm_action=True)
    ring = ring_for(sb, K)
    rollout_expert(sb, K, replay=ring, reset=(11, 0), source="llm")
    twin = eager_matches(shapes, E, N, dtype, K, ring, source="llm", llm_action=True)
    for a, b in zip(sb.get_state(), twin.get_state()):
        assert torch.equal(a, b)


def test_chains_and_episode_boundaries(shapes, tmp_path):
    from marl_llm_amd.rollout import rollout_expert, save_expert_data
    E, N, K = 8, 32, 10
    one, two = make_batch(shapes, E, N), make_batch(shapes, E, N)
    r1, r2 = ring_for(one, 3 * K + 1), ring_for(two, 3 * K + 1)    # 3 K transitions + the sealed slot
    _, s1 = rollout_expert(one, 2 * K, replay=r1, reset=(5, 0))
    rollout_expert(two, K, replay=r2, reset=(5, 0))
    _, s2 = rollout_expert(two, K, replay=r2)
    assert all(torch.equal(getattr(r1, k), getattr(r2, k)) for k in RING) and r1.cur == r2.cur == 2 * K
    assert torch.equal(s1[K:], s2)
    # a second episode through reset=: the slot holding the first episode's last next_obs is sealed, not overwritten
    rollout_expert(two, K, replay=r2, reset=(5, 1))
    assert r2._sealed == {2 * K} and r2.cur == 3 * K + 1
    n = E * N
    z = np.load(save_expert_data(r2, str(tmp_path)))
    assert z["obs_buffs"].shape == (3 * K * n, two.obs_dim)
    last = slice((2 * K - 1) * n, 2 * K * n)
    first = slice(2 * K * n, (2 * K + 1) * n)
    assert np.array_equal(z["next_obs_buffs"][last], r2.obs[2 * K].double().cpu().numpy())
    assert np.array_equal(z["obs_buffs"][first], r2.obs[2 * K + 1].double().cpu().numpy())
    assert not np.array_equal(z["next_obs_buffs"][last], z["obs_buffs"][first])
    # every exported transition is a true one: next_obs of step t is obs of step t + 1 within each episode
    for ep in (range(0, 2 * K - 1), range(2 * K, 3 * K - 1)):
        for t in ep:
            assert np.array_equal(z["next_obs_buffs"][t * n:(t + 1) * n], z["obs_buffs"][(t + 1) * n:(t + 2) * n])


def _untouched(ring, snap, sb, state):
    assert all(torch.equal(getattr(ring, k), snap[k]) for k in RING)
    if sb is not None:
        for a, b in zip(sb.get_state(), state):
            assert torch.equal(a, b)


def test_rejections_leave_ring_and_state_untouched(shapes):
    from marl_llm_amd._lib import SwarmError
    from marl_llm_amd.env import AssemblySwarmEnv, AssemblySwarmWrapper, make_args
    from marl_llm_amd.rollout import rollout_expert
    E, N = 4, 30

    def attempt(sb, ring, exc, **kw):
        obs = sb.reset(2, 0)
        state = sb.get_state()
        ring.obs[ring.cur].copy_(obs.view(ring.n, -1)); ring._chained = True
        snap = {k: getattr(ring, k).clone() for k in RING}
        keep = (ring.cur, ring.count, set(ring._sealed))
        with pytest.raises(exc):
            rollout_expert(sb, 5, replay=ring, **kw)
        _untouched(ring, snap, sb, state)
        assert (ring.cur, ring.count, set(ring._sealed)) == keep

    sb = make_batch(shapes, E, N, torch.float64)                       # fp64 observation rows
    attempt(sb, ring_for(sb, 4), SwarmError)
    sb = make_batch(shapes, E, N, g_max=130)                           # the rule expert's list cap
    attempt(sb, ring_for(sb, 4), SwarmError)
    sb = make_batch(shapes, E, N)                                      # llm source without llm_action
    attempt(sb, ring_for(sb, 4), SwarmError, source="llm")
    # not observed: cells and state set, no observation pass yet
    sb = make_batch(shapes, E, N)
    ring = ring_for(sb, 4)
    snap = {k: getattr(ring, k).clone() for k in RING}
    with pytest.raises(SwarmError, match="not observed"):
        rollout_expert(sb, 5, replay=ring, obs=torch.zeros((E, N, sb.obs_dim), device=sb.device))
    _untouched(ring, snap, None, None)
    assert ring.count == 0 and not ring._chained
    # an AssemblySwarmEnv that is not in rule mode
    np.random.seed(1)
    env = AssemblySwarmWrapper(AssemblySwarmEnv(obs_dtype="float32"),
                               make_args(n_a=N, results_file=shapes, agent_strategy="input")).env
    obs = env.reset_tensor()
    state = env._backend().get_state()
    ring = ring_for(env._backend(), 4)
    snap = {k: getattr(ring, k).clone() for k in RING}
    with pytest.raises(ValueError, match="agent_strategy 'rule'"):
        rollout_expert(env, 5, obs=obs, replay=ring)
    _untouched(ring, snap, env._backend(), state)
    assert env.simulation_time == 0


def test_assembly_env_reference_shaped_collection(shapes, tmp_path):
    """collect_expert_data.py's loop on the numpy API (env.step + ReplayBufferExpert.push, restated) and rollout_expert +
    save_expert_data from the same start state give the same rows in float32."""
    from marl_llm_amd.env import AssemblySwarmEnv, AssemblySwarmWrapper, make_args
    from marl_llm_amd.rollout import ChainedReplay, rollout_expert, save_expert_data
    N, T = 30, 20
    np.random.seed(4)
    env = AssemblySwarmWrapper(AssemblySwarmEnv(n_envs=1, obs_dtype="float32"),
                               make_args(n_a=N, results_file=shapes, agent_strategy="rule", is_collected=True))
    obs = env.reset()
    base = env.env
    p0, dp0 = [x.clone() for x in base._backend().get_state()]
    rows = {k: [] for k in ("obs_buffs", "ac_buffs", "next_obs_buffs", "done_buffs")}
    agent_actions = np.zeros((2, env.n_a))
    idx = slice(0, env.n_a)
    for _ in range(T):
        next_obs, rewards, dones, _, agent_actions = env.step(agent_actions)
        for k, a in zip(rows, (obs, agent_actions, next_obs, dones)):      # ReplayBufferExpert.push: a[:, index].T
            rows[k].append(np.asarray(a, np.float64)[:, idx].T)
        obs = next_obs
    want = {k: np.concatenate(v, 0) for k, v in rows.items()}
    end_metrics = env.env.metrics_tensor().clone()
    # the device path from the same start state
    base.set_state(p0.cpu().numpy(), dp0.cpu().numpy())
    b = base._backend()
    obs_t = b.observe()
    t0, v0 = base.simulation_time, base._state_version
    ring = ChainedReplay(T, N, b.obs_dim, 2, b.device, obs_dtype=torch.float32)
    rollout_expert(base, T, obs=obs_t, replay=ring, source="rule")
    assert base.simulation_time == pytest.approx(t0 + T * base.dt) and base._state_version > v0
    got = np.load(save_expert_data(ring, str(tmp_path)))
    for k in want:
        assert got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].astype(np.float32), want[k].astype(np.float32)), k
    assert torch.equal(env.env.metrics_tensor(), end_metrics)           # metrics() read after the call: the new state
    assert env.coverage_rate() == float(end_metrics[0, 0])


def test_full_size_bitwise(shapes):
    from marl_llm_amd.rollout import rollout_expert
    E, N, K = 4096, 64, 20
    sb = make_batch(shapes, E, N)
    ring = ring_for(sb, K)
    rollout_expert(sb, K, replay=ring, reset=(226, 0), track_reward=False)
    twin = eager_matches(shapes, E, N, torch.float32, K, ring, seed=226)
    for a, b in zip(sb.get_state(), twin.get_state()):
        assert torch.equal(a, b)
