"""resets= of the device loops (rollout_device, rollout_expert, rollout_eval): whole-batch and per-env episode boundaries
inside one call.  The yardstick is the eager loop -- reset / reset_envs into the ring slot new_chain() hands out, then one-step
calls of the same loop -- and every comparison is bit for bit: every ring column slot by slot, the sealed slots, cur, count,
the reward statistics, the evaluation trace and the final env state.  Inputs: tests/reset_envs_inputs.py (conditions asserted
by tests/test_reset_envs_host.py)."""
import numpy as np
import pytest

import reset_envs_inputs as inputs
from helpers import shape_batch

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SLOTS = 12
STEPS = inputs.ROLLOUT_STEPS
GEOS = [(8, 16), (64, 8)]
GEO_IDS = ["n8_e16", "n64_e8"]
COLUMNS = ("obs", "act", "rew", "done", "act_prior", "log_pi")


@pytest.fixture(scope="module")
def s3():
    return inputs.mixed_shape_set()


@pytest.fixture(scope="module")
def policy():
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP
    torch.manual_seed(0)
    return FusedPolicy(PolicyMLP(192, 2, 180).cuda())


def _ring(sb, log_pi=False):
    from marl_llm_amd.rollout import ChainedReplay
    return ChainedReplay(SLOTS - 1, sb.n_env * sb.n_agents, sb.obs_dim, 2, sb.device, obs_dtype=sb.obs_dtype, log_pi=log_pi)


def _eager(sb, ring, sched, steps, one_step, after_reset=None):
    """The loop resets= stands for: at a scheduled step the reset writes into the slot new_chain() returns, then one step."""
    out = []
    for t in range(steps):
        if t in sched:
            r = sched[t]
            slot = ring.new_chain()
            off = r[2] if len(r) > 2 else 0
            if np.ndim(r[1]) == 0:
                sb.reset(r[0], r[1], off, out=ring.obs[slot])
            else:
                sb.reset_envs(r[0], r[1], off, out=ring.obs[slot])
            if after_reset is not None:
                after_reset(t)
        out.append(one_step(t))
    return out


def _assert_same_ring(a, b, what):
    for k in COLUMNS:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            for j in range(a.S):
                assert torch.equal(x[j], y[j]), (what, k, "slot %d" % j)
    assert (a.cur, a.count, a._chained, a._sealed) == (b.cur, b.count, b._chained, b._sealed), what


def _assert_same_env(a, b, what):
    for x, y, k in zip(a.get_state(), b.get_state(), ("p", "dp")):
        assert torch.equal(x, y), (what, k)
    ca, cb = a.get_cells(), b.get_cells()
    assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1]), what
    assert np.array_equal(a.get_shape_index(), b.get_shape_index()) and a.path_envs() == b.path_envs(), what


@pytest.mark.parametrize("n_a,n_env,log_pi", [(8, 16, False), (64, 8, False), (64, 8, True)], ids=GEO_IDS + ["n64_e8_logpi"])
def test_rollout_device_equals_the_eager_loop(s3, policy, n_a, n_env, log_pi):
    from marl_llm_amd.rollout import rollout_device
    seed = inputs.ROLLOUT[(n_a, n_env)]
    sched = inputs.rollout_schedule(seed, n_env)
    kw = dict(noise_scale=0.1, seed=21, row_offset=3, log_pi=log_pi)
    A, B = shape_batch(s3, n_env, n_a), shape_batch(s3, n_env, n_a)
    try:
        ra, rb = _ring(A, log_pi), _ring(B, log_pi)
        obs, stats = rollout_device(A, policy, STEPS, replay=ra, resets=sched, step0=50, **kw)
        per_step = _eager(B, rb, sched, STEPS, lambda t: rollout_device(B, policy, 1, replay=rb, step0=50 + t, **kw))
        torch.cuda.synchronize()
        _assert_same_ring(ra, rb, "rollout_device")
        assert ra._sealed == {3, 6, 8} and ra.cur == STEPS + 3 and ra.count == STEPS + 3 and len(ra) == STEPS * ra.n
        assert torch.equal(stats, torch.cat([s for _, s in per_step])) and torch.equal(obs, per_step[-1][0])
        assert obs.data_ptr() == ra.obs[ra.cur].data_ptr()
        _assert_same_env(A, B, "rollout_device")
        # a kept env's row in the slot behind a seal equals its row in the sealed slot; a reset env's does not
        E, N = n_env, n_a
        for t, sealed in ((3, 3), (6, 8)):
            took = torch.from_numpy(sched[t][1] >= 0).to(A.device)
            prev, new = ra.obs[sealed].view(E, N, -1), ra.obs[sealed + 1].view(E, N, -1)
            assert torch.equal(prev[~took], new[~took]) and not torch.equal(prev[took], new[took]), t
        # sample(): mark every slot's act rows with (slot, row) and draw
        for j in range(ra.S):
            ra.act[j, :, 0] = float(j); ra.act[j, :, 1] = torch.arange(ra.n, device=A.device, dtype=torch.float32)
        g = torch.Generator(device=A.device).manual_seed(1)
        o, a, r, nx, d, pr = ra.sample(2000, generator=g)
        j, row = a[:, 0].long(), a[:, 1].long()
        assert set(j.tolist()) == set(ra._valid_starts()) and not set(j.tolist()) & ra._sealed
        assert torch.equal(o, ra.obs[j, row]) and torch.equal(nx, ra.obs[(j + 1) % ra.S, row])
    finally:
        A.close(); B.close()


def test_step0_reset_and_a_split_at_t_equal_reset(s3, policy):
    """resets={0: (seed, ep)} is reset=(seed, ep); a whole-batch reset at step t equals two calls split at t, reset= on the second."""
    from marl_llm_amd.rollout import rollout_device
    n_a, n_env = 8, 16
    kw = dict(noise_scale=0.1, seed=4)
    A, B = shape_batch(s3, n_env, n_a), shape_batch(s3, n_env, n_a)
    try:
        ra, rb = _ring(A), _ring(B)
        _, sa = rollout_device(A, policy, 6, replay=ra, resets={0: (5, 1), 4: (5, 2)}, **kw)
        _, s1 = rollout_device(B, policy, 4, replay=rb, reset=(5, 1), **kw)
        _, s2 = rollout_device(B, policy, 2, replay=rb, reset=(5, 2), step0=4, **kw)
        torch.cuda.synchronize()
        _assert_same_ring(ra, rb, "split")
        assert torch.equal(sa, torch.cat([s1, s2]))
        _assert_same_env(A, B, "split")
    finally:
        A.close(); B.close()


EXPERT = [(8, 16, "rule", False), (64, 8, "llm", False), (300, 2, "rule", True)]


@pytest.mark.parametrize("n_a,n_env,source,big", EXPERT, ids=["n8_e16_rule", "n64_e8_llm", "n300_e2_rule_large"])
def test_rollout_expert_equals_the_eager_loop(s3, n_a, n_env, source, big):
    from marl_llm_amd.rollout import rollout_expert
    seed = inputs.ROLLOUT[(n_a, n_env)]
    sched = inputs.large_schedule(seed, n_env) if big else inputs.rollout_schedule(seed, n_env)
    steps = 4 if big else STEPS
    mk = lambda: shape_batch(s3, n_env, n_a, large_swarm=big, llm_action=(source == "llm"))
    A, B = mk(), mk()
    try:
        ra, rb = _ring(A), _ring(B)
        obs, stats = rollout_expert(A, steps, replay=ra, resets=sched, source=source)
        per_step = _eager(B, rb, sched, steps, lambda t: rollout_expert(B, 1, replay=rb, source=source))
        torch.cuda.synchronize()
        _assert_same_ring(ra, rb, "rollout_expert")
        cuts = len(sched) - 1
        assert len(ra._sealed) == cuts and ra.cur == steps + cuts and len(ra) == steps * ra.n
        assert torch.equal(stats, torch.cat([s for _, s in per_step])) and torch.equal(obs, per_step[-1][0])
        _assert_same_env(A, B, "rollout_expert")
    finally:
        A.close(); B.close()


@pytest.mark.parametrize("n_a,n_env", GEOS, ids=GEO_IDS)
def test_rollout_eval_equals_the_eager_loop(s3, policy, n_a, n_env):
    from marl_llm_amd.rollout import rollout_eval
    seed = inputs.ROLLOUT[(n_a, n_env)]
    sched = inputs.rollout_schedule(seed, n_env)
    switch = {4: 1, 6: np.where(np.arange(n_env) % 3 == 0, 0, -1)}         # a batch-wide and a per-env switch beside the resets
    A, B = shape_batch(s3, n_env, n_a), shape_batch(s3, n_env, n_a)
    try:
        ra, rb = _ring(A), _ring(B)
        obs, tr = rollout_eval(A, policy, STEPS, replay=ra, resets=sched, switch=switch, trace_state=True)
        fresh = {}

        def after_reset(t):                                    # what p[t] / dp[t] / metrics[t] of a reset step must be
            fresh[t] = [x.clone() for x in B.get_state()]
            if t not in switch:
                fresh[t].append(B.metrics().clone())

        per_step = _eager(B, rb, sched, STEPS,
                          lambda t: rollout_eval(B, policy, 1, replay=rb, switch={0: switch[t]} if t in switch else None, trace_state=True),
                          after_reset)
        torch.cuda.synchronize()
        _assert_same_ring(ra, rb, "rollout_eval")
        for k in ("metrics", "p", "dp", "reward_stats"):
            want = torch.cat([getattr(t, k) for _, t in per_step])
            got = getattr(tr, k)
            assert got.shape == want.shape and torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0)), k
        for t, f in fresh.items():
            assert torch.equal(tr.p[t], f[0]) and torch.equal(tr.dp[t], f[1]), t
            if len(f) > 2:
                assert torch.equal(torch.nan_to_num(tr.metrics[t], nan=-7.0), torch.nan_to_num(f[2], nan=-7.0)), t
        assert sorted(fresh) == [0, 3, 5, 6] and len(fresh[3]) == 3
        assert np.array_equal(tr.shape, np.concatenate([t.shape for _, t in per_step]))
        assert torch.equal(obs, per_step[-1][0])
        _assert_same_env(A, B, "rollout_eval")
    finally:
        A.close(); B.close()


def test_episode_clock_equals_the_schedule_written_out(s3, policy):
    from marl_llm_amd.rollout import EpisodeClock, rollout_device
    n_a, n_env = 8, 16
    odd = np.arange(n_env) % 2 == 1
    vec = lambda who, ep: np.where(who, ep, -1).astype(np.int64)
    by_hand = [{0: (9, 0, 0), 2: (9, vec(odd, 1), 0)},                                     # global steps 0 .. 2
               {1: (9, vec(~odd, 1), 0), 3: (9, vec(odd, 2), 0), 5: (9, vec(~odd, 2), 0)}]    # global steps 3 .. 9: resets at 4, 6, 8
    clock = EpisodeClock(n_env, 4, groups=2, seed=9)
    kw = dict(noise_scale=0.1, seed=2)
    A, B = shape_batch(s3, n_env, n_a), shape_batch(s3, n_env, n_a)
    try:
        ra, rb = _ring(A), _ring(B)
        t0 = 0
        for k, hand in zip((3, 7), by_hand):
            sched = clock.resets(k)
            assert sorted(sched) == sorted(hand)
            for t in hand:
                assert sched[t][0] == hand[t][0] and np.array_equal(sched[t][1], hand[t][1]) and sched[t][2] == hand[t][2], t
                assert np.ndim(sched[t][1]) == np.ndim(hand[t][1])
            rollout_device(A, policy, k, replay=ra, resets=sched, step0=t0, **kw)
            rollout_device(B, policy, k, replay=rb, resets=hand, step0=t0, **kw)
            t0 += k
        torch.cuda.synchronize()
        _assert_same_ring(ra, rb, "clock")
        assert ra.cur == (10 + 4) % ra.S and len(ra) == 8 * ra.n            # 10 steps + 4 cuts in a ring of 12: it wrapped over steps 0, 1
        _assert_same_env(A, B, "clock")
    finally:
        A.close(); B.close()


def test_a_rejected_schedule_enqueues_nothing(s3, policy):
    from marl_llm_amd._lib import SwarmError
    from marl_llm_amd.rollout import rollout_device, rollout_eval, rollout_expert
    n_a, n_env = 8, 16
    sb = shape_batch(s3, n_env, n_a)
    bare = shape_batch(s3, n_env, n_a, upload=False)                       # cells and state, but no shape set
    try:
        ring = _ring(sb)
        rollout_device(sb, policy, 3, replay=ring, reset=(1, 0))
        cells, n_g = sb.get_cells()
        bare.set_cells(cells, n_g, np.asarray(s3["l_cell"], np.float64)[sb.get_shape_index()])
        bare.set_state(*sb.get_state())
        bring = _ring(bare)
        rollout_device(bare, policy, 2, obs=bare.observe(), replay=bring)
        torch.cuda.synchronize()

        def frozen(b, r):
            cols = [getattr(r, k).clone() for k in COLUMNS if getattr(r, k) is not None]
            return cols + [x.clone() for x in b.get_state()] + [(r.cur, r.count, r._chained, set(r._sealed))]

        def same(x, y):
            return all(torch.equal(a, c) if isinstance(a, torch.Tensor) else a == c for a, c in zip(x, y))

        loops = [lambda b, r, **kw: rollout_device(b, policy, 4, replay=r, **kw), lambda b, r, **kw: rollout_eval(b, policy, 4, replay=r, **kw),
                 lambda b, r, **kw: rollout_expert(b, 4, replay=r, **kw)]
        before, bbefore = frozen(sb, ring), frozen(bare, bring)
        for loop in loops:
            with pytest.raises(SwarmError, match="shape set"):
                loop(bare, bring, resets={2: (1, 1)})
            for bad in ({2: (1, np.zeros(n_env))}, {2: (1, [0, 1, 2])}, {1: (1, 1), 4: (1, 2)},
                        {1: (1, torch.zeros(n_env, dtype=torch.int32, device=sb.device))}):
                with pytest.raises(ValueError):
                    loop(sb, ring, resets=bad)
            with pytest.raises(ValueError):
                loop(sb, ring, reset=(1, 0), resets={0: (1, 0)})
        torch.cuda.synchronize()
        assert same(frozen(sb, ring), before) and same(frozen(bare, bring), bbefore)
        assert sb.lib.hipGetLastError() == 0
    finally:
        sb.close(); bare.close()
