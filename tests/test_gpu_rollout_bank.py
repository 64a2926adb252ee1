"""The device loops with an actor bank (FusedPolicyBank; include/swarm_rollout.h: env e acts with member e / (E / M)).

Two configurations, five steps each: N = 30, E = 6, M = 3 -- a member's 60 rows end inside a 32-row tile, inside a workgroup --
and N = 64, E = 4, M = 2.  rollout_device and rollout_eval with the bank must leave, bit for bit, what an eager loop written
here leaves: per step, PLAIN FusedPolicy handles (one per member) on the segments of the ring's slot, then SwarmBatch.step --
obs, act, rew, done, prior, and log_pi with log_pi=True, also with coin="env" and per-env epsilon and sigma.  A bank of
identical members equals the plain FusedPolicy; E % M != 0 is refused by each of the four entry points with the ring and the env
untouched."""
import ctypes

import numpy as np
import pytest

from helpers import shape_batch
from test_gpu_rollout_eval import eager_eval

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RING = ("obs", "act", "rew", "done", "act_prior")
CONFIGS = [(30, 6, 3), (64, 4, 2)]            # N, E, M
K = 5


def _modules(M, seed0=40):
    from marl_llm_amd.rollout import PolicyMLP
    mods = []
    for k in range(M):
        torch.manual_seed(seed0 + k)
        m = PolicyMLP(192, 2, 180)
        with torch.no_grad():
            for fc in (m.fc1, m.fc2, m.fc3, m.fc4):
                fc.weight.mul_(2.0); fc.bias.uniform_(-0.3, 0.3)
        mods.append(m.cuda())
    return mods


@pytest.fixture(scope="module", params=["bf16", "bf16x3"])
def actors(request):
    """{M: (bank, segmented twin of plain handles)} at one precision."""
    from marl_llm_amd.rollout import FusedPolicy, FusedPolicyBank
    out = {}
    for M in (2, 3):
        mods = _modules(M)
        out[M] = (FusedPolicyBank(mods, precision=request.param), Segments([FusedPolicy(m, precision=request.param) for m in mods]))
    return out


class Segments:
    """What the parent commit offers: one plain handle per member, handle m on rows [m R, (m + 1) R) of a call."""

    def __init__(self, handles):
        self.handles, self.lib, self.device = handles, handles[0].lib, handles[0].device

    def __call__(self, obs, out=None, noise_scale=0.0, seed=0, step=0, log_pi=None, row_offset=0):
        rows, M = obs.shape[0], len(self.handles)
        assert rows % M == 0
        R = rows // M
        out = torch.empty((rows, 2), device=obs.device) if out is None else out.view(rows, 2)
        for m, f in enumerate(self.handles):
            f(obs[m * R:(m + 1) * R], out=out[m * R:(m + 1) * R], noise_scale=noise_scale, seed=seed, step=step,
              log_pi=None if log_pi is None else log_pi[m * R:(m + 1) * R], row_offset=row_offset + m * R)
        return out


def new_ring(sb, steps, dtype, log_pi=True):
    from marl_llm_amd.rollout import ChainedReplay
    return ChainedReplay(steps, sb.n_env * sb.n_agents, sb.obs_dim, 2, sb.device, obs_dtype=dtype, log_pi=log_pi)


def eager_loop(mb, seg, ring, steps, obs, noise_scale, seed, step0, log_pi, explore=None):
    """The loop of rollout() on the ring's slots with the segmented plain handles; explore = (epsilon [E], sigma [E], log_c [E])
    device tensors: the actor without noise, then swarm_explore_envs in place (coin="env")."""
    from marl_llm_amd import _lib
    E, N = mb.n_env, mb.n_agents
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for t in range(steps):
        sl = ring.begin_step(obs)
        lp = sl["log_pi"].view(-1) if log_pi else None
        if explore is None:
            seg(sl["obs_in"], out=sl["act"], noise_scale=noise_scale, seed=seed, step=step0 + t, log_pi=lp)
        else:
            seg(sl["obs_in"], out=sl["act"], noise_scale=0.0, seed=seed, step=step0 + t)
            ex = _lib.SwarmExplore(explore[0].data_ptr(), explore[1].data_ptr(), explore[2].data_ptr(), None)
            rc = seg.lib.swarm_explore_envs(sl["act"].data_ptr(), lp.data_ptr() if log_pi else None, E * N, N, ctypes.byref(ex), None,
                                            seed, step0 + t, 0, st)
            assert rc == 0, seg.lib.swarm_rollout_last_error()
        obs, rew, done, pri = mb.step(sl["act"].view(E, N, 2), out=dict(obs=sl["next_obs"], rew=sl["rew"], done=sl["done"], prior=sl["prior"]))
        ring.end_step()
    return obs


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def assert_same(sb, mb, ra, rb, oa, ob, log_pi):
    torch.cuda.synchronize()
    for k in RING + (("log_pi",) if log_pi else ()):
        assert torch.equal(bits(getattr(ra, k)), bits(getattr(rb, k))), k
    assert (ra.cur, ra.count) == (rb.cur, rb.count) and torch.equal(oa, ob)
    assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), mb.get_state()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32rows", "bf16rows"])
@pytest.mark.parametrize("mode", ["noise", "log_pi", "coin_env"])
@pytest.mark.parametrize("N,E,M", CONFIGS, ids=["N30-E6-M3", "N64-E4-M2"])
def test_device_loop_equals_the_eager_loop_of_plain_handles(shapes, actors, N, E, M, mode, dtype):
    from marl_llm_amd.rollout import explore_log_c, rollout_device
    bank, seg = actors[M]
    sb, mb = shape_batch(shapes, E, N, dtype), shape_batch(shapes, E, N, dtype)
    log_pi = mode != "noise"
    ra, rb = new_ring(sb, K, dtype), new_ring(mb, K, dtype)
    seed, step0, scale = 11, 100, 0.2
    if mode == "coin_env":
        eps = np.linspace(0.0, 0.8, E).astype(np.float32)
        sig = np.linspace(0.05, 0.4, E).astype(np.float32); sig[1] = 0.0
        coin_out = torch.zeros((K, E), dtype=torch.uint8, device=sb.device)
        oa, _ = rollout_device(sb, bank, K, obs=sb.reset(seed=5), replay=ra, noise_scale=sig, epsilon=eps, seed=seed, step0=step0,
                               log_pi=True, coin="env", coin_out=coin_out)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(mb.device)
        ob = eager_loop(mb, seg, rb, K, mb.reset(seed=5), 0.0, seed, step0, True, (dev(eps), dev(sig), dev(explore_log_c(sig))))
        assert 0 < int(coin_out.sum()) < K * E                      # both branches were taken
    else:
        oa, _ = rollout_device(sb, bank, K, obs=sb.reset(seed=5), replay=ra, noise_scale=scale, seed=seed, step0=step0, log_pi=log_pi)
        ob = eager_loop(mb, seg, rb, K, mb.reset(seed=5), scale, seed, step0, log_pi)
    assert_same(sb, mb, ra, rb, oa, ob, log_pi)
    # the members act differently: env group m's actions are not what the next member's handle gives on its rows
    R = E * N // M
    for m in range(M):
        other = seg.handles[(m + 1) % M](ra.obs[0][m * R:(m + 1) * R], noise_scale=0.0)
        mine = seg.handles[m](ra.obs[0][m * R:(m + 1) * R], noise_scale=0.0)
        assert not torch.equal(mine, other)
    assert np.array_equal(bank.member_of_env(E), np.arange(E) // (E // M))
    sb.close(); mb.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32rows", "bf16rows"])
@pytest.mark.parametrize("N,E,M", CONFIGS, ids=["N30-E6-M3", "N64-E4-M2"])
def test_eval_loop_with_metrics_and_a_shape_switch(shapes, actors, N, E, M, dtype):
    from marl_llm_amd.rollout import ChainedReplay, rollout_eval
    bank, seg = actors[M]
    sched = {2: 4}
    n = E * N
    sb, mb = shape_batch(shapes, E, N, dtype), shape_batch(shapes, E, N, dtype)
    ring = ChainedReplay(K, n, sb.obs_dim, 2, sb.device, obs_dtype=dtype)
    obs, tr = rollout_eval(sb, bank, K, reset=(5, 0), replay=ring, switch=sched, trace_state=True)
    twin = ChainedReplay(K, n, mb.obs_dim, 2, mb.device, obs_dtype=dtype)
    o, met, ps, dps, stats = eager_eval(mb, seg, twin, K, mb.reset(5), sched, shapes)
    torch.cuda.synchronize()
    for k in RING:
        assert torch.equal(getattr(ring, k), getattr(twin, k)), k
    assert ring.cur == K and ring.count == K and torch.equal(obs, o)
    assert np.array_equal(tr.metrics.cpu().numpy(), met.cpu().numpy(), equal_nan=True)
    assert torch.equal(tr.p, ps) and torch.equal(tr.dp, dps)
    assert np.array_equal(tr.reward_stats.cpu().numpy(), stats)
    assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), mb.get_state()))
    sb.close(); mb.close()


@pytest.mark.parametrize("N,E,M", CONFIGS, ids=["N30-E6-M3", "N64-E4-M2"])
def test_a_bank_of_identical_members_equals_the_plain_policy(shapes, N, E, M):
    from marl_llm_amd.rollout import FusedPolicy, FusedPolicyBank, rollout_device
    m = _modules(1, seed0=9)[0]
    runs = []
    for policy in (FusedPolicyBank([m] * M), FusedPolicy(m)):
        sb = shape_batch(shapes, E, N)
        ring = new_ring(sb, K, torch.float32)
        obs, stats = rollout_device(sb, policy, K, obs=sb.reset(seed=5), replay=ring, noise_scale=0.2, epsilon=0.0, seed=3, step0=7, log_pi=True)
        torch.cuda.synchronize()
        runs.append((sb, ring, obs.clone(), stats.clone()))
    (sa, ra, oa, ta), (sb_, rb, ob, tb) = runs
    assert_same(sa, sb_, ra, rb, oa, ob, True)
    assert torch.equal(ta, tb)
    sa.close(); sb_.close()


def test_envs_that_are_no_multiple_of_the_members_are_refused_by_every_entry_point(shapes, actors):
    from marl_llm_amd import _lib
    from marl_llm_amd._lib import SwarmError
    from marl_llm_amd.rollout import rollout_device, rollout_eval
    bank, _ = actors[3]
    E, N = 4, 30                                   # 4 envs, 3 members
    sb = shape_batch(shapes, E, N)
    ring = new_ring(sb, K, torch.float32)
    obs = sb.reset(seed=5)
    ring.new_chain(obs)
    torch.cuda.synchronize()
    state = [x.clone() for x in sb.get_state()]
    before = {k: getattr(ring, k).clone() for k in RING + ("log_pi",)}
    cur, count = ring.cur, ring.count
    eps = np.full(E, 0.5, np.float32)
    calls = [("swarm_rollout:", lambda: rollout_device(sb, bank, K, replay=ring, noise_scale=0.2)),
             ("swarm_rollout_logpi:", lambda: rollout_device(sb, bank, K, replay=ring, noise_scale=0.2, log_pi=True)),
             ("swarm_rollout_explore:", lambda: rollout_device(sb, bank, K, replay=ring, noise_scale=eps, epsilon=eps, coin="env")),
             ("swarm_rollout_eval:", lambda: rollout_eval(sb, bank, K, replay=ring))]
    for who, call in calls:
        with pytest.raises(SwarmError) as e:
            call()
        msg = str(e.value)
        assert who in msg and "n_env 4" in msg and "members 3" in msg, msg
        assert _lib.load().swarm_rollout_last_error().decode().startswith(who)
        torch.cuda.synchronize()
        assert (ring.cur, ring.count) == (cur, count)
        for k, v in before.items():
            assert torch.equal(bits(getattr(ring, k)), bits(v)), (who, k)
        assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), state)), who
    sb.close()
