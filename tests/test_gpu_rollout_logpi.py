"""The device rollout loop with log-probabilities (rollout_device(log_pi=True) -> swarm_rollout_logpi, include/swarm_rollout.h):
the transitions are bit for bit those of the loop without log-pi, every stored log-pi is the eager policy call's for the same
(seed, step, row_offset) or the coin constant, across episode boundaries and for a rank's shard; rollout()'s fused path
records the same values; a ring without the column is refused before anything runs."""
import numpy as np
import pytest

from helpers import shape_batch as make_batch

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RING = ("obs", "act", "rew", "done", "act_prior")
UNIFORM = np.float32(-2.0 * np.log(2.0))


@pytest.fixture(scope="module")
def policy():
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP
    torch.manual_seed(0)
    return FusedPolicy(PolicyMLP(192, 2, 180).cuda())


def check_slots(ring, policy, slots, steps, coins, seed, row_offset, scale):
    """Every stored log-pi of `slots` (taken at `steps`) is the eager call's, or the coin constant; the actions agree too."""
    for c, t, coin in zip(slots, steps, coins):
        lp = ring.log_pi[c, :, 0]
        if coin:
            assert (lp == float(UNIFORM)).all(), (c, t)
            continue
        act, want = policy(ring.obs[c], noise_scale=scale, seed=seed, step=t, log_pi=True, row_offset=row_offset)
        assert torch.equal(act, ring.act[c]), (c, t)
        assert torch.equal(lp.view(torch.int32), want.view(torch.int32)), (c, t)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,E", [(30, 256), (64, 4096)])
def test_device_loop_log_pi_is_the_eager_calls_and_changes_nothing(shapes, policy, N, E, dtype):
    """200 steps, epsilon 0.3, an episode boundary (reset=) after 96, in chunks of 8 steps: the run with log-pi and the run
    without it leave the same rings and states after every chunk, and every log-pi is the eager FusedPolicy call's."""
    from marl_llm_amd.rollout import ChainedReplay, rollout_device
    K, n, seed, scale = 8, E * N, 17, 0.2
    runs = []
    for lp in (False, True):
        sb = make_batch(shapes, E, N, dtype)
        runs.append((sb, ChainedReplay(K, n, sb.obs_dim, 2, sb.device, obs_dtype=dtype, log_pi=lp), np.random.RandomState(5)))
    n_coin = n_pol = 0
    t0 = 0
    for chunk in range(25):
        reset = (9, chunk // 12) if chunk % 12 == 0 else None
        slots = None
        for lp, (sb, ring, rng) in zip((False, True), runs):
            rollout_device(sb, policy, K, replay=ring, noise_scale=scale, epsilon=0.3, host_rng=rng, seed=seed, step0=t0,
                           reset=reset, log_pi=lp)
            if lp:
                slots = [(ring.cur - K + i) % ring.S for i in range(K)]
        torch.cuda.synchronize()
        (sa, ra, _), (sb_, rb, _) = runs
        assert all(torch.equal(getattr(ra, k), getattr(rb, k)) for k in RING), chunk
        assert (ra.cur, ra.count, ra._sealed) == (rb.cur, rb.count, rb._sealed)
        assert all(torch.equal(x, y) for x, y in zip(sa.get_state(), sb_.get_state()))
        coins = np.random.RandomState(5)
        for _ in range(t0):                        # the coin sequence of this chunk
            coins.random()
        cs = [coins.random() < 0.3 for _ in range(K)]
        check_slots(rb, policy, slots, range(t0, t0 + K), cs, seed, 0, scale)
        n_coin += sum(cs); n_pol += K - sum(cs)
        t0 += K
    assert n_coin > 20 and n_pol > 100
    for sb, _, _ in runs:
        sb.close()


def test_rank_shard_log_pi_is_a_slice_of_the_whole_batch(shapes, policy):
    """A rank that runs envs [e0, e0 + E1) with row_offset = e0 * N records the whole-batch call's log-pi rows."""
    from marl_llm_amd.rollout import ChainedReplay, rollout_device
    E, E1, e0, N, K = 12, 5, 4, 32, 6
    whole, shard = make_batch(shapes, E, N), make_batch(shapes, E1, N)
    rw = ChainedReplay(K, E * N, whole.obs_dim, 2, whole.device, log_pi=True)
    rs = ChainedReplay(K, E1 * N, shard.obs_dim, 2, shard.device, log_pi=True)
    rollout_device(whole, policy, K, replay=rw, reset=(3, 0), noise_scale=0.15, seed=2, step0=40, log_pi=True)
    rollout_device(shard, policy, K, replay=rs, reset=(3, 0, e0), noise_scale=0.15, seed=2, step0=40, row_offset=e0 * N,
                   log_pi=True)
    torch.cuda.synchronize()
    s = slice(e0 * N, (e0 + E1) * N)
    assert torch.equal(rw.obs[:K, s], rs.obs[:K])                           # the same envs ...
    assert torch.equal(rw.act[:K, s], rs.act[:K])
    assert torch.equal(rw.log_pi[:K, s], rs.log_pi[:K])                     # ... and the same log-pi rows
    check_slots(rs, policy, range(K), range(40, 40 + K), [False] * K, 2, e0 * N, 0.15)
    whole.close(); shard.close()


def test_no_noise_gives_minus_zero_and_the_private_ring_gets_a_column(shapes, policy):
    from marl_llm_amd.rollout import rollout_device
    sb = make_batch(shapes, 4, 32)
    obs, _ = rollout_device(sb, policy, 2, reset=(1, 0))                    # the private ring, no column yet
    assert sb._rollout_ring.log_pi is None
    obs, _ = rollout_device(sb, policy, 3, obs=obs, noise_scale=0.0, log_pi=True)
    torch.cuda.synchronize()
    ring = sb._rollout_ring
    lp = ring.log_pi[(ring.cur - 1) % ring.S, :, 0]
    assert (lp == 0).all() and torch.signbit(lp).all()
    sb.close()


def test_a_ring_without_the_column_is_refused_and_left_alone(shapes, policy):
    from marl_llm_amd.rollout import ChainedReplay, rollout_device
    sb = make_batch(shapes, 4, 32)
    ring = ChainedReplay(4, 128, sb.obs_dim, 2, sb.device)
    obs, _ = rollout_device(sb, policy, 2, replay=ring, reset=(1, 0), noise_scale=0.1)
    torch.cuda.synchronize()
    before = {k: getattr(ring, k).clone() for k in RING}, ring.cur, ring.count, set(ring._sealed)
    state = [x.clone() for x in sb.get_state()]
    for kw in (dict(obs=obs), dict(reset=(1, 1))):
        with pytest.raises(ValueError, match="log_pi=True"):
            rollout_device(sb, policy, 3, replay=ring, noise_scale=0.1, log_pi=True, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(getattr(ring, k), v) for k, v in before[0].items()) and (ring.cur, ring.count, ring._sealed) == before[1:]
    assert all(torch.equal(x, y) for x, y in zip(state, sb.get_state()))
    sb.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_python_fused_loop_records_the_device_loops_log_pi(shapes, policy, dtype):
    """rollout()'s fused path (FusedPolicy + ChainedReplay + SwarmBatch) and its eager FusedPolicy path record what
    rollout_device records on policy steps, and the constant on coin steps (their actions differ: torch's uniform draw)."""
    from marl_llm_amd.rollout import ChainedReplay, rollout, rollout_device
    E, N, K = 6, 32, 5
    n = E * N
    class Eager:                                    # not a SwarmBatch: rollout() takes its eager path (policy call + push)
        def __init__(self, sb):
            self.step = sb.step

    rings = []
    for mode in ("device", "fused", "eager"):
        sb = make_batch(shapes, E, N, dtype)
        ring = ChainedReplay(K, n, sb.obs_dim, 2, sb.device, obs_dtype=dtype, log_pi=True)
        obs = sb.reset(seed=4)
        if mode == "device":
            rollout_device(sb, policy, K, obs=obs, replay=ring, noise_scale=0.1, seed=3, step0=10, log_pi=True)
        else:
            rollout(sb if mode == "fused" else Eager(sb), policy, K, obs, replay=ring, noise_scale=0.1, seed=3, step0=10,
                    log_pi=True)
        torch.cuda.synchronize()
        rings.append(ring)
        sb.close()
    a = rings[0]
    for b in rings[1:]:
        assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in RING + ("log_pi",))
    # coin steps in the fused Python loop hold the constant
    sb = make_batch(shapes, E, N, dtype)
    ring = ChainedReplay(K, n, sb.obs_dim, 2, sb.device, obs_dtype=dtype, log_pi=True)
    rollout(sb, policy, K, sb.reset(seed=4), replay=ring, noise_scale=0.1, epsilon=1.0, log_pi=True)
    torch.cuda.synchronize()
    assert (ring.log_pi[:K] == float(UNIFORM)).all()
    sb.close()
