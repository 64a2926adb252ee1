"""Per-env exploration on the device (include/swarm_rollout.h "Per-env exploration": swarm_rollout_explore,
swarm_explore_envs, rollout_device(coin="env")), bit for bit:

1. with epsilon 0 and one sigma it is the scalar path (swarm_rollout / swarm_rollout_logpi with that noise_scale);
2. with epsilon 1 everywhere it is the scalar path with every step a uniform step;
3. mixed epsilon and sigma per env: the coins are the restatement's (tests/explore_inputs.py), a coin env's rows are the
   restated uniform actions, every other row is the scalar forward at its env's sigma, and the env follows an eager mirror;
4. two calls over env halves with row_offset reproduce the whole batch (the coin is keyed by the GLOBAL env);
5. the device loop equals rollout(coin="env"), a resets= cut, a side stream behind a delay, arrays rewritten between two
   calls, refusals that enqueue nothing, a large_swarm handle and a wide policy.
Comparisons of actions and log-pi go through the int32 view: -0.0 is not 0.0 here."""
import ctypes

import numpy as np
import pytest

import explore_inputs as X
from helpers import shape_batch as make_batch
from test_gpu_streams import Delayed, Serial, cycles_per_ms  # noqa: F401  (cycles_per_ms is a fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RING = ("obs", "act", "rew", "done", "act_prior")


@pytest.fixture(scope="module")
def policy():
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP
    torch.manual_seed(0)
    return FusedPolicy(PolicyMLP(192, 2, 180).cuda())


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def same_ring(a, b, log_pi=False):
    keys = RING + (("log_pi",) if log_pi else ())
    return [k for k in keys if not same(getattr(a, k), getattr(b, k))] == [] and (a.cur, a.count) == (b.cur, b.count)


def same_state(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.get_state(), b.get_state()))


def new_ring(sb, K, dtype=torch.float32, log_pi=True):
    from marl_llm_amd.rollout import ChainedReplay
    return ChainedReplay(K, sb.n_env * sb.n_agents, sb.obs_dim, 2, sb.device, obs_dtype=dtype, log_pi=log_pi)


class Always:
    """host_rng whose coin always fires (random() = 0 < epsilon)."""
    def random(self):
        return 0.0


# ------------------------------------------------------------------------------------------------------------------------
# 1. and 2.: the scalar path
# ------------------------------------------------------------------------------------------------------------------------
SCALAR_CASES = [(6, 32, torch.float32), (5, 64, torch.float32), (7, 30, torch.float32), (1, 8, torch.float32), (5, 64, torch.bfloat16)]
SCALAR_IDS = ["e6_n32", "e5_n64", "e7_n30", "e1_n8", "e5_n64_bf16"]


@pytest.mark.parametrize("log_pi", [False, True], ids=["act", "logpi"])
@pytest.mark.parametrize("E,N,dtype", SCALAR_CASES, ids=SCALAR_IDS)
def test_constant_sigma_without_coins_is_the_scalar_path(shapes, policy, E, N, dtype, log_pi):
    """N = 30 puts env boundaries inside a wave; 7 x 30 and 1 x 8 leave a partial last workgroup; 7 steps wrap the 4 slots."""
    from marl_llm_amd.rollout import rollout_device
    sigma, steps = 0.2, 7
    out = []
    for per_env in (False, True):
        sb = make_batch(shapes, E, N, dtype)
        ring = new_ring(sb, 3, dtype, log_pi)
        kw = dict(replay=ring, seed=11, step0=100, log_pi=log_pi, reset=(5, 0))
        if per_env:                                               # a zero array with the log-pi column, NULL without
            eps = np.zeros(E, np.float32) if log_pi else 0.0
            obs, st = rollout_device(sb, policy, steps, noise_scale=np.full(E, sigma, np.float32), epsilon=eps, coin="env", **kw)
        else:
            obs, st = rollout_device(sb, policy, steps, noise_scale=sigma, **kw)
        torch.cuda.synchronize()
        out.append((sb, ring, obs.clone(), st.clone()))
    (sa, ra, oa, sta), (sb_, rb, ob, stb) = out
    diff = {k: int((bits(getattr(ra, k)) != bits(getattr(rb, k))).sum()) for k in RING + (("log_pi",) if log_pi else ())}
    print("differing elements per column:", diff)
    assert same_ring(ra, rb, log_pi), diff
    assert ra.S == 4 and ra.count == 3 and same(oa, ob) and same_state(sa, sb_) and torch.equal(sta, stb)
    assert (ra.act.abs() < 1).any() and not same(ra.act[0], ra.act[1])
    sa.close(); sb_.close()


def test_all_coins_is_the_scalar_path_with_every_step_uniform(shapes, policy):
    from marl_llm_amd.rollout import LOG_PI_UNIFORM, rollout_device
    E, N, steps = 7, 30, 5
    out = []
    for per_env in (False, True):
        sb = make_batch(shapes, E, N)
        ring = new_ring(sb, steps)
        kw = dict(replay=ring, seed=4, step0=17, log_pi=True, reset=(2, 1), noise_scale=0.3)
        if per_env:
            coin_out = torch.zeros((steps, E), dtype=torch.uint8, device=sb.device)
            obs, _ = rollout_device(sb, policy, steps, epsilon=np.array([1.0] * (E - 1) + [2.0], np.float32), coin="env", coin_out=coin_out, **kw)
            assert coin_out.min().item() == 1
        else:
            obs, _ = rollout_device(sb, policy, steps, epsilon=1.0, host_rng=Always(), **kw)
        out.append((sb, ring, obs.clone()))
    (sa, ra, oa), (sb_, rb, ob) = out
    assert same_ring(ra, rb, log_pi=True) and same(oa, ob) and same_state(sa, sb_)
    assert (rb.log_pi[:steps] == LOG_PI_UNIFORM).all()
    assert same(rb.act[2], torch.from_numpy(X.uniform_actions(4, 19, E * N)).to(sa.device))
    sa.close(); sb_.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. mixed epsilon and sigma per env
# ------------------------------------------------------------------------------------------------------------------------
def mixed_arrays(E):
    """Every pair of epsilon in {0, 0.3, 1} and sigma in {0, 0.1, 0.25}, repeated over the envs."""
    eps = np.array([(0.0, 0.3, 1.0)[e % 3] for e in range(E)], np.float32)
    sig = np.array([(0.0, 0.1, 0.25)[(e // 3) % 3] for e in range(E)], np.float32)
    return eps, sig


def expected_step(policy, rows_obs, seed, step, N, eps, sig, row_offset=0):
    """One step's (coin [E], act [n, 2], log_pi [n]) from the restated coins and uniform actions and, for every other row, the
    existing scalar forward at its env's sigma: one whole-batch call per distinct sigma, rows selected."""
    from marl_llm_amd.rollout import LOG_PI_UNIFORM
    n, dev = rows_obs.shape[0], rows_obs.device
    coin, branch = X.branches(seed, step, N, eps, sig, row_offset)
    act, lp = policy(rows_obs, noise_scale=0.0, seed=seed, step=step, log_pi=True, row_offset=row_offset)
    act, lp = act.clone(), lp.clone()
    assert (lp == 0).all() and torch.signbit(lp).all()
    row_sig = np.repeat(sig, N)
    for s in sorted(set(sig[sig > 0].tolist())):
        a_s, lp_s = policy(rows_obs, noise_scale=s, seed=seed, step=step, log_pi=True, row_offset=row_offset)
        pick = torch.from_numpy((branch == X.NOISE) & (row_sig == np.float32(s))).to(dev)
        act[pick], lp[pick] = a_s[pick], lp_s[pick]
    pick = torch.from_numpy(branch == X.COIN).to(dev)
    act[pick] = torch.from_numpy(X.uniform_actions(seed, step, n, row_offset)).to(dev)[pick]
    lp[pick] = LOG_PI_UNIFORM
    return coin, act, lp


def test_mixed_envs_follow_the_header_and_a_mirror_loop(shapes, policy):
    from marl_llm_amd.rollout import rollout_device
    E, N, steps, seed, step0 = 18, 30, 8, 21, 40
    n = E * N
    eps, sig = mixed_arrays(E)
    table = X.coin_table(seed, step0, steps, eps)
    mid = table[:, eps == np.float32(0.3)]
    assert mid.any() and not mid.all()                            # at epsilon 0.3 some env-steps fire and some do not
    assert not table[:, eps == 0].any() and table[:, eps == 1].all()
    sb, mb = make_batch(shapes, E, N), make_batch(shapes, E, N)
    ring = new_ring(sb, steps)
    coin_out = torch.full((steps, E), 7, dtype=torch.uint8, device=sb.device)
    obs, _ = rollout_device(sb, policy, steps, obs=sb.reset(seed=9), replay=ring, noise_scale=sig, epsilon=eps, seed=seed,
                            step0=step0, log_pi=True, coin="env", coin_out=coin_out, track_reward=False)
    assert np.array_equal(coin_out.cpu().numpy(), table)
    o = mb.reset(seed=9)
    for t in range(steps):
        rows = o.reshape(n, -1)
        coin, act, lp = expected_step(policy, rows, seed, step0 + t, N, eps, sig)
        assert np.array_equal(coin, table[t])
        assert torch.equal(ring.obs[t], rows), t
        bad = (bits(ring.act[t]) != bits(act)).any(dim=1)
        assert not bad.any(), (t, sorted(set((torch.nonzero(bad)[:, 0] // N).tolist())))       # the envs that differ
        assert same(ring.log_pi[t, :, 0], lp), t
        o, rew, done, pri = mb.step(act.view(E, N, 2))
        assert torch.equal(ring.rew[t].view(E, N), rew) and torch.equal(ring.act_prior[t].view(E, N, 2), pri), t
        assert torch.equal(ring.done[t].view(E, N), done.to(torch.uint8)), t
    assert torch.equal(obs, o) and same_state(sb, mb)
    # the three branches really differ: sigma 0 rows are the bare actor, noisy rows are not, coin rows are uniform
    c0, b0 = X.branches(seed, step0, N, eps, sig)
    det = policy(ring.obs[0], noise_scale=0.0)
    plain, noisy = torch.from_numpy(b0 == X.PLAIN).to(sb.device), torch.from_numpy(b0 == X.NOISE).to(sb.device)
    assert plain.any() and noisy.any() and same(ring.act[0][plain], det[plain]) and (ring.act[0][noisy] != det[noisy]).any()
    sb.close(); mb.close()


def test_epsilon_zero_never_fires_even_where_u_is_zero(policy):
    """The coin is u < epsilon, not u <= epsilon: at (seed 21, step 40) global env 31564759 draws u = 0 exactly (found by
    search over the restatement), so epsilon = 0 must not fire there and the smallest epsilon above it must.  Through the
    eager entry point, the batch placed at that global env by row_offset."""
    from marl_llm_amd import _lib
    seed, step, ge, N = 21, 40, 31564759, 8
    E, off = 3, ge - 1
    u = X.coin_uniforms(seed, step, E, env_offset=off)
    assert u[1] == 0 and u[0] > 2.0 ** -20 and u[2] > 2.0 ** -20
    dev = policy.device
    sig = torch.zeros(E, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for eps, want in ((0.0, [0, 0, 0]), (2.0 ** -30, [0, 1, 0])):
        assert X.coins(seed, step, np.full(E, eps, np.float32), off).tolist() == want
        act = torch.full((E * N, 2), 0.5, device=dev)
        coin = torch.full((E,), 9, dtype=torch.uint8, device=dev)
        eps_t = torch.full((E,), eps, device=dev)
        ex = _lib.SwarmExplore(eps_t.data_ptr(), sig.data_ptr(), None, None)
        assert policy.lib.swarm_explore_envs(act.data_ptr(), None, E * N, N, ctypes.byref(ex), coin.data_ptr(), seed, step, off * N, stream) == 0
        torch.cuda.synchronize()
        assert coin.tolist() == want
        uni = torch.from_numpy(X.uniform_actions(seed, step, E * N, off * N)).to(dev)
        fired = torch.tensor(want, device=dev).repeat_interleave(N).bool()
        assert same(act, torch.where(fired[:, None], uni, torch.full_like(act, 0.5)))


# ------------------------------------------------------------------------------------------------------------------------
# 4. sharding
# ------------------------------------------------------------------------------------------------------------------------
def test_env_halves_with_row_offset_reproduce_the_whole_batch(shapes, policy):
    from marl_llm_amd._lib import SwarmError
    from marl_llm_amd.rollout import rollout_device
    E, N, steps, seed, step0 = 6, 30, 6, 3, 70
    H = E // 2
    eps = np.array([0.3, 0.5, 0.7, 0.3, 0.5, 0.7], np.float32)
    sig = np.array([0.1, 0.25, 0.1, 0.25, 0.1, 0.25], np.float32)
    table = X.coin_table(seed, step0, steps, eps)
    assert not np.array_equal(table[:, :H], table[:, H:])          # a coin keyed by the local env would repeat the first half
    assert not np.array_equal(X.coin_table(seed, step0, steps, eps[H:]), table[:, H:])

    def run(n_env, env_offset, e, s):
        sb = make_batch(shapes, n_env, N)
        ring = new_ring(sb, steps)
        coin_out = torch.zeros((steps, n_env), dtype=torch.uint8, device=sb.device)
        obs, _ = rollout_device(sb, policy, steps, replay=ring, reset=(8, 2, env_offset), noise_scale=s, epsilon=e, seed=seed,
                                step0=step0, row_offset=env_offset * N, log_pi=True, coin="env", coin_out=coin_out, track_reward=False)
        torch.cuda.synchronize()
        return sb, ring, coin_out, obs.clone()

    whole, lo, hi = run(E, 0, eps, sig), run(H, 0, eps[:H], sig[:H]), run(H, H, eps[H:], sig[H:])
    assert np.array_equal(whole[2].cpu().numpy(), table)
    assert torch.equal(torch.cat([lo[2], hi[2]], dim=1), whole[2])
    for k in RING + ("log_pi",):
        w, a, b = (getattr(r[1], k) for r in (whole, lo, hi))
        assert same(torch.cat([a, b], dim=1), w), k
    assert same(torch.cat([lo[3], hi[3]], dim=0), whole[3])
    # a coin belongs to a whole env: a row_offset inside an env is refused, and nothing happened
    sb, ring = lo[0], lo[1]
    before = {k: getattr(ring, k).clone() for k in RING}
    state = (ring.cur, ring.count, set(ring._sealed))
    with pytest.raises(SwarmError, match=r"swarm_rollout_explore: row_offset 31 is no multiple of n_agents 30"):
        rollout_device(sb, policy, 2, replay=ring, noise_scale=sig[:H], epsilon=eps[:H], row_offset=N + 1, coin="env")
    torch.cuda.synchronize()
    assert all(torch.equal(getattr(ring, k), v) for k, v in before.items()) and (ring.cur, ring.count, set(ring._sealed)) == state
    for r in (whole, lo, hi):
        r[0].close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. the remaining cases
# ------------------------------------------------------------------------------------------------------------------------
def witness_pair(make, policy, steps, eps, sig, dtype=torch.float32, **kw):
    """rollout_device(coin="env") and its witness rollout(coin="env") on twin handles: ((batch, ring, coins, obs), ...)."""
    from marl_llm_amd.rollout import rollout, rollout_device
    out = []
    for device_loop in (True, False):
        sb = make()
        obs = sb.reset(seed=5)
        ring = new_ring(sb, steps, dtype)
        coin_out = torch.zeros((steps, sb.n_env), dtype=torch.uint8, device=sb.device)
        if device_loop:
            obs, _ = rollout_device(sb, policy, steps, obs=obs, replay=ring, noise_scale=sig, epsilon=eps, log_pi=True, coin="env",
                                    coin_out=coin_out, **kw)
        else:
            obs, _ = rollout(sb, policy, steps, obs, replay=ring, noise_scale=sig, epsilon=eps, log_pi=True, coin="env",
                             coin_out=coin_out, **kw)
        torch.cuda.synchronize()
        out.append((sb, ring, coin_out, obs.clone()))
    return out


def assert_witness(pair, table):
    (sa, ra, ca, oa), (sb_, rb, cb, ob) = pair
    assert np.array_equal(ca.cpu().numpy(), table) and torch.equal(ca, cb)
    assert same_ring(ra, rb, log_pi=True) and same(oa, ob) and same_state(sa, sb_)
    sa.close(); sb_.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_device_loop_equals_the_python_loop(shapes, policy, dtype):
    E, N, steps = 9, 32, 5
    eps, sig = mixed_arrays(E)
    pair = witness_pair(lambda: make_batch(shapes, E, N, dtype), policy, steps, eps, sig, dtype, seed=6, step0=30)
    assert_witness(pair, X.coin_table(6, 30, steps, eps))


def test_large_swarm_handle(shapes, policy):
    E, N, steps = 2, 257, 2
    eps, sig = np.array([1.0, 0.0], np.float32), np.array([0.1, 0.25], np.float32)
    pair = witness_pair(lambda: make_batch(shapes, E, N, torch.float32, large_swarm=True), policy, steps, eps, sig, seed=1, step0=2)
    ring = pair[0][1]
    assert same(ring.act[0][:N], torch.from_numpy(X.uniform_actions(1, 2, N)).to(ring.act.device))
    noisy = policy(ring.obs[0], noise_scale=0.25, seed=1, step=2)
    assert same(ring.act[0][N:], noisy[N:])
    assert_witness(pair, X.coin_table(1, 2, steps, eps))


def test_wide_policy():
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP
    from test_gpu_rollout_wide import D, E, N, batch, one_shape_set
    torch.manual_seed(0)
    wide = FusedPolicy(PolicyMLP(D, 2, 200).cuda())
    assert wide.wide is True
    s1 = one_shape_set(True)
    eps, sig = np.array([0.0, 1.0, 0.0], np.float32), np.array([0.2, 0.2, 0.0], np.float32)
    pair = witness_pair(lambda: batch(s1, torch.float32), wide, 2, eps, sig, seed=8, step0=0)
    ring = pair[0][1]
    noisy, det = wide(ring.obs[1], noise_scale=0.2, seed=8, step=1), wide(ring.obs[1])
    assert same(ring.act[1][:N], noisy[:N]) and same(ring.act[1][2 * N:], det[2 * N:])
    assert_witness(pair, X.coin_table(8, 0, 2, eps))
    wide.close()


def test_a_resets_schedule_with_one_cut(shapes, policy):
    from marl_llm_amd.rollout import rollout_device
    E, N, steps, cut = 6, 32, 7, 4
    eps, sig = mixed_arrays(E)
    eps[0] = 0.5
    out = []
    for one_call in (True, False):
        sb = make_batch(shapes, E, N)
        ring = new_ring(sb, 10)
        coin_out = torch.zeros((steps, E), dtype=torch.uint8, device=sb.device)
        kw = dict(replay=ring, noise_scale=sig, epsilon=eps, seed=2, log_pi=True, coin="env")
        if one_call:
            obs, st = rollout_device(sb, policy, steps, resets={0: (3, 0), cut: (3, 1)}, step0=50, coin_out=coin_out, **kw)
        else:
            _, s0 = rollout_device(sb, policy, cut, reset=(3, 0), step0=50, coin_out=coin_out[:cut], **kw)
            obs, s1 = rollout_device(sb, policy, steps - cut, reset=(3, 1), step0=50 + cut, coin_out=coin_out[cut:], **kw)
            st = torch.cat([s0, s1])
        torch.cuda.synchronize()
        out.append((sb, ring, coin_out, obs.clone(), st))
    (sa, ra, ca, oa, sta), (sb_, rb, cb, ob, stb) = out
    assert np.array_equal(ca.cpu().numpy(), X.coin_table(2, 50, steps, eps)) and torch.equal(ca, cb)
    assert same_ring(ra, rb, log_pi=True) and ra._sealed == rb._sealed == {cut} and ra.cur == steps + 1
    assert same(oa, ob) and torch.equal(sta, stb) and same_state(sa, sb_)
    sa.close(); sb_.close()


def test_a_side_stream_behind_a_delay(shapes, policy, cycles_per_ms):
    """tests/test_gpu_streams.py's method: the observation rows and the exploration arrays are rewritten behind a delay on a
    side stream and the call is enqueued behind them; work that went to another stream computes on the old values."""
    from marl_llm_amd.rollout import rollout_device
    E, N, steps, case = 4, 64, 3, "explore"
    n = E * N
    eps_a, sig_a = np.zeros(E, np.float32), np.full(E, 0.05, np.float32)
    eps_b, sig_b = np.array([0.0, 1.0, 0.0, 0.0], np.float32), np.array([0.3, 0.3, 0.0, 0.3], np.float32)
    res, a_act = [], None
    for m in (Serial(), Delayed(cycles_per_ms, case)):
        sb = make_batch(shapes, E, N)
        ring = new_ring(sb, 8)
        dev = sb.device
        eps, sig = torch.from_numpy(eps_a).to(dev), torch.from_numpy(sig_a).to(dev)
        log_c = torch.from_numpy(X.log_c(sig_a)).to(dev)
        coin_out = torch.zeros((steps, E), dtype=torch.uint8, device=dev)
        b = {k: torch.from_numpy(v).to(dev) for k, v in dict(eps=eps_b, sig=sig_b, log_c=X.log_c(sig_b)).items()}
        kw = dict(replay=ring, noise_scale=sig, epsilon=eps, log_c=log_c, log_pi=True, coin="env", seed=3, step0=5)
        obs_buf = sb.reset(seed=4).clone()
        o, _ = rollout_device(sb, policy, steps, obs=obs_buf, coin_out=coin_out, **kw)          # warm-up on state A
        obs_b = o.clone()
        a_act = ring.act[:steps].clone() if a_act is None else a_act
        sb.reset(seed=4)
        torch.cuda.synchronize()
        r = {}
        with m.stream():
            m.delay()
            obs_buf.copy_(obs_b)
            eps.copy_(b["eps"]); sig.copy_(b["sig"]); log_c.copy_(b["log_c"])
            start = ring.cur + 1                                  # a fresh obs tensor seals slot cur: the chain starts behind it
            o, r["stats"] = rollout_device(sb, policy, steps, obs=obs_buf, coin_out=coin_out, **kw); m.enqueued("swarm_rollout_explore")
            r.update({k: getattr(ring, k)[start:start + steps].clone() for k in RING + ("log_pi",)})
            r.update(obs_last=o.clone(), coin=coin_out.clone())
            m.done()
        res.append(r)
        sb.close()
    want, got = res
    for k in want:
        assert same(got[k], want[k]), f"{case}: {k} differs from the default-stream run"
    assert np.array_equal(want["coin"].cpu().numpy(), X.coin_table(3, 5, steps, eps_b))
    assert not same(want["act"], a_act)
    assert same(want["act"][0][N:2 * N], torch.from_numpy(X.uniform_actions(3, 5, n)).to(want["act"].device)[N:2 * N])
    assert (want["log_pi"][:, 2 * N:3 * N] == 0).all()


def test_arrays_rewritten_between_two_calls_are_seen_by_the_second_only(shapes, policy):
    from marl_llm_amd.rollout import LOG_PI_UNIFORM, rollout_device
    E, N, steps = 4, 64, 2
    n = E * N
    sb = make_batch(shapes, E, N)
    ring = new_ring(sb, 8)
    dev = sb.device
    eps, sig = torch.zeros(E, device=dev), torch.full((E,), 0.1, device=dev)
    log_c = torch.from_numpy(X.log_c(np.full(E, 0.1, np.float32))).to(dev)
    coins = torch.full((2 * steps, E), 9, dtype=torch.uint8, device=dev)
    kw = dict(replay=ring, noise_scale=sig, epsilon=eps, log_c=log_c, log_pi=True, coin="env", seed=7, track_reward=False)
    rollout_device(sb, policy, steps, reset=(1, 0), step0=0, coin_out=coins[:steps], **kw)
    eps.fill_(1.0); sig.zero_()                                   # enqueued behind the first call, in front of the second
    rollout_device(sb, policy, steps, step0=steps, coin_out=coins[steps:], **kw)
    torch.cuda.synchronize()
    assert coins.cpu().tolist() == [[0] * E] * steps + [[1] * E] * steps
    for t in range(steps):                                        # the first call: sigma 0.1's scalar path, no coin
        a, lp = policy(ring.obs[t], noise_scale=0.1, seed=7, step=t, log_pi=True)
        assert same(ring.act[t], a) and same(ring.log_pi[t, :, 0], lp), t
    for t in range(steps, 2 * steps):
        assert same(ring.act[t], torch.from_numpy(X.uniform_actions(7, t, n)).to(dev)), t
        assert (ring.log_pi[t] == LOG_PI_UNIFORM).all()
    sb.close()


def test_rejected_calls_enqueue_nothing(shapes, policy):
    from marl_llm_amd import _lib
    from marl_llm_amd.rollout import ChainedReplay, rollout_device
    E, N = 4, 32
    n = E * N
    sb = make_batch(shapes, E, N)
    obs = sb.reset(seed=1)
    state = [x.clone() for x in sb.get_state()]
    sig = np.full(E, 0.1, np.float32)

    def rejected(ring, err, match, **kw):
        before = {k: getattr(ring, k).clone() for k in RING}
        book = (ring.cur, ring.count, ring._chained, set(ring._sealed))
        coin_out = torch.full((3, E), 5, dtype=torch.uint8, device=sb.device)
        args = dict(obs=obs, replay=ring, noise_scale=sig, epsilon=0.5, coin="env", coin_out=coin_out)
        args.update(kw)
        with pytest.raises(err, match=match):
            rollout_device(sb, policy, 3, **args)
        torch.cuda.synchronize()
        assert all(torch.equal(getattr(ring, k), v) for k, v in before.items())
        assert (ring.cur, ring.count, ring._chained, set(ring._sealed)) == book and (coin_out == 5).all()

    rejected(ChainedReplay(2, n + 1, sb.obs_dim, 2, sb.device), _lib.SwarmError, "swarm_rollout_explore: ring rows")
    rejected(ChainedReplay(0, n, sb.obs_dim, 2, sb.device), _lib.SwarmError, "swarm_rollout_explore: ring n_slots")
    rejected(ChainedReplay(2, n, sb.obs_dim, 2, sb.device), _lib.SwarmError, "no multiple of n_agents", row_offset=5)
    rejected(ChainedReplay(2, n, sb.obs_dim, 2, sb.device), ValueError, "built with log_pi=True", log_pi=True)
    rejected(ChainedReplay(2, n, sb.obs_dim, 2, sb.device, log_pi=True), ValueError, "needs log_c=", log_pi=True,
             noise_scale=torch.from_numpy(sig).to(sb.device))
    # through the C ABI: no sigma, and a log-pi column without the constants
    ring = ChainedReplay(2, n, sb.obs_dim, 2, sb.device, log_pi=True)
    ring.new_chain(obs)
    before = {k: getattr(ring, k).clone() for k in RING + ("log_pi",)}
    r = _lib.SwarmRing(ring.obs.data_ptr(), ring.act.data_ptr(), ring.rew.data_ptr(), ring.done.data_ptr(), ring.act_prior.data_ptr(),
                       n, sb.obs_dim, _lib.F32, ring.S, ring.cur)
    dsig = torch.from_numpy(sig).to(sb.device)
    lib, stream = policy.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ex, lp, msg in ((_lib.SwarmExplore(None, None, None, None), None, b"null ex or ex->sigma"),
                        (_lib.SwarmExplore(None, dsig.data_ptr(), None, None), ring.log_pi.data_ptr(), b"ex->log_c")):
        rc = lib.swarm_rollout_explore(sb.handle, policy.handle, ctypes.byref(r), lp, 3, ctypes.byref(ex), 0, 0, 0, None, stream)
        assert rc == 1 and msg in lib.swarm_rollout_last_error()
    act = ring.act[0]
    assert lib.swarm_explore_envs(act.data_ptr(), None, n, N, ctypes.byref(_lib.SwarmExplore(None, dsig.data_ptr(), None, None)), None,
                                  0, 0, N + 1, stream) == 1
    assert b"swarm_explore_envs: row_offset" in lib.swarm_rollout_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(getattr(ring, k), v) for k, v in before.items())
    assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), state))
    # the handle still works after all of that
    _, st = rollout_device(sb, policy, 2, obs=obs, noise_scale=sig, epsilon=0.5, coin="env")
    assert st.shape == (2, 2) and torch.isfinite(st).all()
    sb.close()
