"""The device loops with a WIDE fused actor (csrc/policy_wide.hip): the smallest env whose observation rows exceed the narrow
kernel's 192 columns -- num_obs_grid_max = 100, obs_dim 232 -- with PolicyMLP(232, 2, 200), 8 agents, 3 envs, on a lattice
shape and on an off-lattice shape of the reference's own set (tests/golden/fig_cells.npz), f32 and bf16 rows.
rollout_device (noise, one uniform step, log-pi, a ring that wraps) and rollout_eval must be bit for bit the eager loops of
FusedPolicy.__call__ + SwarmBatch.step; a narrow handle on this env is still refused."""
import numpy as np
import pytest

from helpers import fig_shapes
from test_gpu_rollout_device import uniform_actions
from test_gpu_rollout_eval import RING, eager_eval

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

E, N, G_MAX, D = 3, 8, 100, 232
UNIFORM = np.float32(-2.0 * np.log(2.0))        # LOG_PI_UNIFORM: the log-pi of a coin step


def one_shape_set(lattice):
    """A one-shape set: the first shape of fig_cells.npz, or (off the lattice) the same cells jittered by 4 mm."""
    figs = fig_shapes()
    g = np.asarray(figs["grid_coords"][0], np.float64)
    if not lattice:
        g = g + np.random.default_rng(12).normal(0, 0.004, g.shape)
    return {"grid_coords": [g], "l_cell": [float(figs["l_cell"][0])]}


def batch(shapes, dtype):
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.shapes import r_avoid_for
    ng = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    sb = SwarmBatch(n_env=E, n_agents=N, n_cells_max=ng, r_avoid=r_avoid_for(N, shapes), obs_dtype=dtype, g_max=G_MAX)
    sb.set_shapes(shapes)
    assert sb.obs_dim == D
    return sb


@pytest.fixture(scope="module", params=["bf16", "bf16x3"])
def policy(request):
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP
    torch.manual_seed(0)
    f = FusedPolicy(PolicyMLP(D, 2, 200).cuda(), precision=request.param)
    assert f.wide is True
    return f


class Coins:
    """host_rng of rollout_device: with epsilon 0.5 the third of five steps is a uniform step."""
    def __init__(self):
        self.seq = iter((0.9, 0.8, 0.1, 0.9, 0.7))

    def random(self):
        return next(self.seq)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32rows", "bf16rows"])
@pytest.mark.parametrize("lattice", [True, False], ids=["lattice", "off-lattice"])
def test_device_loop_equals_the_eager_loop(policy, lattice, dtype):
    from marl_llm_amd.rollout import ChainedReplay, rollout_device
    shapes = one_shape_set(lattice)
    K, n, seed, step0, scale = 5, E * N, 11, 100, 0.2
    sb, mb = batch(shapes, dtype), batch(shapes, dtype)
    ring = ChainedReplay(3, n, D, 2, sb.device, obs_dtype=dtype, log_pi=True)        # 4 slots: five steps wrap
    assert ring.S == 4
    obs, _ = rollout_device(sb, policy, K, reset=(5, 0), replay=ring, noise_scale=scale, epsilon=0.5, host_rng=Coins(),
                            seed=seed, step0=step0, log_pi=True)
    o = mb.reset(5)
    first = ring.cur - K                       # the slot of step 0, modulo the ring
    for t in range(K):
        c = (first + t) % ring.S
        row = o.reshape(n, -1)
        if t == 2:
            act = torch.from_numpy(uniform_actions(seed, step0 + t, n)).to(mb.device)
            lp = torch.full((n,), float(UNIFORM), device=mb.device)
        else:
            act, lp = policy(row, noise_scale=scale, seed=seed, step=step0 + t, log_pi=True)
        nobs, rew, done, pri = mb.step(act.view(E, N, 2))
        if t >= K - 3:                         # the three newest transitions are still in the ring
            assert torch.equal(ring.obs[c], row), t
            assert torch.equal(ring.act[c].view(torch.int32), act.view(torch.int32)), t
            assert torch.equal(ring.log_pi[c, :, 0].view(torch.int32), lp.view(torch.int32)), t
            assert torch.equal(ring.rew[c].view(E, N), rew) and torch.equal(ring.act_prior[c].view(E, N, 2), pri), t
        o = nobs.clone()
    assert torch.equal(obs, o) and torch.equal(ring.obs[ring.cur].view(E, N, D), o)
    assert sb.lattice_envs() == (E if lattice else 0)
    assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), mb.get_state()))
    sb.close(); mb.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32rows", "bf16rows"])
@pytest.mark.parametrize("lattice", [True, False], ids=["lattice", "off-lattice"])
def test_eval_loop_equals_the_eager_loop(policy, lattice, dtype):
    from marl_llm_amd.rollout import ChainedReplay, rollout_eval
    shapes = one_shape_set(lattice)
    steps, n = 3, E * N
    sb, mb = batch(shapes, dtype), batch(shapes, dtype)
    ring = ChainedReplay(steps, n, D, 2, sb.device, obs_dtype=dtype)
    obs, tr = rollout_eval(sb, policy, steps, reset=(5, 0), replay=ring, trace_state=True)
    twin = ChainedReplay(steps, n, D, 2, mb.device, obs_dtype=dtype)
    o, met, ps, dps, stats = eager_eval(mb, policy, twin, steps, mb.reset(5), {}, shapes)
    torch.cuda.synchronize()
    for k in RING:
        assert torch.equal(getattr(ring, k), getattr(twin, k)), k
    assert ring.cur == steps and ring.count == steps and torch.equal(obs, o)
    assert np.array_equal(tr.metrics.cpu().numpy(), met.cpu().numpy(), equal_nan=True)
    assert torch.equal(tr.p, ps) and torch.equal(tr.dp, dps)
    assert np.array_equal(tr.reward_stats.cpu().numpy(), stats)
    assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), mb.get_state()))
    sb.close(); mb.close()


def test_a_narrow_handle_is_still_refused():
    from marl_llm_amd._lib import SwarmError
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP, rollout_device
    sb = batch(one_shape_set(True), torch.float32)
    narrow = FusedPolicy(PolicyMLP(192, 2, 180).cuda())
    assert narrow.wide is False
    with pytest.raises(SwarmError, match="policy in_dim 192 != env obs_dim 232"):
        rollout_device(sb, narrow, 2, reset=(1, 0))
    sb.close()
