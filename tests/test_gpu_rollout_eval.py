"""Device evaluation rollouts (rollout_eval -> swarm_rollout_eval, SwarmBatch.select_shape -> swarm_select_shape): the loop of
eval_assembly.py:145-186 in one library call.  Everything here is a re-ordering of entry points that are already pinned to
the oracle, so every comparison is exact: the loop equals the eager loop built from the entry points that existed before
it (FusedPolicy.__call__, SwarmBatch.set_cells + observe, metrics, step, get_state), its metrics equal the oracle's
restatement of the wrapper, and a rejected call leaves everything as it was."""
import ctypes

import numpy as np
import pytest

from helpers import shape_batch as make_batch
from test_eval_boundary_cases import boundary_cases, near_tie_states

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RING = ("obs", "act", "rew", "done", "act_prior")


def shape_arrays(shapes):
    """The shape set in the uploaded layout: cells [S, 2, ng_max] zero padded, n_g [S], l_cell [S]."""
    grids = [np.asarray(g, np.float64).T for g in shapes["grid_coords"]]
    ng_max = max(g.shape[1] for g in grids)
    cells = np.zeros((len(grids), 2, ng_max)); n_g = np.zeros(len(grids), np.int32)
    for k, g in enumerate(grids):
        cells[k, :, : g.shape[1]] = g; n_g[k] = g.shape[1]
    return cells, n_g, np.asarray(shapes["l_cell"], np.float64)


def eager_switch(sb, shapes, s):
    cells, n_g, l_cell = shape_arrays(shapes)
    E = sb.n_env
    sb.set_cells(np.repeat(cells[s][None], E, 0), np.full(E, n_g[s], np.int32), np.full(E, l_cell[s]))
    return sb.observe()


def eager_eval(sb, policy, ring, steps, obs, sched, shapes):
    """eval_assembly.py:145-186 from the entry points that existed before swarm_rollout_eval; fills `ring` slots 0..steps."""
    E, N = sb.n_env, sb.n_agents
    n = E * N
    met, ps, dps, stats = [], [], [], []
    obs = obs.clone()
    for t in range(steps):
        p, dp = sb.get_state()
        ps.append(p.clone()); dps.append(dp.clone())
        if sched.get(t) is not None:
            eager_switch(sb, shapes, sched[t])
        met.append(sb.metrics().clone())
        act = policy(obs.reshape(n, -1), noise_scale=0).clone()
        nobs, rew, done, pri = sb.step(act.view(E, N, 2))
        ring.obs[t] = obs.reshape(n, -1); ring.obs[t + 1] = nobs.reshape(n, -1)
        ring.act[t] = act; ring.rew[t] = rew.reshape(n, 1); ring.done[t] = done.reshape(n, 1); ring.act_prior[t] = pri.reshape(n, 2)
        c = float(rew.double().sum().item()); m = c / n; a = 1.0 - m          # include/swarm_rollout.h 'Reward statistics'
        stats.append([m, np.sqrt((c * (a * a) + (n - c) * (m * m)) / n)])
        obs = nobs.clone()
    return obs, torch.stack(met), torch.stack(ps), torch.stack(dps), np.array(stats)


def run_pair(shapes, policy, E, N, dtype, steps, sched, seed=5):
    from marl_llm_amd.rollout import ChainedReplay, rollout_eval
    n = E * N
    sb, mb = make_batch(shapes, E, N, dtype), make_batch(shapes, E, N, dtype)
    ring = ChainedReplay(steps, n, sb.obs_dim, 2, sb.device, obs_dtype=dtype)
    obs, tr = rollout_eval(sb, policy, steps, reset=(seed, 0), replay=ring, switch=sched, trace_state=True)
    twin = ChainedReplay(steps, n, mb.obs_dim, 2, mb.device, obs_dtype=dtype)
    o = mb.reset(seed)
    o, met, ps, dps, stats = eager_eval(mb, policy, twin, steps, o, sched, shapes)
    torch.cuda.synchronize()
    for k in RING:
        assert torch.equal(getattr(ring, k), getattr(twin, k)), k
    assert ring.cur == steps and ring.count == steps and torch.equal(obs, o)
    assert torch.equal(tr.metrics, met) or np.array_equal(tr.metrics.cpu().numpy(), met.cpu().numpy(), equal_nan=True)
    assert torch.equal(tr.p, ps) and torch.equal(tr.dp, dps)
    assert np.array_equal(tr.reward_stats.cpu().numpy(), stats)
    assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), mb.get_state()))
    return sb, mb, ring, tr, obs, o


@pytest.fixture(scope="module", params=["bf16", "bf16x3"])
def policy(request):
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP
    torch.manual_seed(0)
    return FusedPolicy(PolicyMLP(192, 2, 180).cuda(), precision=request.param)


@pytest.fixture(scope="module")
def policy16():
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP
    torch.manual_seed(0)
    return FusedPolicy(PolicyMLP(192, 2, 180).cuda())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,E", [(30, 16), (64, 64)])
def test_eval_loop_equals_the_eager_loop(shapes, policy, N, E, dtype):
    n_g = [np.asarray(g).shape[0] for g in shapes["grid_coords"]]
    assert n_g[4] != n_g[5]                                        # the switches change n_g
    sb, mb, ring, tr, _, _ = run_pair(shapes, policy, E, N, dtype, 40, {0: 4, 17: 5})
    assert tr.shape.tolist() == [4] * 17 + [5] * 23 and sb.shape_in_force == 5
    assert not torch.equal(tr.metrics[16], tr.metrics[17])
    sb.close(); mb.close()


def test_trace_metrics_equal_the_oracle(shapes, policy16):
    from marl_llm_amd.shapes import r_avoid_for
    from oracle.oracle_py import wrapper_metrics
    E, N, steps = 6, 30, 24
    sb, mb, ring, tr, _, _ = run_pair(shapes, policy16, E, N, torch.float32, steps, {0: 2, 11: 6})
    cells, n_g, _ = shape_arrays(shapes)
    ra = r_avoid_for(N, shapes)
    p, m = tr.p.cpu().numpy(), tr.metrics.cpu().numpy()
    for t in (0, 1, 10, 11, 12, 23):
        s = int(tr.shape[t])
        assert s == (2 if t < 11 else 6)
        for e in (0, 3, 5):
            ref = wrapper_metrics(p[t, e], np.ascontiguousarray(cells[s][:, : n_g[s]]), ra)
            assert np.array_equal(m[t, e], ref, equal_nan=True), (t, e, m[t, e], ref)
    sb.close(); mb.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_without_switch_it_is_the_deterministic_device_rollout(shapes, policy16, dtype):
    from marl_llm_amd import _lib
    from marl_llm_amd.rollout import ChainedReplay, _ring_struct, rollout_device, rollout_eval
    E, N, steps = 9, 32, 7
    n = E * N
    rings, stats = [], []
    for mode in ("device", "eval", "abi"):
        sb = make_batch(shapes, E, N, dtype)
        ring = ChainedReplay(4, n, sb.obs_dim, 2, sb.device, obs_dtype=dtype)       # 7 > slots: the ring wraps
        if mode == "device":
            obs, st = rollout_device(sb, policy16, steps, reset=(3, 1), replay=ring, noise_scale=0.0, epsilon=0.0)
        elif mode == "eval":
            obs, tr = rollout_eval(sb, policy16, steps, reset=(3, 1), replay=ring)
            st = tr.reward_stats
            assert tr.p is None and tr.dp is None and tr.shape.tolist() == [-1] * steps
        else:                                                                         # no metrics at all: out = NULL
            sb.reset(3, 1, out=ring.obs[0])
            r = _ring_struct(sb, ring)
            rc = sb.lib.swarm_rollout_eval(sb.handle, policy16.handle, ctypes.byref(r), steps, None, None,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, sb.lib.swarm_rollout_last_error()
            st = None
        torch.cuda.synchronize()
        rings.append({k: getattr(ring, k).clone() for k in RING}); stats.append(st)
        sb.close()
    for other in rings[1:]:
        assert all(torch.equal(rings[0][k], other[k]) for k in RING)
    assert torch.equal(stats[0], stats[1])


def test_handle_after_the_call_and_select_shape_alone(shapes, policy16):
    E, N = 8, 30
    sb, mb, ring, tr, obs, o = run_pair(shapes, policy16, E, N, torch.float32, 12, {3: 1, 9: 3})
    cells, n_g, _ = shape_arrays(shapes)
    assert torch.equal(sb.metrics(), mb.metrics())
    c1, g1 = sb.get_cells(); c2, g2 = mb.get_cells()
    assert np.array_equal(c1, c2) and np.array_equal(g1, g2) and np.array_equal(c1[0], cells[3]) and (g1 == n_g[3]).all()
    assert (sb.get_shape_index() == 3).all() and sb.lattice_envs() == mb.lattice_envs() == E
    act = policy16(obs.reshape(E * N, -1), noise_scale=0).view(E, N, 2)
    assert all(torch.equal(x, y) for x, y in zip(sb.step(act), mb.step(act)))
    # select_shape on its own against set_cells + observe, mid-trajectory
    oa = sb.select_shape(5).clone()
    ob = eager_switch(mb, shapes, 5).clone()
    assert torch.equal(oa, ob) and (sb.get_shape_index() == 5).all() and (mb.get_shape_index() == -1).all()
    assert sb.shape_in_force == 5 and sb.lattice_envs() == mb.lattice_envs()
    ia, ib = sb.indices(), mb.indices()
    assert all(torch.equal(ia[k], ib[k]) for k in ia)
    assert torch.equal(sb.metrics(), mb.metrics())
    c1, g1 = sb.get_cells(); c2, g2 = mb.get_cells()
    assert np.array_equal(c1, c2) and np.array_equal(g1, g2)
    for _ in range(3):
        ra, rb = sb.step(act), mb.step(act)
        assert all(torch.equal(x, y) for x, y in zip(ra, rb))
    out = torch.empty((E, N, sb.obs_dim), device=sb.device)
    assert sb.select_shape(0, out=out).data_ptr() == out.data_ptr() and torch.equal(out, eager_switch(mb, shapes, 0))
    sb.close(); mb.close()


@pytest.mark.parametrize("flags", [0, 1])
def test_loop_metrics_on_the_decision_boundaries(policy16, flags):
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.rollout import rollout_eval
    from oracle.oracle_py import wrapper_metrics
    ra = 0.37
    cases = boundary_cases(ra)
    E, N, G = len(cases), 4, 4
    sb = SwarmBatch(n_env=E, n_agents=N, n_cells_max=G, r_avoid=ra, debug_flags=flags)
    cells = np.zeros((E, 2, G)); n_g = np.zeros(E, np.int32)
    for e, (p, g) in enumerate(cases):
        cells[e, :, : g.shape[1]] = g; n_g[e] = g.shape[1]
    sb.set_cells(cells, n_g, np.full(E, 0.06))
    p = np.stack([c[0] for c in cases])
    sb.set_state(p, np.zeros_like(p))
    obs = sb.observe()
    want = sb.metrics().cpu().numpy()
    _, tr = rollout_eval(sb, policy16, 2, obs=obs, trace_state=True)
    got = tr.metrics.cpu().numpy()
    assert np.array_equal(tr.p[0].cpu().numpy(), p)
    for e, (pe, g) in enumerate(cases):
        ref = wrapper_metrics(pe, g, ra)
        assert np.array_equal(got[0, e], ref, equal_nan=True), (e, got[0, e], ref)
    assert np.array_equal(got[0], want, equal_nan=True)
    assert np.array_equal(got[1], sb_metrics_of(sb, tr.p[1], tr.dp[1]), equal_nan=True)
    sb.close()


def test_loop_metrics_with_nan_positions(policy16):
    """NaN inputs give swarm_metrics' bits too: a NaN agent never covers a cell, but as agent 0 it seeds np.argmin's running
    minimum and then owns every cell."""
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.rollout import rollout_eval
    ra = 0.37
    cases = boundary_cases(ra)
    E, N, G = len(cases), 4, 4
    sb = SwarmBatch(n_env=E, n_agents=N, n_cells_max=G, r_avoid=ra)
    cells = np.zeros((E, 2, G)); n_g = np.zeros(E, np.int32)
    for e, (p, g) in enumerate(cases):
        cells[e, :, : g.shape[1]] = g; n_g[e] = g.shape[1]
    sb.set_cells(cells, n_g, np.full(E, 0.06))
    p = np.stack([c[0] for c in cases])
    p[1, :, 0] = np.nan; p[3, 0, 0] = np.nan; p[4, :, 1] = np.nan; p[5, 1, 3] = np.nan; p[6, :, :] = np.nan
    sb.set_state(p, np.zeros_like(p))
    obs = sb.observe()
    want = sb.metrics().cpu().numpy()
    _, tr = rollout_eval(sb, policy16, 1, obs=obs)
    got = tr.metrics.cpu().numpy()[0]
    assert np.array_equal(got, want, equal_nan=True), (got, want)
    assert want[1, 0] == 0.0 and want[5, 0] == 1.0                 # the NaN agent covers nothing; the others still do
    sb.close()


def sb_metrics_of(sb, p, dp):
    """swarm_metrics of a recorded state (the handle's state is put back afterwards)."""
    keep = [x.clone() for x in sb.get_state()]
    sb.set_state(p, dp)
    m = sb.metrics().cpu().numpy()
    sb.set_state(*keep); sb.observe()
    return m


@pytest.mark.parametrize("N,E", [(2, 5), (7, 5), (8, 9), (30, 6), (64, 5), (129, 3), (130, 3), (250, 2), (256, 2),
                                 (2, 2050), (30, 2049), (64, 2051), (130, 2049), (256, 2049)])
def test_loop_metrics_across_the_size_classes(shapes, policy16, N, E):
    """The loop's metrics kernel against swarm_metrics (k_metrics, its in-repo reference) and the oracle: N below / at numpy's
    8-accumulator threshold, around its 128-element block (129, 130, 250 split into unequal and nested halves), the cap 256;
    small batches (four waves per env) and batches of 8 envs per compute unit or more (one wave per env, four envs per
    workgroup, E not a multiple of four)."""
    from marl_llm_amd.rollout import rollout_eval
    from marl_llm_amd.shapes import r_avoid_for
    from oracle.oracle_py import wrapper_metrics
    sb = make_batch(shapes, E, N)
    _, tr = rollout_eval(sb, policy16, 12, reset=(8, 0), switch={1: 2}, trace_state=True)
    cells, n_g, _ = shape_arrays(shapes)
    p, m = tr.p.cpu().numpy(), tr.metrics.cpu().numpy()
    for t in (1, 6, 11):
        assert np.array_equal(m[t], sb_metrics_of(sb, tr.p[t], tr.dp[t]), equal_nan=True), t
        for e in range(min(E, 3)):
            ref = wrapper_metrics(p[t, e], np.ascontiguousarray(cells[2][:, : n_g[2]]), r_avoid_for(N, shapes))
            assert np.array_equal(m[t, e], ref, equal_nan=True), (t, e, m[t, e], ref)
    sb.close()


def test_loop_metrics_on_near_ties(policy16):
    """Hundreds of cells whose two nearest agents are within a few ulps of each other in squared distance (the kernel's exact
    fallback), and agents within a few ulps of r_avoid / 2 of a cell: swarm_metrics and the oracle, exactly."""
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.rollout import rollout_eval
    from oracle.oracle_py import wrapper_metrics
    ra = 0.37
    p, cells = near_tie_states(ra)
    E, _, N = p.shape
    G = cells.shape[2]
    sb = SwarmBatch(n_env=E, n_agents=N, n_cells_max=G, r_avoid=ra)
    sb.set_cells(cells, np.full(E, G, np.int32), np.full(E, 0.06))
    sb.set_state(p, np.zeros_like(p))
    obs = sb.observe()
    want = sb.metrics().cpu().numpy()
    _, tr = rollout_eval(sb, policy16, 1, obs=obs)
    got = tr.metrics.cpu().numpy()[0]
    assert np.array_equal(got, want, equal_nan=True)
    for e in range(E):
        assert np.array_equal(got[e], wrapper_metrics(p[e], cells[e], ra), equal_nan=True), e
    sb.close()


def test_a_non_lattice_shape_in_the_set(shapes, policy16):
    jit = {k: list(v) for k, v in shapes.items()}
    g = np.array(jit["grid_coords"][1], np.float64)
    jit["grid_coords"][1] = g + np.random.RandomState(0).uniform(-2e-3, 2e-3, g.shape)
    E, N = 10, 30
    sb, mb, ring, tr, _, _ = run_pair(jit, policy16, E, N, torch.float32, 30, {0: 0, 8: 1, 19: 2})
    assert sb.lattice_envs() == mb.lattice_envs() == E
    sb.select_shape(1); eager_switch(mb, jit, 1)
    assert sb.lattice_envs() == mb.lattice_envs() == 0
    sb.select_shape(0); eager_switch(mb, jit, 0)
    assert sb.lattice_envs() == mb.lattice_envs() == E
    act = torch.zeros((E, N, 2), device=sb.device)
    assert all(torch.equal(x, y) for x, y in zip(sb.step(act), mb.step(act)))
    sb.close(); mb.close()


def test_rejected_calls_change_nothing(shapes, policy16):
    from marl_llm_amd import _lib
    from marl_llm_amd.env import AssemblySwarmEnv, make_args
    from marl_llm_amd.rollout import ChainedReplay, _ring_struct, rollout_eval
    E, N = 4, 30
    n = E * N
    S = len(shapes["l_cell"])

    def unchanged(sb, ring, fn, exc, match):
        before = {k: getattr(ring, k).clone() for k in RING}
        counters = (ring.cur, ring.count, ring._chained, set(ring._sealed))
        state = [x.clone() for x in sb.get_state()]
        cells = sb.get_cells()
        with pytest.raises(exc, match=match):
            fn()
        torch.cuda.synchronize()
        assert all(torch.equal(getattr(ring, k), v) for k, v in before.items())
        assert (ring.cur, ring.count, ring._chained, set(ring._sealed)) == counters
        assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), state))
        assert all(np.array_equal(x, y) for x, y in zip(sb.get_cells(), cells))

    sb = make_batch(shapes, E, N)
    ring = ChainedReplay(6, n, sb.obs_dim, 2, sb.device)
    obs, _ = rollout_eval(sb, policy16, 2, reset=(1, 0), replay=ring)
    unchanged(sb, ring, lambda: rollout_eval(sb, policy16, 3, replay=ring, switch={1: S}), ValueError, "outside")
    unchanged(sb, ring, lambda: rollout_eval(sb, policy16, 3, reset=(1, 1), replay=ring, switch=[0, S + 3, -1]), ValueError, "outside")
    unchanged(sb, ring, lambda: rollout_eval(sb, policy16, 3, replay=ring, switch={3: 0}), ValueError, "switch")
    # through the C ABI: a schedule entry out of range, p without dp
    lib, stream = sb.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def abi(sw, out, code, msg):
        def f():
            r = _ring_struct(sb, ring)
            rc = lib.swarm_rollout_eval(sb.handle, policy16.handle, ctypes.byref(r), 3,
                                        sw.ctypes.data_as(ctypes.c_void_p) if sw is not None else None, out, stream)
            assert rc == code, rc
            raise _lib.SwarmError(lib.swarm_rollout_last_error().decode())
        unchanged(sb, ring, f, _lib.SwarmError, msg)

    abi(np.array([-1, S, 0], np.int32), None, 1, "swarm_rollout_eval: switch_to")
    abi(np.array([-2, 0, 0], np.int32), None, 1, "swarm_rollout_eval: switch_to")
    pbuf = torch.empty((3, E, 2, N), dtype=torch.float64, device=sb.device)
    abi(None, ctypes.byref(_lib.SwarmEvalOut(None, pbuf.data_ptr(), None, None)), 1, "p and dp together")
    assert lib.swarm_select_shape(sb.handle, S, None) == 1 and lib.swarm_select_shape(sb.handle, -1, None) == 1
    # no shape set
    nb = make_batch(shapes, E, N, upload=False)
    cells, n_g, l_cell = shape_arrays(shapes)
    nb.set_cells(np.repeat(cells[0][None], E, 0), np.full(E, n_g[0], np.int32), np.full(E, l_cell[0]))
    nb.set_state(*sb.get_state())
    o = nb.observe()
    nring = ChainedReplay(3, n, nb.obs_dim, 2, nb.device)
    unchanged(nb, nring, lambda: rollout_eval(nb, policy16, 3, obs=o, replay=nring, switch={0: 0}), _lib.SwarmError, "shape set")
    with pytest.raises(_lib.SwarmError, match="no shape set"):
        nb.select_shape(0)
    r = _ring_struct(nb, nring)
    nring.obs[0] = o.reshape(n, -1)
    sw = np.array([0, -1, -1], np.int32)
    assert lib.swarm_rollout_eval(nb.handle, policy16.handle, ctypes.byref(r), 3, sw.ctypes.data_as(ctypes.c_void_p), None, stream) == 3
    assert b"shape set" in lib.swarm_rollout_last_error()
    # an AssemblySwarmEnv takes no switch=
    env = AssemblySwarmEnv(n_envs=E, obs_dtype="float32", rng="device", seed=7)
    env.__reinit__(make_args(n_a=16, results_file=shapes))
    eo = env.reset_tensor()
    t0 = env.simulation_time
    with pytest.raises(ValueError, match="switch="):
        rollout_eval(env, policy16, 3, obs=eo, switch={0: 1})
    assert env.simulation_time == t0
    # everything still works
    _, tr = rollout_eval(sb, policy16, 2, replay=ring, switch={0: 1})
    _, tr2 = rollout_eval(nb, policy16, 2, obs=o, replay=nring)
    torch.cuda.synchronize()
    assert tr.metrics.shape == (2, E, 3) and tr2.shape.tolist() == [-1, -1]
    env.close(); sb.close(); nb.close()


def test_assembly_env_time_and_fresh_metrics(shapes, policy16):
    from marl_llm_amd.env import AssemblySwarmEnv, make_args
    from marl_llm_amd.rollout import rollout_eval
    env = AssemblySwarmEnv(n_envs=4, obs_dtype="float32", rng="device", seed=77)
    env.__reinit__(make_args(n_a=16, results_file=shapes))
    obs = env.reset_tensor()
    m0 = env.metrics_tensor().clone()
    obs, tr = rollout_eval(env, policy16, 5, obs=obs, trace_state=True)
    assert torch.equal(tr.metrics[0], m0)
    m1 = env.metrics_tensor().clone()                              # the would-be metrics[5], not the cached m0
    assert torch.equal(m1, env._backend().metrics()) and not torch.equal(m1, m0)
    assert abs(env.simulation_time - 5 * env.dt) < 1e-12 and obs.shape == (4, 16, 192)
    obs, tr2 = rollout_eval(env, policy16, 2, obs=obs, trace_state=True)
    assert torch.equal(tr2.metrics[0], m1) and abs(env.simulation_time - 7 * env.dt) < 1e-12
    p, _ = env._backend().get_state()
    assert not torch.equal(tr2.p[1], tr2.p[0]) and tr2.p.shape == (2, 4, 2, 16) and not torch.equal(p, tr2.p[1])
    env.close()
