"""The rule-based expert above 256 agents: k_rule_large (csrc/rule_expert.hip) behind swarm_rule_action and
swarm_rollout_expert on large_swarm handles of 257 to 1024 agents, and behind debug_flags bit 5 on default handles, where it
must write the bits k_rule writes.

What holds it.  Below 257 agents the two kernels run on identical export lists (default handles, debug_flags 0 against 32)
and every output is compared as bits.  Above, the fp64 action is held to the float64 restatement oracle_py.rule_action under
test_gpu_rule_contract.py's rules (compare() below is that module's: equal NaN masks, exactly +-1 on saturated components,
1e-12 absolute on unsaturated ones -- the only inexact operation is cos, see that module) on calm inputs whose conditions are
asserted from the restatement alone (large_rule_inputs.py; test_large_rule_host.py asserts them on the CPU), the fused loop to
the eager one bit for bit, and the surfaces (AssemblySwarmEnv, tools/collect_expert.py) to an eager twin.

Whether the loaded library honours bit 5 cannot be seen from a default handle -- the bit changes no output by design -- so
the same-bits tests ask the library whether it has k_rule_large at all: a large handle of 257 agents either serves
rule_action() or refuses it with the parent's message.  A library that refuses SKIPS those tests; it does not pass them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import calm_batch, calm_case, pad_cells, rule_details, shape_batch
from large_rule_inputs import ENVS, large_calm_reference

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-12                 # test_gpu_rule_contract.py
D_SEN = 0.4
RING = ("obs", "act", "rew", "done", "act_prior")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- plumbing (bits_equal and compare are test_gpu_rule_contract.py's) -------------------------------------------------
def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def compare(got, want, info, what=""):
    """got, want [E, 2, N]: equal NaN masks; 1e-12 where the restatement's unclipped |sum| < 1; exactly the reference's +-1
    elsewhere.  Returns the number of unsaturated components compared."""
    raw = info["raw"]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN masks differ", np.argwhere(np.isnan(got) != nan)[:4])
    with np.errstate(invalid="ignore"):
        free = np.abs(raw) < 1
    sat = ~free & ~nan
    assert np.array_equal(got[sat], want[sat]), (what, "saturated components", np.argwhere(sat & (got != want))[:4])
    err = np.abs(got[free] - want[free])
    print(f"{what}: {free.sum()} unsaturated of {free.size} components, max |err| {err.max() if err.size else 0:.3g}")
    assert err.size == 0 or err.max() <= TOL, (what, float(err.max()), np.argwhere(free & (np.abs(got - want) > TOL))[:4])
    return int(free.sum())


def make_batch(cases, r_avoid, dtype=torch.float32, **kw):
    from marl_llm_amd.batched import SwarmBatch
    cells, n_g = pad_cells([c[2] for c in cases], max(c[2].shape[1] for c in cases))
    sb = SwarmBatch(n_env=len(cases), n_agents=cases[0][0].shape[1], n_cells_max=cells.shape[2], r_avoid=r_avoid, obs_dtype=dtype, **kw)
    sb.set_cells(cells, n_g, [c[3] for c in cases])
    sb.set_state(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]))
    return sb


def ring_for(sb, K):
    from marl_llm_amd.rollout import ChainedReplay
    return ChainedReplay(K, sb.n_env * sb.n_agents, sb.obs_dim, 2, sb.device, obs_dtype=sb.obs_dtype)


def snapshot(sb, ring):
    return [x.clone() for x in sb.get_state()], {k: getattr(ring, k).clone() for k in RING}, ring.cur, ring.count


def assert_untouched(sb, ring, before):
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before[0], sb.get_state()))
    assert all(torch.equal(before[1][k], getattr(ring, k)) for k in RING) and (ring.cur, ring.count) == before[2:]


def large_actions(cases, r_avoid, dtype=torch.float32, **kw):
    """swarm_rule_action's fp64 action [E, 2, N] (numpy) of a large handle on `cases`; through rollout_expert(sb, 1) -- the
    instantiation with the f32 row -- the act row must be its f32 rounding and the step must have consumed the action itself."""
    from marl_llm_amd.rollout import rollout_expert
    sb = make_batch(cases, r_avoid, dtype, large_swarm=True, **kw)
    twin = make_batch(cases, r_avoid, dtype, large_swarm=True, **kw)
    try:
        obs = sb.observe()
        u = sb.rule_action().clone()
        ring = ring_for(sb, 1)
        rollout_expert(sb, 1, obs=obs, replay=ring, track_reward=False)
        assert bits_equal(ring.act[0].view(sb.n_env, sb.n_agents, 2), u.float())
        twin.observe()
        twin.step(u)
        for a, b in zip(sb.get_state(), twin.get_state()):
            assert bits_equal(a, b)
        return u.cpu().numpy().transpose(0, 2, 1)
    finally:
        sb.close(); twin.close()


# ---- 1. the same bits as k_rule, where k_rule exists ------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiled_kernel(shapes):
    """Skips unless the loaded library has k_rule_large (see the module's docstring)."""
    from marl_llm_amd._lib import SwarmError
    sb = shape_batch(shapes, 1, 257, large_swarm=True)
    try:
        sb.reset(seed=1)
        try:
            sb.rule_action()
        except SwarmError as e:
            if "256" in str(e):
                pytest.skip("this library has no k_rule_large: it ignores debug_flags bit 5, nothing to compare")
            raise
    finally:
        sb.close()


VARIANTS = {"f32": dict(), "bf16": dict(dtype=torch.bfloat16), "generic": dict(debug_flags=2), "cap45": dict(g_max=45)}


def _expert_run(cases, r_avoid, flags, dtype=torch.float32, **kw):
    """rule_action() and a three-step expert rollout of a default handle: (u, ring act / obs / rew, final state)."""
    from marl_llm_amd.rollout import rollout_expert
    sb = make_batch(cases, r_avoid, dtype, debug_flags=flags, **kw)
    try:
        obs = sb.observe()
        u = sb.rule_action().clone()
        ring = ring_for(sb, 3)
        rollout_expert(sb, 3, obs=obs, replay=ring, track_reward=False)
        torch.cuda.synchronize()
        return [u, ring.act.clone(), ring.obs.clone(), ring.rew.clone()] + [x.clone() for x in sb.get_state()]
    finally:
        sb.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n_a", [1, 7, 64, 65, 200, 256])
def test_same_bits_as_k_rule(tiled_kernel, shapes, n_a, variant):
    """Default handles, debug_flags without and with bit 5 (k_rule / k_rule_large on the same export lists): rule_action(),
    and through rollout_expert(sb, 3) the ring's act, obs and rew and the final state, all as bits (NaN included).  One
    agent, a partial first tile, a full tile, one agent past it, a partial last tile and k_rule's cap; float32 and bfloat16
    rows, the generic export, and an odd list cap (ties of the subsample rounded to even)."""
    from marl_llm_amd.shapes import r_avoid_for
    kw = dict(VARIANTS[variant])
    base = kw.pop("debug_flags", 0)
    r_avoid = r_avoid_for(n_a, shapes)
    cases = calm_batch(shapes, n_a, r_avoid, seed=1, agents=1536)
    a = _expert_run(cases, r_avoid, base, **kw)
    b = _expert_run(cases, r_avoid, base | 32, **kw)
    for k, (x, y) in enumerate(zip(a, b)):
        assert bits_equal(x, y), ("u", "act", "obs", "rew", "p", "dp")[k]
    assert bool((a[0].abs() < 1).any()) and bool((a[1] != 0).any())


def test_same_bits_on_non_finite_states(tiled_kernel, shapes):
    """Coincident agents (r_avoid / 0 * 0 = NaN) and NaN state components: the NaNs of the two kernels are the same bits."""
    from marl_llm_amd.shapes import r_avoid_for
    n_a = 200
    r_avoid = r_avoid_for(n_a, shapes)
    rng = np.random.default_rng(8)
    cases = []
    for k in range(6):
        p, dp, g, l_cell = calm_case(rng, shapes, n_a, r_avoid)
        i, j = rng.choice(n_a, 2, replace=False)
        if k % 3 == 0:
            p[:, j] = p[:, i]
        elif k % 3 == 1:
            p[int(rng.integers(0, 2)), i] = np.nan
        else:
            dp[int(rng.integers(0, 2)), i] = np.nan
        cases.append((p, dp, g, l_cell))
    out = []
    for flags in (0, 32):
        sb = make_batch(cases, r_avoid, debug_flags=flags)
        sb.observe()
        out.append(sb.rule_action().clone())
        sb.close()
    assert bits_equal(out[0], out[1])
    assert bool(torch.isnan(out[0]).any(dim=2).any(dim=1).all()) and bool(torch.isfinite(out[0]).any())


# ---- 2. the restatement above 256 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a", sorted(ENVS))
def test_calm_states_match_the_restatement(shapes, n_a):
    """Large handles at 257 (one agent past four tiles), 300, 513 and 1024 (the cap: sixteen full tiles)."""
    cases, r_avoid, want, info = large_calm_reference(shapes, n_a)
    got = large_actions(cases, r_avoid)
    n = compare(got, want, info, f"N={n_a}")
    assert 3 * n >= want.size


@pytest.mark.parametrize("variant", ["generic", "bf16", "f64"])
def test_calm_states_at_300_on_other_handles(shapes, variant):
    """debug_flags 2 (large handles ignore every bit), bfloat16 and float64 rows: the same fp64 bits as the float32 handle."""
    from marl_llm_amd.rollout import rollout_expert
    cases, r_avoid, want, info = large_calm_reference(shapes, 300)
    ref = large_actions(cases, r_avoid)
    if variant == "f64":                           # (swarm_rollout_expert rejects fp64 rows: rule_action only)
        sb = make_batch(cases, r_avoid, torch.float64, large_swarm=True)
        sb.observe()
        got = sb.rule_action().cpu().numpy().transpose(0, 2, 1)
        sb.close()
    else:
        got = large_actions(cases, r_avoid, **(dict(debug_flags=2 | 32) if variant == "generic" else dict(dtype=torch.bfloat16)))
    compare(got, want, info, f"N=300 {variant}")
    assert got.tobytes() == ref.tobytes()


# ---- 3. fused equals eager above 256 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["rule", "llm"])
@pytest.mark.parametrize("n_a", [300, 1024])
def test_fused_equals_the_eager_loop(shapes, n_a, source):
    """rollout_expert(sb, 4) against `u = rule_action(); step(u)` ('llm': `step(None)` on llm_action handles) on a twin from
    the same device reset: ring, final state and reward statistics."""
    from marl_llm_amd.rollout import rollout_expert
    E, K = 2, 4
    kw = dict(large_swarm=True, llm_action=(source == "llm"))
    sb, twin = shape_batch(shapes, E, n_a, **kw), shape_batch(shapes, E, n_a, **kw)
    try:
        ring = ring_for(sb, K)
        obs, stats = rollout_expert(sb, K, replay=ring, reset=(11, n_a), source=source)
        assert ring.cur == K and obs.data_ptr() == ring.obs[K].data_ptr()
        o = twin.reset(11, n_a)
        assert torch.equal(ring.obs[0].view_as(o), o)
        n = E * n_a
        for t in range(K):
            u = twin.rule_action() if source == "rule" else twin.llm_action()
            o, rew, done, pri = twin.step(u if source == "rule" else None)
            assert bits_equal(ring.act[t], u.float().view(n, 2)), t
            assert bits_equal(ring.obs[t + 1], o.view(n, -1)), t
            assert torch.equal(ring.rew[t], rew.view(n, 1)) and torch.equal(ring.done[t], done.view(n, 1)), t
            assert torch.equal(ring.act_prior[t], pri.view(n, 2)), t
        for a, b in zip(sb.get_state(), twin.get_state()):
            assert bits_equal(a, b)
        assert bool((ring.act[:K].abs() < 1).any()) and bool((ring.act[:K] != 0).any())
        # reward statistics: (mean, population std) of every step's rewards; the mean is count / rows, one IEEE division
        r, st = ring.rew[:K, :, 0].double().cpu().numpy(), stats.cpu().numpy()
        assert np.array_equal(st[:, 0], r.sum(1) / r.shape[1])
        np.testing.assert_allclose(st[:, 1], r.std(1), rtol=1e-12, atol=0)
    finally:
        sb.close(); twin.close()


# ---- 4. thresholds at N = 300 -----------------------------------------------------------------------------------------
def straddle(norm, target, t0):
    """t_lo, t_hi: adjacent doubles around t0 with norm(t_lo) < target <= norm(t_hi) (test_gpu_rule_contract.py's)."""
    t = t0
    for _ in range(4096):
        if norm(t) < target:
            break
        t = np.nextafter(t, -np.inf)
    for _ in range(4096):
        if not norm(np.nextafter(t, np.inf)) < target:
            break
        t = np.nextafter(t, np.inf)
    assert norm(t) < target <= norm(np.nextafter(t, np.inf))
    return t, np.nextafter(t, np.inf)


def threshold_scene(rng, shapes, n_a, r_avoid, target):
    """Four envs of one calm scene: the last agent (tile 4, a partial word) on a ray from agent i, the float64 norm the
    reference computes two and one double below `target`, then on or just past it and one double further."""
    p, dp, g, l_cell = calm_case(rng, shapes, n_a, r_avoid, off_shape=0.0)
    j, i = n_a - 1, int(rng.integers(0, n_a - 1))
    th = rng.uniform(-np.pi, np.pi)
    d = np.array([np.cos(th), np.sin(th)])
    origin = p[:, i].copy()
    norm = lambda t: np.linalg.norm((origin + d * t)[:, None] - p[:, [i]], axis=0)[0]
    lo, hi = straddle(norm, target, target)
    cases = []
    for t, inside in ((np.nextafter(lo, -np.inf), True), (lo, True), (hi, False), (np.nextafter(hi, np.inf), False)):
        assert (norm(t) < target) == inside
        q = p.copy()
        q[:, j] = origin + d * t
        cases.append((q, dp, g, l_cell))
    return cases, i


@pytest.mark.parametrize("kind", ["d_sen", "r_avoid"])
def test_threshold_placements_at_300(shapes, kind):
    """A neighbour whose norm lands one double either side of d_sen (decides n_near) and of r_avoid (decides n_avoid).  Eight
    scenes, kept when the restatement says the two sides differ by exactly that neighbour and the agent has an unsaturated
    component on all four placements: all eight qualify for either threshold; the floor is four."""
    from marl_llm_amd.shapes import r_avoid_for
    n_a = 300
    r_avoid = r_avoid_for(n_a, shapes)
    rng = np.random.default_rng([6, kind == "d_sen"])
    scenes = [threshold_scene(rng, shapes, n_a, r_avoid, D_SEN if kind == "d_sen" else r_avoid) for _ in range(8)]
    cases = [c for s in scenes for c in s[0]]
    want, info = rule_details(cases, r_avoid)
    good = 0
    for k, (_, i) in enumerate(scenes):
        sl = slice(4 * k, 4 * k + 4)
        q = info["n_near" if kind == "d_sen" else "n_avoid"][sl, i]
        with np.errstate(invalid="ignore"):
            unsat = (np.abs(info["raw"][sl, :, i]) < 1).any(axis=1).all()
        good += bool(unsat and q[0] == q[1] and q[2] == q[3] and q[1] == q[2] + 1)
    print(kind, "scenes with a decided difference on an unsaturated agent:", good)
    assert good >= 4
    compare(large_actions(cases, r_avoid), want, info, f"threshold {kind}")


def sparse_scene(rng, nan):
    """300 agents around a 3 x 3 shape: agent 0 on it, its own r_avoid / 2 disc over all nine cells (sensed, all filtered:
    v_exp exactly 0); agent 1 its one neighbour; agent 2 alone in a corner (n_near == 0: no division); the rest on a coarse
    grid away from the shape.  nan: a NaN position component in one grid agent, a NaN velocity component in another."""
    n_a, l_cell = 300, 0.06
    xs = (np.arange(3) - 1) * l_cell
    g = np.ascontiguousarray(np.stack([np.tile(xs, 3), np.repeat(xs, 3)]))
    th = rng.uniform(-np.pi, np.pi)
    corner = np.array([2.25, 2.25])
    pts = np.array([(x, y) for x in np.arange(-9, 10) * 0.25 for y in np.arange(-9, 10) * 0.25])
    pts = pts[(np.linalg.norm(pts, axis=1) > 0.9) & (np.linalg.norm(pts - corner, axis=1) > 0.45)]
    pts = pts[rng.permutation(len(pts))[: n_a - 3]] + rng.uniform(-0.01, 0.01, (n_a - 3, 2))
    p = np.concatenate([rng.uniform(-0.01, 0.01, (1, 2)), rng.uniform(0.3, 0.39) * np.array([[np.cos(th), np.sin(th)]]), corner[None], pts]).T
    dp = rng.uniform(-0.05, 0.05, (2, n_a))
    if nan:
        p[0, 17] = np.nan
        dp[1, 211] = np.nan
    return np.ascontiguousarray(p), dp, g, l_cell


def test_empty_list_lonely_agent_and_nan_at_300():
    r_avoid = 0.22
    rng = np.random.default_rng(3)
    cases = [sparse_scene(rng, nan=k >= 2) for k in range(4)]
    want, info = rule_details(cases, r_avoid)
    assert (info["n_sensed"][:, 0] == 9).all() and (info["n_filtered"][:, 0] == 0).all() and (info["in_flag"][:, 0] == 1).all()
    assert (info["n_near"][:, 0] == 1).all() and (np.abs(info["raw"][:, :, 0]) < 1).all()
    assert (info["n_near"][:, 2] == 0).all() and (info["in_flag"][:, 2] == 0).all()
    assert np.isfinite(want[:2]).all() and np.isnan(want[2:]).any(axis=(1, 2)).all() and np.isfinite(want[2:]).any()
    assert (np.isnan(want[2:]).sum(axis=(1, 2)) > 2).all()              # the NaN velocity reaches the neighbours' sums
    compare(large_actions(cases, r_avoid), want, info, "sparse scenes")


# ---- 5. surfaces --------------------------------------------------------------------------------------------------------
def test_env_rule_mode_with_300_agents(shapes):
    """AssemblySwarmEnv(n_a=300, agent_strategy='rule', is_collected=True): three steps, each returning as its fifth value
    the rule_action() of a twin batch put on the env's state."""
    from marl_llm_amd.env import AssemblySwarmEnv, AssemblySwarmWrapper, make_args
    n_a = 300
    np.random.seed(5)
    env = AssemblySwarmWrapper(AssemblySwarmEnv(), make_args(n_a=n_a, results_file=shapes, agent_strategy="rule", is_collected=True))
    twin = None
    try:
        env.reset()
        b = env.env
        assert b._backend().large_swarm
        g = np.ascontiguousarray(b._cells[0][:, : b._n_g[0]])
        twin = make_batch([(np.zeros((2, n_a)), np.zeros((2, n_a)), g, float(b._l_cell[0]))], b.r_avoid, torch.float64, large_swarm=True)
        for t in range(3):
            p, dp = [x.cpu().numpy() for x in b._backend().get_state()]
            twin.set_state(p, dp)
            twin.observe()
            want = twin.rule_action().cpu().numpy()[0].T
            _, _, _, _, u = env.step(np.zeros((2, n_a), np.float32))
            assert u.shape == (2, n_a) and u.dtype == np.float64 and u.tobytes() == want.tobytes(), t
            assert (np.abs(u) < 1).any()
    finally:
        env.close()
        if twin is not None:
            twin.close()


def test_env_llm_mode_with_300_agents(shapes):
    from marl_llm_amd.env import AssemblySwarmEnv, AssemblySwarmWrapper, make_args
    n_a = 300
    np.random.seed(5)
    env = AssemblySwarmWrapper(AssemblySwarmEnv(), make_args(n_a=n_a, results_file=shapes, agent_strategy="llm", is_collected=True))
    try:
        env.reset()
        for t in range(3):
            want = env.env._backend().llm_action().cpu().numpy()[0].T
            _, _, _, _, u = env.step(np.zeros((2, n_a), np.float32))
            assert u.shape == (2, n_a) and np.array_equal(u, want) and (u != 0).any(), t
    finally:
        env.close()


def test_collect_expert_tool_with_300_agents(shapes, tmp_path):
    """tools/collect_expert.py --n_a 300, 2 episodes x 5 steps: ac_buffs are the f32-rounded rule actions of an eager twin
    from the same device reset, the observations its observations."""
    n_a, E, L = 300, 2, 5
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "collect_expert.py"), "--n_a", str(n_a), "--n_episodes", str(E),
                          "--episode_length", str(L), "--envs-per-call", str(E), "--seed", "226", "--out", str(tmp_path)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert run.returncode == 0, run.stdout
    z = np.load(os.path.join(str(tmp_path), "expert_data.npz"))
    assert z["ac_buffs"].shape == (L * E * n_a, 2) and z["obs_buffs"].shape[0] == L * E * n_a
    twin = shape_batch(shapes, E, n_a, large_swarm=True)
    try:
        obs = twin.reset(226, 0, 0)
        acts, rows, nxt = [], [], []
        for _ in range(L):
            u = twin.rule_action()
            acts.append(u.float().view(E * n_a, 2).cpu().numpy())
            rows.append(obs.view(E * n_a, -1).cpu().numpy().copy())
            obs = twin.step(u)[0]
            nxt.append(obs.view(E * n_a, -1).cpu().numpy().copy())
        assert np.array_equal(z["ac_buffs"], np.concatenate(acts).astype(np.float64))
        assert np.array_equal(z["obs_buffs"], np.concatenate(rows).astype(np.float64))
        assert np.array_equal(z["next_obs_buffs"], np.concatenate(nxt).astype(np.float64))
        assert (np.abs(z["ac_buffs"]) < 1).any()
    finally:
        twin.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def _refused(sb, obs, calls):
    """Every call of `calls` (a message pattern, a function of (sb, ring, obs)) raises, nothing moves, a good step follows."""
    from marl_llm_amd._lib import SwarmError
    ring = ring_for(sb, 4)
    before = snapshot(sb, ring)
    for pattern, call in calls:
        with pytest.raises(SwarmError, match=pattern):
            call(sb, ring, obs)
        assert_untouched(sb, ring, before)
    sb.observe()
    out = sb.step(torch.zeros((sb.n_env, sb.n_agents, 2), device=sb.device))
    assert torch.isfinite(out[0].float()).all()


def _rule(sb, ring, obs):
    sb.rule_action()


def _rollout(source):
    def call(sb, ring, obs):
        from marl_llm_amd.rollout import rollout_expert
        rollout_expert(sb, 2, obs=obs, replay=ring, source=source)
    return call


def test_list_cap_130_is_refused_at_300(shapes):
    sb = shape_batch(shapes, 2, 300, large_swarm=True, g_max=130)
    try:
        _refused(sb, sb.reset(seed=3), [(r"error 1: .*num_obs_grid_max", _rule), (r"error 1: .*num_obs_grid_max", _rollout("rule"))])
    finally:
        sb.close()


def test_llm_source_needs_llm_action_at_300(shapes):
    from marl_llm_amd.rollout import rollout_expert
    sb = shape_batch(shapes, 2, 300, large_swarm=True)
    try:
        obs = sb.reset(seed=3)
        _refused(sb, obs, [(r"error 1: .*llm_action", _rollout("llm"))])
        ring = ring_for(sb, 2)
        rollout_expert(sb, 2, obs=sb.observe(), replay=ring, source="rule")           # the rule source of the same handle runs
        assert ring.cur == 2 and bool((ring.act[:2] != 0).any())
    finally:
        sb.close()


def test_unobserved_handle_is_refused_at_300(shapes):
    from marl_llm_amd.shapes import r_avoid_for
    n_a = 300
    r_avoid = r_avoid_for(n_a, shapes)
    rng = np.random.default_rng(1)
    sb = make_batch([calm_case(rng, shapes, n_a, r_avoid) for _ in range(2)], r_avoid, large_swarm=True)     # (no observe())
    try:
        obs = torch.zeros((2, n_a, sb.obs_dim), device=sb.device)
        _refused(sb, obs, [(r"error 3: .*observed", _rule), (r"error 3: .*observed", _rollout("rule"))])
        assert bool((sb.rule_action().abs() < 1).any())
    finally:
        sb.close()


def test_fp64_rows_are_refused_in_the_rollout_at_300(shapes):
    sb = shape_batch(shapes, 2, 300, torch.float64, large_swarm=True)
    try:
        _refused(sb, sb.reset(seed=3), [(r"error 1: .*fp64 rows", _rollout("rule"))])
        assert bool((sb.rule_action().abs() < 1).any())                              # (swarm_rule_action serves fp64 handles)
    finally:
        sb.close()


def test_large_handle_at_256_still_refuses(shapes):
    """The boundary of the feature: at 256 agents or fewer a large handle keeps the parent's refusal, the default handle
    serves those counts (test_gpu_large_swarm.py pins the same at 200)."""
    sb = shape_batch(shapes, 2, 256, large_swarm=True)
    try:
        _refused(sb, sb.reset(seed=3), [("256", _rule), ("256", _rollout("rule"))])
    finally:
        sb.close()


# ---- 7. stream ------------------------------------------------------------------------------------------------------------
def test_rule_action_runs_on_the_side_stream_behind_a_delay(shapes):
    """The method of test_gpu_large_swarm.py's stream test: on a non-blocking side stream a 150 ms delay, then a step that
    moves the state, then rule_action().  A kernel launched on the null stream runs at once, on the state (or the lists) from
    before the step."""
    E, n_a = 3, 300
    torch.cuda._sleep(1_000_000); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 50_000_000
    a.record(); torch.cuda._sleep(n); b.record(); b.synchronize()
    cpm = n / a.elapsed_time(b)
    ref, dut = [shape_batch(shapes, E, n_a, large_swarm=True) for _ in range(2)]
    try:
        g = torch.Generator(device="cpu").manual_seed(1)
        act = (torch.rand((E, n_a, 2), generator=g) * 2 - 1).cuda()
        for sb in (ref, dut):                 # state A, every lazy allocation of the entry points done
            sb.reset(seed=2); sb.step(act); sb.rule_action()
        torch.cuda.synchronize()
        u_a = ref.rule_action().clone()
        ref.step(act)
        want = ref.rule_action().clone()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            torch.cuda._sleep(int(150.0 * cpm))
            guard = torch.cuda.Event(); guard.record(side)
            dut.step(act)
            got = dut.rule_action()
            assert not guard.query(), "delay too short, or the call waited for the stream"
        side.synchronize()
        assert bits_equal(got, want) and not bits_equal(want, u_a)
        for x, y in zip(dut.get_state(), ref.get_state()):
            assert torch.equal(x, y)
    finally:
        ref.close(); dut.close()
