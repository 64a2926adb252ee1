"""Mixed batches: envs whose cells the lattice row walk serves beside envs it does not, in ONE batch.

The step kernel's cell path is chosen per workgroup (include/swarm_env.h swarm_path_envs): a batch that holds both kinds is
stepped by two launches over the same grid, the generic kernel taking every workgroup with an env whose device lattice record
is empty and the lattice kernel the others.  Results are bit for bit what one generic launch gives (debug_flags bit 1, and bit 3:
the whole-batch demotion that was the only behaviour before).  Tolerances are test_gpu_parity.py's: everything exact.

Three kinds of env do not walk (KINDS): "j" cells jittered off the lattice, "s" lattice points that are not in row-major order,
"f" a lattice scaled to spacing 0.053, whose sensing window is 16 rows (one more than the walk serves).

Workgroups: N < 64 packs EPB = 64 // npad envs into one workgroup (npad = N rounded up to a power of two, at least 8), and an
env that does not walk takes its whole workgroup to the generic launch.  PARITY below places the non-walking envs so that the
batch holds a mixed workgroup, an all-generic one, an all-lattice one and a partial tail workgroup; a grid of only three
workgroups cannot hold all four, so there the tail doubles as the all-lattice (N = 32, 8) or the all-generic (N = 16) one.

Mutants of env_launch's mixed branch, each built once as a scratch library and run once against tests 1 and 2 of this file
on an MI355X (memory-safe: a skipped launch leaves its envs unstepped, a doubled one steps envs twice with the kernel that
serves any cell set; no kernel ever sees a record it does not handle).  Failing cases of 8 (test_oracle_parity) and of 6
(test_twins):

  mutant                                                   test_oracle_parity   test_twins   how it shows
  the generic launch of a mixed batch is skipped           8 of 8 fail          6 of 6 fail  NaN outputs / stale state of the scan envs
  the lattice launch of a mixed batch is skipped           8 of 8 fail          6 of 6 fail  the same, of the walk envs
  filter 2 ignored: the generic launch steps every env     7 of 8 fail          6 of 6 fail  walk envs are stepped by both launches

Under the third mutant n8_e17 passes: its only walking workgroup is the one-env tail, which the two launches step at the same
time from the same state, writing the same values; every case with more walking envs fails.

A mutant that runs the lattice kernel on an env with an empty record is not built: whether that is memory-safe is not
established.  Test 3 cannot observe the workgroup geometry (no public call shows it): that an all-walk batch takes the
half-occupied geometry again after select_shape(tiled) rests on set_lattice_mode, and on the steps at (8, 24) equalling the twin's.
"""
import functools

import numpy as np
import pytest

from helpers import ThreadedOracle, lat_nrs, make_case, pad_cells
from lockstep import IDX, OBSERVE, compare, device_layout, host_copy, oracle_action

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZE_A = 0.035
FINE = 0.053                       # lattice spacing whose sensing window is 16 rows
DEMOTE, SERIAL, NO_LATTICE = 8, 16, 2           # debug_flags bits 3, 4 and 1
# test 1: (N, E, {env: kind of its non-walking cell set})
PARITY = [
    (64, 5, {0: "j", 2: "s", 4: "f"}),
    (30, 7, {0: "j", 2: "s", 3: "f", 6: "j"}),          # EPB 2: [0 1] mixed, [2 3] generic, [4 5] lattice, [6] tail, generic
    (32, 5, {0: "s", 2: "f", 3: "j"}),                  # EPB 2: [0 1] mixed, [2 3] generic, [4] tail, lattice
    (16, 9, {0: "f", 2: "s", 8: "j"}),                  # EPB 4: [0..3] mixed, [4..7] lattice, [8] tail, generic
    (8, 17, {0: "j", 8: "s", 9: "f", 10: "j", 11: "s", 12: "f", 13: "j", 14: "s", 15: "f"}),   # EPB 8: mixed, generic, [16] lattice
    (100, 3, {1: "j"}),
    (128, 3, {0: "s", 2: "f"}),
    (256, 2, {1: "j"}),
]
STEPS = 5


def _epb(n_a):
    npad = 8
    while npad < n_a:
        npad *= 2
    return 64 // npad if npad < 64 else 1


def _path_counts(scan, n_env, n_a):
    """(walk, scan) envs by workgroup of EPB envs: one env of `scan` sends its whole workgroup to the generic launch."""
    epb = _epb(n_a)
    n_scan = sum(min(epb, n_env - b) for b in range(0, n_env, epb) if any(e in scan for e in range(b, min(b + epb, n_env))))
    return n_env - n_scan, n_scan


def _unwalk(kind, rng, p, g, l_cell):
    """One env's state and cells (2, n_g) turned into a set the row walk does not serve."""
    if kind == "j":
        return p, np.ascontiguousarray(g + rng.normal(0, 0.004, g.shape)), l_cell
    if kind == "s":
        return p, np.ascontiguousarray(g[:, rng.permutation(g.shape[1])]), l_cell
    assert kind == "f"
    ctr = g.mean(axis=1, keepdims=True)
    k = FINE / l_cell
    return np.ascontiguousarray(ctr + (p - ctr) * k), np.ascontiguousarray(ctr + (g - ctr) * k), FINE


def _mixed_batch(shapes, n_a, n_env, kinds, seed):
    """n_env make_case envs, agents clustered on the shape; env e of `kinds` gets a non-walking cell set.  Agents (0, 1) and
    (2, 3) start 0.05 apart -- a contact (centres closer than 2 size_a) -- at a common velocity."""
    rng = np.random.default_rng([seed, n_a, n_env])
    cases = []
    for e in range(n_env):
        p, dp, g, l_cell = make_case(rng, shapes, n_a, 1)
        if e in kinds:
            p, g, l_cell = _unwalk(kinds[e], rng, p, g, l_cell)
        on = rng.choice(g.shape[1], 2, replace=False)
        for (a, b), c in zip(((0, 1), (2, 3)), on):
            th = rng.uniform(0, 2 * np.pi)
            p[:, a] = g[:, c]
            p[:, b] = p[:, a] + 0.05 * np.array([np.cos(th), np.sin(th)])
            dp[:, b] = dp[:, a] = 0.1 * dp[:, a]
        cases.append((np.ascontiguousarray(p), np.ascontiguousarray(dp), g, l_cell))
    cells, n_g = pad_cells([c[2] for c in cases], max(c[2].shape[1] for c in cases))
    return dict(cells=cells, n_g=n_g, l_cell=np.array([c[3] for c in cases]), p=np.stack([c[0] for c in cases]),
                dp=np.stack([c[1] for c in cases]))


def _pair_actions(rng, p):
    """[E, N, 2] float32 actions for the state p [E, 2, N]: uniform, except that agents (0, 1) and (2, 3) push towards each
    other at full throttle -- the contact spring (k_ball (2 size_a - d) <= 2.1) balances it near d = 0.037, so the pairs stay
    in contact for the whole run."""
    E, _, N = p.shape
    a = rng.uniform(-1, 1, (E, N, 2))
    for i, j in ((0, 1), (2, 3)):
        d = p[:, :, j] - p[:, :, i]
        u = d / np.linalg.norm(d, axis=1, keepdims=True)
        a[:, i] = u; a[:, j] = -u
    return a.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(n_a, n_env, kinds_key):
    """The inputs of one parity case and the oracle's trajectory of them: the first observation, then STEPS chained steps.
    Computed once per case; nothing in it is modified afterwards."""
    from marl_llm_amd.shapes import r_avoid_for, synthetic_shape_set
    from oracle.oracle_py import Oracle
    shapes = synthetic_shape_set()
    sy = _mixed_batch(shapes, n_a, n_env, dict(kinds_key), seed=909)
    ra = r_avoid_for(n_a, shapes)
    rng = np.random.default_rng([n_a, n_env, 17])
    with ThreadedOracle(Oracle(), sy["cells"], sy["n_g"], sy["l_cell"], ra) as to:
        first = to.observe(sy["p"], sy["dp"])
        p, dp, nei, steps = sy["p"], sy["dp"], first["neighbor_index"], []
        for _ in range(STEPS):
            act = _pair_actions(rng, p)
            o = to.step(p, dp, oracle_action(act), nei)
            o["act"] = act
            steps.append(o)
            p, dp, nei = o["p"], o["dp"], o["neighbor_index"]
    return sy, ra, first, steps


def _assert_reached(sy, first, steps):
    """From the oracle's output alone: every env, at every compared observation, has an agent inside the shape, an agent with
    a non-empty sensed list and a pair of agents in contact."""
    states = [(sy["p"], first)] + [(o["p"], o) for o in steps]
    for t, (p, o) in enumerate(states):
        assert (o["in_flags"] == 1).any(axis=1).all(), ("in_flags", t)
        assert (o["sensed_index"][:, :, 0] >= 0).any(axis=1).all(), ("sensed", t)
        d = p[:, :, :, None] - p[:, :, None, :]
        dc = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2) + 10.0 * np.eye(p.shape[2])
        assert (dc.reshape(len(p), -1).min(axis=1) < 2 * SIZE_A).all(), ("contact", t)


def _batch(sy, n_a, ra, flags=0, dtype=None):
    from marl_llm_amd.batched import SwarmBatch
    sb = SwarmBatch(n_env=len(sy["n_g"]), n_agents=n_a, n_cells_max=sy["cells"].shape[2], r_avoid=ra,
                    obs_dtype=dtype or torch.float64, debug_flags=flags)
    sb.set_cells(sy["cells"], sy["n_g"], sy["l_cell"])
    sb.set_state(sy["p"], sy["dp"])
    return sb


def _nan_outputs(sb):
    """Caller-owned step outputs filled with what no launch writes: NaN (255 for done)."""
    E, N, D = sb.n_env, sb.n_agents, sb.obs_dim
    kw = dict(device=sb.device)
    return dict(obs=torch.full((E, N, D), float("nan"), dtype=sb.obs_dtype, **kw), rew=torch.full((E, N), float("nan"), **kw),
                done=torch.full((E, N), 255, dtype=torch.uint8, **kw), prior=torch.full((E, N, 2), float("nan"), dtype=sb.obs_dtype, **kw))


# ------------------------------------------------------------------------------------------------------------------------
# 1. oracle parity, float64 handles
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a,n_env,kinds", PARITY, ids=[f"n{c[0]}_e{c[1]}" for c in PARITY])
def test_oracle_parity(n_a, n_env, kinds):
    sy, ra, first, steps = _reference(n_a, n_env, tuple(sorted(kinds.items())))
    _assert_reached(sy, first, steps)
    assert {"j", "s", "f"} >= set(kinds.values())
    for e, kind in kinds.items():                      # the fine lattice is a lattice whose window is 16 rows; the others walk
        if kind == "f":
            assert lat_nrs(sy["cells"][e:e + 1], sy["n_g"][e:e + 1]) == 16
    walkers = [e for e in range(n_env) if e not in kinds]
    assert walkers and lat_nrs(sy["cells"][walkers], sy["n_g"][walkers]) <= 15
    sb = _batch(sy, n_a, ra)
    try:
        assert sb.path_envs() == _path_counts(kinds, n_env, n_a)
        assert sb.lattice_envs() == n_env - sum(k != "f" for k in kinds.values())
        compare(host_copy(sb, sb.observe(), state=False, indices=True), device_layout(first), "observe", fields=OBSERVE)
        for t, o in enumerate(steps):
            out = _nan_outputs(sb)
            sb.step(torch.from_numpy(o["act"]).to(sb.device), out=out)
            compare(host_copy(sb, out, indices=True), device_layout(o), f"step {t}")
        assert sb.path_envs() == _path_counts(kinds, n_env, n_a)
    finally:
        sb.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. twins: the two-launch dispatch, the whole-batch demotion, the serial form and the generic kernel alone
# ------------------------------------------------------------------------------------------------------------------------
def _free_run(sb, steps):
    """`steps` prior-policy steps (the first action zero); every output of every step, and the final state."""
    act = torch.zeros((sb.n_env, sb.n_agents, 2), dtype=torch.float32, device=sb.device)
    outs = [sb.observe().clone()]
    for _ in range(steps):
        obs, rew, done, pri = sb.step(act)
        outs += [obs.clone(), rew.clone(), done.clone(), pri.clone()]
        act = pri.to(torch.float32)
    return outs + list(sb.get_state())


TWINS = [(64, 6, {0: "j", 3: "s", 5: "f"}), (16, 9, {0: "f", 2: "s", 8: "j"})]


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f64"])
@pytest.mark.parametrize("n_a,n_env,kinds", TWINS, ids=[f"n{c[0]}_e{c[1]}" for c in TWINS])
def test_twins(shapes, n_a, n_env, kinds, dtype):
    from marl_llm_amd.shapes import r_avoid_for
    dt = dict(f32=torch.float32, bf16=torch.bfloat16, f64=torch.float64)[dtype]
    sy = _mixed_batch(shapes, n_a, n_env, kinds, seed=404)
    ra = r_avoid_for(n_a, shapes)
    want = {0: _path_counts(kinds, n_env, n_a), DEMOTE: (0, n_env), SERIAL: _path_counts(kinds, n_env, n_a), NO_LATTICE: (0, n_env)}
    ref = None
    for flags in (0, DEMOTE, SERIAL, NO_LATTICE):
        sb = _batch(sy, n_a, ra, flags, dt)
        try:
            assert sb.path_envs() == want[flags], flags
            got = _free_run(sb, 20)
        finally:
            sb.close()
        if ref is None:
            ref = got
            assert all(torch.isfinite(x.double()).all() for x in ref)
            continue
        for k, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, b), (flags, k)


# ------------------------------------------------------------------------------------------------------------------------
# 3. device reset from a shape set with both kinds, and shape switches
# ------------------------------------------------------------------------------------------------------------------------
def _mixed_shape_set():
    """Two tiled shapes and a jittered copy of a third (shape index 2)."""
    from marl_llm_amd.shapes import SHAPE_NAMES, synthetic_shape_set
    s = synthetic_shape_set(SHAPE_NAMES[:3])
    g = np.asarray(s["grid_coords"][2], np.float64)
    s["grid_coords"][2] = g + np.random.default_rng(12).normal(0, 0.004, g.shape)
    return s


def _step_pair(sb, twin, gen, what):
    act = torch.rand((sb.n_env, sb.n_agents, 2), device=sb.device, generator=gen) * 2 - 1
    got, ref = sb.step(act), twin.step(act)
    for name, a, b in zip(("obs", "reward", "done", "a_prior"), got, ref):
        assert torch.equal(a, b), (what, name)
    for name, a, b in zip(("p", "dp"), sb.get_state(), twin.get_state()):
        assert torch.equal(a, b), (what, name)


@pytest.mark.parametrize("n_a,n_env", [(8, 24), (64, 8)])
def test_device_reset_and_shape_switch(n_a, n_env):
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.shapes import r_avoid_for
    s3 = _mixed_shape_set()
    ra = r_avoid_for(n_a, s3)
    ng_max = max(np.asarray(g).shape[0] for g in s3["grid_coords"])
    mk = lambda flags: SwarmBatch(n_env=n_env, n_agents=n_a, n_cells_max=ng_max, r_avoid=ra, obs_dtype=torch.float64, debug_flags=flags)
    sb, twin = mk(0), mk(NO_LATTICE)
    try:
        sb.set_shapes(s3); twin.set_shapes(s3)
        sb.reset(seed=77)
        drawn = sb.get_shape_index()
        assert (drawn == 2).any() and (drawn != 2).any()                     # the draw holds both kinds
        assert sb.path_envs() == _path_counts(set(np.nonzero(drawn == 2)[0]), n_env, n_a)
        assert sb.lattice_envs() == 0                                         # not every shape of the set is a lattice
        cells, n_g = sb.get_cells()
        twin.set_cells(cells, n_g, np.asarray(s3["l_cell"], np.float64)[drawn])
        twin.set_state(*sb.get_state())
        twin.observe()
        assert twin.path_envs() == (0, n_env)
        gen = torch.Generator(device=sb.device).manual_seed(3)
        for t in range(3):
            _step_pair(sb, twin, gen, f"after reset, step {t}")
        for shape, counts in ((2, (0, n_env)), (0, (n_env, 0)), (2, (0, n_env)), (1, (n_env, 0))):
            assert torch.equal(sb.select_shape(shape), twin.select_shape(shape)), shape
            assert sb.path_envs() == counts and twin.path_envs() == (0, n_env)
            assert sb.lattice_envs() == (0 if shape == 2 else n_env)
            for t in range(2):
                _step_pair(sb, twin, gen, f"shape {shape}, step {t}")
    finally:
        sb.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------------------
# 4. envs leave and rejoin the row walk mid-trajectory, against the oracle
# ------------------------------------------------------------------------------------------------------------------------
def test_switching_mid_trajectory(oracle, shapes):
    from marl_llm_amd.shapes import r_avoid_for
    from marl_llm_amd.synth import synthetic_batch
    n_a, E, seg = 64, 8, 20
    sy = synthetic_batch(E, n_a, shapes, seed=5151, assembled_fraction=1.0)
    ra = r_avoid_for(n_a, shapes)
    cells, n_g, l_cell = sy["cells"], sy["n_g"], sy["l_cell"]
    jit = cells.copy()
    for e in range(E):
        jit[e, :, : n_g[e]] += np.random.default_rng(e).normal(0, 0.004, (2, n_g[e]))
    sb = _batch(sy, n_a, ra)
    to = ThreadedOracle(oracle, cells, n_g, l_cell, ra)
    st = dict(p=sy["p"], dp=sy["dp"], act=torch.zeros((E, n_a, 2), dtype=torch.float32, device=sb.device))

    def observe(what):
        o = to.observe(st["p"], st["dp"])
        compare(host_copy(sb, sb.observe(), state=False, indices=True), device_layout(o), f"{what}: observe", fields=OBSERVE)
        st["nei"] = o["neighbor_index"]
        st["act"] = st["act"].clone()

    def run(what):
        for t in range(seg):
            a = oracle_action(st["act"])
            out = sb.step(st["act"])
            o = to.step(st["p"], st["dp"], a, st["nei"])
            last = t == seg - 1                            # the four index lists on the last step of a run
            compare(host_copy(sb, out, indices=last), device_layout(o), f"{what} step {t}", indices=last)
            st.update(p=o["p"], dp=o["dp"], nei=o["neighbor_index"], act=out[3].to(torch.float32), last=o)

    def put(envs, src):
        c = to.cells.copy()
        for e in envs:
            sb.set_cells(src[e:e + 1], n_g[e:e + 1], l_cell[e:e + 1], env_begin=e)
            c[e] = src[e]
        to.set_cells(c, n_g, l_cell)

    try:
        assert sb.path_envs() == (E, 0)
        observe("all walk"); run("all walk")
        put([5], jit)
        assert sb.path_envs() == (E - 1, 1) and sb.lattice_envs() == E - 1
        observe("one jittered"); run("one jittered")
        put([1, 6], jit)
        assert sb.path_envs() == (E - 3, 3) and sb.lattice_envs() == E - 3
        observe("three jittered"); run("three jittered")
        put([1, 5, 6], cells)
        assert sb.path_envs() == (E, 0) and sb.lattice_envs() == E
        observe("restored"); run("restored")
        assert st["last"]["in_flags"].any()
    finally:
        to.close(); sb.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. every other caller of the step kernel's launch on a mixed batch, against a twin that never takes the lattice path
# ------------------------------------------------------------------------------------------------------------------------
CALLERS = [(30, 6, {0: "j", 3: "s", 5: "f"}), (64, 4, {1: "j", 3: "f"})]


def _twin_pair(shapes, n_a, n_env, kinds, dtype=torch.float32, **kw):
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.shapes import r_avoid_for
    sy = _mixed_batch(shapes, n_a, n_env, kinds, seed=606)
    ra = r_avoid_for(n_a, shapes)
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])           # room for any shape of the set (set_shapes)
    sy["cells"] = np.concatenate([sy["cells"], np.zeros((n_env, 2, ng_max - sy["cells"].shape[2]))], axis=2)
    pair = []
    for flags in (0, NO_LATTICE):
        sb = SwarmBatch(n_env=n_env, n_agents=n_a, n_cells_max=sy["cells"].shape[2], r_avoid=ra, obs_dtype=dtype, debug_flags=flags, **kw)
        sb.set_cells(sy["cells"], sy["n_g"], sy["l_cell"]); sb.set_state(sy["p"], sy["dp"])
        pair.append(sb)
    assert pair[0].path_envs() == _path_counts(kinds, n_env, n_a) and pair[1].path_envs() == (0, n_env)
    return pair


@pytest.mark.parametrize("n_a,n_env,kinds", CALLERS, ids=[f"n{c[0]}_e{c[1]}" for c in CALLERS])
def test_indices_and_rule_action(shapes, n_a, n_env, kinds):
    sb, twin = _twin_pair(shapes, n_a, n_env, kinds)
    try:
        assert torch.equal(sb.observe(), twin.observe())
        a, b = sb.indices(), twin.indices()
        for k in IDX:
            assert torch.equal(a[k], b[k]), k
        ra, rb = sb.rule_action(), twin.rule_action()
        assert torch.equal(ra, rb) and torch.isfinite(ra).all()
    finally:
        sb.close(); twin.close()


@pytest.mark.parametrize("n_a,n_env,kinds", CALLERS, ids=[f"n{c[0]}_e{c[1]}" for c in CALLERS])
def test_rollout_loops(shapes, n_a, n_env, kinds):
    from marl_llm_amd.rollout import ChainedReplay, FusedPolicy, PolicyMLP, rollout_device, rollout_eval, rollout_expert
    from marl_llm_amd.shapes import SHAPE_NAMES, synthetic_shape_set
    sb, twin = _twin_pair(shapes, n_a, n_env, kinds)
    torch.manual_seed(0)
    module = PolicyMLP(sb.obs_dim, 2, 180).to(sb.device)
    pols = [FusedPolicy(module, device=sb.device) for _ in range(2)]
    two = synthetic_shape_set(SHAPE_NAMES[:2])
    try:
        rings, obs = [], []
        for b in (sb, twin):
            b.set_shapes(two)
            rings.append(ChainedReplay(32, n_env * n_a, b.obs_dim, 2, b.device))
            obs.append(b.observe().clone())
        assert torch.equal(obs[0], obs[1])
        res = []
        for b, pol, ring, o in zip((sb, twin), pols, rings, obs):
            o, st_e = rollout_expert(b, 5, obs=o, replay=ring, source="rule")
            o, st_d = rollout_device(b, pol, 10, obs=o, replay=ring, noise_scale=0.0)
            mixed_before_switch = b.path_envs()
            o, tr = rollout_eval(b, pol, 10, obs=o, replay=ring, switch={6: 1})
            res.append([o.clone(), st_e, st_d, tr.metrics, tr.reward_stats, ring.obs.clone(), ring.act.clone(), ring.rew.clone(),
                        ring.act_prior.clone(), *b.get_state()])
            assert mixed_before_switch == (_path_counts(kinds, n_env, n_a) if b is sb else (0, n_env))
        assert sb.path_envs() == (n_env, 0)                   # the switch left every env on a tiled shape
        for k, (a, b) in enumerate(zip(*res)):
            assert torch.equal(a, b), k
    finally:
        for x in pols:
            x.close()
        sb.close(); twin.close()


def _numpy_envs(n_envs, rng, results):
    """An AssemblySwarmEnv and its twin whose backend never takes the lattice path.  The env has no public debug_flags: the
    twin's backend is put in place of the one the env would create, with the env's own configuration."""
    from types import SimpleNamespace
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.env import AssemblySwarmEnv
    args = SimpleNamespace(n_a=30, is_boundary=True, dynamics_mode="Cartesian", agent_strategy="input", is_con_self_state=True,
                           training_method="llm_rl", results_file=results)
    envs = []
    for flags in (0, NO_LATTICE):
        env = AssemblySwarmEnv(n_envs=n_envs, rng=rng, seed=11)
        env.__reinit__(args)
        env._batch = SwarmBatch(n_env=n_envs, n_agents=30, n_cells_max=env.n_cells_max, r_avoid=env.r_avoid, obs_dtype=torch.float64,
                                debug_flags=flags)
        envs.append(env)
    return envs


def _numpy_steps(envs, n_envs, steps=3):
    rng = np.random.default_rng(8)
    for t in range(steps):
        a = rng.uniform(-1, 1, (2, 30 * n_envs))
        got, ref = envs[0].step(a), envs[1].step(a)
        for k in (0, 1, 2, 4):                                    # obs, reward, done, a_prior
            assert np.array_equal(got[k], ref[k]), (t, k)
        assert np.isfinite(got[0]).all()


def test_host_path_one_env_with_assigned_cells(shapes):
    """AssemblySwarmEnv.step (swarm_step_host: pinned staging of the action, export kernel, one copy back) after the eval
    script's shape switch, `env.grid_center = ...` (eval_assembly.py:34-57), to cells that are no lattice: all scan."""
    envs = _numpy_envs(1, "counter", shapes)
    try:
        first = [env.reset() for env in envs]
        assert np.array_equal(first[0], first[1])
        assert envs[0]._batch.path_envs() == (1, 0)
        for env in envs:
            g = env.grid_center
            env.grid_center = g + np.random.default_rng(2).normal(0, 0.004, g.shape)
        _numpy_steps(envs, 1)
        assert envs[0]._batch.path_envs() == (0, 1) and envs[1]._batch.path_envs() == (0, 1)
    finally:
        for env in envs:
            env.close()


def test_host_path_three_envs_mixed_by_the_device_reset():
    """The same host path on a mixed batch: three envs (N = 30: two envs per workgroup) reset on the device from a shape set
    that holds a shape off the lattice.  Episodes are drawn until the envs hold both kinds (each draw is mixed with
    probability 2 / 3)."""
    envs = _numpy_envs(3, "device", _mixed_shape_set())
    try:
        for episode in range(8):
            first = [env.reset() for env in envs]
            assert np.array_equal(first[0], first[1])
            assert np.array_equal(envs[0].shape_index, envs[1].shape_index)
            off = set(np.nonzero(envs[0].shape_index == 2)[0])
            want = _path_counts(off, 3, 30)
            assert envs[0]._batch.path_envs() == want and envs[1]._batch.path_envs() == (0, 3)
            if 0 < want[0] < 3:
                break
        else:
            raise AssertionError("no episode of eight drew both kinds of shape")
        _numpy_steps(envs, 3)
        assert envs[0]._batch.path_envs() == want
    finally:
        for env in envs:
            env.close()
