"""The rule-based expert kernel k_rule through its two entry points, swarm_rule_action (the instantiations without the f32
row) and swarm_rollout_expert (those with it), held to the float64 restatement oracle_py.rule_action (numpy in the reference's call order, itself pinned to the recorded reference actions by
g5_rule_n*.npz) at every launch shape, on both export paths, on the decision thresholds and on non-finite states.

Why a module of its own.  The kernel exports only the action after np.clip(-1, 1).  On the states the older tests use
(helpers.make_case(cluster=1), or 30 expert steps from synthetic_batch) most components are exactly +-1, and a 1e-12
tolerance on such a component checks the sign of the sum and nothing else.  Measured with the restatement alone
(rule_action(detail=True), share of components with an unclipped |sum| >= 1):
    make_case(cluster=1):                          N = 30: 78 %, N = 64: 70 %, N = 200 / 256: 59 %
    test_gpu_rule.py's inputs (synthetic_batch seed 77 + 30 expert steps on the device, that state restated):
                                                   N = 30 x 16 envs: 47 %, N = 64 x 8 envs: 35 %
So this module compares on inputs built to stay inside (-1, 1) (helpers.calm_batch) and asserts from the restatement's own
detail output -- never from kernel output -- how many components are unsaturated and which branches they reached.

Unsaturated share and branch counts of calm_batch (seed 0; agents with a component of |sum| < 1; from
test_rule_contract_host.py, which asserts the same conditions on the CPU):
    N     envs  share  n_near>=1  in r_avoid  in_flag==0  list non-empty  subsampled
    1      64   0.95        0          0          42            0             0
    2      64   0.98        0          0          42            0             0
    7      64   0.59       19         19         200          129             0
    8     768   0.61      303        303        2875         1846             0
    9     683   0.59      381        381        2556         2066            11
    30    205   0.60     3058       1719        2787         2178           203
    63     98   0.66     4577       2167        2885         2592           195
    64     96   0.66     4490       2081        2829         2495           237
    65     95   0.65     4583       2137        2874         2494           220
    127    49   0.71     5412       2723        2894         2848           268
    128    48   0.69     5316       2631        2890         2707           172
    129    48   0.71     5434       2665        2894         2818           269
    191    33   0.75     5790       2992        2980         2996           702
    192    32   0.75     5655       3044        2858         2979           623
    193    32   0.75     5680       3083        2864         2973           576
    200    31   0.77     5804       3048        2899         3099           687
    255    25   0.77     5961       3289        2904         3179           465
    256    24   0.79     5777       3155        2917         2987           503
Required (helpers.assert_calm_conditions): N >= 8: share >= 1/3 and >= 100 agents in each of the first four columns; the
subsample column >= 100 for N >= 30 (below that an in-shape agent's own r_avoid / 2 disc removes so many of the ~127 cells
inside d_sen that at most g_max = 80 are left; agents outside the shape keep their whole list but v_ent + v_exp saturates
them).  N < 8: share > 0.

Tolerance: the existing 1e-12 absolute on unsaturated components, exact equality (+-1 with the reference's sign) on
saturated ones, equal NaN masks.  The only inexact operation is cos (device libm vs numpy, both within a few ulp of a value
<= 1): psi = 0.5 (1 + cos) carries an absolute error <= 4 * 2^-53 per cell, v_exp = k_2 * sum(psi rel) / sum(psi) is a weighted
mean of |rel| < d_sen = 0.4, so its error is <= 15 * 0.4 * 2 * 4 * 2^-53 / min-weight-share ~ 1e-14 unless the weights nearly
vanish; 1e-12 leaves two decades for that and is not sharpened here.

Threshold placements (section "thresholds" below): `nr < r_avoid` switches a term that is exactly 0 at nr == r_avoid
(-k_3 (r_avoid / nr - 1) rel), and `|p_j - p_i| < d_sen + r_avoid / 2` cannot change the filtered list except by rounding
(a sensed cell within r_avoid / 2 of j puts j within d_sen + r_avoid / 2 by the triangle inequality); for those two the
decided quantity asserted is n_avoid, resp. that the list is the same on both sides.

Odd list caps: with g_max - 1 even, i * (n_s - 1) / (g_max - 1) can land on k + 0.5.  The controller rounds such a tie to even
(np.round, assembly.py:564), the observation away from zero (std::round, AssemblyEnv.cpp:223).  The kernel reads the
observation's list, so for odd caps it disagreed with the restatement (cap 45: 251 of 355 subsampled agents meet a tie;
max error 0.53).  test_filtered_count_on_the_cap found it; the export pass of the expert now rounds as numpy does and
test_odd_list_caps_round_ties_as_numpy_does pins both roundings.  The default cap of 80 has no ties.

Long runs (teacher-forced every 10 of 200 steps after a device reset), unclipped share of all components per quarter of the
episode (steps 0-40, 50-90, 100-140, 150-190):
    N = 30 x 32 envs:  0.61  0.79  0.90  0.92
    N = 64 x 16 envs:  0.64  0.86  0.93  0.94
    N = 256 x 4 envs:  0.69  0.90  0.96  0.94
The expert calms its own states down: the later part of an episode is almost entirely unsaturated.

Mutants, each built into a scratch copy of the library in both kernels of that time -- the entry points did not share one
yet -- (so that fused-equals-eager still held) and run
once against the old tests (test_gpu_rule.py, test_gpu_rollout_expert.py without the 64 x 4096 case: 21 tests) and against
38 tests of this module (the lattice variant of every N, non-lattice sets, fig shapes, list caps, long runs, the lattice
threshold placements, the emptied list, cell_1e-9):
    mutant                          old tests failing                                   this module failing
    1  k_3 = 16                     6 (the 5 of test_gpu_rule.py, teacher_forced)       34 (N >= 7, every other group)
    2  k_2 = 14                     6 (the same)                                        35
    3  / (n_near + 1)               8 (the same + fused_equals_eager 30x16, both dtypes) 35
    4  nr <= r_avoid                0                                                   0   equivalent: the switched term
                                                                                           -k_3 (r_avoid / nr - 1) rel is
                                                                                           exactly 0 at nr == r_avoid
    5  mask word one bit short      12 (fused_equals_eager, all 10; teacher_forced;     35
       (the rollout's kernel only)     reference_shaped_collection)
    6  + 1e-8 dropped               6 (as 1)                                            37 (N = 1 and 2 as well: every
                                                                                           in_flag == 0 agent moves by
                                                                                           about 1e-8 / nr)
    7  psi without 0.5 (control)    0                                                   0   cancels in sx / den
The old tests catch every non-equivalent mutant too -- their inputs are less saturated than make_case's -- but only up to
64 agents against the restatement; above that they compare the two entry points with each other, which a mutant in both
(today: in the one kernel) passes.
"""
import numpy as np
import pytest

from helpers import (RULE_NS, assert_calm_conditions, calm_batch, calm_case, fig_shapes, make_case, pad_cells, rule_branch_counts,
                     rule_details)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-12                 # test_gpu_rule.py
D_SEN = 0.4


# ---- plumbing ----------------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def make_batch(cases, r_avoid, dtype=torch.float32, **kw):
    from marl_llm_amd.batched import SwarmBatch
    cells, n_g = pad_cells([c[2] for c in cases], max(c[2].shape[1] for c in cases))
    sb = SwarmBatch(n_env=len(cases), n_agents=cases[0][0].shape[1], n_cells_max=cells.shape[2], r_avoid=r_avoid, obs_dtype=dtype, **kw)
    sb.set_cells(cells, n_g, [c[3] for c in cases])
    sb.set_state(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]))
    return sb


def device_actions(cases, r_avoid, dtype=torch.float32, ring=True, lattice=None, **kw):
    """Both entry points on `cases`: swarm_rule_action's fp64 action u [E, 2, N] (numpy), and -- through rollout_expert(sb, 1),
    the same kernel's instantiation with the f32 row -- that the act row is u's f32 rounding and that the step consumed u itself (next state bitwise equal to an eager
    twin's `step(u)`)."""
    from marl_llm_amd.rollout import ChainedReplay, rollout_expert
    sb = make_batch(cases, r_avoid, dtype, **kw)
    if lattice is not None:
        assert sb.lattice_envs() == (len(cases) if lattice else 0)
    obs = sb.observe()
    u = sb.rule_action().clone()
    E, N = sb.n_env, sb.n_agents
    if ring:
        rg = ChainedReplay(1, E * N, sb.obs_dim, 2, sb.device, obs_dtype=dtype)
        rollout_expert(sb, 1, obs=obs, replay=rg, track_reward=False)
        assert bits_equal(rg.act[0].view(E, N, 2), u.float())
        twin = make_batch(cases, r_avoid, dtype, **kw)
        twin.observe()
        twin.step(u)
        for a, b in zip(sb.get_state(), twin.get_state()):
            assert bits_equal(a, b)
        twin.close()
    out = u.cpu().numpy().transpose(0, 2, 1)
    sb.close()
    return out


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


_CALM = {}


def calm_reference(shapes, n_a):
    """calm_batch of one agent count, its restatement and the input conditions (asserted), cached for the variants."""
    from marl_llm_amd.shapes import r_avoid_for
    if n_a not in _CALM:
        r_avoid = r_avoid_for(n_a, shapes)
        cases = calm_batch(shapes, n_a, r_avoid)
        want, info = rule_details(cases, r_avoid)
        assert np.isfinite(info["raw"]).all()
        counts = assert_calm_conditions(n_a, info)
        print(n_a, len(cases), counts)
        _CALM[n_a] = (cases, r_avoid, want, info)
    return _CALM[n_a]


# ---- unsaturated comparison at every launch shape, on every path (issue sections 2 and 3) ----------------------------------
# (f64: swarm_rollout_expert rejects fp64 observation rows, so only swarm_rule_action runs on that handle)
VARIANTS = {"lattice": dict(lattice=True), "generic": dict(debug_flags=2, lattice=False), "exact": dict(debug_flags=1),
            "periodic": dict(is_boundary=False), "bf16": dict(dtype=torch.bfloat16), "f64": dict(dtype=torch.float64, ring=False)}
ARENA = 4.8                 # side of the default boundary (-2.4 .. 2.4): the length a periodic handle wraps by


def wrap_only_pairs(cases, d_sen=D_SEN):
    """Agent-agent and agent-cell pairs of `cases` that are within d_sen only through the periodic wrap (plain distance
    >= d_sen, minimum-image distance < d_sen): where a controller that wrapped would decide differently."""
    def count(a, b):
        d = a[:, :, None] - b[:, None, :]
        w = d - ARENA * np.round(d / ARENA)
        return int(((np.linalg.norm(d, axis=0) >= d_sen) & (np.linalg.norm(w, axis=0) < d_sen)).sum())
    return sum(count(p, p) // 2 for p, _, _, _ in cases), sum(count(p, g) for p, _, g, _ in cases)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n_a", RULE_NS)
def test_calm_states_match_the_restatement(shapes, n_a, variant):
    """Both sides of the 64 / 256-thread launch switch and of every mask-word boundary of k_rule, N = 1 and 2 (no
    neighbour: no division; empty lists), on the lattice and the generic export, with the exact paths forced, periodic
    (the rule path takes no wrap: assembly.py:530-601 reads p directly) and for the three obs_dtype handles, whose fp64
    action must be the same bits."""
    cases, r_avoid, want, info = calm_reference(shapes, n_a)
    if variant == "periodic" and n_a >= 8:
        # the inputs hold pairs that only a wrap brings within d_sen (4 to 249 agent pairs, 30 to 599 agent-cell pairs over
        # the agent counts): a controller that wrapped would count them as neighbours / sensed cells and disagree
        pairs, cells = wrap_only_pairs(cases)
        assert pairs >= 4 and cells >= 30, (pairs, cells)
    got = device_actions(cases, r_avoid, **VARIANTS[variant])
    n = compare(got, want, info, f"N={n_a} {variant}")
    assert n > 0 and (n_a < 8 or 3 * n >= want.size)
    if variant != "lattice":                                          # one state, every handle: the same fp64 bits
        if ("u", n_a) not in _CALM:
            _CALM[("u", n_a)] = device_actions(cases, r_avoid, ring=False)
        assert got.tobytes() == _CALM[("u", n_a)].tobytes()


@pytest.mark.parametrize("n_a", [30, 129])
def test_non_lattice_cell_sets(shapes, n_a):
    """Jittered cells (off-lattice) and shuffled cells (on-lattice points out of row-major order): the generic scan."""
    from marl_llm_amd.shapes import r_avoid_for
    rng = np.random.default_rng(31 + n_a)
    r_avoid = r_avoid_for(n_a, shapes)
    cases = []
    for k in range(max(8, 2048 // n_a)):
        p, dp, g, l_cell = calm_case(rng, shapes, n_a, r_avoid) if k % 3 else make_case(rng, shapes, n_a, 1)
        g = g + rng.normal(0, 0.004, g.shape) if k % 2 == 0 else g[:, rng.permutation(g.shape[1])]
        cases.append((p, dp, np.ascontiguousarray(g), l_cell))
    want, info = rule_details(cases, r_avoid)
    got = device_actions(cases, r_avoid, lattice=False)
    assert compare(got, want, info, f"non-lattice N={n_a}") * 4 >= want.size


def test_reference_fig_shapes():
    from marl_llm_amd.shapes import r_avoid_for
    figs = fig_shapes()
    n_a = 64
    r_avoid = r_avoid_for(n_a, figs)
    cases = calm_batch(figs, n_a, r_avoid, seed=5, agents=4096)
    want, info = rule_details(cases, r_avoid)
    c = rule_branch_counts(info)                                      # (these shapes leave the subsample to few agents)
    assert c["share"] >= 1 / 3 and min(c[k] for k in ("near", "avoid", "outside", "sensed")) >= 100, c
    compare(device_actions(cases, r_avoid, lattice=True), want, info, "fig shapes")


@pytest.mark.parametrize("g_max", [16, 128])
@pytest.mark.parametrize("n_a", [30, 200])
def test_other_list_caps(shapes, n_a, g_max):
    """num_obs_grid_max 16 and 128 (the documented cap): the n_s > g_max selection runs with another step.  About 127 cells
    fit in a disc of d_sen = 0.4, so the cap of 128 is tried with d_sen = 0.5 (about 200 cells)."""
    from marl_llm_amd.shapes import r_avoid_for
    r_avoid = r_avoid_for(n_a, shapes)
    d_sen = 0.4 if g_max == 16 else 0.5
    cases = calm_batch(shapes, n_a, r_avoid, seed=g_max, agents=6144)
    want, info = rule_details(cases, r_avoid, g_max=g_max, d_sen=d_sen)
    c = rule_branch_counts(info)
    print(n_a, g_max, c)
    assert c["share"] >= 1 / 3 and c["subsampled"] >= 100
    # (a sensing window wider than 15 lattice rows, d_sen = 0.5 here, is served by the generic scan whatever the cells)
    got = device_actions(cases, r_avoid, g_max=g_max, d_sen=d_sen, lattice=True if g_max == 16 else None)
    compare(got, want, info, f"g_max={g_max} N={n_a}")
    got = device_actions(cases, r_avoid, g_max=g_max, d_sen=d_sen, debug_flags=2, lattice=False if g_max == 16 else None)
    compare(got, want, info, f"g_max={g_max} N={n_a} generic")


def test_list_cap_129_is_rejected_by_both_entry_points(shapes):
    from marl_llm_amd._lib import SwarmError
    from marl_llm_amd.rollout import ChainedReplay, rollout_expert
    from marl_llm_amd.shapes import r_avoid_for
    n_a = 30
    r_avoid = r_avoid_for(n_a, shapes)
    cases = calm_batch(shapes, n_a, r_avoid, agents=240)
    sb = make_batch(cases, r_avoid, g_max=129)
    obs = sb.observe()
    state = [x.clone() for x in sb.get_state()]
    with pytest.raises(SwarmError, match=r"error 1: .*num_obs_grid_max"):          # SWARM_ERR_INVALID
        sb.rule_action()
    rg = ChainedReplay(4, sb.n_env * n_a, sb.obs_dim, 2, sb.device, obs_dtype=torch.float32)
    rg.new_chain(obs)
    snap = {k: getattr(rg, k).clone() for k in ("obs", "act", "rew", "done", "act_prior")}
    keep = (rg.cur, rg.count)
    with pytest.raises(SwarmError, match=r"error 1: .*num_obs_grid_max"):
        rollout_expert(sb, 3, replay=rg)
    assert all(torch.equal(getattr(rg, k), v) for k, v in snap.items()) and (rg.cur, rg.count) == keep
    for a, b in zip(sb.get_state(), state):
        assert torch.equal(a, b)
    sb.close()


# ---- long expert runs, teacher-forced (issue section 4) ---------------------------------------------------------------
@pytest.mark.parametrize("n_a,n_env", [(30, 32), (64, 16), (256, 4)])
def test_long_expert_runs_teacher_forced(shapes, n_a, n_env):
    """200 expert steps (collect_expert.py's episode length) in chained calls of 10; before each, every env of the device's
    state goes through the restatement and must agree with the eager action, whose f32 rounding the ring then holds."""
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.rollout import ChainedReplay, rollout_expert
    from marl_llm_amd.shapes import r_avoid_for
    K, every = 200, 10
    r_avoid = r_avoid_for(n_a, shapes)
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    sb = SwarmBatch(n_env=n_env, n_agents=n_a, n_cells_max=ng_max, r_avoid=r_avoid)
    sb.set_shapes(shapes)
    rg = ChainedReplay(K, n_env * n_a, sb.obs_dim, 2, sb.device, obs_dtype=torch.float32)
    rollout_expert(sb, 0, replay=rg, reset=(13, 0))
    cells, n_g = sb.get_cells()
    l_cell = np.asarray(shapes["l_cell"], np.float64)[sb.get_shape_index()]
    free = []
    for t in range(0, K, every):
        p, dp = [x.cpu().numpy() for x in sb.get_state()]
        u = sb.rule_action().clone()
        rollout_expert(sb, every, replay=rg, track_reward=False)
        assert bits_equal(rg.act[t].view(n_env, n_a, 2), u.float()), t
        cases = [(p[e], dp[e], np.ascontiguousarray(cells[e][:, : n_g[e]]), float(l_cell[e])) for e in range(n_env)]
        want, info = rule_details(cases, r_avoid)
        free.append(compare(u.cpu().numpy().transpose(0, 2, 1), want, info, f"N={n_a} t={t}") / want.size)
    print(f"N={n_a}: unclipped share per quarter of the episode", [round(float(np.mean(free[q * 5:(q + 1) * 5])), 3) for q in range(4)])
    assert np.sum(free) > 0
    sb.close()


# ---- threshold placements (issue section 5) ---------------------------------------------------------------------------
OFFSETS = (0.0, 1e-12, 1e-9)       # one ulp (the two sides of the crossing themselves), then further out


def straddle(norm, target, t0):
    """t_lo, t_hi: adjacent doubles around t0 with norm(t_lo) < target <= norm(t_hi) (norm non-decreasing near t0)."""
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


def placements(norm, target, t0):
    """[(t, inside)] for the six placements: each side of the crossing at one ulp, 1e-12 and 1e-9."""
    lo, hi = straddle(norm, target, t0)
    out = [(lo - d, True) for d in OFFSETS] + [(hi + d, False) for d in OFFSETS]
    assert all((norm(t) < target) == inside for t, inside in out)
    return out


def _unit(rng):
    th = rng.uniform(-np.pi, np.pi)
    return np.array([np.cos(th), np.sin(th)])


def threshold_scene(rng, shapes, n_a, r_avoid, kind):
    """Six envs (one per placement) of one calm scene with one agent moved along a line of sight onto threshold `kind`.
    Returns (cases, i, key): agent i's detail `key` is what the threshold decides."""
    p, dp, g, l_cell = calm_case(rng, shapes, n_a, r_avoid, off_shape=0.0)
    j = n_a - 1
    i = int(rng.integers(0, n_a - 1))
    d = _unit(rng)
    if kind in ("d_sen", "r_avoid", "filter_reach"):               # agent j on the ray from agent i
        target = {"d_sen": D_SEN, "r_avoid": r_avoid, "filter_reach": D_SEN + r_avoid / 2}[kind]
        key = {"d_sen": "n_near", "r_avoid": "n_avoid", "filter_reach": None}[kind]
        mover, origin, other = j, p[:, i].copy(), p[:, [i]]
        norm = lambda t: np.linalg.norm(np.stack([p[:, k] if k != j else origin + d * t for k in range(n_a)], 1) - other, axis=0)[j]
    elif kind == "cell_cover":                                     # agent j on a ray from a cell that agent i senses
        di = np.linalg.norm(g - p[:, [i]], axis=0)                  # (outside agent i's own r_avoid / 2 disc)
        free = [c for c in np.where((di > r_avoid / 2 + 0.03) & (di < 0.8 * D_SEN))[0]
                if np.linalg.norm(p[:, :j] - g[:, [c]], axis=0).min() > r_avoid / 2 + 0.01]
        c = int(rng.choice(free)) if free else int(np.argmin(np.abs(di - 0.25)))
        target, key, mover, origin = r_avoid / 2, "n_filtered", j, g[:, c].copy()
        norm = lambda t: np.linalg.norm(g[:, [c]] - (origin + d * t)[:, None], axis=0)[0]
    else:                                                          # agent i itself on a ray from a cell
        if kind == "cell_sensed":
            c = int(rng.integers(0, g.shape[1]))
            target, key = D_SEN, "n_sensed"
            d = p[:, i] - g[:, c]
            d = d / np.linalg.norm(d) if np.linalg.norm(d) > 0 else _unit(rng)
        else:                                                      # in_flag: outward from the cell farthest from the centre
            c = int(np.argmax(np.linalg.norm(g - g.mean(axis=1, keepdims=True), axis=0)))
            target, key = np.sqrt(2) * l_cell / 2, "in_flag"
            d = g[:, c] - g.mean(axis=1)
            d = d / np.linalg.norm(d)
        mover, origin = i, g[:, c].copy()
        norm = lambda t: np.linalg.norm(g - (origin + d * t)[:, None], axis=0)[c]
    cases = []
    for t, inside in placements(norm, target, target):
        q = p.copy()
        q[:, mover] = origin + d * t
        cases.append((q, dp, g, l_cell))
    return cases, i, key


KINDS = ["d_sen", "r_avoid", "filter_reach", "cell_cover", "cell_sensed", "in_flag"]


@pytest.mark.parametrize("flags", [0, 2], ids=["lattice", "generic"])
@pytest.mark.parametrize("kind", KINDS)
def test_threshold_placements(shapes, kind, flags):
    """One agent moved with np.nextafter until the float64 norm the reference computes lands on each side of a threshold of
    the controller.  Scenes are kept when the restatement says the two sides differ in the decided quantity and the affected
    agent has an unsaturated component on all six placements.  Of the 48 scenes per kind 34 (d_sen), 25 (r_avoid), 23
    (filter_reach), 18 (cell_cover), 29 (cell_sensed) and 21 (in_flag) qualify; the floor is 16 for every kind.  The others
    are compared too, but prove nothing about the threshold."""
    from marl_llm_amd.shapes import r_avoid_for
    n_a = 30
    r_avoid = r_avoid_for(n_a, shapes)
    rng = np.random.default_rng([5, KINDS.index(kind)])
    scenes = [threshold_scene(rng, shapes, n_a, r_avoid, kind) for _ in range(48)]
    cases = [c for s in scenes for c in s[0]]
    want, info = rule_details(cases, r_avoid)
    good = 0
    for k, (_, i, key) in enumerate(scenes):
        sl = slice(6 * k, 6 * k + 6)
        with np.errstate(invalid="ignore"):
            unsat = (np.abs(info["raw"][sl, :, i]) < 1).any(axis=1).all()
        if key is None:                # by the triangle inequality the list cannot depend on this threshold
            assert len(set(info["n_filtered"][sl, i].tolist())) == 1
            differs = True
        else:
            q = info[key][sl, i]
            differs = len(set(q[:3].tolist())) == 1 and len(set(q[3:].tolist())) == 1 and q[0] != q[3]
        good += bool(unsat and differs)
    print(kind, "scenes with a decided difference on an unsaturated agent:", good)
    assert good >= 16
    got = device_actions(cases, r_avoid, debug_flags=flags, lattice=not flags)
    compare(got, want, info, f"threshold {kind}")


def test_filtered_count_on_the_cap(shapes):
    """A filtered list of exactly g_max cells (kept whole) and of g_max + 1 (subsampled): the cap is set from the list
    length m of unsaturated agents, num_obs_grid_max = m and m - 1."""
    from marl_llm_amd.shapes import r_avoid_for
    n_a = 30
    r_avoid = r_avoid_for(n_a, shapes)
    cases = calm_batch(shapes, n_a, r_avoid, seed=3, agents=1536)
    _, info = rule_details(cases, r_avoid, g_max=128)
    with np.errstate(invalid="ignore"):
        free = (np.abs(info["raw"]) < 1).any(axis=1)
    lengths = info["n_filtered"][free & (info["n_filtered"] >= 8)]
    m = int(np.bincount(lengths).argmax())                             # the most common list length
    for g_max, sub in ((m, False), (m - 1, True)):
        want, inf = rule_details(cases, r_avoid, g_max=g_max)
        on_cap = (inf["n_filtered"] == m) & (np.abs(inf["raw"]) < 1).any(axis=1)
        assert on_cap.sum() >= 4 and (inf["subsampled"][on_cap] != 0).all() == sub and (inf["subsampled"][on_cap] != 0).any() == sub
        compare(device_actions(cases, r_avoid, g_max=g_max), want, inf, f"list of {m} cells, cap {g_max}")


@pytest.mark.parametrize("g_max", [33, 45, 79])
def test_odd_list_caps_round_ties_as_numpy_does(oracle, shapes, g_max):
    """With g_max - 1 even, i * (n_s - 1) / (g_max - 1) can land on k + 0.5.  The controller selects with np.round (ties to
    even, assembly.py:564), the observation with std::round (ties away from zero, AssemblyEnv.cpp:223): the expert's export
    pass must follow the first while swarm_get_indices keeps following the second, before and after an expert call."""
    from marl_llm_amd.shapes import r_avoid_for
    n_a = 30
    r_avoid = r_avoid_for(n_a, shapes)
    cases = calm_batch(shapes, n_a, r_avoid, seed=3, agents=1536)
    want, info = rule_details(cases, r_avoid, g_max=g_max)
    steps = (info["n_filtered"] - 1) / (g_max - 1)
    ties = [(np.arange(g_max) * s) % 1 == 0.5 for s in steps[info["subsampled"] != 0]]
    assert sum(t.any() for t in ties) >= 8                              # agents whose selection meets an exact tie
    for flags in (0, 2):
        compare(device_actions(cases, r_avoid, g_max=g_max, debug_flags=flags), want, info, f"cap {g_max} flags={flags}")
    sb = make_batch(cases, r_avoid, g_max=g_max)
    sb.observe()
    before = sb.indices()["sensed_index"].cpu().numpy()
    sb.rule_action()
    after = sb.indices()["sensed_index"].cpu().numpy()
    for e, (p, dp, g, l_cell) in enumerate(cases):
        o = oracle.get_observation(p, dp, g, l_cell, r_avoid, g_max=g_max)
        assert np.array_equal(before[e], o["sensed_index"]) and np.array_equal(after[e], o["sensed_index"]), e
    sb.close()


def test_filter_empties_the_sensed_list():
    """A 3 x 3 shape under an agent whose own r_avoid / 2 disc covers all of it: sensed, all filtered, v_exp exactly 0."""
    l_cell, r_avoid = 0.06, 0.22
    xs = (np.arange(3) - 1) * l_cell
    g = np.ascontiguousarray(np.stack([np.tile(xs, 3), np.repeat(xs, 3)]))
    rng = np.random.default_rng(2)
    cases = []
    for _ in range(16):
        p = np.concatenate([rng.uniform(-0.01, 0.01, (2, 1)), rng.uniform(0.3, 0.39, (1, 1)) * _unit(rng)[:, None]], axis=1)
        cases.append((p, rng.uniform(-0.05, 0.05, (2, 2)), g, l_cell))
    want, info = rule_details(cases, r_avoid)
    assert (info["n_sensed"][:, 0] == 9).all() and (info["n_filtered"][:, 0] == 0).all() and (info["in_flag"][:, 0] == 1).all()
    assert (info["n_near"][:, 0] == 1).all() and (np.abs(info["raw"][:, :, 0]) < 1).all()
    for flags in (0, 2):
        compare(device_actions(cases, r_avoid, debug_flags=flags), want, info, "emptied list")


# ---- non-finite and degenerate states (issue section 6) --------------------------------------------------------------
def degenerate_cases(shapes, n_a, r_avoid, kind, n_env=12):
    rng = np.random.default_rng(77)
    cases, placed = [], []
    for _ in range(n_env):
        p, dp, g, l_cell = calm_case(rng, shapes, n_a, r_avoid)
        i, j = rng.choice(n_a, 2, replace=False)
        if kind == "coincident":
            p[:, j] = p[:, i]
        elif kind == "nan_position":
            p[int(rng.integers(0, 2)), i] = np.nan
        elif kind == "nan_velocity":
            dp[int(rng.integers(0, 2)), i] = np.nan
        else:                          # nearest cell 1e-9 away, outside by the l_cell scale: v_ent divides by nr + 1e-8
            l_cell = 1e-9
            p[:, i] = g[:, int(rng.integers(0, g.shape[1]))] + 1e-9 * _unit(rng)
        cases.append((p, dp, g, l_cell)); placed.append(int(i))
    return cases, placed


@pytest.mark.parametrize("n_a", [30, 129])
@pytest.mark.parametrize("kind", ["coincident", "nan_position", "nan_velocity", "cell_1e-9"])
def test_degenerate_states(shapes, n_a, kind):
    """np.clip passes NaN through, and so must the kernels: two coincident agents give r_avoid / 0 * 0 = NaN in both of their
    components, a NaN coordinate or velocity spreads exactly as numpy spreads it (NaN compares false: a NaN agent is nobody's
    neighbour; its velocity difference poisons the neighbours' v_int)."""
    from marl_llm_amd.shapes import r_avoid_for
    r_avoid = r_avoid_for(n_a, shapes)
    cases, placed = degenerate_cases(shapes, n_a, r_avoid, kind)
    want, info = rule_details(cases, r_avoid)
    if kind == "cell_1e-9":
        assert np.isfinite(want).all() and (info["in_flag"] == 0).all()
        # the placed agent's v_ent is 1e-9 / (1e-9 + 1e-8) of a unit vector: the term the + 1e-8 decides must be visible
        free = [(np.abs(info["raw"][e, :, i]) < 1).any() for e, i in enumerate(placed)]
        print(kind, n_a, "placed agents with an unsaturated component:", sum(free), "of", len(free))
        assert sum(free) >= len(free) // 2
    else:
        assert np.isnan(want).any(axis=(1, 2)).all() and np.isfinite(want).any()
    for flags in (0, 2):
        compare(device_actions(cases, r_avoid, debug_flags=flags), want, info, f"{kind} N={n_a} flags={flags}")
