"""GPU parity tests: the HIP path (through the C ABI, via marl_llm_amd.batched.SwarmBatch) against the oracle
(oracle/assembly_oracle.c) and against the golden vectors recorded from the reference.

Tolerances, stated once:
  * state (p, dp), every index / flag array, done and reward: BIT-EXACT (==).
  * obs / a_prior with obs_dtype=float64: BIT-EXACT.
  * obs / a_prior with obs_dtype=float32 (the product dtype): equal to the oracle's double value rounded once to
    float32 -- i.e. exact equality after casting the oracle's output to float32 (|err| <= 2^-24 relative).
  The only outputs that touch a non-correctly-rounded primitive are the reward's cos() terms (device libm vs
  glibc, <= a few ulp); a flip of the 0.05 threshold from that has probability ~1e-14 per agent-step.
"""
import os

import numpy as np
import pytest

from helpers import GOLDEN_DIR, golden_files, load_golden, make_case, oracle_run, pad_cells, random_actions
from helpers import adversarial_case as _adversarial_case
from lockstep import compare, device_layout, hold, host_copy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _batch(**kw):
    from marl_llm_amd.batched import SwarmBatch
    return SwarmBatch(**kw)


# lockstep's field -> its key in the golden files
GOLDEN = dict(p="p_next", dp="dp_next", obs="obs", a_prior="a_prior", reward="rew", neighbor_index="nei", in_flags="in_flags",
              sensed_index="sensed", occupied_index="occupied")


@pytest.mark.parametrize("path", golden_files(), ids=os.path.basename)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_golden_steps(path, dtype):
    """Every recorded reference step, teacher-forced through the HIP path (E = 1)."""
    z = load_golden(path)
    T, _, n_a = z["p"].shape
    n_g = z["grid"].shape[1]
    odt = torch.float64 if dtype == "f64" else torch.float32
    sb = _batch(n_env=1, n_agents=n_a, n_cells_max=n_g, r_avoid=float(z["r_avoid"]), d_sen=float(z["d_sen"]),
                is_boundary=bool(z["is_boundary"]), with_self=bool(z["with_self"]), obs_dtype=odt,
                boundary=tuple(z["boundary"]))
    try:
        sb.set_cells(z["grid"][None], [n_g], [float(z["l_cell"])])
        for t in range(T):
            sb.set_state(z["p"][t][None], z["dp"][t][None])
            sb.observe()
            assert np.array_equal(sb.indices(False, False)["neighbor_index"][0].cpu().numpy(), z["nei_prev"][t])
            act = torch.from_numpy(np.ascontiguousarray(z["a"][t].T)[None]).to(sb.device)       # (2,N) -> [1,N,2]
            dev = host_copy(sb, sb.step(act), indices=True)
            compare(dev, device_layout({k: z[g][t][None] for k, g in GOLDEN.items()}, dtype), t)
    finally:
        sb.close()


@pytest.mark.parametrize("n_a", [30, 100, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_golden_batches(n_a, dtype):
    """Three recorded reference episodes of one agent count (own seed, own target shape: ragged cell sets) teacher-forced
    through the HIP path as ONE 3-env batch: the batched layout, env-indexed cell sets and the agent counts that are not
    powers of two held against the reference itself (make_golden.py r3b), not only against the pinned oracle."""
    zs = [load_golden(p) for p in golden_files(f"g11_n{n_a}_s*.npz")]
    assert len(zs) == 3
    E, T = len(zs), min(z["p"].shape[0] for z in zs)
    cells, n_g = pad_cells([z["grid"] for z in zs], max(z["grid"].shape[1] for z in zs))
    assert len({float(z["r_avoid"]) for z in zs}) == 1 and len(set(n_g.tolist())) > 1
    odt = torch.float64 if dtype == "f64" else torch.float32
    sb = _batch(n_env=E, n_agents=n_a, n_cells_max=cells.shape[2], r_avoid=float(zs[0]["r_avoid"]), d_sen=float(zs[0]["d_sen"]),
                obs_dtype=odt, boundary=tuple(zs[0]["boundary"]))
    st = lambda k, t: np.stack([z[k][t] for z in zs])
    try:
        sb.set_cells(cells, n_g, [float(z["l_cell"]) for z in zs])
        for t in range(T):
            sb.set_state(st("p", t), st("dp", t))
            sb.observe()
            assert np.array_equal(sb.indices(False, False)["neighbor_index"].cpu().numpy(), st("nei_prev", t))
            act = torch.from_numpy(np.ascontiguousarray(st("a", t).transpose(0, 2, 1))).to(sb.device)      # (E,2,N) -> [E,N,2]
            dev = host_copy(sb, sb.step(act), indices=True)
            compare(dev, device_layout({k: st(g, t) for k, g in GOLDEN.items()}, dtype), t)
    finally:
        sb.close()


def test_known_answer_case():
    """SURVEY.md section 8c hand-checkable case (topo=2, G=4, OCC=5) through the HIP path."""
    z = load_golden(os.path.join(GOLDEN_DIR, "g1_kat_n3.npz"))
    sb = _batch(n_env=1, n_agents=3, n_cells_max=4, r_avoid=0.15, d_sen=0.4, topo=2, g_max=4, occ_max=5,
                obs_dtype=torch.float64)
    sb.set_cells(z["grid"][None], [4], [0.06])
    sb.set_state(z["p"][None], z["dp"][None])
    obs = sb.observe()
    idx = sb.indices()
    assert idx["neighbor_index"][0].cpu().tolist() == [[1, -1], [0, -1], [-1, -1]]
    assert idx["in_flags"][0].cpu().tolist() == [1, 0, 0]
    assert idx["sensed_index"][0].cpu().tolist() == [[2, -1, -1, -1], [0, 1, 2, -1], [-1, -1, -1, -1]]
    assert idx["occupied_index"][0].cpu().tolist() == [[0, 1, -1, -1, -1], [-1] * 5, [-1] * 5]
    assert np.array_equal(obs[0].cpu().numpy(), device_layout(dict(obs=z["obs"][None]))["obs"][0])
    sb.close()


CONFIGS = [  # (n_a, n_env, cluster, periodic, with_self, steps)
    (3, 5, 1, False, True, 4), (8, 16, 1, False, True, 6), (8, 9, 0, True, True, 4), (30, 6, 1, False, True, 6),
    (32, 8, 1, False, False, 6), (32, 5, 0, False, True, 4), (64, 6, 1, False, True, 8), (64, 4, 0, False, True, 4),
    (64, 3, 1, True, True, 4), (100, 3, 1, False, True, 3), (128, 2, 1, False, True, 3), (256, 2, 1, False, True, 3),
    (200, 2, 0, True, False, 2),
]


@pytest.mark.parametrize("flags", [0, 2], ids=["lattice", "generic"])
@pytest.mark.parametrize("n_a,n_env,cluster,periodic,with_self,steps", CONFIGS)
def test_batched_trajectories_vs_oracle(oracle, shapes, n_a, n_env, cluster, periodic, with_self, steps, flags):
    """E independent envs with different shapes / rotations, free-running for several steps: the state
    trajectory, all masks and fp64 outputs stay bit-identical to E sequential oracle envs."""
    from marl_llm_amd.shapes import r_avoid_for
    rng = np.random.default_rng(7000 + 13 * n_a + n_env)
    ra = r_avoid_for(n_a, shapes)
    cases = [make_case(rng, shapes, n_a, cluster) for _ in range(n_env)]
    # random float32 actions alternating with the fed-back prior (assembles the swarm; exercises the occupied filter harder)
    ref = oracle_run(oracle, cases, random_actions(rng, steps, n_env, n_a), ra, periodic=periodic, with_self=with_self)
    # the synthetic shapes are tiled lattices like the reference's: recognised unless the path is disabled
    hold(cases, ref, lattice=n_env if flags == 0 else 0, r_avoid=ra, is_boundary=not periodic, with_self=with_self,
         obs_dtype=torch.float64, debug_flags=flags)


def test_small_caps(oracle, shapes):
    """Shrunk caps so both round(i*step) sub-samplings (80-cell and 200-cell lists) are exercised."""
    from marl_llm_amd.shapes import r_avoid_for
    rng = np.random.default_rng(5)
    n_a, n_env = 32, 4
    ra = r_avoid_for(n_a, shapes)
    cases = [make_case(rng, shapes, n_a, 1) for _ in range(n_env)]
    # (G-1 odd -> integer cap arithmetic; G-1 even -> the reference's fp64 round(), ties possible)
    for topo, g_max, occ_max in ((3, 10, 7), (6, 80, 20), (1, 6, 200), (2, 5, 9), (6, 81, 33), (4, 21, 11)):
        first = [oracle.get_observation(p, dp, g, l_cell, ra, topo=topo, g_max=g_max, occ_max=occ_max) for p, dp, g, l_cell in cases]
        hold(cases, (first, []), pad=0, r_avoid=ra, topo=topo, g_max=g_max, occ_max=occ_max, obs_dtype=torch.float64)


@pytest.mark.parametrize("n_a,n_env,env_offset", [
    (64, 4096, 0),            # BASELINE config 2 (headline): one wavefront per env and split
    (32, 1024, 0),            # BASELINE config 1: two envs per wavefront (EPB = 2)
    (256, 4096, 0),           # BASELINE config 4: 1024-thread workgroups, LDS-atomic pair masks, dense O(N^2) path
    (64, 4096, 3 * 4096),     # one rank's shard of BASELINE config 3 (64 x 32768 over 8 GPUs): envs [12288, 16384)
    (32, 1023, 0),            # env count not divisible by the envs per workgroup: the `e >= n_env` tail lanes
    (30, 1021, 0),            # the reference's default agent count, padded lanes inside every wavefront
], ids=["64x4096", "32x1024", "256x4096", "64x4096_shard3", "32x1023", "30x1021"])
def test_full_size_properties(oracle, shapes, n_a, n_env, env_offset):
    """Every BASELINE shape at FULL size: size-independent invariants over the whole batch plus an exact oracle
    comparison on a sample of environments (incl. the first and the last), in the product dtype (float32 obs)."""
    from marl_llm_amd.shapes import r_avoid_for
    from marl_llm_amd.synth import synthetic_batch
    ra = r_avoid_for(n_a, shapes)
    sy = synthetic_batch(n_env, n_a, shapes, seed=226, assembled_fraction=0.5, env_offset=env_offset)
    if env_offset:            # a shard is the same slice of the global generation (counter-based inputs)
        ref = synthetic_batch(8, n_a, shapes, seed=226, assembled_fraction=0.5, env_offset=env_offset + 100)
        assert np.array_equal(ref["p"], sy["p"][100:108]) and np.array_equal(ref["cells"], sy["cells"][100:108])
    sb = _batch(n_env=n_env, n_agents=n_a, n_cells_max=sy["cells"].shape[2], r_avoid=ra)
    sb.set_cells(sy["cells"], sy["n_g"], sy["l_cell"])
    sb.set_state(sy["p"], sy["dp"])
    sb.observe()
    nei0 = sb.indices(False, False)["neighbor_index"].cpu().numpy()
    rng = np.random.default_rng(1)
    act = rng.uniform(-1, 1, (n_env, n_a, 2)).astype(np.float32)
    try:
        dev = host_copy(sb, sb.step(torch.from_numpy(act).to(sb.device)), indices=True)
        obs_c, pg, sen = dev["obs"], dev["p"], dev["sensed_index"]
        assert np.isfinite(obs_c).all() and np.isfinite(pg).all()
        assert set(np.unique(dev["reward"])).issubset({0.0, 1.0})
        assert np.abs(dev["dp"]).max() <= 0.8 and np.abs(dev["a_prior"]).max() <= 1.0
        assert (obs_c[:, :, 0] == pg[:, 0, :].astype(np.float32)).all()          # self block = absolute state
        assert ((sen[:, :, 1:] < 0) | (sen[:, :, :-1] >= 0)).all()               # valid slots form a prefix
        assert (np.diff(np.where(sen >= 0, sen, 1 << 20), axis=-1) > 0)[(sen[:, :, 1:] >= 0)].all()   # ascending cell index
        assert sb.lattice_envs() == n_env                                       # tiled shapes: the row-walk path (N <= 64)
        compare(dev, None, "whole batch", fields=("done", "unused"))            # no done, unused slots zero in obs: every env
        sample = np.unique(np.concatenate([[0, 1, n_env - 2, n_env - 1], rng.choice(n_env, 24 if n_a <= 64 else 10, replace=False)]))
        ref = [oracle.step(sy["p"][e], sy["dp"][e], np.ascontiguousarray(act[e].T), sy["cells"][e][:, : sy["n_g"][e]], nei0[e],
                           float(sy["l_cell"][e]), ra) for e in sample]
        compare(dev, device_layout(ref, "f32"), "sample", envs=sample)
    finally:
        sb.close()


def test_error_behaviour(shapes):
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd._lib import SwarmError
    with pytest.raises(SwarmError):
        SwarmBatch(n_env=1, n_agents=300, n_cells_max=10, r_avoid=0.1)
    sb = SwarmBatch(n_env=2, n_agents=8, n_cells_max=600, r_avoid=0.5)
    with pytest.raises(SwarmError):                  # step before cells/state/observe
        sb.step(torch.zeros((2, 8, 2), device=sb.device))
    with pytest.raises(SwarmError):
        sb.observe()
    with pytest.raises(SwarmError):                  # wrong action shape
        sb.step(torch.zeros((2, 7, 2), device=sb.device))
    sb.close()


@pytest.mark.parametrize("n_a,n_env,force", [(64, 24, 0), (64, 8, 1), (64, 12, 2), (64, 6, 3), (32, 16, 0), (32, 8, 2), (8, 16, 0),
                                             (256, 3, 0), (100, 4, 1)])
def test_threshold_adversarial_inputs(oracle, shapes, n_a, n_env, force):
    """The fp32 pre-filter must hand every borderline decision to the exact fp64 path: masks, flags and the
    step stay bit-identical to the oracle on inputs constructed to sit on the thresholds.  force=1 runs the
    same inputs with every exact fallback forced (debug flag bit 0); bit 1 disables the lattice row walk, so both
    the lattice and the generic all-cells paths are exercised -- all must agree with the oracle."""
    from marl_llm_amd.shapes import r_avoid_for
    rng = np.random.default_rng(4242 + n_a + force)
    ra = r_avoid_for(n_a, shapes)
    cases = [_adversarial_case(rng, shapes, n_a, ra) for _ in range(n_env)]
    ref = oracle_run(oracle, cases, [np.zeros((n_env, n_a, 2), np.float32)], ra)      # zero action: the agents stay near the thresholds
    hold(cases, ref, pad=0, r_avoid=ra, obs_dtype=torch.float64, debug_flags=force)


def test_forced_exact_paths_equal_fast_paths(shapes):
    """Whole-batch consistency: fast and forced-exact runs, lattice walk and generic scan (debug_flags 0..3) give
    identical outputs over several free-running steps at a BASELINE-sized agent count (tools/stress_consistency.py
    runs the same comparison at millions of agent-steps)."""
    from marl_llm_amd.shapes import r_avoid_for
    from marl_llm_amd.synth import synthetic_batch
    n_a, n_env = 64, 512
    ra = r_avoid_for(n_a, shapes)
    sy = synthetic_batch(n_env, n_a, shapes, seed=11, assembled_fraction=0.6)
    outs = []
    for force in (0, 1, 2, 3):
        sb = _batch(n_env=n_env, n_agents=n_a, n_cells_max=sy["cells"].shape[2], r_avoid=ra, debug_flags=force)
        sb.set_cells(sy["cells"], sy["n_g"], sy["l_cell"]); sb.set_state(sy["p"], sy["dp"]); sb.observe()
        act = torch.zeros((n_env, n_a, 2), device=sb.device)
        rews = []
        for t in range(12):
            obs, rew, done, act = sb.step(act)
            rews.append(rew.clone())
        p, dp = sb.get_state()
        idx = sb.indices()
        outs.append((obs.clone(), torch.stack(rews), p, dp, idx["sensed_index"], idx["occupied_index"], idx["in_flags"]))
        sb.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    assert outs[0][1].sum().item() > 0          # some agents do earn the reward in this workload


def test_diagnostic_repeat_hooks_do_not_change_results(shapes):
    """tools/ablate.py relies on every phase being idempotent: running any phase extra times (debug hook) must
    leave every output bit-identical."""
    from marl_llm_amd.shapes import r_avoid_for
    from marl_llm_amd.synth import synthetic_batch
    n_a, n_env = 64, 96
    ra = r_avoid_for(n_a, shapes)
    sy = synthetic_batch(n_env, n_a, shapes, seed=5, assembled_fraction=0.6)
    ref = None
    for flags in [0] + [(k << 8) | (2 << 12) for k in range(1, 13)]:
        sb = _batch(n_env=n_env, n_agents=n_a, n_cells_max=sy["cells"].shape[2], r_avoid=ra, debug_flags=flags)
        sb.set_cells(sy["cells"], sy["n_g"], sy["l_cell"]); sb.set_state(sy["p"], sy["dp"]); sb.observe()
        act = torch.zeros((n_env, n_a, 2), device=sb.device)
        for t in range(4):
            obs, rew, done, act = sb.step(act)
        p, dp = sb.get_state()
        idx = sb.indices()
        out = (obs.clone(), rew.clone(), act.clone(), p, dp, idx["sensed_index"], idx["occupied_index"], idx["neighbor_index"])
        sb.close()
        if ref is None:
            ref = out
        else:
            for a, b in zip(ref, out):
                assert torch.equal(a, b), flags


def test_non_lattice_cells_fall_back_to_generic_path(oracle, shapes):
    """Arbitrary (jittered, shuffled) cell sets are not a lattice: the generic scan serves them, same results."""
    from marl_llm_amd.shapes import r_avoid_for
    rng = np.random.default_rng(77)
    n_a, n_env = 32, 6
    ra = r_avoid_for(n_a, shapes)
    cases = []
    for k in range(n_env):
        p, dp, g, l_cell = make_case(rng, shapes, n_a, 1)
        if k % 2 == 0:
            g = g + rng.normal(0, 0.004, g.shape)               # jitter: off-lattice
        else:
            g = np.ascontiguousarray(g[:, rng.permutation(g.shape[1])])   # on-lattice points, but not row-major order
        cases.append((p, dp, np.ascontiguousarray(g), l_cell))
    first = [oracle.get_observation(p, dp, g, l_cell, ra) for p, dp, g, l_cell in cases]
    hold(cases, (first, []), lattice=0, pad=0, r_avoid=ra, obs_dtype=torch.float64)


@pytest.mark.parametrize("n_a", [64, 24])
def test_wide_lattice_uses_64_bit_row_masks(oracle, n_a):
    """A shape wider than 32 lattice columns (the reference's are not) takes the 64-bit row-mask instantiation of the
    lattice walk: observation, index scratch and a step against the oracle, including agents on the decision thresholds."""
    rng = np.random.default_rng(9 + n_a)
    l_cell, ra = 0.055, 0.12
    cols, rows = 44, 12
    keep = rng.uniform(size=(rows, cols)) > 0.12                       # holes; every row keeps some cells
    keep[:, 0] = True; keep[:, -1] = True
    bb, aa = np.nonzero(keep)                                          # row-major: rows ascending, columns ascending
    base = np.stack([aa * l_cell, bb * l_cell]).astype(np.float64)
    n_env = 6
    cases = []
    for e in range(n_env):
        th = rng.uniform(-np.pi, np.pi)
        rot = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]])
        g = np.ascontiguousarray(rot @ (base - base.mean(1, keepdims=True)) + rng.uniform(-0.8, 0.8, (2, 1)))
        p = g[:, rng.integers(0, g.shape[1], n_a)] + rng.normal(0, 0.05, (2, n_a))
        for i in range(0, n_a, 3):                                     # threshold cases: d_sen, r_avoid/2, midpoints
            c = int(rng.integers(0, g.shape[1])); u = rng.normal(size=2); u /= np.linalg.norm(u)
            p[:, i] = g[:, c] + u * [0.4, ra / 2, 0.5 * l_cell][i % 3] * (1 + [0.0, 1e-13, -1e-10][(i // 3) % 3])
        dp = rng.uniform(-0.3, 0.3, (2, n_a))
        cases.append((np.ascontiguousarray(p), dp, g, l_cell))
    ref = oracle_run(oracle, cases, [rng.uniform(-1, 1, (n_env, n_a, 2)).astype(np.float32)], ra)
    hold(cases, ref, lattice=n_env, pad=0, r_avoid=ra, obs_dtype=torch.float64)


@pytest.mark.parametrize("n_a,periodic", [(64, False), (36, True), (200, False)])
def test_exact_distance_ties_in_the_neighbour_list(oracle, shapes, n_a, periodic):
    """Agents on an exactly representable square grid: every agent has several neighbours at EXACTLY equal distance, so the
    order of its list is decided by the tie rule alone (lower index first -- the reference's std::sort leaves ties
    unspecified, CPP:641; oracle and kernel both take the lower index).  Exercises the exact fallback of the key-based
    neighbour selection (keys that agree in all but the index bits)."""
    from marl_llm_amd.shapes import r_avoid_for
    rng = np.random.default_rng(4)
    ra = r_avoid_for(n_a, shapes)
    side = int(np.ceil(np.sqrt(n_a)))
    E = 3
    cases = []
    for e in range(E):
        _, dp, g, l_cell = make_case(rng, shapes, n_a, 0)
        pitch = [0.125, 0.1875, 0.25][e]                    # exact in binary: distances tie exactly
        ij = rng.permutation(side * side)[:n_a]            # random index <-> grid position assignment
        p = np.stack([(ij % side) * pitch - 1.0, (ij // side) * pitch - 1.0])
        cases.append((np.ascontiguousarray(p), dp, g, l_cell))
    # one free step from a zero (float64) action: rewards / priors on tied lists (collision flag = nearest listed neighbour)
    ref = oracle_run(oracle, cases, [np.zeros((E, n_a, 2))], ra, periodic=periodic)
    ties = 0
    for (p, dp, g, l_cell), o in zip(cases, ref[0]):
        nei = o["neighbor_index"]
        for i in range(n_a):                                # count lists that really contain a tie
            js = nei[i][nei[i] >= 0]
            d = np.sum((p[:, js] - p[:, [i]]) ** 2, axis=0)
            ties += int(len(d) > 1 and (np.diff(d) == 0).any())
    assert ties > n_a                                       # most lists do
    hold(cases, ref, pad=0, r_avoid=ra, is_boundary=not periodic, obs_dtype=torch.float64)


def test_near_ties_whose_norms_coincide(oracle, shapes):
    """Two neighbours whose SQUARED distances differ by an ulp or two but whose norms (sqrt) are equal: the reference
    sorts by the norm (CPP:636-641), so they tie and the lower index comes first -- although its squared distance is the
    LARGER one.  A selection that orders by squared distance gets these lists wrong."""
    from marl_llm_amd.shapes import r_avoid_for
    n_a, E = 8, 6
    rng = np.random.default_rng(11)
    ra = r_avoid_for(n_a, shapes)
    cases, collapsed = [], 0
    while len(cases) < E:
        x, y = rng.uniform(0.05, 0.25, 2)
        hit = None
        for k in range(1, 6):
            bx = x
            for _ in range(k):
                bx = np.nextafter(bx, 1.0)
            d_small, d_large = x * x + y * y, y * y + bx * bx
            if d_small != d_large and np.sqrt(d_small) == np.sqrt(d_large):
                hit = bx
                break
        if hit is None:
            continue
        _, dp, g, l_cell = make_case(rng, shapes, n_a, 0)
        p = rng.uniform(-2.3, 2.3, (2, n_a))
        p[:, 0] = 0.0                                      # agent 0 at the origin: relative positions are exact
        p[:, 1] = (y, hit)                                 # lower index, larger squared distance, same norm
        p[:, 2] = (x, y)
        far = np.sum(p[:, 3:] ** 2, axis=0) < 0.45 ** 2    # keep the others out of agent 0's sensing range
        p[:, 3:][:, far] += 1.0
        cases.append((np.ascontiguousarray(p), dp, g, l_cell))
    first = [oracle.get_observation(p, dp, g, l_cell, ra) for p, dp, g, l_cell in cases]
    for (p, dp, g, l_cell), o in zip(cases, first):
        assert list(o["neighbor_index"][0][:2]) == [1, 2]           # the oracle (= reference rule): tie, lower index first
        d2 = np.sum(p[:, 1:3] ** 2, axis=0)
        collapsed += int(d2[0] > d2[1])
    assert collapsed == E
    hold(cases, (first, []), pad=0, r_avoid=ra, obs_dtype=torch.float64)


@pytest.mark.parametrize("n_a,n_env,periodic", [(8, 37, False), (16, 9, True), (30, 21, False), (32, 64, False), (32, 5, True)])
def test_half_occupied_geometry_equals_the_full_one(oracle, shapes, n_a, n_env, periodic):
    """Small batches of N < 64 agents run with half of the agent threads empty and eight lanes per agent in the list phase
    (twice the workgroups: Geo<NPAD, true>); debug_flags bit 2 keeps the full geometry.  Both must give the same bits as
    each other on free-running steps, and the oracle's on the last one."""
    from marl_llm_amd.shapes import r_avoid_for
    from marl_llm_amd.synth import synthetic_batch
    ra = r_avoid_for(n_a, shapes)
    sy = synthetic_batch(n_env, n_a, shapes, seed=17 + n_a, assembled_fraction=0.7)
    outs = []
    for flags in (0, 4):
        sb = _batch(n_env=n_env, n_agents=n_a, n_cells_max=sy["cells"].shape[2], r_avoid=ra, is_boundary=not periodic,
                    obs_dtype=torch.float64, debug_flags=flags)
        sb.set_cells(sy["cells"], sy["n_g"], sy["l_cell"]); sb.set_state(sy["p"], sy["dp"]); sb.observe()
        act = torch.zeros((n_env, n_a, 2), dtype=torch.float64, device=sb.device)
        rews = []
        for t in range(12):
            if t == 11:
                p0, dp0 = [x.cpu().numpy() for x in sb.get_state()]
                nei0 = sb.indices(False, False)["neighbor_index"].cpu().numpy()
                a0 = act.cpu().numpy()
            obs, rew, done, pri = sb.step(act)
            act = pri.clone()
            rews.append(rew.clone())
        idx = sb.indices()
        p, dp = sb.get_state()
        outs.append((obs.clone(), torch.stack(rews), pri.clone(), p, dp, idx["sensed_index"], idx["occupied_index"],
                     idx["neighbor_index"], idx["in_flags"], p0, dp0, nei0, a0,
                     host_copy(sb, (obs, rew, done, pri), state=(p, dp), indices=idx, rows=slice(0, 6))))
        sb.close()
    for a, b in zip(outs[0][:9], outs[1][:9]):
        assert torch.equal(a, b)
    p0, dp0, nei0, a0, dev = outs[0][9:]
    ref = [oracle.step(p0[e], dp0[e], np.ascontiguousarray(a0[e].T), sy["cells"][e][:, : sy["n_g"][e]], nei0[e], float(sy["l_cell"][e]),
                       ra, is_boundary=not periodic) for e in range(min(n_env, 6))]
    compare(dev, device_layout(ref), "last step")


def _reward_threshold_case(oracle, rng, shapes, n_a, ra, d_sen=0.4):
    """One env whose in-shape agents sit 1e-12 .. 1e-9 from the reward's `|v| < 0.05` decision: starting at a cell centre and
    half a cell away with different oracle rewards, each is bisected along that segment down to adjacent doubles, then moved
    that far off the crossing to either side at random -- far inside the fp32 sums' error (~1e-7), far outside the fp64
    path's documented cos() deviation (~1e-16, test_gpu_parity.py docstring).  They start at least d_sen + r_avoid apart (nothing sensed, occupied or colliding in common,
    so they are bisected together); the other agents wait in two arena corners out of everyone's range.  Zero velocity: a
    zero-action step leaves every position as it is, so the step's reward is decided at these positions.
    Returns (p, g, l_cell, number of agents whose crossing is the |v| test itself: same in-flag and sensed list both sides)."""
    s = int(rng.integers(0, len(shapes["l_cell"])))
    l_cell = float(shapes["l_cell"][s])
    th = rng.uniform(-np.pi, np.pi)
    rot = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]])
    g = shapes["grid_coords"][s].T
    g = np.ascontiguousarray(rot @ (g - g.mean(axis=1, keepdims=True)))
    cand = []
    for c in rng.permutation(g.shape[1]):
        if all(np.hypot(*(g[:, c] - g[:, k])) > d_sen + ra for k in cand):
            cand.append(c)
    park = np.array([(x, y) for x in np.arange(1.8, 2.35, 0.1) for y in np.arange(1.8, 2.35, 0.1)]).T
    park = np.concatenate([park, -park], axis=1)
    K = min(len(cand), n_a)
    p = np.zeros((2, n_a))
    p[:, :K] = g[:, cand[:K]]
    p[:, K:] = park[:, : n_a - K]
    assert np.hypot(*g).max() < 1.6 and n_a - K <= park.shape[1]       # corners >= 0.95 from every cell
    zero = np.zeros((2, n_a))

    def reward(q):
        o = oracle.get_observation(q, zero, g, l_cell, ra, d_sen=d_sen)
        return oracle.get_reward(q, g, o["neighbor_index"], o["in_flags"], o["sensed_index"], ra, d_sen=d_sen)[0], o

    r0, o0 = reward(p)
    lo, hi = p.copy(), p.copy()
    live = np.zeros(n_a, bool)
    for a in rng.permutation(8) * (np.pi / 4):
        q = p.copy()
        q[:, :K] += 0.5 * l_cell * np.array([[np.cos(a)], [np.sin(a)]])
        r, o = reward(q)
        new = (np.arange(n_a) < K) & ~live & (r != r0) & (o["in_flags"] == 1) & (o0["in_flags"] == 1)
        hi[:, new] = q[:, new]
        live |= new
    u = hi - lo
    u /= np.where(live, np.hypot(*u), 1.0)
    for _ in range(64):
        mid = lo.copy()
        mid[:, live] = lo[:, live] + 0.5 * (hi[:, live] - lo[:, live])
        r, _ = reward(mid)
        same = r == r0
        lo[:, live & same] = mid[:, live & same]
        hi[:, live & ~same] = mid[:, live & ~same]
    r_lo, o_lo = reward(lo)
    r_hi, o_hi = reward(hi)
    assert (r_lo[live] != r_hi[live]).all()
    exact = live & (o_lo["in_flags"] == o_hi["in_flags"]) & (o_lo["sensed_index"] == o_hi["sensed_index"]).all(axis=1)
    side = rng.uniform(size=n_a) < 0.5
    off = u * 10.0 ** rng.uniform(-12, -9, n_a)
    p = np.where(live, np.where(side, hi + off, lo - off), lo)
    return np.ascontiguousarray(p), g, l_cell, int(exact.sum())


@pytest.mark.parametrize("n_a,flags", [(64, 0), (64, 1), (64, 2), (32, 0)], ids=["64-lattice", "64-forced", "64-generic", "32-lattice"])
def test_reward_threshold_placements(oracle, shapes, n_a, flags):
    """Agents placed on the reward's 0.05 threshold to within an ulp: the fp32 sums of the lattice path and of the generic
    scan can only decide outside their guard bands, so every one of these rewards must come out of the exact fp64 path and
    equal the oracle's (a guard band that is missing or too narrow lets the fp32 verdict through for about half of them)."""
    from marl_llm_amd.shapes import r_avoid_for
    rng = np.random.default_rng(900 + n_a)
    ra = r_avoid_for(n_a, shapes)
    E = 48
    cases = [_reward_threshold_case(oracle, rng, shapes, n_a, ra) for _ in range(E)]
    assert sum(c[3] for c in cases) >= 16           # agents whose crossing is the |v| test itself (not in-flag / list)
    # zero velocity, zero (float64) action: a step leaves every position as it is
    cases = [(p, np.zeros_like(p), g, l_cell) for p, g, l_cell, _ in cases]
    ref = oracle_run(oracle, cases, [np.zeros((E, n_a, 2))], ra)
    assert sum(int(s["reward"].sum()) for s in ref[1][0]) > 0
    seen = hold(cases, ref, lattice=0 if flags & 2 else E, pad=0, r_avoid=ra, obs_dtype=torch.float64, debug_flags=flags)
    assert np.array_equal(seen[1]["p"], np.stack([c[0] for c in cases]))    # nothing moved: the reward was decided at the placed positions
