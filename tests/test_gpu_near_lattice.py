"""The lattice row walk against the oracle at the edge of detect_lattice's fit, and detect_lattice's structural edges.

detect_lattice (csrc/env_api.hip) accepts a cell set whose fitted coordinates lie within 1e-6 lattice steps of integers, and
the lattice kernels decide sensed cells, covered cells, the nearest cell and the fp32 reward from the fitted frame, reading
the stored cell only inside guard bands that budget for that figure: lat_m (the window margin), lat_dlt (the nearest-cell
tie band) and rew_ga_lat (the reward's band).  The other GPU files step lattices that are exact to rounding (residuals
around 4e-13 steps) or sets the fit rejects outright; here the sets of near_lattice_inputs.near_lattice carry residuals of
5e-7 and 9e-7 steps in both coordinates (walk) and 1.5e-6 and 3e-6 (scan), with agents standing on the thresholds of the
STORED cells, a few 1e-7 steps to either side.  test_near_lattice_host.py shows on the CPU that every accepted case holds
agents whose nearest cell, sensed set, covered set and in-shape flag differ between the fitted frame's cells and the stored
ones, so no test below can pass by evaluating the model alone.

Every comparison is exact (lockstep.compare: state, reward, done and the four index lists bit-equal to the oracle on the
stored cells; obs / a_prior as helpers.as_obs_dtype rounds the oracle's double), and every case asserts lattice_envs() and
path_envs() as near_lattice_inputs.lattice_fit predicts them.  profiles/r28 records three mutants of the library run against
this file.
"""
import numpy as np
import pytest

from helpers import obs_feedback, oracle_run, random_actions
from lockstep import OBSERVE, compare, device_layout, dtype_name, hold, host_copy, to_host
from near_lattice_inputs import CASES, STEPS, build_case, edge_case, edge_sets, expected_paths, lattice_fit, near_lattice
from test_gpu_mixed_paths import _path_counts

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TORCH_DT = dict(f64=torch.float64, f32=torch.float32, bf16=torch.bfloat16)
FORCED, NO_LATTICE, FULL_GEO = 1, 2, 4          # debug_flags: exact paths forced, generic kernel, full geometry at N < 64
_REF = {}


def _trajectory(oracle, shapes, name):
    """(case, oracle_run's result on the STORED cells) of one case, computed once per session and never modified: observe,
    then STEPS steps of random float32 actions alternating with the prior a handle of the case's dtype feeds back."""
    if name not in _REF:
        case = build_case(name, shapes)
        topo, g_max, occ_max = case["caps"]
        rng = np.random.default_rng([list(CASES).index(name), 31])
        acts = random_actions(rng, STEPS, len(case["cases"]), case["n_a"])
        ref = oracle_run(oracle, case["cases"], acts, case["r_avoid"], periodic=case.get("periodic", False), topo=topo, g_max=g_max,
                         occ_max=occ_max, feedback=obs_feedback(case.get("dtype", "f32")))
        _REF[name] = (case, ref)
    return _REF[name]


def _hold(case, ref, flags=0):
    """lockstep.hold of a case with the classification lattice_fit predicts: lattice_envs() and path_envs() by workgroup."""
    n_env, n_a = len(case["cases"]), case["n_a"]
    n_lat, scan = expected_paths(case)
    topo, g_max, occ_max = case["caps"]
    return hold(case["cases"], ref, lattice=0 if flags & NO_LATTICE else n_lat,
                paths=(0, n_env) if flags & NO_LATTICE else _path_counts(scan, n_env, n_a), r_avoid=case["r_avoid"],
                is_boundary=not case.get("periodic", False), topo=topo, g_max=g_max, occ_max=occ_max,
                obs_dtype=TORCH_DT[case.get("dtype", "f32")], debug_flags=flags)


# ---- 1. all envs walk ----
WALKS = [("n64", 0), ("n64_f64", 0), ("n64_bf16", 0), ("n57", 0), ("n30", 0), ("n30", FULL_GEO), ("n16", 0), ("n16", FULL_GEO),
         ("n100", 0), ("n256", 0), ("periodic", 0), ("caps", 0)]


@pytest.mark.parametrize("name,flags", WALKS, ids=[n + ("_fullgeo" if f else "") for n, f in WALKS])
def test_walks(oracle, shapes, name, flags):
    """Accepted sets of residual 5e-7 and 9e-7 steps (and an exact parent) on the row walk: the N = 64 kernels in all three
    row dtypes, a partial group of 64, several envs per workgroup in the half-occupied and the full geometry (these small
    batches take the half-occupied one; debug_flags bit 2 keeps the full one), more than one wave, the periodic arena and
    a binding sensed cap."""
    case, ref = _trajectory(oracle, shapes, name)
    assert expected_paths(case) == (len(case["cases"]), set())
    _hold(case, ref, flags)


# ---- 2. walking and scanning sets in one batch ----
@pytest.mark.parametrize("name", ["mixed64", "mixed16"])
def test_mixed(oracle, shapes, name):
    """Exact and 9e-7 sets (walk) beside 1.5e-6 and 3e-6 sets (the fit rejects them: scan) in one batch, two launches:
    path_envs() is what lattice_fit predicts, by workgroup."""
    case, ref = _trajectory(oracle, shapes, name)
    n_lat, scan = expected_paths(case)
    assert scan == {2, 3} and n_lat == len(case["cases"]) - 2
    walk = _path_counts(scan, len(case["cases"]), case["n_a"])[0]
    assert 0 < walk < len(case["cases"])
    _hold(case, ref)


# ---- 3. twins ----
@pytest.mark.parametrize("name", ["n64", "n30"])
def test_twins(oracle, shapes, name):
    """The row walk, the forced exact paths and the generic kernel on the same inputs: each equals the oracle, and the three
    handles' states, rewards and index lists equal each other."""
    case, ref = _trajectory(oracle, shapes, name)
    seen = [_hold(case, ref, flags) for flags in (0, FORCED, NO_LATTICE)]
    for other in seen[1:]:
        for t, (a, b) in enumerate(zip(seen[0], other)):
            for k in a:
                assert np.array_equal(a[k], b[k]), (t, k)


# ---- 4. the rule expert reads the same export lists ----
def test_rule_expert(oracle, shapes):
    from marl_llm_amd.batched import SwarmBatch
    from helpers import pad_cells
    case, _ = _trajectory(oracle, shapes, "n64")
    cells, n_g = pad_cells([c[2] for c in case["cases"]], max(c[2].shape[1] for c in case["cases"]))
    out = []
    for flags in (0, NO_LATTICE):
        sb = SwarmBatch(n_env=len(n_g), n_agents=case["n_a"], n_cells_max=cells.shape[2], r_avoid=case["r_avoid"], debug_flags=flags)
        try:
            sb.set_cells(cells, n_g, [c[3] for c in case["cases"]])
            sb.set_state(np.stack([c[0] for c in case["cases"]]), np.stack([c[1] for c in case["cases"]]))
            assert sb.path_envs() == ((0, len(n_g)) if flags else (len(n_g), 0))
            sb.observe()
            out.append(sb.rule_action().clone())
        finally:
            sb.close()
    assert torch.equal(out[0], out[1]) and torch.isfinite(out[0]).all()


# ---- 5. device poses: the frame rotated analytically, the cells one by one ----
def _pose_shape_set(shapes):
    """One exact shipped shape in its own pose, its 9e-7 perturbation and its 3e-6 perturbation."""
    rng = np.random.default_rng(55)
    g, l = np.asarray(shapes["grid_coords"][2], np.float64).T, float(shapes["l_cell"][2])
    sets = [g, near_lattice(g, l, 9e-7, rng), near_lattice(g, l, 3e-6, rng)]
    assert [lattice_fit(s)[0] for s in sets] == [True, True, False]
    return dict(l_cell=[l] * 3, grid_coords=[np.ascontiguousarray(s.T) for s in sets])


def _free_run_pair(sb, twin, steps, what):
    act = torch.zeros((sb.n_env, sb.n_agents, 2), dtype=torch.float32, device=sb.device)
    for t in range(steps):
        got, ref = sb.step(act), twin.step(act)
        for name, a, b in zip(("obs", "reward", "done", "a_prior"), got, ref):
            assert torch.equal(a, b), (what, t, name)
        for name, a, b in zip(("p", "dp"), sb.get_state(), twin.get_state()):
            assert torch.equal(a, b), (what, t, name)
        act = got[3].to(torch.float32)


def _oracle_step(oracle, sb, obs, l_cell, ra, envs, seed, what):
    """The current observation `obs`, and one random step, of the envs `envs` against the oracle on get_cells()'s cells."""
    cells, n_g = sb.get_cells()
    grids = [np.ascontiguousarray(cells[e][:, : n_g[e]]) for e in envs]
    p, dp = [to_host(x) for x in sb.get_state()]
    dev = host_copy(sb, obs, state=False, indices=True)
    ref = [oracle.get_observation(p[e], dp[e], g, l_cell, ra) for e, g in zip(envs, grids)]
    compare(dev, device_layout(ref, dtype_name(sb)), what + " observe", fields=OBSERVE, envs=envs)
    act = np.random.default_rng(seed).uniform(-1, 1, (sb.n_env, sb.n_agents, 2)).astype(np.float32)
    out = sb.step(torch.from_numpy(act).to(sb.device))
    ref = [oracle.step(p[e], dp[e], np.ascontiguousarray(act[e].T.astype(np.float64)), g, dev["neighbor_index"][e], l_cell, ra)
           for e, g in zip(envs, grids)]
    compare(host_copy(sb, out, indices=True), device_layout(ref, dtype_name(sb)), what + " step", envs=envs)
    return torch.from_numpy(act).to(sb.device)


@pytest.mark.parametrize("n_a,n_env", [(64, 6), (16, 6)])
def test_device_poses(oracle, shapes, n_a, n_env):
    """reset(seed) and select_shapes(index, pose) on a shape set of an exact shape, its 9e-7 and its 3e-6 perturbation: the
    device rotates the lattice frame analytically and the cells one by one.  Every output of 5 free-running steps equals
    a debug_flags = 2 twin's, two or three envs equal the oracle on the cells get_cells() returns, the envs of the 3e-6 shape scan
    and the others walk."""
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.shapes import r_avoid_for
    s3 = _pose_shape_set(shapes)
    ra, l = r_avoid_for(n_a, s3), s3["l_cell"][0]
    ng_max = max(g.shape[0] for g in s3["grid_coords"])
    mk = lambda flags: SwarmBatch(n_env=n_env, n_agents=n_a, n_cells_max=ng_max, r_avoid=ra, debug_flags=flags)
    sb, twin = mk(0), mk(NO_LATTICE)
    try:
        sb.set_shapes(s3); twin.set_shapes(s3)
        obs = sb.reset(seed=28)
        assert torch.equal(obs, twin.reset(seed=28))
        drawn = sb.get_shape_index()
        assert np.array_equal(drawn, twin.get_shape_index())
        assert sb.path_envs() == _path_counts(set(np.nonzero(drawn == 2)[0]), n_env, n_a) and twin.path_envs() == (0, n_env)
        envs = sorted({0, int(np.argmax(drawn == 1))})
        act = _oracle_step(oracle, sb, obs, l, ra, envs, 1, "reset")
        twin.step(act)
        _free_run_pair(sb, twin, 5, "reset")
        rng = np.random.default_rng([n_a, 56])
        index = np.array([2, 1, 2, 0, 0, 1])              # N = 16, four envs per workgroup: [0..3] scans, [4 5] walks
        ang, off = rng.uniform(-np.pi, np.pi, n_env), rng.uniform(-0.9, 0.9, (n_env, 2))
        obs = sb.select_shapes(index, angle=ang, offset=off)
        assert torch.equal(obs, twin.select_shapes(index, angle=ang, offset=off))
        want = _path_counts(set(np.nonzero(index == 2)[0]), n_env, n_a)
        assert sb.path_envs() == want and want[0] > 0 and twin.path_envs() == (0, n_env)
        act = _oracle_step(oracle, sb, obs, l, ra, [0, 1, 5], 2, "select_shapes")
        twin.step(act)
        _free_run_pair(sb, twin, 5, "select_shapes")
        assert sb.path_envs() == want
    finally:
        sb.close(); twin.close()


# ---- 6. structural edges of detect_lattice ----
@pytest.mark.parametrize("n_a", [64, 16])
@pytest.mark.parametrize("name", list(edge_sets()))
def test_structural_edges(oracle, shapes, name, n_a):
    """detect_lattice on the accept / reject boundary of the row and column count (64 / 65; agents in rows 0, 62 and 63 of
    the kernels' 64-entry row tables and beyond both ends), an empty row, rows stored top to bottom (the mirror retry),
    column-major order, a duplicated cell, a single column, two cells, one cell and two swapped cells: lattice_envs() and
    path_envs() are lattice_fit's prediction (which test_near_lattice_host.py holds to the expectation where one is
    stated), and observe + 2 steps equal the oracle."""
    cases, path, ok, want, ra = edge_case(name, n_a, shapes)
    assert want is None or path == want
    rng = np.random.default_rng([list(edge_sets()).index(name), n_a, 33])
    ref = oracle_run(oracle, cases, random_actions(rng, 2, len(cases), n_a), ra, feedback=obs_feedback("f64"))
    hold(cases, ref, lattice=len(cases) if ok else 0, paths=(len(cases), 0) if path == "walk" else (0, len(cases)), r_avoid=ra,
         obs_dtype=torch.float64)
