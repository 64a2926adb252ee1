"""Pin the oracle (oracle/assembly_oracle.c) against the reference's own C++ compiled unmodified
(oracle/_ref/libAssemblyEnv.so, built by oracle/Makefile from
/root/reference/cus_gym/gym/envs/customized_envs/envs_cplus/src/AssemblyEnv.cpp).
Both are IEEE double with the same operation order, so equality is exact (==), not a tolerance.

The hand-built cases of the legacy symbols (helpers.legacy_specs, what tests/test_gpu_legacy_contract.py feeds the HIP shim) run
here first: every named input is defined in the reference, and the oracle -- the witness where oracle/_ref was not built --
agrees with it bit for bit.  No input had to be dropped.  Two things the cases stay clear of because the reference leaves
them open: agents at equal distance from an agent in _get_observation (std::sort's order of equal keys, AssemblyEnv.cpp:641)
and dim != 2 (the reference reads dim rows of every two-row input), which only the shim's refusal path is given."""
import numpy as np
import pytest

from helpers import (BIG_BOX, CAPS_DTYPE_NS, CAPS_DTYPE_ROWS, CAPS_NS, CAPS_ROWS, DEFAULT_BOX, DYNAMICS_ROWS, OFF_BOX, as_obs_dtype,
                     assert_same, bf16_direct, caps_reach, caps_trajectory, config_case, legacy_cache_configs, legacy_call, legacy_case,
                     legacy_reach, legacy_specs, make_case, physics)
from marl_llm_amd.shapes import r_avoid_for
from oracle.oracle_py import numpy_dist_b2b, ref_step

CASES = [(n, c, per, ws) for n in (3, 8, 32, 64) for c in (0, 1) for per in (False, True) for ws in (True, False)]
CASES += [(256, 1, False, True), (256, 0, True, True)]


@pytest.mark.parametrize("n_a,cluster,periodic,with_self", CASES)
def test_functions_and_step_match_reference(oracle, reflib, shapes, n_a, cluster, periodic, with_self):
    rng = np.random.default_rng(1000 * n_a + 100 * cluster + 10 * periodic + with_self)
    p, dp, g, l_cell = make_case(rng, shapes, n_a, cluster)
    ra = r_avoid_for(n_a, shapes)
    a = oracle.get_observation(p, dp, g, l_cell, ra, is_periodic=periodic, with_self=with_self)
    b = reflib.get_observation(p, dp, g, l_cell, ra, is_periodic=periodic, with_self=with_self)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    ra_ = oracle.get_reward(p, g, a["neighbor_index"], a["in_flags"], a["sensed_index"], ra, is_periodic=periodic)
    rb_ = reflib.get_reward(p, g, a["neighbor_index"], a["in_flags"], a["sensed_index"], ra, is_periodic=periodic,
                            occupied_index=a["occupied_index"])
    assert np.array_equal(ra_, rb_)
    assert np.array_equal(oracle.action_prior(p, dp, g, a["neighbor_index"], l_cell, ra),
                          reflib.action_prior(p, dp, g, a["neighbor_index"], l_cell, ra))
    dc, de, co = oracle.dist_b2b(p, is_periodic=periodic)
    dc2, de2, co2 = numpy_dist_b2b(p, periodic)
    assert np.array_equal(dc, dc2) and np.array_equal(de, de2) and np.array_equal(co, co2)
    assert np.array_equal(oracle.sf_b2b_all(p, de, co, dc, is_periodic=periodic),
                          reflib.sf_b2b_all(p, de, co, dc, is_periodic=periodic))
    wa, wb = oracle.dist_b2w(p), reflib.dist_b2w(p)
    assert np.array_equal(wa[0], wb[0]) and np.array_equal(wa[1], wb[1])
    act = rng.uniform(-1, 1, (2, n_a)).astype(np.float32)
    s1 = oracle.step(p, dp, act, g, a["neighbor_index"], l_cell, ra, is_boundary=not periodic, with_self=with_self)
    s2 = ref_step(reflib, p, dp, act, g, a["neighbor_index"], l_cell, ra, is_boundary=not periodic,
                  with_self=with_self)
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k


@pytest.mark.parametrize("g_max,occ_max,topo", [(10, 7, 3), (80, 20, 6), (5, 200, 1)])
def test_small_caps_exercise_subsampling(oracle, reflib, shapes, g_max, occ_max, topo):
    """The 200-cell occupied cap is never reached at the shipped cell sizes; shrink the caps so the
    round(i*step) sub-sampling (AssemblyEnv.cpp:218-228,238-256) is exercised on both lists."""
    rng = np.random.default_rng(g_max * 1000 + occ_max)
    for n_a in (8, 32):
        p, dp, g, l_cell = make_case(rng, shapes, n_a, 1)
        ra = r_avoid_for(n_a, shapes)
        a = oracle.get_observation(p, dp, g, l_cell, ra, topo=topo, g_max=g_max, occ_max=occ_max)
        b = reflib.get_observation(p, dp, g, l_cell, ra, topo=topo, g_max=g_max, occ_max=occ_max)
        assert (a["occupied_index"][:, -1] >= 0).any() or occ_max == 200
        for k in a:
            assert np.array_equal(a[k], b[k]), k


# ---- list caps: the rows test_gpu_caps_parity.py holds the HIP step to (helpers.CAPS_ROWS) ----
@pytest.mark.parametrize("with_self", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("periodic", [False, True], ids=["walls", "periodic"])
@pytest.mark.parametrize("n_a", [8, 30, 64])
@pytest.mark.parametrize("row", list(CAPS_ROWS))
def test_step_matches_reference_across_list_caps(oracle, reflib, shapes, row, n_a, periodic, with_self):
    """oracle.step == ref_step, exact on every key, at every row of list caps: an observation, then three chained steps from a
    state clustered on the shape.  The caps enter the reference's own _get_observation; the reward walks the capped and
    sub-sampled sensed list it returns, the prior the neighbour list cut to topo."""
    topo, g_max, occ_max = CAPS_ROWS[row]
    cap = dict(topo=topo, g_max=g_max, occ_max=occ_max)
    rng = np.random.default_rng([list(CAPS_ROWS).index(row), n_a, periodic, with_self])
    p, dp, g, l_cell = make_case(rng, shapes, n_a, 1)
    ra = r_avoid_for(n_a, shapes)
    a = oracle.get_observation(p, dp, g, l_cell, ra, is_periodic=periodic, with_self=with_self, **cap)
    b = reflib.get_observation(p, dp, g, l_cell, ra, is_periodic=periodic, with_self=with_self, **cap)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    nei = a["neighbor_index"]
    for t in range(3):
        act = rng.uniform(-1, 1, (2, n_a)).astype(np.float32)
        s1 = oracle.step(p, dp, act, g, nei, l_cell, ra, is_boundary=not periodic, with_self=with_self, **cap)
        s2 = ref_step(reflib, p, dp, act, g, nei, l_cell, ra, is_boundary=not periodic, with_self=with_self, **cap)
        for k in s1:
            assert np.array_equal(s1[k], s2[k]), (t, k)
        p, dp, nei = s1["p"], s1["dp"], s1["neighbor_index"]


# (row, dtype of the handle that feeds its prior back): the caps matrix runs float64, the dtype matrix float32 and bfloat16
CAPS_REACH = [(r, "f64") for r in CAPS_ROWS if r != "default"] + [(r, d) for r in CAPS_DTYPE_ROWS for d in ("f32", "bf16")]


@pytest.mark.parametrize("row,dtype", CAPS_REACH, ids=["%s-%s" % c for c in CAPS_REACH])
def test_caps_inputs_reach_the_caps(oracle, shapes, row, dtype):
    """The inputs test_gpu_caps_parity.py runs (helpers.caps_trajectory, the same calls), judged by the oracle alone and summed
    over the row's agent counts: rows with g_max <= 33 cap the sensed list of >= 100 agent-steps, t6_g33_o33 also leaves >= 100
    uncapped; rows with occ_max <= 64 cap >= 100 occupied lists; t4_g128_o11 caps no sensed list; every row sees both reward
    values and both full and short neighbour lists; t6_g79_o64 and t5_g81 (g_max - 1 even and no power of two) cap a list of a
    length at which the integer form of the cap and the reference's fp64 round() select different cells
    (helpers.cap_round_parts_ways).  No row needed an exemption.  bfloat16: some obs / a_prior value of the
    row differs between the contract's double -> float32 -> bfloat16 and a single rounding (helpers.as_obs_dtype)."""
    topo, g_max, occ_max = CAPS_ROWS[row]
    tot, twice = {}, 0
    for n_a in (CAPS_NS if dtype == "f64" else CAPS_DTYPE_NS):
        cases, ref, ra = caps_trajectory(oracle, shapes, row, n_a, dtype)
        for k, v in caps_reach(oracle, cases, row, ref, ra).items():
            tot[k] = tot.get(k, 0) + v
        if dtype == "bf16":
            for s in ref[0] + [s for step in ref[1] for s in step]:
                twice += sum(int((bf16_direct(s[k]) != as_obs_dtype(s[k], "bf16")).sum()) for k in ("obs", "a_prior") if k in s)
    print(row, dtype, tot, twice)
    if g_max <= 33:
        assert tot["sensed_over"] >= 100, tot
    if row == "t6_g33_o33":
        assert tot["sensed_under"] >= 100, tot
    if occ_max <= 64:
        assert tot["occ_over"] >= 100, tot
    if row == "t4_g128_o11":
        assert tot["sensed_over"] == 0, tot
    if row in ("t6_g79_o64", "t5_g81"):
        assert tot["tie_below"] >= 1, tot
    assert tot["rew1"] >= 1 and tot["rew0"] >= 1, tot
    assert tot["nei_full"] >= 1 and tot["nei_part"] >= 1, tot
    if dtype == "bf16":
        assert twice >= 1


# ---- away from the reference's constants: the configurations test_gpu_config_parity.py holds the HIP step to ----
SENSING = [(0.25, None), (0.6, None), (1.0, None), (0.25, 0.30), (0.4, 0.08)]        # (d_sen, r_avoid; None = r_avoid_for)
CONFIG_ROWS = [(name, phys, DEFAULT_BOX, 0.4, None) for name, phys in DYNAMICS_ROWS]
CONFIG_ROWS += [("off_box", {}, OFF_BOX, 0.4, None), ("off_box_all", DYNAMICS_ROWS[-1][1], OFF_BOX, 0.4, None),
                ("big_box", {}, BIG_BOX, 0.4, None)]
CONFIG_ROWS += [("sense_%g_%s" % (d, r), dict(size_a=0.05) if k in (1, 3) else {}, DEFAULT_BOX, d, r) for k, (d, r) in enumerate(SENSING)]


@pytest.mark.parametrize("n_a", [8, 64])
@pytest.mark.parametrize("periodic", [False, True], ids=["walls", "periodic"])
@pytest.mark.parametrize("name,phys,boundary,d_sen,r_avoid", CONFIG_ROWS, ids=[r[0] for r in CONFIG_ROWS])
def test_step_matches_reference_away_from_the_defaults(oracle, reflib, shapes, name, phys, boundary, d_sen, r_avoid, periodic, n_a):
    """oracle.step == ref_step, exact on every key, with size_a / k_ball / boundary entering the reference's own C++ calls,
    k_wall / c_wall / vel_max / dt the restated numpy glue, and d_sen / r_avoid both; three free-running steps from a state
    with wall contacts (or wraps), agent contacts and near-clipped velocities (helpers.config_case).
    prior_gain other than (2, 3, 2) cannot be pinned this way: the reference's C++ has no such parameter (the gains are
    literals, AssemblyEnv.cpp:1128-1132).  The default is pinned above, and the gains enter orc_action_prior_g as three
    multiplications in the reference's operation order."""
    rng = np.random.default_rng([n_a, periodic, len(name)] + [ord(c) for c in name])
    ph = physics(**phys)
    ra = r_avoid_for(n_a, shapes) if r_avoid is None else r_avoid
    b = np.array(boundary, np.float64)
    p, dp, g, l_cell = config_case(rng, shapes, n_a, boundary, ph["size_a"], ph["vel_max"], ph["dt"])
    nei = oracle.get_observation(p, dp, g, l_cell, ra, d_sen=d_sen, boundary=b, is_periodic=periodic)["neighbor_index"]
    clipped = 0
    for t in range(3):
        act = rng.uniform(-1, 1, (2, n_a)).astype(np.float32)
        s1 = oracle.step(p, dp, act, g, nei, l_cell, ra, d_sen=d_sen, boundary=b, is_boundary=not periodic, **ph)
        s2 = ref_step(reflib, p, dp, act, g, nei, l_cell, ra, d_sen=d_sen, boundary=b, is_boundary=not periodic, **ph)
        for k in s1:
            assert np.array_equal(s1[k], s2[k]), (t, k)
        clipped += int((np.abs(s1["dp"]) == ph["vel_max"]).sum())
        p, dp, nei = s1["p"], s1["dp"], s1["neighbor_index"]
    assert clipped > 0


@pytest.mark.parametrize("n_a", [8, 64])
@pytest.mark.parametrize("periodic", [False, True], ids=["walls", "periodic"])
def test_functions_match_reference_on_the_off_centre_box(oracle, reflib, shapes, periodic, n_a):
    """Every function on the non-square, off-centre box (w_half != h_half, neither edge pair symmetric about 0), with
    size_a = 0.05 and k_ball = 45: a swapped axis or a boundary entry taken from the wrong slot changes bits here."""
    rng = np.random.default_rng(31 * n_a + periodic)
    b = np.array(OFF_BOX, np.float64)
    size_a, k_ball, d_sen = 0.05, 45.0, 0.6
    ra = r_avoid_for(n_a, shapes)
    p, dp, g, l_cell = config_case(rng, shapes, n_a, OFF_BOX, size_a)
    a = oracle.get_observation(p, dp, g, l_cell, ra, d_sen=d_sen, boundary=b, is_periodic=periodic)
    r = reflib.get_observation(p, dp, g, l_cell, ra, d_sen=d_sen, boundary=b, is_periodic=periodic)
    for k in a:
        assert np.array_equal(a[k], r[k]), k
    if periodic:            # the edge agents are neighbours through the wrap only
        plain = oracle.get_observation(p, dp, g, l_cell, ra, d_sen=d_sen, boundary=b, is_periodic=False)
        assert 2 in a["neighbor_index"][0] and 2 not in plain["neighbor_index"][0]
        assert 3 in a["neighbor_index"][1] and 3 not in plain["neighbor_index"][1]
    assert np.array_equal(oracle.get_reward(p, g, a["neighbor_index"], a["in_flags"], a["sensed_index"], ra, d_sen=d_sen, boundary=b, is_periodic=periodic),
                          reflib.get_reward(p, g, a["neighbor_index"], a["in_flags"], a["sensed_index"], ra, d_sen=d_sen, boundary=b,
                                            is_periodic=periodic, occupied_index=a["occupied_index"]))
    dc, de, co = oracle.dist_b2b(p, b, periodic, size_a)
    dc2, de2, co2 = numpy_dist_b2b(p, periodic, (b[2] - b[0]) / 2, (b[1] - b[3]) / 2, size_a)
    assert np.array_equal(dc, dc2) and np.array_equal(de, de2) and np.array_equal(co, co2)
    assert co[4, 5] and co[0, 2] == periodic and not co[2, 0]       # numpy wraps agent 0's row only
    assert np.array_equal(oracle.sf_b2b_all(p, de, co, dc, b, periodic, k_ball), reflib.sf_b2b_all(p, de, co, dc, b, periodic, k_ball))
    wa, wb = oracle.dist_b2w(p, b, size_a), reflib.dist_b2w(p, b, size_a)
    assert np.array_equal(wa[0], wb[0]) and np.array_equal(wa[1], wb[1])
    assert wa[1][:, :4].diagonal().all()                             # agent w touches wall w


# ---- the hand-built inputs of the five legacy symbols (helpers.legacy_specs) ----
LEGACY = legacy_specs()


@pytest.mark.parametrize("spec", LEGACY, ids=[s[0] for s in LEGACY])
def test_legacy_cases_are_defined_in_the_reference_and_the_oracle_agrees(oracle, reflib, spec):
    """Each case reaches what it was built for, by the reference's outputs and by the oracle's alike, and the two libraries
    return the same bits in every output buffer, none of which keeps the junk it was handed with."""
    case = legacy_case(spec)
    assert legacy_reach(case, reflib) == legacy_reach(case, oracle)
    a, b = legacy_call(reflib, case), legacy_call(oracle, case)
    assert_same(a, b, spec[0])
    assert_same(a, legacy_call(reflib, case), spec[0])                 # the same call twice: nothing undefined was read
    for k, v in a.items():
        assert v.dtype == bool or not (v == (7.0 if v.dtype.kind == "f" else -7)).any(), k


def test_legacy_cache_configurations_differ_in_the_reference(oracle, reflib):
    res = {k: legacy_call(reflib, c) for k, c in legacy_cache_configs().items()}
    for k, c in legacy_cache_configs().items():
        assert_same(res[k], legacy_call(oracle, c), k)
    for k in "BCD":
        assert res[k]["obs"].shape != res["A"]["obs"].shape or not np.array_equal(res[k]["obs"], res["A"]["obs"]), k
