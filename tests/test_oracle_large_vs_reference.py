"""The oracle above 256 agents.  (a) It equals the reference's compiled C++ at N = 300, 512 and 1024 -- an observation and two
chained steps on a scattered and a clustered case (skipped where oracle/_ref is absent, as test_oracle_vs_reference.py).
(b) From the oracle alone: what the inputs of tests/test_gpu_large_swarm.py's lockstep cases reach.  Over the scatter and the
cluster case of every N, three random-action steps, each counter must be positive: rewards of 1, agents in shape, sensed
lists at the cap, non-empty occupied lists, full neighbour lists, agent-agent contacts."""
import numpy as np
import pytest

from helpers import make_case
from marl_llm_amd.shapes import r_avoid_for
from oracle.oracle_py import G_MAX, ref_step


def _case(shapes, n_a, cluster):
    return make_case(np.random.default_rng([7, n_a, cluster]), shapes, n_a, cluster)


@pytest.mark.parametrize("cluster", [0, 1], ids=["scatter", "cluster"])
@pytest.mark.parametrize("n_a", [300, 512, 1024])
def test_oracle_equals_the_reference_above_256(oracle, reflib, shapes, n_a, cluster):
    p, dp, g, l_cell = _case(shapes, n_a, cluster)
    ra = r_avoid_for(n_a, shapes)
    a = oracle.get_observation(p, dp, g, l_cell, ra)
    b = reflib.get_observation(p, dp, g, l_cell, ra)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    rng = np.random.default_rng([8, n_a, cluster])
    nei = a["neighbor_index"]
    for t in range(2):
        act = rng.uniform(-1, 1, (2, n_a)).astype(np.float32)
        s1 = oracle.step(p, dp, act, g, nei, l_cell, ra)
        s2 = ref_step(reflib, p, dp, act, g, nei, l_cell, ra)
        for k in s1:
            assert np.array_equal(s1[k], s2[k]), (t, k)
        p, dp, nei = s1["p"], s1["dp"], s1["neighbor_index"]


@pytest.mark.parametrize("n_a", [257, 300, 512, 1024])
def test_large_inputs_reach_every_branch(oracle, shapes, n_a):
    ra = r_avoid_for(n_a, shapes)
    total = dict(reward1=0, in_shape=0, capped=0, occupied=0, full_nei=0, contacts=0)
    for cluster in (0, 1):
        p, dp, g, l_cell = _case(shapes, n_a, cluster)
        rng = np.random.default_rng([9, n_a, cluster])
        nei = oracle.get_observation(p, dp, g, l_cell, ra)["neighbor_index"]
        for t in range(3):
            total["contacts"] += int(oracle.dist_b2b(p)[2].sum()) // 2
            act = rng.uniform(-1, 1, (2, n_a)).astype(np.float32)
            s = oracle.step(p, dp, act, g, nei, l_cell, ra)
            total["reward1"] += int((s["reward"] == 1).sum())
            total["in_shape"] += int((s["in_flags"] == 1).sum())
            total["capped"] += int((s["sensed_index"][:, G_MAX - 1] >= 0).sum())
            total["occupied"] += int((s["occupied_index"][:, 0] >= 0).sum())
            total["full_nei"] += int((s["neighbor_index"] >= 0).all(axis=1).sum())
            p, dp, nei = s["p"], s["dp"], s["neighbor_index"]
    assert all(v > 0 for v in total.values()), total
