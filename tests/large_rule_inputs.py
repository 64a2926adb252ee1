"""Inputs of the rule-expert tests above 256 agents (test_gpu_large_rule.py on the device, test_large_rule_host.py on the CPU):
calm envs built with helpers.calm_case as helpers.calm_batch builds them, but only as many envs as the quadratic numpy
restatement (oracle_py.rule_action, Python loops) computes in a few seconds.  Measured on helpers.rule_details' process pool:
0.6 s for five envs of 257 or 300 agents, 1.1 s for five of 513, 3 s for four of 1024 (about 0.3 / 0.6 / 1 s an env alone).

Env 0 is packed on its shape (neighbours inside r_avoid, the occupied-cell filter).  The others keep 90 agents on the shape
and put the rest away from it (v_ent): with more agents on it nearly every sensed cell is occupied and no filtered list
is longer than g_max = 80.  They use the shapes with at least 110 cells within d_sen of the centroid; each such env then
sends 25 to 46 agents through the round(i * step) subsample.

Conditions on the inputs, asserted from the restatement's detail output alone (helpers.rule_branch_counts), never from kernel
output, the contract module's own: the share of unsaturated components is at least 1/3, and at least 100 agents with an
unsaturated component sit in each of the columns near / avoid / outside / sensed / subsampled.  Counts of these inputs:
    N     envs  share  near  avoid  outside  sensed  subsampled
    257    5    0.80   1224   614     682     571      150
    300    5    0.82   1430   622     844     606      145
    513    5    0.77   2424   955    1691     751      147
    1024   4    0.71   3672  1666    2824     874      114"""
import numpy as np

from helpers import calm_case, rule_branch_counts, rule_details

ENVS = {257: 5, 300: 5, 513: 5, 1024: 4}
ON_SHAPE = 90                                  # agents the envs after the first keep on the shape
COLUMNS = ("near", "avoid", "outside", "sensed", "subsampled")
D_SEN = 0.4
_CACHE = {}


def dense_shapes(shapes, d_sen=D_SEN):
    """The shapes with at least 110 cells within d_sen of their centroid: an agent in their middle senses more than g_max."""
    grids = [np.asarray(g, np.float64) for g in shapes["grid_coords"]]
    return [s for s, g in enumerate(grids) if (np.linalg.norm(g - g.mean(axis=0), axis=1) < d_sen).sum() >= 110]


def large_calm_cases(shapes, n_a, seed=0):
    """ENVS[n_a] calm envs as described above.  Returns (cases, r_avoid)."""
    from marl_llm_amd.shapes import r_avoid_for
    r_avoid = r_avoid_for(n_a, shapes)
    rng = np.random.default_rng([seed, n_a, 19])
    dense = dense_shapes(shapes)
    return [calm_case(rng, shapes, n_a, r_avoid) if e == 0 else
            calm_case(rng, shapes, n_a, r_avoid, shape=dense[e % len(dense)], away=1 - ON_SHAPE / n_a, off_shape=0.05, spacing=2.0)
            for e in range(ENVS[n_a])], r_avoid


def assert_large_conditions(n_a, info):
    c = rule_branch_counts(info)
    assert np.isfinite(info["raw"]).all()
    assert c["share"] >= 1 / 3, (n_a, c)
    for k in COLUMNS:
        assert c[k] >= 100, (n_a, k, c)
    return c


def large_calm_reference(shapes, n_a):
    """(cases, r_avoid, want [E, 2, N], info) of large_calm_cases, the conditions asserted; computed once per session and
    never modified."""
    if n_a not in _CACHE:
        cases, r_avoid = large_calm_cases(shapes, n_a)
        want, info = rule_details(cases, r_avoid)
        print(n_a, len(cases), assert_large_conditions(n_a, info))
        _CACHE[n_a] = (cases, r_avoid, want, info)
    return _CACHE[n_a]
