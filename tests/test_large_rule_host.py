"""CPU side of test_gpu_large_rule.py: the calm inputs above 256 agents (large_rule_inputs.py) meet the conditions that
module puts on them, from the float64 restatement alone, and no two agents of an env coincide (coincident agents give
r_avoid / 0 * 0 = NaN, which the comparison of finite actions must not meet)."""
import numpy as np
import pytest

from large_rule_inputs import ENVS, large_calm_reference


@pytest.mark.parametrize("n_a", sorted(ENVS))
def test_large_calm_states_meet_the_conditions(shapes, n_a):
    cases, r_avoid, want, info = large_calm_reference(shapes, n_a)        # (asserts share and the five columns)
    assert len(cases) == ENVS[n_a] and want.shape == (len(cases), 2, n_a) and np.isfinite(want).all()
    for p, dp, g, l_cell in cases:
        assert p.shape == (2, n_a)
        d = np.linalg.norm(p[:, :, None] - p[:, None, :], axis=0)
        assert d[~np.eye(n_a, dtype=bool)].min() > 0
