"""CPU side of test_gpu_rule_contract.py: the restatement's detail output leaves its action untouched, and the calm-state
generator meets the conditions the GPU module puts on its inputs, using the restatement alone."""
import os

import numpy as np
import pytest

from helpers import GOLDEN_DIR, RULE_NS, assert_calm_conditions, calm_batch, load_golden, rule_details


@pytest.mark.parametrize("n_a", [8, 32])
def test_detail_output_leaves_the_action_bit_identical(n_a):
    """rule_action(detail=True) on the recorded g5 states: the same bits as rule_action(), which is within 1e-12 of the
    recorded reference action, and the detail is consistent with it."""
    from oracle.oracle_py import RULE_DETAIL_KEYS, rule_action
    z = load_golden(os.path.join(GOLDEN_DIR, f"g5_rule_n{n_a}.npz"))
    for t in range(z["p"].shape[0]):
        plain = rule_action(z["p"][t], z["dp"][t], z["grid"], float(z["l_cell"]), float(z["r_avoid"]))
        a, info = rule_action(z["p"][t], z["dp"][t], z["grid"], float(z["l_cell"]), float(z["r_avoid"]), detail=True)
        assert plain.tobytes() == a.tobytes()
        assert np.abs(plain - z["u"][t]).max() <= 1e-12
        assert tuple(info) == RULE_DETAIL_KEYS
        assert np.array_equal(np.clip(info["raw"], -1, 1), a)
        assert (info["n_filtered"] <= info["n_sensed"]).all() and (info["n_avoid"] <= info["n_near"]).all()
        assert (info["n_filtered"][info["in_flag"] == 0] == info["n_sensed"][info["in_flag"] == 0]).all()
        assert np.array_equal(info["subsampled"] != 0, info["n_filtered"] > 80)
        assert info["n_near"].max() <= n_a - 1


@pytest.mark.parametrize("n_a", RULE_NS)
def test_calm_states_meet_the_contract_conditions(shapes, n_a):
    from marl_llm_amd.shapes import r_avoid_for
    r_avoid = r_avoid_for(n_a, shapes)
    cases = calm_batch(shapes, n_a, r_avoid)
    a, info = rule_details(cases, r_avoid)
    assert np.isfinite(info["raw"]).all()
    c = assert_calm_conditions(n_a, info)
    print(n_a, len(cases), c)
