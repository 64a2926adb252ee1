"""save_eval_results and the switch= normaliser of rollout_eval (marl_llm_amd/rollout.py) on hand-made CPU traces: the files
eval_assembly.py:168-174,195-205 writes (metrics.pkl, state_data.npz) for one env of the batch, and metrics_batch.npz."""
import os
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def make_trace(T=7, E=4, N=5, state=True, as_torch=False, seed=0):
    from marl_llm_amd.rollout import EvalTrace
    rs = np.random.RandomState(seed)
    m = rs.random_sample((T, E, 3))
    p, dp = (rs.standard_normal((T, E, 2, N)), rs.standard_normal((T, E, 2, N))) if state else (None, None)
    shape = np.array([-1, -1, 4, 4, 4, 5, 5][:T])
    if as_torch:
        m, p, dp = torch.from_numpy(m), torch.from_numpy(p), torch.from_numpy(dp)
    return EvalTrace(m, p, dp, None, shape)


@pytest.mark.parametrize("as_torch", [False, True])
def test_metrics_pkl_is_the_reference_list_of_dicts(tmp_path, as_torch):
    from marl_llm_amd.rollout import save_eval_results
    tr = make_trace(as_torch=as_torch)
    paths = save_eval_results(tr, str(tmp_path), env=2)
    assert [os.path.basename(p) for p in paths] == ["metrics.pkl", "state_data.npz", "metrics_batch.npz"]
    rows = pickle.load(open(paths[0], "rb"))
    m = np.asarray(tr.metrics)
    assert isinstance(rows, list) and len(rows) == 7
    for t, d in enumerate(rows):
        assert list(d) == ["coverage_rate", "uniformity_degree", "voronoi_uniformity", "et_index", "shape_count"]
        assert (d["coverage_rate"], d["uniformity_degree"], d["voronoi_uniformity"]) == tuple(m[t, 2])
        assert d["et_index"] == t and type(d["et_index"]) is int
        assert d["shape_count"] == int(tr.shape[t]) + 1          # logged after the reference's increment
    assert [d["shape_count"] for d in rows] == [0, 0, 5, 5, 5, 6, 6]


def test_state_data_has_the_reference_keys_and_shapes(tmp_path):
    from marl_llm_amd.rollout import save_eval_results
    tr = make_trace(T=6, E=3, N=5)
    save_eval_results(tr, str(tmp_path), env=1)
    z = np.load(os.path.join(str(tmp_path), "state_data.npz"))
    assert sorted(z.files) == ["pos", "t_step", "vel"]
    assert z["pos"].shape == (2, 5, 6) and z["vel"].shape == (2, 5, 6) and int(z["t_step"]) == 5
    for t in range(6):                                             # p_store[:, :, et_index] = env.p
        assert np.array_equal(z["pos"][:, :, t], tr.p[t, 1]) and np.array_equal(z["vel"][:, :, t], tr.dp[t, 1])


def test_a_trace_without_state_raises_before_writing(tmp_path):
    from marl_llm_amd.rollout import save_eval_results
    with pytest.raises(ValueError, match="trace_state=True"):
        save_eval_results(make_trace(state=False), str(tmp_path / "out"))
    assert not os.path.exists(str(tmp_path / "out"))
    with pytest.raises(ValueError, match="env"):
        save_eval_results(make_trace(E=4), str(tmp_path / "out"), env=4)


def test_metrics_batch_is_nan_aware(tmp_path):
    from marl_llm_amd.rollout import save_eval_results
    tr = make_trace(T=5, E=4)
    tr.metrics[1, 2, 1] = np.nan                                   # one env's 0/0 uniformity
    tr.metrics[3, :, 1] = np.nan                                   # every env's
    tr.shape = tr.shape[:5]
    save_eval_results(tr, str(tmp_path))
    z = np.load(os.path.join(str(tmp_path), "metrics_batch.npz"))
    m = tr.metrics
    assert np.array_equal(z["metrics"], m, equal_nan=True) and z["mean"].shape == (5, 3) and z["std"].shape == (5, 3)
    keep = [0, 1, 3]
    assert z["mean"][1, 1] == np.mean(m[1, keep, 1]) and z["std"][1, 1] == np.std(m[1, keep, 1])
    assert np.isnan(z["mean"][3, 1]) and np.isnan(z["std"][3, 1])
    assert np.array_equal(z["mean"][:, 0], m[:, :, 0].mean(axis=1)) and np.array_equal(z["std"][:, 2], m[:, :, 2].std(axis=1))
    assert z["nan_count"][1, 1] == 1 and z["nan_count"][3, 1] == 4 and z["nan_count"].sum() == 5
    rows = pickle.load(open(os.path.join(str(tmp_path), "metrics.pkl"), "rb"))
    assert np.isnan(rows[3]["uniformity_degree"])


def test_switch_normaliser():
    from marl_llm_amd.rollout import _switch_schedule
    a = _switch_schedule({0: 4, 5: 2}, 8)
    b = _switch_schedule([4, -1, -1, None, -1, 2, -1, -1], 8)
    assert a.dtype == np.int32 and a.tolist() == [4, -1, -1, -1, -1, 2, -1, -1] and np.array_equal(a, b)
    assert _switch_schedule(None, 8) is None and _switch_schedule({}, 8) is None and _switch_schedule([-1] * 3, 3) is None
    for bad in ({8: 1}, {-1: 1}, {2.5: 1}, {0: -1}, {0: 1.5}, [1, 2], [0] * 9, [-2] * 8):
        with pytest.raises(ValueError, match="switch"):
            _switch_schedule(bad, 8)
