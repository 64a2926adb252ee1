"""CPU-side checks of the per-env shape switch's public surface (swarm_select_shapes, SwarmBatch.select_shapes, the per-env
entries of rollout_eval's switch=, save_eval_by_shape): the symbol is declared, bound and exported at ABI version 5, argument
errors raise before the library is called, the schedule parser sorts int and per-env entries, and the by-shape statistics
are what numpy gives for each group of envs."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "swarm_env.h")


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def test_select_shapes_is_declared_bound_and_exported(lib):
    from marl_llm_amd import _lib
    from marl_llm_amd.batched import SwarmBatch
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+swarm_select_shapes\s*\(\s*swarm_env_t\s*\*\s*h\s*,\s*const\s+int32_t\s*\*\s*shape_index\s*,"
                     r"\s*const\s+double\s*\*\s*pose\s*,\s*void\s*\*\s*obs\s*\)", src)
    assert "swarm_select_shapes" in _lib.BATCHED_SYMBOLS and hasattr(lib, "swarm_select_shapes")
    assert len(lib.swarm_select_shapes.argtypes) == 4
    assert callable(getattr(SwarmBatch, "select_shapes", None))
    # a NULL handle is refused before anything else is looked at
    idx = (ctypes.c_int32 * 4)(0, 0, 0, 0)
    assert lib.swarm_select_shapes(None, ctypes.cast(idx, ctypes.c_void_p), None, None) == 1     # SWARM_ERR_INVALID
    assert lib.swarm_select_shapes(None, None, None, None) == 1


def test_abi_version_is_still_5(lib):
    from marl_llm_amd import _lib
    assert _lib.ABI_VERSION == 5 and lib.swarm_abi_version() == 5
    assert re.search(r"#define\s+SWARM_ABI_VERSION\s+5\b", open(HEADER).read())


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def _hostless_batch(E=4, S=3):
    """A SwarmBatch that was never created on a device: enough of it for the argument checks, and a library that fails the
    test when touched."""
    torch = pytest.importorskip("torch")
    from marl_llm_amd.batched import SwarmBatch
    sb = object.__new__(SwarmBatch)
    sb.handle, sb.lib = None, _NoLibrary()
    sb.n_env, sb.n_shapes, sb.device = E, S, torch.device("cuda", 0)
    sb.shape_in_force, sb.shape_env_in_force, sb._posed_env = -1, None, None
    return sb


@pytest.mark.parametrize("kw", [
    dict(index=[0, 1, 2, 0], pose=np.zeros((4, 4)), angle=np.zeros(4)),           # both forms
    dict(index=[0, 1, 2, 0], pose=np.zeros((4, 4)), offset=np.zeros((4, 2))),
    dict(index=[0, 1, 2], angle=None),                                            # wrong shapes
    dict(index=[[0, 1, 2, 0]]),
    dict(index=[0.0, 1.0, 2.0, 0.0]),                                             # not integers
    dict(index=[0, 1, 2, 0], pose=np.zeros((4, 3))),
    dict(index=[0, 1, 2, 0], angle=np.zeros(3)),
    dict(index=[0, 1, 2, 0], offset=np.zeros((4, 3))),
    dict(index=[0, 1, 3, 0]),                                                     # host index out of range: n_shapes
    dict(index=[0, -2, 1, 0]),                                                    # below the documented keep
    dict(index=[0, 2 ** 31 - 1, 1, 0]),
])
def test_argument_errors_raise_before_the_library_is_called(kw):
    sb = _hostless_batch()
    with pytest.raises(ValueError):
        sb.select_shapes(**kw)
    assert sb.shape_env_in_force is None and sb.shape_in_force == -1


def test_checked_arguments_are_the_documented_arrays():
    sb = _hostless_batch()
    ang, off = np.array([0.0, 0.5, -3.0, 1.25]), np.arange(8.0).reshape(4, 2)
    idx, pose = sb._shapes_args([2, -1, 0, 1], angle=ang, offset=off)
    assert idx.dtype == np.int32 and idx.tolist() == [2, -1, 0, 1]
    assert pose.dtype == np.float64 and pose.flags.c_contiguous and pose.shape == (4, 4)
    assert np.array_equal(pose, np.column_stack([np.cos(ang), np.sin(ang), off]))
    idx, pose = sb._shapes_args(np.array([0, 0, 0, 0]), offset=off)
    assert np.array_equal(pose, np.column_stack([np.ones(4), np.zeros(4), off]))          # angle 0: cos 1, sin 0
    assert sb._shapes_args([1, 1, 1, 1])[1] is None
    given = np.arange(16.0).reshape(4, 4)
    assert np.array_equal(sb._shapes_args([1, 1, 1, 1], pose=given)[1], given)


def test_bookkeeping_of_host_indices():
    sb = _hostless_batch()
    sb._note_shapes(np.array([2, -1, 0, 1], np.int32), False)
    assert sb.shape_env_in_force.dtype == np.int64 and sb.shape_env_in_force.tolist() == [2, -1, 0, 1] and sb.shape_in_force == -1
    sb._note_shapes(np.array([1, 1, 1, -1], np.int32), False)
    assert sb.shape_env_in_force.tolist() == [1, 1, 1, 1] and sb.shape_in_force == 1      # all known, one shape, no pose
    sb._note_shapes(np.array([-1, 1, -1, -1], np.int32), True)
    assert sb.shape_env_in_force.tolist() == [1, 1, 1, 1] and sb.shape_in_force == -1     # one env holds it at a pose
    sb._note_shapes(np.array([-1, 1, -1, -1], np.int32), False)
    assert sb.shape_in_force == 1
    sb._note_shapes(None, True)                                                           # a device index
    assert sb.shape_env_in_force is None and sb.shape_in_force == -1
    sb._note_shapes(np.array([-1, -1, -1, -1], np.int32), False)
    assert sb.shape_env_in_force is None


def test_switch_schedule_parses_per_env_entries():
    torch = pytest.importorskip("torch")
    from marl_llm_amd.rollout import _switch_schedule
    per = {}
    a = _switch_schedule({0: [0, 1, 2], 2: 4, 3: dict(index=[1, -1, -1], angle=[0.5, 0, 0])}, 6, per)
    assert a.dtype == np.int32 and a.tolist() == [-1, -1, 4, -1, -1, -1]
    assert sorted(per) == [0, 3] and per[0] == {"index": [0, 1, 2]} and sorted(per[3]) == ["angle", "index"]
    per = {}
    b = _switch_schedule([np.array([0, 1]), None, -1, torch.tensor([1, 0]), 3, np.int64(2)], 6, per)
    assert b.tolist() == [-1, -1, -1, -1, 3, 2] and sorted(per) == [0, 3]
    per = {}
    assert _switch_schedule({1: [0, 1]}, 4, per) is None and sorted(per) == [1]            # no batch-wide entry at all
    # ints only: what it always returned, with or without the dict
    assert np.array_equal(_switch_schedule({0: 4, 5: 2}, 8, {}), _switch_schedule({0: 4, 5: 2}, 8))
    for bad in ({0: dict(angle=[0, 0])}, {0: dict(index=[0, 1], scale=2)}, {9: [0, 1]}, [[0, 1]] * 3):
        with pytest.raises(ValueError, match="switch"):
            _switch_schedule(bad, 6, {})
    with pytest.raises(ValueError, match="switch"):
        _switch_schedule({0: [0, 1]}, 6)                                                   # nobody takes per-env entries


def test_eval_device_all_shapes_pieces():
    import importlib.util
    pytest.importorskip("torch")
    from marl_llm_amd.rollout import _switch_schedule
    spec = importlib.util.spec_from_file_location("eval_device", os.path.join(ROOT, "tools", "eval_device.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    sw = tool.all_shapes_switch(10, 7)
    assert list(sw) == [0] and sw[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 0, 1, 2]
    per = {}
    assert _switch_schedule(sw, 5, per) is None and list(per) == [0]
    table = tool.by_shape_table(np.array([[0.5, 0.25, 0.125], [np.nan] * 3]), np.array([3, 0])).splitlines()
    assert len(table) == 3 and table[1].split("|")[1].strip() == "3" and "0.5000" in table[1] and "nan" in table[2]


def test_save_eval_by_shape(tmp_path):
    from marl_llm_amd.rollout import EvalTrace, save_eval_by_shape, save_eval_results
    rng = np.random.default_rng(3)
    T, E, S = 4, 6, 4
    m = rng.uniform(0, 1, (T, E, 3))
    m[1, 2, 1] = np.nan                                    # one env of shape 1's group
    m[2, [0, 3], 1] = np.nan                               # the whole group of shape 0 at step 2
    shape_env = np.array([[0, 1, 1, 0, 2, -1]] * 2 + [[0, 1, 1, 0, 1, 1]] * 2)            # shape 3: nobody, ever
    tr = EvalTrace(m, shape=np.full(T, -1), shape_env=shape_env)
    path = save_eval_by_shape(tr, str(tmp_path), S)
    assert os.path.basename(path) == "metrics_by_shape.npz"
    z = np.load(path)
    assert z["mean"].shape == z["std"].shape == (T, S, 3) and z["count"].shape == (T, S)
    assert z["count"].tolist() == [[2, 2, 1, 0]] * 2 + [[2, 4, 0, 0]] * 2
    assert np.isnan(z["mean"][:, 3]).all() and np.isnan(z["std"][:, 3]).all()              # a shape nobody holds
    assert np.isnan(z["mean"][2:, 2]).all()
    assert np.array_equal(z["mean"][0, 0], m[0, [0, 3]].mean(axis=0)) and np.array_equal(z["std"][0, 0], m[0, [0, 3]].std(axis=0))
    assert z["mean"][1, 1, 1] == m[1, 1, 1] and z["std"][1, 1, 1] == 0.0                   # the NaN env is left out
    assert z["mean"][1, 1, 0] == np.mean(m[1, [1, 2], 0])
    assert np.isnan(z["mean"][2, 0, 1]) and np.isnan(z["std"][2, 0, 1])                    # all NaN stays NaN
    assert z["mean"][2, 0, 0] == np.mean(m[2, [0, 3], 0])
    assert np.array_equal(z["mean"][3, 1], m[3, [1, 2, 4, 5]].mean(axis=0))
    with pytest.raises(ValueError, match="shape_env"):
        save_eval_by_shape(EvalTrace(m), str(tmp_path), S)
    # save_eval_results: shape_count of env e is that env's own shape + 1
    import pickle
    tr.p = tr.dp = np.zeros((T, E, 2, 5))
    for e, want in ((4, [3, 3, 2, 2]), (5, [0, 0, 2, 2])):
        save_eval_results(tr, str(tmp_path), env=e)
        rows = pickle.load(open(os.path.join(str(tmp_path), "metrics.pkl"), "rb"))
        assert [r["shape_count"] for r in rows] == want
