"""CPU-side checks of the actor bank (include/swarm_policy.h "Actor bank"): swarm_policy_bank_create validates everything before it
looks for a device, so every refusal below is decided here, without a GPU, with SWARM_POLICY_ERR_INVALID, a null handle and a
message that starts "swarm_policy_bank_create:"; a table that passes fails here with "no HIP device" (with a device the same
call succeeds: tests/test_gpu_policy_bank.py).  Also FusedPolicyBank's shape check (before any library call),
save_eval_by_member against a numpy restatement, and the argument checks tools/eval_device.py gained."""
import argparse
import ctypes
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_HIP = 1, 2      # SWARM_POLICY_ERR_INVALID, SWARM_POLICY_ERR_HIP
PREFIX = b"swarm_policy_bank_create:"


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def _has_device():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _bank_create(lib, members, in_dim, hidden, act_dim, wide, null=None, table_members=None, out=True):
    """swarm_policy_bank_create on zero fp32 host weights (entry `null` of the table NULL)."""
    shapes = [(hidden, in_dim), (hidden,), (hidden, hidden), (hidden,), (hidden, hidden), (hidden,), (act_dim, hidden), (act_dim,)]
    n = max(1, members) if table_members is None else table_members
    ws = [np.zeros(max(1, int(np.prod(s))), np.float32) for _ in range(n) for s in shapes]
    table = (ctypes.c_void_p * len(ws))(*[None if i == null else w.ctypes.data for i, w in enumerate(ws)])
    h = ctypes.c_void_p()
    rc = lib.swarm_policy_bank_create(table, members, in_dim, hidden, act_dim, wide, -1, ctypes.byref(h) if out else None)
    return rc, h, lib.swarm_policy_last_error()


@pytest.mark.parametrize("members", [0, 257, -1])
def test_member_counts_outside_1_to_256_are_rejected(lib, members):
    rc, h, msg = _bank_create(lib, members, 192, 180, 2, 0, table_members=1)
    assert rc == ERR_INVALID and not h.value and msg.startswith(PREFIX)
    assert str(members).encode() in msg and b"256" in msg


@pytest.mark.parametrize("null", [0, 7, 8, 13, 23])
def test_a_null_entry_of_the_table_is_rejected(lib, null):
    rc, h, msg = _bank_create(lib, 3, 192, 180, 2, 0, null=null)
    assert rc == ERR_INVALID and not h.value and msg.startswith(PREFIX + b" null weight pointer")
    assert ("member %d, array %d" % (null // 8, null % 8)).encode() in msg


def test_a_null_table_and_a_bad_geometry_flag_are_rejected(lib):
    h = ctypes.c_void_p()
    assert lib.swarm_policy_bank_create(None, 2, 192, 180, 2, 0, -1, ctypes.byref(h)) == ERR_INVALID and not h.value
    assert lib.swarm_policy_last_error().startswith(PREFIX + b" null weight table")
    rc, h, msg = _bank_create(lib, 2, 192, 180, 2, 2)
    assert rc == ERR_INVALID and not h.value and msg.startswith(PREFIX) and b"wide must be 0" in msg


@pytest.mark.parametrize("in_dim,hidden,act_dim", [
    (196, 180, 2), (190, 180, 2), (2, 180, 2), (0, 180, 2),       # in_dim: 4..192, multiple of 4
    (192, 192, 2), (192, 0, 2),                                   # hidden: 1..191
    (192, 180, 0), (192, 180, 5),                                 # act_dim: 1..4
])
def test_narrow_shape_limits(lib, in_dim, hidden, act_dim):
    rc, h, msg = _bank_create(lib, 2, in_dim, hidden, act_dim, 0)
    assert rc == ERR_INVALID and not h.value and msg.startswith(PREFIX)
    assert b"narrow" in msg and b"in_dim <= 192" in msg and b"hidden <= 191" in msg and b"act_dim <= 4" in msg


@pytest.mark.parametrize("in_dim,hidden,act_dim", [
    (388, 180, 2), (386, 180, 2), (2, 180, 2), (0, 180, 2),       # in_dim: 4..384, multiple of 4
    (192, 257, 2), (192, 0, 2),                                   # hidden: 1..256
    (192, 180, 0), (192, 180, 5),                                 # act_dim: 1..4
])
def test_wide_shape_limits(lib, in_dim, hidden, act_dim):
    rc, h, msg = _bank_create(lib, 2, in_dim, hidden, act_dim, 1)
    assert rc == ERR_INVALID and not h.value and msg.startswith(PREFIX)
    assert b"wide" in msg and b"in_dim <= 384" in msg and b"hidden <= 256" in msg and b"act_dim <= 4" in msg


def test_null_out_is_rejected(lib):
    rc, _, msg = _bank_create(lib, 2, 192, 180, 2, 0, out=False)
    assert rc == ERR_INVALID and msg.startswith(PREFIX) and b"null out" in msg


@pytest.mark.parametrize("members,shape,wide", [(1, (192, 180, 2), 0), (256, (8, 16, 1), 0), (3, (384, 256, 4), 1), (2, (192, 180, 2), 1)])
def test_a_valid_table_gets_as_far_as_the_device(lib, members, shape, wide):
    """Both ends of the member range and both geometries: without a device the call fails with "no HIP device"."""
    rc, h, msg = _bank_create(lib, members, *shape, wide)
    if _has_device():
        assert rc == 0 and h.value and lib.swarm_policy_bank_members(h) == members
        lib.swarm_policy_destroy(h)
    else:
        assert rc == ERR_HIP and not h.value and msg.startswith(PREFIX) and b"no HIP device" in msg


def test_members_of_a_null_handle(lib):
    assert lib.swarm_policy_bank_members(None) == 0


def test_header_and_symbol_list():
    src = open(os.path.join(ROOT, "include", "swarm_policy.h")).read()
    from marl_llm_amd._lib import POLICY_SYMBOLS
    for n in ("swarm_policy_bank_create", "swarm_policy_bank_members", "swarm_policy_bank_load_device", "swarm_policy_bank_read_packed"):
        assert n + "(" in src and n in POLICY_SYMBOLS
    assert "e / (E / M)" in open(os.path.join(ROOT, "include", "swarm_rollout.h")).read()


# ------------------------------------------------------------------------------------------------------ FusedPolicyBank
def test_bank_of_differing_shapes_is_a_value_error_before_any_library_call(monkeypatch):
    torch = pytest.importorskip("torch")
    from marl_llm_amd import _lib
    from marl_llm_amd.rollout import FusedPolicyBank, PolicyMLP

    def no_library():
        raise AssertionError("the library was loaded before the shape check")
    monkeypatch.setattr(_lib, "load", no_library)
    a = PolicyMLP(192, 2, 180)
    for other in (PolicyMLP(192, 2, 100), PolicyMLP(64, 2, 180), PolicyMLP(192, 3, 180)):
        with pytest.raises(ValueError, match="module 1"):
            FusedPolicyBank([a, other])
    with pytest.raises(ValueError, match="at least one"):
        FusedPolicyBank([])
    from marl_llm_amd.rollout import FusedPolicy
    assert issubclass(FusedPolicyBank, FusedPolicy)


# --------------------------------------------------------------------------------------------------- save_eval_by_member
def test_save_eval_by_member_against_a_numpy_restatement(tmp_path):
    pytest.importorskip("torch")
    from marl_llm_amd.rollout import EvalTrace, save_eval_by_member
    rng = np.random.default_rng(5)
    T, E, M = 7, 12, 3
    m = rng.random((T, E, 3))
    m[0, :, 1] = np.nan                    # a metric that is NaN for every env at a step
    m[2, 4:8, 0] = np.nan                  # all of member 1's envs at a step, one metric
    m[3, 5, :] = np.nan                    # one env of a member
    m[5, 0, 2] = np.nan
    members = np.arange(E) // (E // M)
    path = save_eval_by_member(EvalTrace(m), members, str(tmp_path))
    assert os.path.basename(path) == "metrics_by_member.npz"
    with np.load(path) as z:
        mean, std, count = z["mean"], z["std"], z["count"]
    assert mean.shape == std.shape == (T, M, 3) and count.shape == (T, M) and (count == E // M).all()
    for t in range(T):
        for g in range(M):
            for j in range(3):
                v = m[t, members == g, j]
                v = v[~np.isnan(v)]
                if v.size == 0:
                    assert np.isnan(mean[t, g, j]) and np.isnan(std[t, g, j])
                else:
                    assert mean[t, g, j] == pytest.approx(v.sum() / v.size, rel=1e-14)
                    assert std[t, g, j] == pytest.approx(np.sqrt(((v - v.sum() / v.size) ** 2).sum() / v.size), rel=1e-12, abs=1e-15)
    # an env in no group, and a member nobody holds
    members2 = np.array([0, 0, 2, 2, -1, -1, 0, 2, 2, 0, 0, -1])
    with np.load(save_eval_by_member(EvalTrace(m), members2, str(tmp_path / "b"))) as z:
        assert (z["count"] == np.array([5, 0, 4])).all() and np.isnan(z["mean"][:, 1]).all()
        assert z["mean"][6, 2, 0] == pytest.approx(m[6, members2 == 2, 0].mean(), rel=1e-14)
    for bad in (members[:-1], members.astype(np.float64), np.full(E, -1), members - 2):
        with pytest.raises(ValueError):
            save_eval_by_member(EvalTrace(m), bad, str(tmp_path / "c"))
    with pytest.raises(ValueError):
        save_eval_by_member(EvalTrace(m[:, :, :2]), members, str(tmp_path / "c"))
    assert not (tmp_path / "c").exists()


# ------------------------------------------------------------------------------------------------------ tools/eval_device
@pytest.fixture(scope="module")
def tool():
    pytest.importorskip("torch")
    spec = importlib.util.spec_from_file_location("eval_device_bank", os.path.join(ROOT, "tools", "eval_device.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(**kw):
    d = dict(model=None, random_actor=False, models=None, random_actors=None, envs=64)
    d.update(kw)
    return argparse.Namespace(**d)


def test_eval_device_actor_argument_checks(tool):
    ok = tool.check_actor_args
    assert ok(_args(models=["a.pt", "b.pt"])) == "" and ok(_args(random_actors=4)) == "" and ok(_args(random_actors=64)) == ""
    assert ok(_args(model="a.pt")) == "" and ok(_args(random_actor=True)) == ""
    assert "mutually exclusive" in ok(_args(model="a.pt", models=["b.pt"]))
    assert "exactly one" in ok(_args()) and "exactly one" in ok(_args(models=["a.pt"], random_actors=2))
    assert "exactly one" in ok(_args(random_actor=True, random_actors=2))
    assert "multiple of the 3 actors" in ok(_args(models=["a", "b", "c"])) and "--envs 64" in ok(_args(random_actors=5))
    assert "1 to 256" in ok(_args(random_actors=0)) and "1 to 256" in ok(_args(random_actors=257, envs=257))


def test_eval_device_by_member_table(tool):
    mean = np.array([[0.5, 0.25, 0.125], [1.0, np.nan, 0.0]])
    lines = tool.by_member_table(mean, np.array([3, 4]), ["a.pt", "b.pt"]).split("\n")
    assert len(lines) == 3 and lines[0].startswith("member | envs")
    assert lines[1].split("|")[0].strip() == "0" and lines[1].split("|")[1].strip() == "3" and lines[1].endswith("a.pt")
    assert "0.5000" in lines[1] and "nan" in lines[2] and lines[2].endswith("b.pt")


def test_eval_device_refuses_bad_bank_options_on_the_command_line(tool, monkeypatch, capsys):
    for argv, what in ((["--models", "a", "b", "c", "--envs", "64"], "multiple of the 3 actors"),
                       (["--model", "a", "--models", "b"], "mutually exclusive"),
                       (["--random-actor", "--random-actors", "2"], "exactly one")):
        monkeypatch.setattr("sys.argv", ["eval_device.py"] + argv)
        with pytest.raises(SystemExit) as e:
            tool.main()
        assert e.value.code == 2 and what in capsys.readouterr().err
