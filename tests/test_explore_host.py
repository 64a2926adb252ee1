"""Per-env exploration (include/swarm_rollout.h "Per-env exploration"), host side: the statistics of the restated coin, the
two new symbols in the header, the binding and the library, the C-side refusals (they never reach a device), and
rollout_device(coin=...) against a stub in place of the library: the host draws, the log-pi constants, the Python-side
refusals, and a ring that a raising call leaves as it was."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

import explore_inputs as X
from helpers import mix64, noise_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "swarm_rollout.h")


# ------------------------------------------------------------------------------------------------------------------------
# the restated coin
# ------------------------------------------------------------------------------------------------------------------------
def _lag1(x):
    """Sample lag-1 correlation of neighbouring entries along axis 0 of a 0 / 1 table, pooled over axis 1."""
    x = x.astype(np.float64) - x.mean()
    return float((x[:-1] * x[1:]).sum() / (x * x).sum())


@pytest.mark.parametrize("eps", [0.1, 0.5])
def test_coin_rate_and_independence(eps):
    steps, E = 1000, 1000                                         # 10^6 coins
    n = steps * E
    c = X.coin_table(seed=12, step0=300, steps=steps, epsilon=np.full(E, eps, np.float32), env_offset=40)
    assert c.shape == (steps, E) and c.dtype == np.uint8 and set(np.unique(c)) == {0, 1}
    e32 = float(np.float32(eps))
    assert abs(c.mean() - e32) <= 4 * math.sqrt(e32 * (1 - e32) / n), c.mean()
    assert abs(_lag1(c)) <= 4 / math.sqrt(n)                      # over steps, env fixed
    assert abs(_lag1(c.T)) <= 4 / math.sqrt(n)                    # over envs, step fixed


def test_coin_limits_and_its_own_salt():
    E = 4096
    u = X.coin_uniforms(3, 9, E)
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
    eps = np.array([0.0, -1.0, np.nan, 1.0, 2.0, np.inf], np.float32)
    for t in range(64):
        assert X.coins(5, t, eps).tolist() == [0, 0, 0, 1, 1, 1]
    # the coin of global env ge is not the uniform-action hash of row ge: the salts differ
    assert X.COIN_SALT != X.UNIFORM_SALT and X.COIN_SALT == 0xA0761D6478BD642F
    ge = np.arange(E)
    for seed, step in ((0, 0), (3, 9), (2 ** 63, 2 ** 40)):
        assert not (X.coin_hash(seed, step, ge) == X.uniform_hash(seed, step, ge)).any()
        assert int(X.coin_hash(seed, step, [7])[0]) ==mix64(mix64(noise_key(seed, step) ^ 0xA0761D6478BD642F) ^ 7)
    # keyed by the GLOBAL env: a shard's coins are the whole batch's
    whole = X.coin_table(1, 0, 5, np.full(12, 0.4, np.float32))
    assert np.array_equal(X.coin_table(1, 0, 5, np.full(6, 0.4, np.float32), env_offset=6), whole[:, 6:])
    assert whole.any() and not whole.all()


def test_branches_compose_per_env():
    N = 3
    eps = np.array([1, 0, 0, 0], np.float32)
    sig = np.array([0.2, 0.2, 0.0, np.nan], np.float32)
    c, b = X.branches(1, 2, N, eps, sig)
    assert c.tolist() == [1, 0, 0, 0]
    assert b.tolist() == [X.COIN] * N + [X.NOISE] * N + [X.PLAIN] * N + [X.PLAIN] * N


# ------------------------------------------------------------------------------------------------------------------------
# the ABI: header, binding, library, C-side refusals
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def test_symbols_in_header_binding_and_library(lib):
    from marl_llm_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+swarm_rollout_explore\s*\(", src) and re.search(r"\bint\s+swarm_explore_envs\s*\(", src)
    assert "swarm_rollout_explore" in _lib.ROLLOUT_SYMBOLS and "swarm_explore_envs" in _lib.EXPLORE_SYMBOLS
    assert lib.swarm_abi_version() == 5 == _lib.ABI_VERSION
    f, g = lib.swarm_rollout_explore, lib.swarm_explore_envs
    assert len(f.argtypes) == 11 and f.argtypes[4] is ctypes.c_int32 and f.argtypes[6] is ctypes.c_uint64
    assert len(g.argtypes) == 10 and g.argtypes[2] is ctypes.c_int64 and g.argtypes[3] is ctypes.c_int32
    body = re.search(r"typedef struct swarm_explore \{(.*?)\} swarm_explore_t;", src, flags=re.S).group(1)
    assert [n for n, _ in _lib.SwarmExplore._fields_] == re.findall(r"\b(\w+)\s*;", body) == ["epsilon", "sigma", "log_c", "coin"]
    assert ctypes.sizeof(_lib.SwarmExplore) == 4 * 8
    assert "0xA0761D6478BD642F" in open(HEADER).read()


def test_the_library_refuses_bad_exploration_arguments(lib):
    from marl_llm_amd._lib import SwarmExplore, SwarmRing
    ring = SwarmRing()
    ring.n_slots, ring.rows = 2, 1
    fake = ctypes.c_void_p(8)                                     # never dereferenced: the pointer checks come first
    err = lib.swarm_rollout_last_error
    ok_ex, no_sigma, no_c = SwarmExplore(None, 8, 8, None), SwarmExplore(8, None, 8, None), SwarmExplore(None, 8, None, None)
    tail = (0, 0, 0, None, None)
    f = lib.swarm_rollout_explore
    assert f(None, None, ctypes.byref(ring), None, 1, ctypes.byref(ok_ex), *tail) == 1
    assert err() == b"swarm_rollout_explore: null env, policy or ring"
    assert f(fake, fake, ctypes.byref(ring), None, 1, None, *tail) == 1
    assert err().startswith(b"swarm_rollout_explore: null ex or ex->sigma")
    assert f(fake, fake, ctypes.byref(ring), None, 1, ctypes.byref(no_sigma), *tail) == 1
    assert err().startswith(b"swarm_rollout_explore: null ex or ex->sigma")
    assert f(fake, fake, ctypes.byref(ring), fake, 1, ctypes.byref(no_c), *tail) == 1
    assert err().startswith(b"swarm_rollout_explore: log_pi is given: ex->log_c")
    g = lib.swarm_explore_envs
    assert g(None, None, 8, 4, ctypes.byref(ok_ex), None, 0, 0, 0, None) == 1 and err() == b"swarm_explore_envs: null act"
    assert g(fake, None, 8, 4, None, None, 0, 0, 0, None) == 1 and err().startswith(b"swarm_explore_envs: null ex or ex->sigma")
    assert g(fake, None, 8, 4, ctypes.byref(no_sigma), None, 0, 0, 0, None) == 1 and b"null ex or ex->sigma" in err()
    assert g(fake, fake, 8, 4, ctypes.byref(no_c), None, 0, 0, 0, None) == 1 and b"ex->log_c" in err()
    for rows, n in ((-4, 4), (8, 0), (9, 4)):
        assert g(fake, None, rows, n, ctypes.byref(ok_ex), None, 0, 0, 0, None) == 1
        assert err().startswith(b"swarm_explore_envs: rows ") and b"multiple of n_agents" in err()
    assert g(fake, None, 8, 4, ctypes.byref(ok_ex), None, 0, 0, 6, None) == 1
    assert err().startswith(b"swarm_explore_envs: row_offset 6 is no multiple of n_agents 4")


# ------------------------------------------------------------------------------------------------------------------------
# rollout_device(coin=...) with a stub library
# ------------------------------------------------------------------------------------------------------------------------
class _StubLib:
    """Stands for libswarmenv.so: logs every rollout call, reads the swarm_explore_t it is handed (host memory here), and
    refuses the calls of `refuse` (a set of call indices) with SWARM_ERR_INVALID."""

    def __init__(self, E):
        self.E, self.calls, self.refuse = E, [], set()

    def _read(self, ptr, dtype, n):
        if not ptr:
            return None
        ct = {np.float32: ctypes.c_float, np.uint8: ctypes.c_uint8}[dtype]
        return np.ctypeslib.as_array((ct * n).from_address(ptr)).copy()

    def _rc(self):
        return 1 if len(self.calls) - 1 in self.refuse else 0

    def swarm_rollout(self, env, pol, ring, steps, coins, noise_scale, seed, step0, row_offset, stats, stream):
        self.calls.append(dict(name="swarm_rollout", steps=steps, noise_scale=noise_scale, step0=step0,
                               coins=self._read(coins.value if coins is not None else None, np.uint8, steps)))
        return self._rc()

    def swarm_rollout_logpi(self, env, pol, ring, log_pi, steps, coins, noise_scale, *rest):
        self.calls.append(dict(name="swarm_rollout_logpi", steps=steps, noise_scale=noise_scale))
        return self._rc()

    def swarm_rollout_explore(self, env, pol, ring, log_pi, steps, ex, seed, step0, row_offset, stats, stream):
        ex = ex._obj
        self.calls.append(dict(name="swarm_rollout_explore", steps=steps, step0=step0, row_offset=row_offset, log_pi=log_pi is not None,
                               epsilon=self._read(ex.epsilon, np.float32, self.E), sigma=self._read(ex.sigma, np.float32, self.E),
                               log_c=self._read(ex.log_c, np.float32, self.E), coin=ex.coin, cur=ring._obj.cur))
        return self._rc()

    def swarm_rollout_last_error(self):
        return b"swarm_rollout_explore: stub refusal"


class _CountingRng:
    def __init__(self):
        self.draws = 0

    def random(self):
        self.draws += 1
        return 0.9


@pytest.fixture()
def stub(monkeypatch):
    """(SwarmBatch stub, FusedPolicy stub, stub library) wired into rollout_device; everything on the host."""
    torch = pytest.importorskip("torch")
    from marl_llm_amd import _lib
    from marl_llm_amd import rollout as R
    from test_reset_envs_host import _stub_batch
    sb = _stub_batch(E=4, N=2, D=3)
    lib = _StubLib(sb.n_env)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    pol = object.__new__(R.FusedPolicy)
    pol.handle = None
    return sb, pol, lib


def _ring(sb, K=6, log_pi=False):
    from marl_llm_amd.rollout import ChainedReplay
    return ChainedReplay(K, sb.n_env * sb.n_agents, sb.obs_dim, 2, "cpu", log_pi=log_pi)


def _state(r):
    return (r.cur, r.count, r._chained, set(r._sealed))


def _obs(sb):
    import torch
    return torch.zeros(sb.n_env, sb.n_agents, sb.obs_dim)


def test_batch_coin_draws_steps_times_and_env_coin_never(stub):
    from marl_llm_amd.rollout import rollout_device
    sb, pol, lib = stub
    ring, rng = _ring(sb), _CountingRng()
    rollout_device(sb, pol, 5, obs=_obs(sb), replay=ring, noise_scale=0.1, epsilon=0.3, host_rng=rng, track_reward=False)
    assert rng.draws == 5                                          # the default is coin="batch": one host draw per step
    assert [c["name"] for c in lib.calls] == ["swarm_rollout", "swarm_rollout"] and lib.calls[1]["coins"].tolist() == [0] * 5
    lib.calls.clear()
    rollout_device(sb, pol, 5, replay=ring, noise_scale=0.1, epsilon=0.3, host_rng=rng, track_reward=False, coin="env")
    assert rng.draws == 5                                          # coin="env": no host draw
    assert [c["name"] for c in lib.calls] == ["swarm_rollout_explore"] * 2 and [c["steps"] for c in lib.calls] == [0, 5]
    c = lib.calls[1]
    assert c["epsilon"].tolist() == [np.float32(0.3)] * 4 and c["sigma"].tolist() == [np.float32(0.1)] * 4
    assert c["log_c"] is None and not c["log_pi"] and c["coin"] is None
    assert _state(ring) == (3, 6, True, set())                     # 10 steps through the 7 slots


def test_scalar_zero_epsilon_passes_null_and_arrays_pass_through(stub):
    from marl_llm_amd.rollout import rollout_device
    sb, pol, lib = stub
    ring = _ring(sb)
    rollout_device(sb, pol, 2, obs=_obs(sb), replay=ring, noise_scale=[0.0, 0.1, 0.25, 0.5], track_reward=False, coin="env")
    assert lib.calls[-1]["epsilon"] is None and lib.calls[-1]["sigma"].tolist() == [0.0, np.float32(0.1), 0.25, 0.5]
    eps = 0.4 ** (1 + 7 * np.arange(4) / 3)
    rollout_device(sb, pol, 2, replay=ring, noise_scale=0.1, epsilon=eps, track_reward=False, coin="env", step0=9, row_offset=6)
    c = lib.calls[-1]
    assert np.array_equal(c["epsilon"], eps.astype(np.float32)) and (c["step0"], c["row_offset"]) == (9, 6)


def test_log_c_follows_the_header_expression(stub):
    import torch
    from marl_llm_amd.rollout import explore_log_c, rollout_device
    sb, pol, lib = stub
    ring = _ring(sb, log_pi=True)
    sig = np.array([0.1, 0.25, 0.0, 1.7], np.float32)
    rollout_device(sb, pol, 3, obs=_obs(sb), replay=ring, noise_scale=sig, epsilon=0.2, log_pi=True, track_reward=False, coin="env")
    c = lib.calls[-1]
    want = [np.float32(2.0 * math.log(float(s) * math.sqrt(2.0 * math.pi))) if s > 0 else np.float32(0) for s in sig]
    assert c["log_pi"] and c["log_c"].dtype == np.float32 and c["log_c"].tolist() == want
    assert np.array_equal(explore_log_c(sig), X.log_c(sig)) and np.array_equal(c["log_c"], X.log_c(sig))
    # the scalar path's constant for the same fp32 value (include/swarm_policy.h): bit for bit
    assert explore_log_c([0.3])[0] == np.float32(2 * math.log(float(np.float32(0.3)) * math.sqrt(2 * math.pi)))
    # a float noise_scale: E equal constants; a tensor on the device with log_c=: passed through
    rollout_device(sb, pol, 1, replay=ring, noise_scale=0.3, log_pi=True, track_reward=False, coin="env")
    assert lib.calls[-1]["log_c"].tolist() == [explore_log_c([0.3])[0]] * 4
    given = torch.tensor([1.0, 2.0, 3.0, 4.0])
    rollout_device(sb, pol, 1, replay=ring, noise_scale=torch.from_numpy(sig), log_c=given, log_pi=True, track_reward=False, coin="env")
    assert lib.calls[-1]["log_c"].tolist() == [1.0, 2.0, 3.0, 4.0]


def test_stretches_slice_coin_out_by_step(stub):
    import torch
    from marl_llm_amd.rollout import rollout_device
    sb, pol, lib = stub
    ring = _ring(sb, K=12)
    coin_out = torch.zeros((6, 4), dtype=torch.uint8)
    rollout_device(sb, pol, 6, replay=ring, noise_scale=0.1, epsilon=0.5, coin="env", coin_out=coin_out, track_reward=False,
                   resets={0: (1, 0), 4: (1, 1)}, step0=20)
    runs = [c for c in lib.calls if c["steps"] > 0]
    assert [(c["steps"], c["step0"]) for c in runs] == [(4, 20), (2, 24)]
    assert [c["coin"] for c in runs] == [coin_out.data_ptr(), coin_out.data_ptr() + 4 * 4]
    assert [c["cur"] for c in runs] == [0, 5]                     # the cut sealed slot 4


@pytest.mark.parametrize("bad", ["coin", "eps shape", "sigma shape", "tensor sigma without log_c", "log_c without log_pi",
                                 "coin_out shape", "coin_out dtype", "batch with coin_out", "batch with log_c", "library"])
def test_a_refused_call_leaves_the_ring_as_it_was(stub, bad):
    import torch
    from marl_llm_amd._lib import SwarmError
    from marl_llm_amd.rollout import rollout_device
    sb, pol, lib = stub
    ring = _ring(sb, log_pi=True)
    rollout_device(sb, pol, 3, obs=_obs(sb), replay=ring, noise_scale=0.1, coin="env", track_reward=False)
    rollout_device(sb, pol, 2, replay=ring, noise_scale=0.1, coin="env", track_reward=False, reset=(1, 0))
    before, n_calls = _state(ring), len(lib.calls)
    assert before == (6, 6, True, {3})
    kw = dict(noise_scale=0.1, epsilon=0.2, coin="env")
    err, match = ValueError, None
    if bad == "coin":
        kw.update(coin="agent"); match = "coin must be 'batch'"
    elif bad == "eps shape":
        kw.update(epsilon=[0.1, 0.2, 0.3]); match = r"epsilon must be a float or hold one value per env, \[4\]"
    elif bad == "sigma shape":
        kw.update(noise_scale=np.zeros((4, 1))); match = "noise_scale must be a float or hold one value per env"
    elif bad == "tensor sigma without log_c":
        kw.update(noise_scale=torch.full((4,), 0.1), log_pi=True); match = "needs log_c="
    elif bad == "log_c without log_pi":
        kw.update(log_c=[0.0] * 4); match = "needs log_pi=True"
    elif bad == "coin_out shape":
        kw.update(coin_out=torch.zeros((3, 4), dtype=torch.uint8)); match = r"coin_out must be a contiguous uint8 tensor \[4, 4\]"
    elif bad == "coin_out dtype":
        kw.update(coin_out=torch.zeros((4, 4), dtype=torch.int32)); match = "coin_out must be"
    elif bad == "batch with coin_out":
        kw.update(coin="batch", epsilon=0.0, coin_out=torch.zeros((4, 4), dtype=torch.uint8)); match = "belong to coin='env'"
    elif bad == "batch with log_c":
        kw.update(coin="batch", epsilon=0.0, log_c=[0.0] * 4); match = "belong to coin='env'"
    else:                                                         # the library's own validation (the zero-step call) refuses
        lib.refuse = {n_calls}; err, match = SwarmError, "swarm_rollout_explore: stub refusal"
    with pytest.raises(err, match=match):
        rollout_device(sb, pol, 4, obs=_obs(sb), replay=ring, track_reward=False, **kw)
    assert _state(ring) == before
    assert len(lib.calls) == n_calls + (1 if bad == "library" else 0)      # a Python-side refusal never reaches the library
    assert not [c for c in lib.calls[n_calls:] if c["steps"] > 0]


def test_rollout_env_coin_needs_the_fused_path():
    torch = pytest.importorskip("torch")
    from marl_llm_amd.rollout import PolicyMLP, rollout
    from test_logpi_host import _ToyEnv
    env = _ToyEnv(1, 4, 8)
    with pytest.raises(ValueError, match="fused path"):
        rollout(env, PolicyMLP(8, 2, 16), 1, torch.zeros(1, 4, 8), coin="env")
    with pytest.raises(ValueError, match="coin must be"):
        rollout(env, PolicyMLP(8, 2, 16), 1, torch.zeros(1, 4, 8), coin="row")
    assert env.t == 0
