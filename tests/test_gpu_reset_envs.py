"""The per-env device reset (swarm_reset_envs, SwarmBatch.reset_envs).  Every comparison is bit for bit and the yardstick is
swarm_reset itself (tests/test_gpu_reset_rollout.py holds it to its numpy restatement and the oracle): envs are independent,
so env e of the handle under test is compared with env e of a twin handle -- one twin per distinct episode number, which ran
reset(seed, ep), and a "kept" twin that never called reset_envs.  Inputs: tests/reset_envs_inputs.py, whose conditions
tests/test_reset_envs_host.py asserts (kept and reset envs inside one step-kernel workgroup, both kinds of shape drawn).

Mutants (scratch libraries, each run once against this file and test_gpu_rollout_resets.py): DESIGN.md "Per-env reset"."""
import ctypes

import numpy as np
import pytest

import reset_envs_inputs as inputs
from helpers import shape_batch
from test_gpu_streams import cycles_per_ms          # noqa: F401 -- the module-scoped fixture (torch.cuda._sleep cycles per ms)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = {"f64": torch.float64, "f32": torch.float32, "bf16": torch.bfloat16}
CASES = [(n, e, big, "f64") for (n, e, big) in sorted(inputs.EQUALITY)] + [(64, 9, False, "f32"), (64, 9, False, "bf16")]
STEP_KEYS = ("obs", "reward", "done", "a_prior")


@pytest.fixture(scope="module")
def s3():
    return inputs.mixed_shape_set()


def _actions(sb, count, seed=5):
    gen = torch.Generator(device=sb.device).manual_seed(seed)
    return [torch.rand((sb.n_env, sb.n_agents, 2), device=sb.device, generator=gen) * 2 - 1 for _ in range(count)]


def _state(sb):
    """Everything an env holds on the device, by env: p, dp, cells, n_g, shape index."""
    p, dp = sb.get_state()
    cells, n_g = sb.get_cells()
    return dict(p=p.cpu().numpy(), dp=dp.cpu().numpy(), cells=cells, n_g=n_g, shape=sb.get_shape_index())


def _steps(sb, acts):
    return [dict(zip(STEP_KEYS, [x.clone() for x in sb.step(a)])) for a in acts]


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    return np.array_equal(a, b, equal_nan=True)


def _assert_env(got, ref, e, what):
    for k in ref:
        assert _same(got[k][e], ref[k][e]), (what, "env %d" % e, k)


def _path_counts(scan, n_env, n_a):
    epb = inputs.envs_per_workgroup(n_a)
    n_scan = sum(min(epb, n_env - b) for b in range(0, n_env, epb) if any(e in scan for e in range(b, min(b + epb, n_env))))
    return n_env - n_scan, n_scan


@pytest.mark.parametrize("n_a,n_env,big,dtype", CASES, ids=["n%d_e%d_%s" % (c[0], c[1], c[3]) for c in CASES])
def test_every_env_equals_its_twin(s3, n_a, n_env, big, dtype):
    seed = inputs.EQUALITY[(n_a, n_env, big)]
    vec = inputs.episode_vector(n_env)
    mk = lambda: shape_batch(s3, n_env, n_a, DTYPES[dtype], large_swarm=big)
    A = mk()
    acts = _actions(A, 6)
    twins, scans = {}, {}
    try:
        A.reset(seed, 0)
        _steps(A, acts[:3])
        obs_a = A.reset_envs(seed, vec).clone()
        state_a = _state(A)
        steps_a = _steps(A, acts[3:])
        idx_a = {k: v.clone() for k, v in A.indices().items()}
        paths_a = A.path_envs()
        # the twins: reset(seed, ep) for every episode number, and the handle that was left alone (-1)
        for ep in sorted(set(vec.tolist())):
            T = twins[ep] = mk()
            if ep < 0:
                T.reset(seed, 0)
                _steps(T, acts[:3])
                obs_t = T.observe().clone()
            else:
                obs_t = T.reset(seed, ep).clone()
            state_t = _state(T)
            steps_t = _steps(T, acts[3:])
            idx_t = {k: v.clone() for k, v in T.indices().items()}
            envs = np.nonzero(vec == ep)[0]
            assert len(envs) > 0
            for e in envs:
                what = "episode %d" % ep
                assert torch.equal(obs_a[e], obs_t[e]), (what, e, "obs of the reset")
                _assert_env(state_a, state_t, e, what)
                for t, (x, y) in enumerate(zip(steps_a, steps_t)):
                    _assert_env(x, y, e, what + ", step %d" % t)
                _assert_env(idx_a, idx_t, e, what + ", index lists")
            scans[ep] = {e for e in envs if state_t["shape"][e] in inputs.OFF_LATTICE}
        assert (state_a["shape"][vec < 0] >= 0).all()
        if not big:
            scan = set().union(*scans.values())
            assert scan and len(scan) < n_env
            assert paths_a == _path_counts(scan, n_env, n_a)
        # the state after the last step, once more, env by env
        end_a = _state(A)
        for ep, T in twins.items():
            end_t = _state(T)
            for e in np.nonzero(vec == ep)[0]:
                _assert_env(end_a, end_t, e, "end, episode %d" % ep)
    finally:
        A.close()
        for T in twins.values():
            T.close()


@pytest.mark.parametrize("n_a,n_env", [(8, 17), (64, 9)])
def test_all_keep_changes_nothing(s3, n_a, n_env):
    A, T = shape_batch(s3, n_env, n_a, torch.float64), shape_batch(s3, n_env, n_a, torch.float64)
    try:
        acts = _actions(A, 5)
        for sb in (A, T):
            sb.reset(3, 1)
            last = _steps(sb, acts[:2])[-1]["obs"]
        before = _state(A)
        out = torch.zeros((n_env, n_a, A.obs_dim), dtype=torch.float64, device=A.device)
        obs = A.reset_envs(3, np.full(n_env, -1))
        obs2 = A.reset_envs(3, torch.full((n_env,), -1, dtype=torch.int64, device=A.device), out=out)
        assert torch.equal(obs, last) and torch.equal(obs2, last) and obs2.data_ptr() == out.data_ptr()
        after = _state(A)
        for k in before:
            assert _same(before[k], after[k]), k
        assert A.path_envs() == T.path_envs()
        for t, (x, y) in enumerate(zip(_steps(A, acts[2:]), _steps(T, acts[2:]))):
            for k in STEP_KEYS:
                assert torch.equal(x[k], y[k]), (t, k)
    finally:
        A.close(); T.close()


@pytest.mark.parametrize("n_a,n_env,big", [(8, 17, False), (64, 9, False), (300, 3, True)])
def test_all_reset_with_one_episode_equals_reset(s3, n_a, n_env, big):
    A, T = (shape_batch(s3, n_env, n_a, torch.float64, large_swarm=big) for _ in range(2))
    try:
        acts = _actions(A, 5)
        A.reset(9, 0)
        _steps(A, acts[:2])
        assert torch.equal(A.reset_envs(9, np.full(n_env, 6), env_offset=40), T.reset(9, 6, env_offset=40))
        sa, st = _state(A), _state(T)
        for k in sa:
            assert _same(sa[k], st[k]), k
        assert A.path_envs() == T.path_envs() and A.lattice_envs() == T.lattice_envs()
        for t, (x, y) in enumerate(zip(_steps(A, acts[2:]), _steps(T, acts[2:]))):
            for k in STEP_KEYS:
                assert torch.equal(x[k], y[k]), (t, k)
        ia, it = A.indices(), T.indices()
        assert all(torch.equal(ia[k], it[k]) for k in ia)
    finally:
        A.close(); T.close()


def test_sharded_reset_envs_equals_the_full_batch(s3):
    """Two 'ranks' of 8 envs with env_offset 0 and 8 reproduce the 16-env call (tests/test_gpu_reset_rollout.py's form)."""
    n_a, vec = 32, inputs.episode_vector(16)
    full = shape_batch(s3, 16, n_a)
    try:
        full.reset(9, 0)
        o_full = full.reset_envs(9, vec).clone()
        s_full = _state(full)
        parts, states = [], []
        for r in range(2):
            sb = shape_batch(s3, 8, n_a)
            sb.reset(9, 0, env_offset=8 * r)
            parts.append(sb.reset_envs(9, vec[8 * r: 8 * r + 8], env_offset=8 * r).clone())
            states.append(_state(sb))
            sb.close()
        assert torch.equal(o_full, torch.cat(parts, dim=0))
        for k in s_full:
            assert _same(s_full[k], np.concatenate([s[k] for s in states])), k
    finally:
        full.close()


def test_a_kept_env_keeps_a_posed_shape(s3):
    """Envs that hold a shape at a pose given through select_shapes(pose=...) -- cells no reset would draw -- keep their cells
    and lattice record (the walk still serves them) and step as before; their neighbours in the workgroup are reset."""
    n_a, n_env = 8, 10
    A, T = shape_batch(s3, n_env, n_a, torch.float64), shape_batch(s3, n_env, n_a, torch.float64)
    try:
        acts = _actions(A, 4)
        index = np.array([0, -1, 1, -1, -1, 0, -1, -1, 2, 1])
        ang, off = np.linspace(-1.0, 1.0, n_env), np.stack([np.linspace(-0.3, 0.3, n_env), np.linspace(0.2, -0.2, n_env)], axis=1)
        # a seed whose resets leave the first workgroup (envs 0-7) to the row walk: none of its reset envs draws the jittered shape
        seed = next(s for s in range(1, 200) if all(inputs.drawn_shape(s, 3, e) not in inputs.OFF_LATTICE for e in (1, 3, 4, 6, 7)))
        for sb in (A, T):
            sb.reset(seed, 0)
            sb.select_shapes(index, angle=ang, offset=off)
            _steps(sb, acts[:1])
        vec = np.where(index >= 0, -1, 3)                      # the posed envs are kept, the others start episode 3
        before = _state(A)
        A.reset_envs(seed, vec)
        after = _state(A)
        posed = index >= 0
        for k in before:
            assert _same(before[k][posed], after[k][posed]), k
            assert not _same(before[k][~posed], after[k][~posed]) or k in ("n_g", "shape"), k
        R = shape_batch(s3, n_env, n_a, torch.float64)
        try:
            R.reset(seed, 3)
            sr = _state(R)
            for e in np.nonzero(~posed)[0]:
                _assert_env(after, sr, e, "reset env")
            scan = {e for e in range(n_env) if after["shape"][e] in inputs.OFF_LATTICE}
            assert A.path_envs() == _path_counts(scan, n_env, n_a) and A.path_envs()[0] > 0
            for t, (x, y, z) in enumerate(zip(_steps(A, acts[1:]), _steps(T, acts[1:]), _steps(R, acts[1:]))):
                for k in STEP_KEYS:
                    assert torch.equal(x[k][posed], y[k][posed]), (t, k, "kept")
                    assert torch.equal(x[k][~posed], z[k][~posed]), (t, k, "reset")
        finally:
            R.close()
    finally:
        A.close(); T.close()


# ------------------------------------------------------------------------------------------------------------------------
# entry-point behaviour
# ------------------------------------------------------------------------------------------------------------------------
def test_a_device_vector_is_read_in_stream_order(s3):
    """The episode tensor is written on the handle's stream, behind a delay, after the host has prepared the call: the kernel
    sees those values, not the ones the tensor held when reset_envs was called."""
    n_a, n_env = 8, 9
    A, T = shape_batch(s3, n_env, n_a), shape_batch(s3, n_env, n_a)
    try:
        vec = inputs.episode_vector(n_env)
        for sb in (A, T):
            sb.reset(2, 0)
        before = T.observe().clone()
        want = T.reset_envs(2, vec).clone()
        assert not torch.equal(want, before)                   # what the stale vector (all keep) would return
        stale = torch.full((n_env,), -1, dtype=torch.int64, device=A.device)
        dev = stale.clone()
        fresh = torch.from_numpy(vec).to(A.device)
        torch.cuda.synchronize()
        torch.cuda._sleep(20_000_000)
        dev.copy_(fresh)                                       # enqueued behind the delay, in front of the reset
        got = A.reset_envs(2, dev)
        assert A.shape_env_in_force is None and A.shape_in_force == -1
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        assert torch.equal(A.reset_envs(2, stale), want)       # all keep: the observation of the present state
    finally:
        A.close(); T.close()


def test_reset_envs_on_a_side_stream_behind_a_delay(s3, cycles_per_ms):
    """tests/test_gpu_streams.py's pattern: the side stream sleeps, the episode vector and the state the kept envs hold are
    rewritten behind the delay, reset_envs is enqueued behind that and must not wait.  Work that went to another stream
    computes on the old values: a value mismatch."""
    from test_gpu_streams import Delayed
    n_a, n_env = 8, 9
    A, T = shape_batch(s3, n_env, n_a), shape_batch(s3, n_env, n_a)
    try:
        vec_a, vec_b = inputs.episode_vector(n_env, 0), inputs.episode_vector(n_env, 1)
        acts = _actions(A, 2)
        for sb in (A, T):                                      # warm-up on the default stream: every entry point, state A
            sb.reset(2, 0); sb.reset_envs(2, vec_a); sb.step(acts[0])
        torch.cuda.synchronize()
        want_obs = T.reset_envs(2, vec_b).clone()
        want_step = _steps(T, acts[1:])[0]
        want_state = _state(T)
        m = Delayed(cycles_per_ms, "reset_envs on a side stream")
        dev = torch.from_numpy(vec_a).to(A.device)
        fresh = torch.from_numpy(vec_b).to(A.device)
        slot = torch.zeros((n_env * n_a, A.obs_dim), dtype=A.obs_dtype, device=A.device)
        torch.cuda.synchronize()
        with m.stream():
            m.delay()
            dev.copy_(fresh)
            got_obs = A.reset_envs(2, dev, out=slot); m.enqueued("swarm_reset_envs")
            got_step = _steps(A, acts[1:])[0]; m.enqueued("swarm_step")
            m.done()
        got_state = _state(A)
        assert torch.equal(got_obs, want_obs), "reset_envs did not run behind the side stream's writes: value mismatch"
        for k in STEP_KEYS:
            assert torch.equal(got_step[k], want_step[k]), k
        for k in want_state:
            assert _same(got_state[k], want_state[k]), k
    finally:
        A.close(); T.close()


def test_refusals_leave_the_state_unchanged(s3):
    from marl_llm_amd._lib import SwarmError
    n_a, n_env = 8, 5
    lib_err = lambda sb: sb.lib.swarm_last_error(sb.handle).decode()
    vec = torch.zeros(n_env, dtype=torch.int64, device="cuda")
    ptr = ctypes.c_void_p(vec.data_ptr())
    sb = shape_batch(s3, n_env, n_a, upload=False)
    try:
        assert sb.lib.swarm_reset_envs(None, 1, ptr, 0, None) == 1                            # SWARM_ERR_INVALID
        assert sb.lib.swarm_reset_envs(sb.handle, 1, None, 0, None) == 1 and lib_err(sb).startswith("swarm_reset_envs:")
        assert sb.lib.swarm_reset_envs(sb.handle, 1, ptr, 0, None) == 3                       # SWARM_ERR_STATE: no shape set
        assert lib_err(sb).startswith("swarm_reset_envs:")
        sb.set_shapes(s3)
        assert sb.lib.swarm_reset_envs(sb.handle, 1, ptr, 0, None) == 3 and lib_err(sb).startswith("swarm_reset_envs:")   # no state
        with pytest.raises(SwarmError, match="swarm_reset_envs:"):
            sb.reset_envs(1, vec)
        sb.set_state(np.zeros((n_env, 2, n_a)), np.zeros((n_env, 2, n_a)))
        assert sb.lib.swarm_reset_envs(sb.handle, 1, ptr, 0, None) == 3 and "cells" in lib_err(sb)     # no cells
        sb.reset(1, 0)
        before = _state(sb)
        for bad in ([0, 1], np.zeros(n_env), torch.zeros(n_env, dtype=torch.int32, device="cuda"), vec[:3]):
            with pytest.raises(ValueError):
                sb.reset_envs(1, bad)
        assert sb.lib.swarm_reset_envs(sb.handle, 1, None, 0, None) == 1
        after = _state(sb)
        for k in before:
            assert _same(before[k], after[k]), k
        assert sb.lib.hipGetLastError() == 0
    finally:
        sb.close()
