"""CPU-side checks of the per-env reset's public surface (swarm_reset_envs, SwarmBatch.reset_envs, resets= of the device
loops, EpisodeClock): the inputs of the GPU tests meet their conditions, the clock's schedule equals a per-env simulation,
the ring accounting of a resets= schedule (slots = steps + cuts, sealed slots never sampled, a rejected schedule leaves the
ring as it was) with a stub in place of the library calls, and the symbol is declared, bound and exported at ABI version 5."""
import ctypes
import os
import re

import numpy as np
import pytest

import reset_envs_inputs as inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "swarm_env.h")


# ------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(inputs.EQUALITY), ids=lambda c: "n%d_e%d" % c[:2])
def test_equality_inputs_meet_their_conditions(case):
    n_a, n_env, _ = case
    got = inputs.conditions(inputs.EQUALITY[case], inputs.episode_vector(n_env), n_a)
    assert all(got.values()), got


@pytest.mark.parametrize("case", [(8, 16), (64, 8)], ids=lambda c: "n%d_e%d" % c)
def test_rollout_inputs_meet_their_conditions(case):
    n_a, n_env = case
    seed = inputs.ROLLOUT[case]
    sched = inputs.rollout_schedule(seed, n_env)
    assert sorted(sched) == [0, 3, 5, 6] and all(0 <= t < inputs.ROLLOUT_STEPS for t in sched)
    for t in (3, 6):
        got = inputs.conditions(seed, sched[t][1], n_a)
        assert all(got.values()), (t, got)
    assert not np.array_equal(sched[3][1], sched[6][1])
    large = inputs.large_schedule(inputs.ROLLOUT[(300, 2)], 2)[2][1]
    assert large.tolist() == [-1, 5]


def test_the_shape_set_holds_both_kinds():
    s = inputs.mixed_shape_set()
    assert len(s["l_cell"]) == 3
    for k, g in enumerate(s["grid_coords"]):                      # a tiled shape's rows share their y; the jittered copy's do not
        ys = np.unique(np.round(np.asarray(g)[:, 1] / s["l_cell"][k], 6))
        assert (len(ys) < 60) == (k not in inputs.OFF_LATTICE), k


# ------------------------------------------------------------------------------------------------------------------------
# EpisodeClock
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,G", [(5, 1), (6, 3), (7, 4)])
def test_episode_clock_equals_a_per_env_simulation(L, G):
    pytest.importorskip("torch")
    from marl_llm_amd.rollout import EpisodeClock
    E = 9
    clock = EpisodeClock(E, L, groups=G, seed=42, env_offset=100)
    got = {}                                                      # global step -> [E] episode started there, -1: none
    t0 = 0
    calls = [1, 4, 2, 3 * L]
    calls[-1] = 3 * L - sum(calls[:-1])
    assert calls[-1] > 0 and len(set(calls)) > 2                  # uneven calls
    for k in calls:
        sched = clock.resets(k)
        for t, (seed, ep, off) in sched.items():
            assert 0 <= t < k and seed == 42 and off == 100
            if np.ndim(ep) == 0:
                assert isinstance(ep, int)
                got[t0 + t] = np.full(E, ep)
            else:
                assert ep.dtype == np.int64 and ep.shape == (E,) and (ep >= 0).any()
                assert (ep < 0).any() or len(set(ep.tolist())) > 1          # else it would be an int entry
                got[t0 + t] = ep
        t0 += k
    assert clock.t == 3 * L
    # brute force: every env counts its own steps
    age = [((e % G) * L) // G for e in range(E)]                  # steps into episode 0 at t = 0
    epi = [0] * E
    for t in range(3 * L):
        want = np.full(E, -1)
        for e in range(E):
            if t > 0:
                age[e] += 1
                if age[e] == L:
                    age[e], epi[e] = 0, epi[e] + 1
                    want[e] = epi[e]
            else:
                want[e] = 0
        if (want >= 0).any():
            assert t in got and np.array_equal(got[t], want), (t, got.get(t), want)
        else:
            assert t not in got, t
    assert (got[0] == 0).all()                                    # every env resets at t = 0


def test_episode_clock_in_phase_is_whole_batch_resets():
    pytest.importorskip("torch")
    from marl_llm_amd.rollout import EpisodeClock
    clock = EpisodeClock(6, 4, groups=1, seed=3)
    a, b = clock.resets(5), clock.resets(7)
    assert a == {0: (3, 0, 0), 4: (3, 1, 0)} and b == {3: (3, 2, 0)}          # global steps 0, 4, 8
    assert all(isinstance(v[1], int) for v in list(a.values()) + list(b.values()))
    with pytest.raises(ValueError):
        EpisodeClock(4, 3, groups=4)


# ------------------------------------------------------------------------------------------------------------------------
# ring accounting, with a stub in place of the library calls
# ------------------------------------------------------------------------------------------------------------------------
def _stub_batch(E=4, N=2, D=3, S=3):
    torch = pytest.importorskip("torch")
    from marl_llm_amd.batched import SwarmBatch

    class Stub(SwarmBatch):
        """No device, no library: the two resets fill the slot they are given and are logged."""
        def reset(self, seed, episode=0, env_offset=0, out=None):
            if self.fail_at is not None and len(self.log) == self.fail_at:
                raise RuntimeError("stub: reset refused")
            self.log.append(("reset", seed, episode, env_offset))
            out.fill_(-1.0 - len(self.log))

        def _reset_envs_ready(self, seed, ready, env_offset=0, out=None):
            if self.fail_at is not None and len(self.log) == self.fail_at:
                raise RuntimeError("stub: reset_envs refused")
            episode, host = ready
            assert isinstance(episode, torch.Tensor) and episode.dtype == torch.int64 and tuple(episode.shape) == (self.n_env,)
            self.log.append(("reset_envs", seed, episode.tolist(), env_offset))
            out.fill_(-1.0 - len(self.log))

        def __del__(self):
            pass

    sb = object.__new__(Stub)
    sb.handle, sb.lib, sb.log, sb.fail_at = None, None, [], None
    sb.n_env, sb.n_agents, sb.obs_dim, sb.n_shapes = E, N, D, S
    sb.device, sb.obs_dtype, sb.with_prior = torch.device("cpu"), torch.float32, True
    return sb


def _ring(sb, K):
    from marl_llm_amd.rollout import ChainedReplay
    return ChainedReplay(K, sb.n_env * sb.n_agents, sb.obs_dim, 2, "cpu")


def _ring_state(r):
    return (r.cur, r.count, r._chained, set(r._sealed))


def _run(sb, ring, steps, resets, reset=None, obs=None):
    """_run_stretches as the device loops call it; the stretch stub writes what the library call would: step t's columns into
    its slot and its next_obs (the value t + 1) into the slot behind."""
    from marl_llm_amd.rollout import _reset_plan, _run_stretches
    calls = []

    def stretch(a, b):
        calls.append((a, b, ring.cur))
        for t in range(a, b):
            j = (ring.cur + t - a) % ring.S
            ring.act[j].fill_(float(t)); ring.obs[(j + 1) % ring.S].fill_(float(t + 1))

    plan = _reset_plan(sb, resets, steps, reset, "test")
    _run_stretches(None, sb, ring, obs, reset, plan, steps, lambda: calls.append("validate"), stretch, "test")
    return calls


def test_slots_are_consumed_as_steps_plus_cuts():
    torch = pytest.importorskip("torch")
    sb = _stub_batch()
    ring = _ring(sb, 12)
    vec = np.array([-1, 2, -1, 5])
    calls = _run(sb, ring, 8, {0: (7, 0), 3: (7, vec), 5: (7, 4, 10), 6: (7, torch.tensor([3, -1, -1, -1]))})
    # step 0 on an empty ring seals nothing: cuts at 3, 5, 6
    assert calls == ["validate", (0, 3, 0), (3, 5, 4), (5, 6, 7), (6, 8, 9)]
    assert sb.log == [("reset", 7, 0, 0), ("reset_envs", 7, vec.tolist(), 0), ("reset", 7, 4, 10), ("reset_envs", 7, [3, -1, -1, -1], 0)]
    assert _ring_state(ring) == ((8 + 3) % 13, 8 + 3, True, {3, 6, 8})
    assert len(ring) == 8 * ring.n and sorted(ring._valid_starts()) == [0, 1, 2, 4, 5, 7, 9, 10]
    # every stored transition keeps its true next_obs: the slot behind step t holds t + 1, never a reset's observation
    for j in ring._valid_starts():
        t = int(ring.act[j][0, 0])
        assert float(ring.obs[(j + 1) % ring.S][0, 0]) == t + 1
    for j in (4, 7, 9):                                           # the resets wrote the slots behind the sealed ones
        assert float(ring.obs[j][0, 0]) < 0
    g = torch.Generator().manual_seed(0)
    obs, act, rew, nxt, done, pri = ring.sample(2000, generator=g)
    starts = {int(a) for a in act[:, 0].tolist()}
    assert starts == set(range(8))
    assert torch.equal(nxt[:, 0], act[:, 0] + 1)                  # no transition starts in a sealed slot
    # a second call continues the chain: the next cut seals again, a full ring drops its oldest steps
    calls = _run(sb, ring, 4, {2: (7, 9)})
    assert calls == ["validate", (0, 2, 11), (2, 4, 1)]
    assert ring.cur == 3 and ring.count == 12 and ring._sealed == {0, 3, 6, 8}
    assert len(ring) == 9 * ring.n and 3 not in ring._valid_starts()          # slot 3 is `cur` now: outside the window


def test_a_schedule_without_entries_is_one_call_and_step0_equals_reset():
    sb = _stub_batch()
    a, b = _ring(sb, 6), _ring(sb, 6)
    assert _run(sb, a, 4, {0: (5, 2)}) == _run(sb, b, 4, None, reset=(5, 2)) == ["validate", (0, 4, 0)]
    assert sb.log == [("reset", 5, 2, 0)] * 2 and _ring_state(a) == _ring_state(b)
    assert _run(sb, a, 3, {}) == ["validate", (0, 3, 4)] and _run(sb, b, 3, None) == ["validate", (0, 3, 4)]
    assert _ring_state(a) == _ring_state(b) and not a._sealed


@pytest.mark.parametrize("bad", ["step", "negative step", "length", "float", "both", "episode", "no shapes"])
def test_a_rejected_schedule_leaves_the_ring_as_it_was(bad):
    torch = pytest.importorskip("torch")
    from marl_llm_amd._lib import SwarmError
    sb = _stub_batch()
    ring = _ring(sb, 6)
    _run(sb, ring, 3, {0: (1, 0), 2: (1, 1)})
    before, log = _ring_state(ring), list(sb.log)
    assert before == (4, 4, True, {2})
    kw, err = dict(reset=None), ValueError
    if bad == "step":
        resets = {4: (1, 2)}
    elif bad == "negative step":
        resets = {1: (1, 2), -1: (1, 3)}
    elif bad == "length":
        resets = {1: (1, 2), 2: (1, [0, -1, 3])}
    elif bad == "float":
        resets = {1: (1, np.array([0.0, -1.0, 3.0, 1.0]))}
    elif bad == "both":
        resets, kw = {0: (1, 2), 2: (1, 3)}, dict(reset=(1, 2))
    elif bad == "episode":
        resets = {1: (1, -2)}
    else:
        resets, sb.n_shapes, err = {1: (1, 2)}, 0, SwarmError
    with pytest.raises(err):
        _run(sb, ring, 4, resets, **kw)
    assert _ring_state(ring) == before and sb.log == log


def test_a_failure_between_stretches_restores_the_ring():
    sb = _stub_batch()
    ring = _ring(sb, 6)
    _run(sb, ring, 2, {0: (1, 0)})
    before = _ring_state(ring)
    sb.fail_at = 2                                                # the second reset of the next call
    with pytest.raises(RuntimeError, match="refused"):
        _run(sb, ring, 5, {1: (1, 1), 3: (1, [2, -1, -1, 2])})
    assert _ring_state(ring) == before


def test_the_device_loops_reject_before_they_touch_the_device():
    """rollout_device / rollout_expert / rollout_eval parse resets= before they load the library or ask for a stream."""
    pytest.importorskip("torch")
    from marl_llm_amd import rollout as R
    sb = _stub_batch()
    ring = _ring(sb, 6)
    before = _ring_state(ring)
    pol = object.__new__(R.FusedPolicy); pol.handle = None

    class AEnv:                                                   # what _device_env takes for an AssemblySwarmEnv
        agent_strategy, is_collected = "input", False
        def _flush_cells(self):
            raise AssertionError("the env was flushed before resets= was refused")

    loops = [lambda env, **kw: R.rollout_device(env, pol, 4, replay=ring, **kw),
             lambda env, **kw: R.rollout_eval(env, pol, 4, replay=ring, **kw),
             lambda env, **kw: R.rollout_expert(env, 4, replay=ring, **kw)]
    for loop in loops:
        for resets in ({4: (1, 2)}, {1: (1, [0, 1])}, {1: (1, np.zeros(4))}, [(1, 2)]):
            with pytest.raises(ValueError, match="resets|episode"):
                loop(sb, resets=resets)
        with pytest.raises(ValueError, match="reset= and resets"):
            loop(sb, reset=(1, 0), resets={0: (1, 0)})
    for loop in loops[:2]:
        with pytest.raises(ValueError, match="reset= needs a SwarmBatch"):
            loop(AEnv(), resets={1: (1, 2)})
    AEnv.agent_strategy = "rule"
    with pytest.raises(ValueError, match="reset= needs a SwarmBatch"):
        loops[2](AEnv(), resets={1: (1, 2)})
    assert _ring_state(ring) == before and sb.log == []


# ------------------------------------------------------------------------------------------------------------------------
# SwarmBatch.reset_envs: argument checks and bookkeeping
# ------------------------------------------------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def _hostless_batch(E=4, S=3):
    torch = pytest.importorskip("torch")
    from marl_llm_amd.batched import SwarmBatch
    sb = object.__new__(SwarmBatch)
    sb.handle, sb.lib = None, _NoLibrary()
    sb.n_env, sb.n_shapes, sb.device = E, S, torch.device("cuda", 0)
    sb.shape_in_force, sb.shape_env_in_force, sb._posed_env = -1, None, None
    return sb


@pytest.mark.parametrize("episode", [[0, 1, 2], [[0, 1, 2, 3]], [0.0, 1.0, -1.0, 2.0], np.zeros(4, np.float32), 3,
                                     np.array([0, 1, 2 ** 63, 0], np.uint64)])
def test_reset_envs_argument_errors_raise_before_the_library_is_called(episode):
    sb = _hostless_batch()
    with pytest.raises(ValueError):
        sb.reset_envs(5, episode)


def test_reset_envs_checked_vector_and_bookkeeping():
    sb = _hostless_batch()
    a = sb._episode_args([3, -1, 0, 2 ** 40])
    assert a.dtype == np.int64 and a.flags.c_contiguous and a.tolist() == [3, -1, 0, 2 ** 40]
    assert sb._episode_args(np.array([1, 0, 1, 0], np.int32)).dtype == np.int64
    sb._note_shapes(np.array([1, 1, 1, 1], np.int32), False)
    assert sb.shape_in_force == 1
    sb._note_reset_envs(np.array([-1, -1, -1, -1]))               # nobody reset: nothing changes
    assert sb.shape_in_force == 1 and sb.shape_env_in_force.tolist() == [1, 1, 1, 1] and not sb._posed_env.any()
    sb._note_reset_envs(np.array([-1, 4, -1, 0]))                 # reset envs: unknown shape, posed
    assert sb.shape_in_force == -1 and sb.shape_env_in_force.tolist() == [1, -1, 1, -1]
    assert sb._posed_env.tolist() == [False, True, False, True]
    sb._note_reset_envs(np.array([0, -1, 0, -1]))                 # now nobody's shape is known
    assert sb.shape_env_in_force is None and sb._posed_env is None and sb.shape_in_force == -1
    sb._note_shapes(np.array([2, 2, 2, 2], np.int32), False)
    sb._note_reset_envs(None)                                     # a device vector: everything unknown
    assert sb.shape_env_in_force is None and sb._posed_env is None and sb.shape_in_force == -1


# ------------------------------------------------------------------------------------------------------------------------
# binding
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def test_reset_envs_is_declared_bound_and_exported(lib):
    from marl_llm_amd import _lib
    from marl_llm_amd.batched import SwarmBatch
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+swarm_reset_envs\s*\(\s*swarm_env_t\s*\*\s*h\s*,\s*uint64_t\s+seed\s*,\s*const\s+int64_t\s*\*\s*episode\s*,"
                     r"\s*int64_t\s+env_offset\s*,\s*void\s*\*\s*obs\s*\)", src)
    assert "swarm_reset_envs" in _lib.BATCHED_SYMBOLS and hasattr(lib, "swarm_reset_envs")
    assert lib.swarm_reset_envs.argtypes == [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert callable(getattr(SwarmBatch, "reset_envs", None))
    ep = (ctypes.c_int64 * 4)(0, -1, 2, 0)
    assert lib.swarm_reset_envs(None, 1, ctypes.cast(ep, ctypes.c_void_p), 0, None) == 1      # SWARM_ERR_INVALID
    assert lib.swarm_reset_envs(None, 1, None, 0, None) == 1


def test_abi_version_is_still_5(lib):
    from marl_llm_amd import _lib
    assert _lib.ABI_VERSION == 5 and lib.swarm_abi_version() == 5
    assert re.search(r"#define\s+SWARM_ABI_VERSION\s+5\b", open(HEADER).read())
