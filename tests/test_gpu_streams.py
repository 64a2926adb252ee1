"""The stream contract of the three headers (DESIGN.md "Stream contract"): every entry point enqueues on the handle's stream
(swarm_set_stream; SwarmBatch hands it torch's current stream), the blocking readers wait for that stream, and the calls
documented as enqueue-only do not wait.

Method.  Two handles of one configuration.  `ref` runs a sequence on the default stream with a device synchronisation after
every call.  `dut` runs the same sequence with a torch pool stream current (non-blocking: no implicit ordering against the
null stream).  Both are first brought, on the default stream, to the same valid synchronised state A, with one warm-up call
of every entry point of the case (every lazy allocation and hipFuncSetAttribute happens there).  Then the side stream gets
a delay (torch.cuda._sleep, DELAY_MS) with a guard event recorded right behind it, and sequence B -- other cells, another
state, other actions; device inputs rewritten in place behind the delay -- is enqueued behind the guard.  Work that went to
another stream, or a readback that did not wait, therefore computes on A (valid memory, wrong numbers), and everything is
compared bit for bit with `ref`, whose B outputs are asserted to differ from its A outputs.

The guard is a condition: where the hazard is armed (before the first blocking call of a delayed stretch) guard.query() must
be False, else the case fails with "delay too short".  After every call documented as enqueue-only the same query is the
no-synchronisation assertion.  Delayed.host_ms collects the host time from a delay's enqueue to its last guard check; the
module prints the largest (DESIGN.md quotes it).

Mutants (scratch libraries, each run once against this file on an MI355X; each computes on state A instead of B) and the
tests that failed under them are listed in DESIGN.md "Stream contract".
"""
import contextlib
import ctypes
import time

import numpy as np
import pytest

from helpers import ThreadedOracle, as_obs_dtype

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DELAY_MS = 150.0
NO_LATTICE, SERIAL = 2, 16                       # debug_flags bits 1 and 4
GEOS = [(8, 9), (64, 4)]                         # (N, E): Geo<8> with a partial last workgroup; the bench geometry
GEO_IDS = ["n8_e9", "n64_e4"]


# ------------------------------------------------------------------------------------------------------------------------
# the delay and the two ways of running a sequence
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond, measured once with two events (as torch's own stream tests do)."""
    from marl_llm_amd import _lib
    _lib.load().hipGetLastError()                # clear what earlier tests of this process left (it returns and resets)
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 50_000_000
    a.record(); torch.cuda._sleep(n); b.record(); b.synchronize()
    cpm = n / a.elapsed_time(b)
    yield cpm
    worst = max(Delayed.host_ms.items(), key=lambda kv: kv[1], default=("none", 0.0))
    print(f"\n[streams] cycles/ms {cpm:.0f}, delay {DELAY_MS:.0f} ms, delays {Delayed.n_delays}, "
          f"largest host time before a guard check {worst[1]:.2f} ms ({worst[0]})")


class Serial:
    """ref: the default stream, a device synchronisation after every call."""
    def stream(self):
        return contextlib.nullcontext()

    def delay(self, what=""):
        torch.cuda.synchronize()

    def enqueued(self, what):
        torch.cuda.synchronize()

    def armed(self, what):
        torch.cuda.synchronize()

    def done(self, checked=True):
        torch.cuda.synchronize()


class Delayed:
    """dut: a side stream; delay() puts DELAY_MS of sleep and a guard event on it."""
    host_ms = {}            # case -> largest host time (ms) from a delay's enqueue to a guard check
    n_delays = 0

    def __init__(self, cpm, case, stream=None):
        self.cpm, self.case = cpm, case
        self.s = stream if stream is not None else torch.cuda.Stream()
        self.guard, self.t0, self.checks = None, None, 0

    def stream(self):
        return torch.cuda.stream(self.s)

    def delay(self, what=""):
        """A new stretch: nothing of the previous one may still be unchecked."""
        assert self.guard is None or self.checks > 0, f"{self.case}: a delayed stretch ended without a guard check"
        self.t0 = time.perf_counter()
        with torch.cuda.stream(self.s):
            torch.cuda._sleep(int(DELAY_MS * self.cpm))
            self.guard = torch.cuda.Event()
            self.guard.record(self.s)
        self.checks = 0
        Delayed.n_delays += 1

    def _check(self, msg):
        running = not self.guard.query()
        ms = (time.perf_counter() - self.t0) * 1e3
        Delayed.host_ms[self.case] = max(Delayed.host_ms.get(self.case, 0.0), ms)
        self.checks += 1
        assert running, f"{self.case}: {msg} ({ms:.1f} ms after the delay of {DELAY_MS:.0f} ms was enqueued)"

    def enqueued(self, what):
        """After a call documented as enqueue-only: the delay in front of it is still running."""
        self._check(f"{what} waited for the stream, or the delay is too short")

    def armed(self, what):
        """Before a blocking call: the hazard is armed only while the delay is still running."""
        self._check(f"delay too short before {what}")

    def done(self, checked=True):
        assert not checked or self.checks > 0, f"{self.case}: no guard check"
        self.s.synchronize()
        self.guard = None


def _modes(cpm, case):
    return Serial(), Delayed(cpm, case)


# ------------------------------------------------------------------------------------------------------------------------
# inputs: state A and state B of one (N, E, path)
# ------------------------------------------------------------------------------------------------------------------------
def _ng_max(shapes):
    return max(np.asarray(g).shape[0] for g in shapes["grid_coords"])


def _inputs(shapes, n_a, n_env, path, seed):
    """A synthetic batch, agents on the shape (rewards of 1 occur); path "mixed": the last env's cells are jittered off the
    lattice, so its workgroup goes to the generic launch and the others walk."""
    from marl_llm_amd.synth import synthetic_batch
    sy = synthetic_batch(n_env, n_a, shapes, seed=seed, assembled_fraction=1.0)
    if path == "mixed":
        e, n = n_env - 1, int(sy["n_g"][n_env - 1])
        sy["cells"][e, :, :n] += np.random.default_rng(seed).normal(0, 0.004, (2, n))
    rng = np.random.default_rng([seed, n_a, n_env])
    sy["act"] = rng.uniform(-1, 1, (4, n_env, n_a, 2)).astype(np.float32)
    return sy


def _mixed_shape_set():
    """Two tiled shapes and a jittered copy of a third (shape index 2), as test_gpu_mixed_paths.py's."""
    from marl_llm_amd.shapes import SHAPE_NAMES, synthetic_shape_set
    s = synthetic_shape_set(SHAPE_NAMES[:3])
    g = np.asarray(s["grid_coords"][2], np.float64)
    s["grid_coords"][2] = g + np.random.default_rng(12).normal(0, 0.004, g.shape)
    return s


def _flags(path):
    return {"lattice": 0, "generic": NO_LATTICE, "mixed": 0, "mixed_serial": SERIAL}[path]


def _make(shapes, n_a, n_env, path, dtype=None, **kw):
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.shapes import r_avoid_for
    return SwarmBatch(n_env=n_env, n_agents=n_a, n_cells_max=_ng_max(shapes), r_avoid=r_avoid_for(n_a, shapes),
                      obs_dtype=dtype or torch.float32, debug_flags=_flags(path), **kw)


class Bufs:
    """Device tensors that hold the A values first and are rewritten in place, on the current stream, with the B values."""

    def __init__(self, A, B, dev):
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        self.A = {k: t(A[k]) for k in ("cells", "p", "dp", "act")}
        self.B = {k: t(B[k]) for k in ("cells", "p", "dp", "act")}
        self.cells, self.p, self.dp, self.act = [self.A[k].clone() for k in ("cells", "p", "dp", "act")]

    def put(self, which, *keys):
        for k in keys:
            getattr(self, k).copy_(getattr(self, which)[k])


def _state_a(sb, bufs, A):
    """Cells, state and one observe of A on the default stream."""
    bufs.put("A", "cells", "p", "dp", "act")
    sb.set_cells(bufs.cells, A["n_g"], A["l_cell"])
    sb.set_state(bufs.p, bufs.dp)
    return sb.observe().clone()


def _expect_paths(sb, path, n_a, n_env):
    epb = 64 // max(8, n_a) if n_a < 64 else 1
    want = {"lattice": (n_env, 0), "generic": (0, n_env)}.get(path)
    if want is None:                                                        # the last env's workgroup scans
        tail = n_env - ((n_env - 1) // epb) * epb
        want = (n_env - tail, tail)
    assert sb.path_envs() == want, (path, sb.path_envs(), want)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and torch.equal(a, b)
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _assert_equal(got, ref, case):
    assert got.keys() == ref.keys(), case
    for k in ref:
        assert _same(got[k], ref[k]), f"{case}: {k} differs from the default-stream run"


def _assert_moved(ref_b, ref_a, keys, case):
    for k in keys:
        assert not _same(ref_b[k], ref_a[k]), f"{case}: {k} of B equals A's -- a stale read would pass"


def _peek(lib):
    return int(lib.hipPeekAtLastError())


# ------------------------------------------------------------------------------------------------------------------------
# 1. the core sequence, per path and geometry
# ------------------------------------------------------------------------------------------------------------------------
def _core_warm(sb, bufs, A):
    """State A with one call of every entry point of the core sequence; returns A's outputs."""
    r = {"obs0": _state_a(sb, bufs, A)}
    for k, v in zip(("obs1", "rew1", "done1", "pri1"), sb.step(bufs.act[0])):
        r[k] = v.clone()
    r["metrics"], r["rule"] = sb.metrics(), sb.rule_action()
    r["p"], r["dp"] = sb.get_state()
    r["cells"], r["n_g"] = sb.get_cells()
    r.update(sb.indices())
    sb.path_envs()
    _state_a(sb, bufs, A)
    torch.cuda.synchronize()
    return r


def _core_b(sb, m, bufs, B):
    r = {}
    with m.stream():
        m.delay()
        bufs.put("B", "cells")
        m.armed("set_cells")
        sb.set_cells(bufs.cells, B["n_g"], B["l_cell"])                     # waits: lattice detection reads the cells back
        m.delay()
        bufs.put("B", "p", "dp")
        m.armed("set_state")
        sb.set_state(bufs.p, bufs.dp)                                       # waits
        m.delay()
        bufs.put("B", "act")
        r["obs0"] = sb.observe().clone(); m.enqueued("swarm_observe")
        for t in range(3):
            for k, v in zip(("obs", "rew", "done", "pri"), sb.step(bufs.act[t])):
                r[f"{k}{t + 1}"] = v.clone()
            m.enqueued("swarm_step")
        r["metrics"] = sb.metrics(); m.enqueued("swarm_metrics")
        r["rule"] = sb.rule_action(); m.enqueued("swarm_rule_action")
        m.armed("get_state")
        r["p"], r["dp"] = sb.get_state()
        m.delay()
        sb.step(bufs.act[3]); m.enqueued("swarm_step")
        m.armed("indices")
        r.update(sb.indices())
        r["cells"], r["n_g"] = sb.get_cells()
        r["paths"] = np.array(sb.path_envs())
        r["p_end"], r["dp_end"] = sb.get_state()
        m.done()
    return r


CORE_PATHS = ["lattice", "generic", "mixed", "mixed_serial"]


@pytest.mark.parametrize("path", CORE_PATHS)
@pytest.mark.parametrize("n_a,n_env", GEOS, ids=GEO_IDS)
def test_core_sequence(shapes, oracle, cycles_per_ms, n_a, n_env, path):
    case = f"core {path} n{n_a}_e{n_env}"
    kind = "mixed" if path.startswith("mixed") else path
    A, B = _inputs(shapes, n_a, n_env, kind, 1), _inputs(shapes, n_a, n_env, kind, 2)
    ref, dut = _make(shapes, n_a, n_env, path), _make(shapes, n_a, n_env, path)
    try:
        bufs_r, bufs_d = Bufs(A, B, ref.device), Bufs(A, B, dut.device)
        a_ref = _core_warm(ref, bufs_r, A)
        _core_warm(dut, bufs_d, A)
        _expect_paths(ref, kind, n_a, n_env); _expect_paths(dut, kind, n_a, n_env)
        m_ref, m_dut = _modes(cycles_per_ms, case)
        want = _core_b(ref, m_ref, bufs_r, B)
        got = _core_b(dut, m_dut, bufs_d, B)
        _assert_equal(got, want, case)
        _assert_moved(want, a_ref, ("obs0", "obs1", "rew1", "pri1", "metrics", "rule", "p", "dp", "cells", "sensed_index"), case)
        assert _peek(dut.lib) == 0
        if path == "lattice" and n_a == 64:                                 # the twin itself, once, against the oracle
            from marl_llm_amd.shapes import r_avoid_for
            with ThreadedOracle(oracle, B["cells"], B["n_g"], B["l_cell"], r_avoid_for(n_a, shapes)) as to:
                first = to.observe(B["p"], B["dp"])
                o = to.step(B["p"], B["dp"], np.swapaxes(B["act"][0], 1, 2).astype(np.float64), first["neighbor_index"])
            f32 = lambda x: as_obs_dtype(np.ascontiguousarray(np.swapaxes(x, 1, 2)), "f32")
            assert np.array_equal(want["obs0"].cpu().numpy(), f32(first["obs"]))
            assert np.array_equal(want["obs1"].cpu().numpy(), f32(o["obs"]))
            assert np.array_equal(want["pri1"].cpu().numpy(), f32(o["a_prior"]))
            assert np.array_equal(want["rew1"].cpu().numpy().astype(np.float64), o["reward"])
    finally:
        ref.close(); dut.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. device reset and shape switch; the blocking readers of cells, shape index and path
# ------------------------------------------------------------------------------------------------------------------------
def _mixed_episode(sb, seed):
    """An episode whose draw from the mixed shape set leaves workgroups of both kinds (default stream)."""
    for ep in range(32):
        sb.reset(seed, ep)
        if 0 < sb.path_envs()[0] < sb.n_env:
            return ep
    raise AssertionError("no episode of thirty-two left a mixed batch")


_PINNED = []


def _pinned_get_cells(sb):
    """swarm_get_cells into pinned host memory (a truly asynchronous copy: only the call's own wait makes it complete)."""
    cells = torch.full((sb.n_env, 2, sb.n_cells_max), float("nan"), dtype=torch.float64).pin_memory()
    n_g = torch.full((sb.n_env,), -7, dtype=torch.int32).pin_memory()
    _PINNED.append((cells, n_g))                   # never handed back to the allocator while a copy could be pending
    sb._sync_stream()
    assert sb.lib.swarm_get_cells(sb.handle, ctypes.c_void_p(cells.data_ptr()), ctypes.c_void_p(n_g.data_ptr())) == 0
    return cells.numpy().copy(), n_g.numpy().copy()


def _reset_b(sb, m, bufs, ep):
    r = {}
    E, N, D = sb.n_env, sb.n_agents, sb.obs_dim
    slot = torch.zeros((E * N, D), dtype=sb.obs_dtype, device=sb.device)            # a ring slot: caller-owned obs rows
    with m.stream():
        m.delay()
        bufs.put("B", "act")
        sb.reset(55, ep, 3, out=slot); m.enqueued("swarm_reset")
        for k, v in zip(("obs", "rew", "done", "pri"), sb.step(bufs.act[0])):
            r[k + "_reset"] = v.clone()
        m.enqueued("swarm_step")
        m.armed("get_shape_index")
        r["shape_index"] = sb.get_shape_index()
        r["slot"] = slot.clone()
        r["paths_reset"] = np.array(sb.path_envs())
        m.delay()
        r["obs_sel"] = sb.select_shape(1).clone(); m.enqueued("swarm_select_shape")
        m.armed("get_cells")
        r["cells_sel"], r["n_g_sel"] = sb.get_cells()
        m.delay()
        r["obs_sel2"] = sb.select_shape(0).clone(); m.enqueued("swarm_select_shape")
        for k, v in zip(("obs", "rew", "done", "pri"), sb.step(bufs.act[1])):
            r[k + "_sel"] = v.clone()
        m.enqueued("swarm_step")
        m.armed("swarm_get_cells (pinned)")
        r["cells_pin"], r["n_g_pin"] = _pinned_get_cells(sb)
        m.delay()
        sb.reset(55, ep, 0); m.enqueued("swarm_reset")
        m.armed("path_envs")
        r["paths_end"] = np.array(sb.path_envs())
        r["shape_index_end"] = sb.get_shape_index()
        r["p"], r["dp"] = sb.get_state()
        m.done()
    return r


@pytest.mark.parametrize("n_a,n_env", GEOS, ids=GEO_IDS)
def test_reset_and_shape_switch(shapes, cycles_per_ms, n_a, n_env):
    case = f"reset n{n_a}_e{n_env}"
    s3 = _mixed_shape_set()
    A, B = _inputs(shapes, n_a, n_env, "lattice", 3), _inputs(shapes, n_a, n_env, "lattice", 4)
    ref, dut = _make(shapes, n_a, n_env, "mixed"), _make(shapes, n_a, n_env, "mixed")
    try:
        bufs = {}
        for sb in (ref, dut):
            sb.set_shapes(s3)
            bufs[sb] = Bufs(A, B, sb.device)
            _state_a(sb, bufs[sb], A)
        ep = _mixed_episode(ref, 55)
        a_out = {}
        for sb in (ref, dut):                                   # warm-up: every entry point of the case, then state A again
            sb.reset(55, ep, 3); sb.step(bufs[sb].act[0]); sb.select_shape(1); sb.select_shape(2); sb.step(bufs[sb].act[0])
            sb.get_cells(); _pinned_get_cells(sb); sb.get_shape_index(); sb.path_envs()
            a_out[sb] = dict(slot=_state_a(sb, bufs[sb], A).reshape(n_env * n_a, -1), shape_index=sb.get_shape_index())
            a_out[sb]["cells_sel"], _ = sb.get_cells()
            a_out[sb]["cells_pin"] = a_out[sb]["cells_sel"]
            a_out[sb]["p"], a_out[sb]["dp"] = sb.get_state()
            assert sb.path_envs() == (n_env, 0)
        torch.cuda.synchronize()
        m_ref, m_dut = _modes(cycles_per_ms, case)
        want = _reset_b(ref, m_ref, bufs[ref], ep)
        got = _reset_b(dut, m_dut, bufs[dut], ep)
        _assert_equal(got, want, case)
        _assert_moved(want, a_out[ref], ("slot", "shape_index", "cells_sel", "cells_pin", "p", "dp"), case)
        assert 0 < want["paths_end"][0] < n_env                              # the last reset left a mixed batch
        assert not np.array_equal(want["cells_pin"], want["cells_sel"])
        assert _peek(dut.lib) == 0
    finally:
        ref.close(); dut.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. the host path: swarm_observe_host / swarm_step_host / swarm_get_llm_action
# ------------------------------------------------------------------------------------------------------------------------
def _host_b(sb, m, bufs, a_host):
    r = {}
    keep = lambda d, tag: r.update({f"{tag}_{k}": v.copy() for k, v in d.items()})
    with m.stream():
        m.delay()
        bufs.put("B", "act")
        sb.step(bufs.act[3]); m.enqueued("swarm_step")
        m.armed("observe_host")
        r["obs_host"] = sb.observe_host().copy()
        m.delay()
        sb.step(bufs.act[0]); m.enqueued("swarm_step")
        m.armed("step_host(numpy)")
        keep(sb.step_host(a_host), "np")
        m.delay()
        sb.step(bufs.act[1]); m.enqueued("swarm_step")
        m.armed("step_host(device)")
        keep(sb.step_host(bufs.act[2]), "dev")
        m.delay()
        sb.step(bufs.act[3]); m.enqueued("swarm_step")
        m.armed("step_host(None)")
        keep(sb.step_host(None), "llm")
        m.delay()
        sb.step(bufs.act[0]); m.enqueued("swarm_step")
        m.armed("llm_action")
        r["llm_action"] = sb.llm_action()
        r["p"], r["dp"] = sb.get_state()
        m.done()
    return r


@pytest.mark.parametrize("n_a,n_env,path", [(8, 9, "lattice"), (64, 4, "mixed")], ids=["n8_e9_lattice", "n64_e4_mixed"])
def test_host_path(shapes, cycles_per_ms, n_a, n_env, path):
    case = f"host {path} n{n_a}_e{n_env}"
    A, B = _inputs(shapes, n_a, n_env, path, 5), _inputs(shapes, n_a, n_env, path, 6)
    a_host = np.random.default_rng(9).uniform(-1, 1, (2, n_env * n_a))
    ref, dut = [_make(shapes, n_a, n_env, path, llm_action=True) for _ in range(2)]
    try:
        bufs, a_out = {}, {}
        for sb in (ref, dut):
            bufs[sb] = Bufs(A, B, sb.device)
            _state_a(sb, bufs[sb], A)
            sb.step(bufs[sb].act[0]); sb.observe_host(); sb.step_host(a_host); sb.step_host(bufs[sb].act[0]); sb.step_host(None); sb.llm_action()
            _state_a(sb, bufs[sb], A)
            a_out[sb] = {"obs_host": sb.observe_host().copy(), "llm_action": sb.llm_action()}
            _state_a(sb, bufs[sb], A)
        _expect_paths(ref, path, n_a, n_env)
        torch.cuda.synchronize()
        m_ref, m_dut = _modes(cycles_per_ms, case)
        want = _host_b(ref, m_ref, bufs[ref], a_host)
        got = _host_b(dut, m_dut, bufs[dut], a_host)
        _assert_equal(got, want, case)
        _assert_moved(want, a_out[ref], ("obs_host", "llm_action"), case)
        assert not np.array_equal(want["np_obs"], want["dev_obs"]) and not np.array_equal(want["dev_obs"], want["llm_obs"])
        _expect_paths(dut, path, n_a, n_env)
        assert _peek(dut.lib) == 0
    finally:
        ref.close(); dut.close()


# ------------------------------------------------------------------------------------------------------------------------
# 4. the policy forwards
# ------------------------------------------------------------------------------------------------------------------------
def _module(obs_dim, seed=0, device="cuda:0"):
    from marl_llm_amd.rollout import PolicyMLP
    torch.manual_seed(seed)
    return PolicyMLP(obs_dim, 2, 180).to(device)


def _policy_b(pol, m, x32, x16, b32):
    r = {}
    with m.stream():
        m.delay()
        x32.copy_(b32); x16.copy_(b32.to(torch.bfloat16))
        r["noise"] = pol(x32, noise_scale=0.3, seed=5, step=2); m.enqueued("swarm_policy_forward_explore_at")
        r["act_lp"], r["lp"] = pol(x32, noise_scale=0.3, seed=5, step=3, log_pi=True); m.enqueued("swarm_policy_forward_explore_logpi")
        r["bf16"] = pol(x16); m.enqueued("swarm_policy_forward_explore_at (bf16 rows)")
        m.done()
    return r


def test_policy_forwards(cycles_per_ms):
    from marl_llm_amd.rollout import FusedPolicy
    dev = torch.device("cuda:0")
    rows, D = 8 * 9 + 5, 192                                    # more than one 32-row tile, not a multiple of it
    gen = torch.Generator(device=dev).manual_seed(1)
    a32, b32 = [torch.rand((rows, D), device=dev, generator=gen) * 2 - 1 for _ in range(2)]
    module = _module(D)
    pols = [FusedPolicy(module, device=dev) for _ in range(2)]
    try:
        res, a_out = [], None
        for pol, m in zip(pols, _modes(cycles_per_ms, "policy")):
            x32, x16 = a32.clone(), a32.to(torch.bfloat16)
            warm = dict(noise=pol(x32, noise_scale=0.3, seed=5, step=2), bf16=pol(x16))
            warm["act_lp"], warm["lp"] = pol(x32, noise_scale=0.3, seed=5, step=3, log_pi=True)
            torch.cuda.synchronize()
            a_out = a_out or warm
            res.append(_policy_b(pol, m, x32, x16, b32))
        _assert_equal(res[1], res[0], "policy")
        _assert_moved(res[0], a_out, ("noise", "act_lp", "bf16"), "policy")      # (lp is a function of the noise alone)
    finally:
        for p in pols:
            p.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. the rollout loops
# ------------------------------------------------------------------------------------------------------------------------
def _ring_dict(ring, tag=""):
    r = {tag + k: getattr(ring, k).clone() for k in ("obs", "act", "rew", "done", "act_prior")}
    if ring.log_pi is not None:
        r[tag + "log_pi"] = ring.log_pi.clone()
    return r


def _loops_b(sb, pol, m, ring, obs_buf, obs_b):
    from marl_llm_amd.rollout import rollout, rollout_device, rollout_eval, rollout_expert
    E, N, D = sb.n_env, sb.n_agents, sb.obs_dim
    r = {}
    with m.stream():
        m.delay()
        obs_buf.copy_(obs_b)
        ring.new_chain(obs_buf)                                  # the chain starts from the rows rewritten behind the delay
        o, r["rew_fused"] = rollout(sb, pol, 4, obs_buf, replay=ring, noise_scale=0.2, seed=3, log_pi=True); m.enqueued("rollout (fused)")
        o, r["st_eps"] = rollout_device(sb, pol, 4, obs=o, replay=ring, noise_scale=0.2, epsilon=0.5, host_rng=np.random.default_rng(7),
                                        seed=4, log_pi=True); m.enqueued("swarm_rollout_logpi")
        o, r["st_dev"] = rollout_device(sb, pol, 2, obs=o, replay=ring, noise_scale=0.2, seed=5); m.enqueued("swarm_rollout")
        o, r["st_reset"] = rollout_device(sb, pol, 2, replay=ring, noise_scale=0.2, seed=6, reset=(21, 1)); m.enqueued("swarm_rollout after swarm_reset")
        o, r["st_rule"] = rollout_expert(sb, 4, obs=o, replay=ring, source="rule"); m.enqueued("swarm_rollout_expert (rule)")
        o, r["st_llm"] = rollout_expert(sb, 4, obs=o, replay=ring, source="llm"); m.enqueued("swarm_rollout_expert (llm)")
        o, tr = rollout_eval(sb, pol, 4, obs=o, replay=ring, switch={2: 1}, trace_state=True); m.enqueued("swarm_rollout_eval")
        r.update(obs_last=o.clone(), ev_metrics=tr.metrics, ev_p=tr.p, ev_dp=tr.dp, ev_stats=tr.reward_stats, ev_shape=tr.shape)
        r.update(_ring_dict(ring))
        m.armed("get_state")
        r["p"], r["dp"] = sb.get_state()
        m.done()
    r["cur"] = np.array([ring.cur, ring.count])
    return r


@pytest.mark.parametrize("n_a,n_env,path", [(8, 9, "lattice"), (64, 4, "mixed")], ids=["n8_e9_lattice", "n64_e4_mixed"])
def test_rollout_loops(shapes, cycles_per_ms, n_a, n_env, path):
    from marl_llm_amd.rollout import ChainedReplay, FusedPolicy, rollout, rollout_device, rollout_eval, rollout_expert
    case = f"loops {path} n{n_a}_e{n_env}"
    s3 = _mixed_shape_set()
    A, B = _inputs(shapes, n_a, n_env, path, 7), _inputs(shapes, n_a, n_env, path, 8)
    ref, dut = [_make(shapes, n_a, n_env, path, llm_action=True) for _ in range(2)]
    module = _module(ref.obs_dim)
    pols = [FusedPolicy(module, device=ref.device) for _ in range(2)]
    try:
        res, a_out = [], None
        for sb, pol, m in zip((ref, dut), pols, _modes(cycles_per_ms, case)):
            sb.set_shapes(s3)
            bufs = Bufs(A, B, sb.device)
            ring = ChainedReplay(40, n_env * n_a, sb.obs_dim, 2, sb.device, log_pi=True)
            obs_a = _state_a(sb, bufs, A)
            obs_buf = obs_a.clone()
            o, _ = rollout(sb, pol, 1, obs_buf, replay=ring, noise_scale=0.2, seed=3, log_pi=True)          # warm-up of every loop
            o, _ = rollout_device(sb, pol, 1, obs=o, replay=ring, noise_scale=0.2, epsilon=0.5, host_rng=np.random.default_rng(1), log_pi=True)
            o, _ = rollout_device(sb, pol, 1, replay=ring, reset=(21, 0))
            o, _ = rollout_expert(sb, 1, obs=o, replay=ring, source="rule")
            o, _ = rollout_expert(sb, 1, obs=o, replay=ring, source="llm")
            o, _ = rollout_eval(sb, pol, 2, obs=o, replay=ring, switch={1: 1}, trace_state=True)
            obs_b = o.clone()                                    # B's first observation: any other valid rows
            _state_a(sb, bufs, A)
            if a_out is None:
                a_out = dict(_ring_dict(ring), obs_last=obs_a)
                a_out["p"], a_out["dp"] = sb.get_state()
            torch.cuda.synchronize()
            assert not torch.equal(obs_a, obs_b)
            res.append(_loops_b(sb, pol, m, ring, obs_buf, obs_b))
        want, got = res
        _assert_equal(got, want, case)
        _assert_moved(want, a_out, ("obs", "act", "rew", "act_prior", "log_pi", "obs_last", "p", "dp"), case)
        stats = ("st_eps", "st_dev", "st_reset", "st_rule", "st_llm", "ev_stats")
        assert all(torch.isfinite(want[k]).all() for k in stats)
        assert sum(int((want[k][:, 0] > 0).sum()) for k in stats) >= 6, case          # a reward count that ran early gives 0
        assert want["ev_shape"].tolist() == [-1, -1, 1, 1]
        assert _peek(dut.lib) == 0
    finally:
        for p in pols:
            p.close()
        ref.close(); dut.close()


def test_rollout_device_bf16(shapes, cycles_per_ms):
    from marl_llm_amd.rollout import ChainedReplay, FusedPolicy, rollout_device
    n_a, n_env, case = 8, 9, "loops bf16"
    A, B = _inputs(shapes, n_a, n_env, "lattice", 9), _inputs(shapes, n_a, n_env, "lattice", 10)
    ref, dut = [_make(shapes, n_a, n_env, "lattice", dtype=torch.bfloat16) for _ in range(2)]
    module = _module(ref.obs_dim)
    pols = [FusedPolicy(module, device=ref.device) for _ in range(2)]
    try:
        res, a_ring = [], None
        for sb, pol, m in zip((ref, dut), pols, _modes(cycles_per_ms, case)):
            bufs = Bufs(A, B, sb.device)
            ring = ChainedReplay(8, n_env * n_a, sb.obs_dim, 2, sb.device, obs_dtype=torch.bfloat16)
            obs_buf = _state_a(sb, bufs, A).clone()
            o, _ = rollout_device(sb, pol, 1, obs=obs_buf, replay=ring, noise_scale=0.2)
            obs_b = o.clone()
            _state_a(sb, bufs, A)
            a_ring = a_ring or _ring_dict(ring)
            torch.cuda.synchronize()
            r = {}
            with m.stream():
                m.delay()
                obs_buf.copy_(obs_b)
                o, r["stats"] = rollout_device(sb, pol, 4, obs=obs_buf, replay=ring, noise_scale=0.2, seed=2); m.enqueued("swarm_rollout (bf16)")
                r.update(_ring_dict(ring), obs_last=o.clone())
                m.done()
            res.append(r)
        _assert_equal(res[1], res[0], case)
        _assert_moved(res[0], a_ring, ("obs", "act", "rew", "act_prior"), case)
        assert (res[0]["stats"][:, 0] > 0).any()
    finally:
        for p in pols:
            p.close()
        ref.close(); dut.close()


# ------------------------------------------------------------------------------------------------------------------------
# 6. two handles on two side streams, interleaved from one host thread
# ------------------------------------------------------------------------------------------------------------------------
def _steps_b(sb, m, bufs, r, t):
    """One interleaved slice: a step and one side kernel."""
    with m.stream():
        for k, v in zip(("obs", "rew", "done", "pri"), sb.step(bufs.act[t])):
            r[f"{k}{t}"] = v.clone()
        m.enqueued("swarm_step")
        r[f"side{t}"] = sb.metrics() if t % 2 == 0 else sb.rule_action()
        m.enqueued("swarm_metrics / swarm_rule_action")


def test_two_handles_two_streams(shapes, cycles_per_ms):
    cfgs = [(8, 9, "lattice"), (64, 4, "mixed")]
    handles, bufs, inputs = [], [], []
    try:
        for n_a, n_env, path in cfgs:
            A, B = _inputs(shapes, n_a, n_env, path, 11), _inputs(shapes, n_a, n_env, path, 12)
            for _ in range(2):                                   # ref, dut
                sb = _make(shapes, n_a, n_env, path)
                handles.append(sb); bufs.append(Bufs(A, B, sb.device)); inputs.append(A)
                _core_warm(sb, bufs[-1], A)
        refs, duts = handles[0::2], handles[1::2]
        ms = [Delayed(cycles_per_ms, f"two handles {c[2]}") for c in cfgs]
        got = [{}, {}]
        for m, b in zip(ms, bufs[1::2]):
            m.delay()
            with m.stream():
                b.put("B", "act")
        for t in range(4):
            for sb, m, b, r in zip(duts, ms, bufs[1::2], got):
                _steps_b(sb, m, b, r, t)
        for m in ms:                                             # both armed before either blocking call
            m.armed("get_state")
        for sb, m, r in zip(duts, ms, got):
            with m.stream():
                r["p"], r["dp"] = sb.get_state()
                m.done()
        for k, (sb, b) in enumerate(zip(refs, bufs[0::2])):
            m, want = Serial(), {}
            b.put("B", "act")
            for t in range(4):
                _steps_b(sb, m, b, want, t)
            want["p"], want["dp"] = sb.get_state()
            _assert_equal(got[k], want, f"two handles {cfgs[k][2]}")
            assert not torch.equal(want["obs0"], want["obs1"])
    finally:
        for sb in handles:
            sb.close()


# ------------------------------------------------------------------------------------------------------------------------
# 7. a handle that changes stream
# ------------------------------------------------------------------------------------------------------------------------
def test_handle_changes_stream(shapes, cycles_per_ms):
    n_a, n_env, path, case = 64, 4, "mixed", "stream change"
    A, B = _inputs(shapes, n_a, n_env, path, 13), _inputs(shapes, n_a, n_env, path, 14)
    ref, dut = _make(shapes, n_a, n_env, path), _make(shapes, n_a, n_env, path)
    try:
        bufs_r, bufs_d = Bufs(A, B, ref.device), Bufs(A, B, dut.device)
        _core_warm(ref, bufs_r, A); _core_warm(dut, bufs_d, A)
        _expect_paths(dut, path, n_a, n_env)
        want, got = {}, {}
        bufs_r.put("B", "act")
        for t in range(4):
            _steps_b(ref, Serial(), bufs_r, want, t)
        want["p"], want["dp"] = ref.get_state()
        m1, m2 = Delayed(cycles_per_ms, case + " s1"), Delayed(cycles_per_ms, case + " s2")
        m1.delay()
        with m1.stream():
            bufs_d.put("B", "act")
        for t in (0, 1):
            _steps_b(dut, m1, bufs_d, got, t)
        m2.s.wait_stream(m1.s)
        m2.delay()
        for t in (2, 3):
            _steps_b(dut, m2, bufs_d, got, t)                    # the auxiliary stream and its events are reused on s2
        with m2.stream():
            m2.armed("get_state")
            got["p"], got["dp"] = dut.get_state()
        m1.done(); m2.done()
        _assert_equal(got, want, case)
        assert _peek(dut.lib) == 0
    finally:
        ref.close(); dut.close()


# ------------------------------------------------------------------------------------------------------------------------
# 8. first use on a side stream: the lazy allocations happen under the delay (results only)
# ------------------------------------------------------------------------------------------------------------------------
def _first_use(sb, pol, m, act, a_host):
    from marl_llm_amd.rollout import rollout_device
    r = {}
    with m.stream():
        m.delay()
        r["obs0"] = sb.observe().clone()
        for k, v in zip(("obs", "rew", "done", "pri"), sb.step(act)):       # a mixed step: the auxiliary stream and its events
            r[k] = v.clone()
        r["rule"] = sb.rule_action()                                         # the export lists
        o, r["stats"] = rollout_device(sb, pol, 2, obs=r["obs"], noise_scale=0.1, seed=1)        # the private two-slot ring
        r["obs_last"] = o.clone()
        r["obs_host"] = sb.observe_host().copy()                             # the host block and its pinned slots
        for k, v in sb.step_host(a_host).items():
            r["host_" + k] = v.copy()
        r.update(sb.indices())
        r["p"], r["dp"] = sb.get_state()
        m.done(checked=False)
    return r


def test_first_use_on_a_side_stream(shapes, cycles_per_ms):
    from marl_llm_amd.rollout import FusedPolicy
    n_a, n_env, path, case = 64, 4, "mixed", "first use"
    A = _inputs(shapes, n_a, n_env, path, 15)
    a_host = np.random.default_rng(3).uniform(-1, 1, (2, n_env * n_a))
    res = []
    for m in _modes(cycles_per_ms, case):
        sb = _make(shapes, n_a, n_env, path)
        pol = FusedPolicy(_module(sb.obs_dim), device=sb.device)
        try:
            sb.set_cells(A["cells"], A["n_g"], A["l_cell"])                  # state A through the plain calls only
            sb.set_state(A["p"], A["dp"])
            act = torch.from_numpy(A["act"][0]).to(sb.device)
            torch.cuda.synchronize()
            res.append(_first_use(sb, pol, m, act, a_host))
            assert _peek(sb.lib) == 0
        finally:
            pol.close(); sb.close()
    _assert_equal(res[1], res[0], case)
    assert torch.isfinite(res[0]["obs"]).all() and (res[0]["sensed_index"] >= 0).any()


# ------------------------------------------------------------------------------------------------------------------------
# 9. lifetime behind pending work
# ------------------------------------------------------------------------------------------------------------------------
def test_close_behind_a_pending_step(shapes, cycles_per_ms):
    """swarm_destroy waits for the handle's stream (and the auxiliary one): the step's caller-owned outputs are complete."""
    n_a, n_env, path, case = 64, 4, "mixed", "close"
    A, B = _inputs(shapes, n_a, n_env, path, 16), _inputs(shapes, n_a, n_env, path, 17)
    res = []
    for m in _modes(cycles_per_ms, case):
        sb = _make(shapes, n_a, n_env, path)
        try:
            bufs = Bufs(A, B, sb.device)
            _core_warm(sb, bufs, A)
            E, N, D = sb.n_env, sb.n_agents, sb.obs_dim
            out = dict(obs=torch.zeros((E, N, D), device=sb.device), rew=torch.full((E, N), -1.0, device=sb.device),
                       done=torch.full((E, N), 255, dtype=torch.uint8, device=sb.device), prior=torch.zeros((E, N, 2), device=sb.device))
            torch.cuda.synchronize()
            with m.stream():
                m.delay()
                bufs.put("B", "act")
                sb.step(bufs.act[0], out=out); m.enqueued("swarm_step")
                m.armed("close")
                sb.close()
                res.append({k: v.cpu() for k, v in out.items()})            # right after close(): the stream is already drained
                m.done()
            assert _peek(sb.lib) == 0
        finally:
            sb.close()
    _assert_equal(res[1], res[0], case)
    assert (res[0]["done"] == 0).all() and (res[0]["rew"] >= 0).all() and res[0]["obs"].abs().sum() > 0


def test_set_shapes_behind_a_pending_reset(shapes, cycles_per_ms):
    """swarm_set_shapes frees the old set (hipFree waits for the device): the pending reset still drew from the old one."""
    from marl_llm_amd.shapes import SHAPE_NAMES, synthetic_shape_set
    n_a, n_env, case = 8, 9, "set_shapes"
    two, other = synthetic_shape_set(SHAPE_NAMES[:2]), synthetic_shape_set(SHAPE_NAMES[3:6])
    A = _inputs(shapes, n_a, n_env, "lattice", 18)
    res = []
    for m in _modes(cycles_per_ms, case):
        sb = _make(shapes, n_a, n_env, "lattice")
        try:
            bufs = Bufs(A, A, sb.device)
            sb.set_shapes(two)
            _state_a(sb, bufs, A)
            sb.reset(1, 0); sb.get_cells(); sb.get_shape_index()
            _state_a(sb, bufs, A)
            torch.cuda.synchronize()
            r = {}
            with m.stream():
                m.delay()
                obs = sb.reset(31, 2); m.enqueued("swarm_reset")
                m.armed("set_shapes")
                sb.set_shapes(other)
                r["obs"] = obs.clone()
                r["shape_index"] = sb.get_shape_index()
                r["cells"], r["n_g"] = sb.get_cells()
                r["obs_new"] = sb.reset(31, 3).clone()
                r["cells_new"], _ = sb.get_cells()
                m.done()
            res.append(r)
            assert _peek(sb.lib) == 0
        finally:
            sb.close()
    _assert_equal(res[1], res[0], case)
    want = res[0]
    grids = [np.asarray(g, np.float64).T for g in two["grid_coords"]]
    for e, s in enumerate(want["shape_index"]):                              # the old set's cells, the old set's indices
        assert s in (0, 1) and want["n_g"][e] == grids[s].shape[1]
    assert not np.array_equal(want["cells"], want["cells_new"])


def test_refresh_behind_a_pending_forward(cycles_per_ms):
    """FusedPolicy.refresh() destroys the old weights' handle behind a pending forward: that forward used the old weights."""
    from marl_llm_amd.rollout import FusedPolicy
    dev = torch.device("cuda:0")
    rows, D = 77, 192
    gen = torch.Generator(device=dev).manual_seed(2)
    a32, b32 = [torch.rand((rows, D), device=dev, generator=gen) * 2 - 1 for _ in range(2)]
    res = []
    for m in _modes(cycles_per_ms, "refresh"):
        module = _module(D, seed=4, device="cpu")                # host weights: refresh() itself makes no device copy that waits
        pol = FusedPolicy(module, device=dev)
        try:
            x = a32.clone()
            pol(x)
            torch.cuda.synchronize()
            r = {}
            with m.stream():
                m.delay()
                x.copy_(b32)
                r["old"] = pol(x); m.enqueued("swarm_policy_forward_explore_at")
                with torch.no_grad():
                    module.fc4.bias += 0.25
                    module.fc1.weight *= 0.5
                m.armed("refresh")
                pol.refresh()
                r["new"] = pol(x)
                m.done()
            res.append(r)
            assert _peek(pol.lib) == 0
        finally:
            pol.close()
    _assert_equal(res[1], res[0], "refresh")
    assert not torch.equal(res[0]["old"], res[0]["new"])
    fresh = FusedPolicy(_module(D, seed=4, device="cpu"), device=dev)        # the old weights, never refreshed
    try:
        assert torch.equal(fresh(b32.clone()), res[0]["old"])
    finally:
        fresh.close()
