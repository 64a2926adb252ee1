"""The per-env device-side shape switch (swarm_select_shapes, SwarmBatch.select_shapes) and rollout_eval's per-env schedule.

The contract is an equivalence, so every comparison is exact: after the call every output of every later call is bit for bit
what it is on a twin batch that was given the same cells through set_cells + observe, where the twin's cells come from numpy
with the header's ELEMENTWISE expression (x = c*sx + s*sy + off_x, y = -s*sx + c*sy + off_y; zeros behind n_g with a pose, the
shape's own row without one).  Kept envs (-1, or any index outside [0, n_shapes)) continue as if nothing had been called.  The
call only enqueues, refuses before it enqueues, and rollout_eval with per-env entries equals the eager loop."""
import ctypes

import numpy as np
import pytest

from helpers import shape_batch
from test_gpu_rollout_eval import RING, shape_arrays
from test_gpu_streams import Delayed, cycles_per_ms          # noqa: F401  (cycles_per_ms is a fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NO_LATTICE = 2                                               # debug_flags bit 1


def jittered(shapes):
    """The set with shape 1 moved off the lattice (as test_gpu_rollout_eval's non-lattice set): its envs take the scan."""
    jit = {k: list(v) for k, v in shapes.items()}
    g = np.array(jit["grid_coords"][1], np.float64)
    jit["grid_coords"][1] = g + np.random.RandomState(0).uniform(-2e-3, 2e-3, g.shape)
    return jit


def posed_cells(shapes, index, pose, current):
    """What select_shapes(index, pose=pose) must leave, from numpy: (cells [E, 2, ng_max], n_g [E], l_cell [E]).  current =
    (cells, n_g, l_cell) of the envs before the call: a kept env's."""
    sc, sn, sl = shape_arrays(shapes)
    cells, n_g, l_cell = [np.array(x) for x in current]
    for e, s in enumerate(index):
        if not 0 <= s < len(sn):
            continue
        n = int(sn[s])
        if pose is None:
            cells[e] = sc[s]
        else:
            c, sn_, ox, oy = pose[e]
            sx, sy = sc[s][0, :n], sc[s][1, :n]
            cells[e] = 0.0
            cells[e, 0, :n] = c * sx + sn_ * sy + ox
            cells[e, 1, :n] = -sn_ * sx + c * sy + oy
        n_g[e], l_cell[e] = n, sl[s]
    return cells, n_g.astype(np.int32), l_cell


def current_of(sb, shapes):
    """(cells, n_g, l_cell) of a batch whose envs all hold a shape of the set (after reset / select_shape)."""
    cells, n_g = sb.get_cells()
    return cells, n_g, np.asarray(shapes["l_cell"], np.float64)[sb.get_shape_index()]


def pair(shapes, E, N, dtype=None, seed=3, start=None, **kw):
    """Two batches in one state: the same device reset, then (start is not None) every env on shape `start`."""
    sb, mb = shape_batch(shapes, E, N, dtype, **kw), shape_batch(shapes, E, N, dtype, **kw)
    for b in (sb, mb):
        b.reset(seed)
        if start is not None:
            b.select_shape(start)
    return sb, mb


def same_handle(sb, mb, shape_index=True):
    c1, g1 = sb.get_cells(); c2, g2 = mb.get_cells()
    assert np.array_equal(c1, c2) and np.array_equal(g1, g2)
    assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), mb.get_state()))
    if shape_index:
        assert np.array_equal(sb.get_shape_index(), mb.get_shape_index())


def lockstep(sb, mb, steps, seed=0, extras=False):
    """`steps` steps of both batches under the same random actions: obs, reward, done, prior and the state equal throughout."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    for t in range(steps):
        act = (torch.rand((sb.n_env, sb.n_agents, 2), generator=g) * 2 - 1).to(sb.device)
        a, b = sb.step(act), mb.step(act)
        for k, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (t, ("obs", "reward", "done", "prior")[k])
        assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), mb.get_state())), t
        if extras:
            ia, ib = sb.indices(), mb.indices()
            assert all(torch.equal(ia[k], ib[k]) for k in ia), t
            ma, mm = sb.metrics().cpu().numpy(), mb.metrics().cpu().numpy()
            assert np.array_equal(ma, mm, equal_nan=True), t


def random_pose(rng, E):
    ang = rng.uniform(-np.pi, np.pi, E)
    return ang, rng.uniform(-1, 1, (E, 2))


# ---- 1. all envs the same: it is select_shape ----
@pytest.mark.parametrize("E,N", [(5, 8), (3, 64)])
def test_all_envs_the_same_is_select_shape(shapes, E, N):
    sb, mb = pair(shapes, E, N)
    oa = sb.select_shapes(np.full(E, 4)).clone()
    ob = mb.select_shape(4).clone()
    assert torch.equal(oa, ob)
    same_handle(sb, mb)
    assert (sb.get_shape_index() == 4).all() and sb.shape_in_force == 4 and sb.shape_env_in_force.tolist() == [4] * E
    assert sb.path_envs() == mb.path_envs()
    lockstep(sb, mb, 5)
    sb.close(); mb.close()


# ---- 2. per-env indices with keeps, a non-lattice shape in the set ----
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_per_env_indices_with_keeps(shapes, dtype):
    jit = jittered(shapes)
    E, N = 9, 30                                             # two envs per workgroup
    index = np.array([0, 1, 2, 3, 1, 1, -1, 4, 5])          # workgroups: mixed, walk, scan, walk (a kept env), walk
    sb, mb = pair(jit, E, N, dtype, start=0)
    want = posed_cells(jit, index, None, current_of(mb, jit))
    oa = sb.select_shapes(index).clone()
    mb.set_cells(*want)
    ob = mb.observe().clone()
    assert torch.equal(oa, ob)
    same_handle(sb, mb, shape_index=False)
    assert sb.get_shape_index().tolist() == [0, 1, 2, 3, 1, 1, 0, 4, 5] and (mb.get_shape_index() == -1).all()
    assert sb.shape_env_in_force.tolist() == [0, 1, 2, 3, 1, 1, 0, 4, 5] and sb.shape_in_force == -1
    assert sb.path_envs() == mb.path_envs() == (5, 4)
    lockstep(sb, mb, 6, extras=True)
    assert sb.path_envs() == mb.path_envs() == (5, 4)
    sb.close(); mb.close()


# ---- 3. poses ----
@pytest.mark.parametrize("N", [30, 64])
def test_poses(shapes, N):
    E = 6
    rng = np.random.default_rng([31, N])
    ang, off = random_pose(rng, E)
    index = np.array([2, 0, 6, 5, 3, 2])
    pose = np.column_stack([np.cos(ang), np.sin(ang), off])
    sb, mb = pair(shapes, E, N)
    nb = shape_batch(shapes, E, N, debug_flags=NO_LATTICE)
    nb.reset(3)
    want = posed_cells(shapes, index, pose, current_of(mb, shapes))
    oa = sb.select_shapes(index, angle=ang, offset=off).clone()
    cells, n_g = sb.get_cells()
    assert np.array_equal(cells, want[0]) and np.array_equal(n_g, want[1])      # the numpy expression, bit for bit
    for e in range(E):
        assert not cells[e, :, n_g[e]:].any() and cells[e, :, : n_g[e]].all()   # zeros behind n_g, and only there
    for b in (mb, nb):
        b.set_cells(*want)
        assert torch.equal(oa, b.observe())
    assert sb.path_envs()[0] > 0 and nb.path_envs() == (0, E)                   # the transformed lattice records were walked
    assert sb.shape_in_force == -1 and sb.shape_env_in_force.tolist() == index.tolist()
    g = torch.Generator(device="cpu").manual_seed(N)
    for t in range(10):
        act = (torch.rand((E, N, 2), generator=g) * 2 - 1).to(sb.device)
        a = sb.step(act)
        for b in (mb, nb):
            assert all(torch.equal(x, y) for x, y in zip(a, b.step(act))), t
            assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), b.get_state())), t
    # pose= as an array and as a device tensor are the same call
    sb.select_shapes(index, pose=pose)
    c2, _ = sb.get_cells()
    sb.select_shapes(torch.from_numpy(index.astype(np.int32)).to(sb.device), pose=torch.from_numpy(pose).to(sb.device))
    c3, _ = sb.get_cells()
    assert np.array_equal(c2, cells) and np.array_equal(c3, cells) and sb.shape_env_in_force is None
    sb.close(); mb.close(); nb.close()


# ---- 4. all -1 ----
def test_all_keep_changes_nothing(shapes):
    E, N = 4, 30
    sb, mb = pair(shapes, E, N)
    lockstep(sb, mb, 2)
    before = (sb.get_cells(), sb.get_shape_index(), [x.clone() for x in sb.get_state()])
    rng = np.random.default_rng(4)
    ang, off = random_pose(rng, E)
    sb.select_shapes(np.full(E, -1), angle=ang, offset=off)
    sb.select_shapes(np.full(E, -1))
    assert np.array_equal(sb.get_cells()[0], before[0][0]) and np.array_equal(sb.get_cells()[1], before[0][1])
    assert np.array_equal(sb.get_shape_index(), before[1])
    assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), before[2]))
    assert sb.shape_env_in_force is None
    lockstep(sb, mb, 8, seed=1)                              # mb was never interrupted
    sb.close(); mb.close()


# ---- 5. out-of-range indices on the device are kept envs ----
def test_out_of_range_device_indices_keep(shapes):
    E, N = 4, 30
    S = len(shapes["l_cell"])
    sb, mb = pair(shapes, E, N)
    before = sb.get_cells()
    held = sb.get_shape_index()
    rng = np.random.default_rng(5)
    ang, off = random_pose(rng, E)
    pose = np.column_stack([np.cos(ang), np.sin(ang), off])
    with pytest.raises(ValueError):
        sb.select_shapes([S, 0, 0, 1])                       # on the host the same values are an error
    index = torch.tensor([S, 2 ** 31 - 1, -7, 1], dtype=torch.int32, device=sb.device)
    oa = sb.select_shapes(index, pose=torch.from_numpy(pose).to(sb.device)).clone()
    ob = mb.select_shapes([-1, -1, -1, 1], pose=pose).clone()
    assert torch.equal(oa, ob)
    same_handle(sb, mb)
    cells, n_g = sb.get_cells()
    assert np.array_equal(cells[:3], before[0][:3]) and np.array_equal(n_g[:3], before[1][:3])
    assert sb.get_shape_index().tolist() == held[:3].tolist() + [1] and sb.shape_env_in_force is None
    lockstep(sb, mb, 3)
    sb.close(); mb.close()


# ---- 6. a large-swarm handle ----
def test_large_swarm(shapes):
    E, N = 2, 300
    sb, mb = pair(shapes, E, N, large_swarm=True)
    rng = np.random.default_rng(6)
    ang, off = random_pose(rng, E)
    index = np.array([5, 1])
    pose = np.column_stack([np.cos(ang), np.sin(ang), off])
    want = posed_cells(shapes, index, pose, current_of(mb, shapes))
    oa = sb.select_shapes(index, pose=pose).clone()
    mb.set_cells(*want)
    assert torch.equal(oa, mb.observe())
    same_handle(sb, mb, shape_index=False)
    assert sb.path_envs() == mb.path_envs() == (0, E)
    lockstep(sb, mb, 2)
    sb.close(); mb.close()


# ---- 7. enqueue only, in stream order ----
def test_enqueue_only_on_a_side_stream(shapes, cycles_per_ms):
    E, N = 4, 30
    rng = np.random.default_rng(7)
    dev = torch.device("cuda", 0)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)
    ang, off = random_pose(rng, E)
    idx_a, idx_b = t([0, 1, 2, 3], torch.int32), t([4, -1, 6, 5], torch.int32)
    pose_a = t(np.column_stack([np.ones(E), np.zeros(E), np.zeros((E, 2))]), torch.float64)
    pose_b = t(np.column_stack([np.cos(ang), np.sin(ang), off]), torch.float64)
    act = t(rng.uniform(-1, 1, (E, N, 2)), torch.float32)

    def run(m):
        sb = shape_batch(shapes, E, N)
        index, pose = idx_a.clone(), pose_a.clone()
        sb.reset(7)
        r = {"obs_a": sb.select_shapes(index, pose=pose).clone()}                 # warm-up: state A, on the default stream
        r["cells_a"] = sb.get_cells()[0]
        torch.cuda.synchronize()
        with m.stream():
            m.delay()
            index.copy_(idx_b); pose.copy_(pose_b)                                # rewritten in place, behind the delay
            r["obs"] = sb.select_shapes(index, pose=pose).clone(); m.enqueued("swarm_select_shapes")
            out = sb.step(act)
            for k, v in zip(("obs1", "rew1", "done1", "pri1"), out):
                r[k] = v.clone()
            m.enqueued("swarm_step behind swarm_select_shapes")
            m.done()
            r["cells"], r["n_g"] = sb.get_cells()
            r["shape"] = sb.get_shape_index()
            r["p"], r["dp"] = [x.clone() for x in sb.get_state()]
        torch.cuda.synchronize()
        sb.close()
        return r

    class Default:
        def stream(self):
            import contextlib
            return contextlib.nullcontext()

        def delay(self):
            torch.cuda.synchronize()

        enqueued = lambda self, what: torch.cuda.synchronize()
        done = lambda self: torch.cuda.synchronize()

    ref = run(Default())
    got = run(Delayed(cycles_per_ms, "select_shapes"))
    assert not np.array_equal(ref["cells"], ref["cells_a"]) and not torch.equal(ref["obs"], ref["obs_a"])   # B is not A
    assert ref["shape"].tolist() == [4, 1, 6, 5]
    for k in ref:
        same = torch.equal(got[k], ref[k]) if isinstance(ref[k], torch.Tensor) else np.array_equal(got[k], ref[k])
        assert same, f"{k} differs from the default-stream run"


# ---- 8. refusals: nothing is enqueued, nothing moves ----
def test_refusals_change_nothing(shapes):
    from marl_llm_amd._lib import SwarmError
    from marl_llm_amd.rollout import ChainedReplay, FusedPolicy, PolicyMLP, rollout_eval
    E, N = 4, 30
    S = len(shapes["l_cell"])
    sb, mb = pair(shapes, E, N)
    lib = sb.lib
    index = torch.zeros(E, dtype=torch.int32, device=sb.device)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def refused(h, args, rc, text):
        assert lib.swarm_select_shapes(h, *args) == rc
        msg = lib.swarm_last_error(h).decode()
        assert msg.startswith("swarm_select_shapes:") and text in msg, msg

    # INVALID: a NULL handle, a NULL shape_index
    assert lib.swarm_select_shapes(None, vp(index), None, None) == 1
    refused(sb.handle, (None, None, None), 1, "shape_index")
    same_handle(sb, mb)
    # STATE: no shape set; a state but no cells; cells for some envs only; cells but no state
    cur = current_of(mb, shapes)
    p, dp = mb.get_state()
    nb = shape_batch(shapes, E, N, upload=False)
    nb.set_cells(*cur); nb.set_state(p, dp); nb.observe()
    refused(nb.handle, (vp(index), None, None), 3, "no shape set")
    with pytest.raises(SwarmError, match="swarm_select_shapes: no shape set"):
        nb.select_shapes(index)                              # a device index passes the host unchecked: the library refuses
    with pytest.raises(ValueError):
        nb.select_shapes([0] * E)                            # a host index is checked against the (empty) set first
    same_handle(nb, mb, shape_index=False)
    lockstep(nb, mb, 2)
    fresh = shape_batch(shapes, E, N)
    refused(fresh.handle, (vp(index), None, None), 3, "state not set")
    fresh.set_state(p, dp)
    refused(fresh.handle, (vp(index), None, None), 3, "cells not set for every env")
    fresh.set_cells(cur[0][:2], cur[1][:2], cur[2][:2])
    refused(fresh.handle, (vp(index), None, None), 3, "cells not set for every env")
    cells, n_g = fresh.get_cells()
    assert np.array_equal(cells[:2], cur[0][:2]) and not cells[2:].any() and n_g.tolist() == cur[1][:2].tolist() + [0, 0]
    assert all(torch.equal(x, y) for x, y in zip(fresh.get_state(), (p, dp)))
    # a rejected per-env schedule: the ring, the state and the cells stay
    torch.manual_seed(0)
    policy = FusedPolicy(PolicyMLP(192, 2, 180).cuda())
    ring = ChainedReplay(6, E * N, sb.obs_dim, 2, sb.device)
    rollout_eval(sb, policy, 2, reset=(1, 0), replay=ring)
    torch.cuda.synchronize()
    kept = {k: getattr(ring, k).clone() for k in RING}
    counters = (ring.cur, ring.count, ring._chained, set(ring._sealed))
    state, cells = [x.clone() for x in sb.get_state()], sb.get_cells()
    for bad in ({0: np.arange(E) % S, 1: [0, 1, S, 0]}, {0: 2, 2: dict(index=[0] * E, pose=np.zeros((E, 4)), angle=np.zeros(E))},
                {1: [0] * (E + 1)}, {0: dict(index=[0] * E, offset=np.zeros((E, 3)))}):
        with pytest.raises(ValueError):
            rollout_eval(sb, policy, 3, replay=ring, switch=bad)
        torch.cuda.synchronize()
        assert all(torch.equal(getattr(ring, k), v) for k, v in kept.items())
        assert (ring.cur, ring.count, ring._chained, set(ring._sealed)) == counters
        assert all(torch.equal(x, y) for x, y in zip(sb.get_state(), state))
        assert all(np.array_equal(x, y) for x, y in zip(sb.get_cells(), cells))
    for b in (sb, mb, nb, fresh):
        b.close()


# ---- 9. rollout_eval with a per-env schedule ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rollout_eval_per_env_schedule(shapes, dtype):
    from marl_llm_amd.rollout import ChainedReplay, FusedPolicy, PolicyMLP, _ring_struct, rollout_eval
    from marl_llm_amd import _lib
    E, N, steps = 8, 30, 6
    n = E * N
    S = len(shapes["l_cell"])
    torch.manual_seed(0)
    policy = FusedPolicy(PolicyMLP(192, 2, 180).cuda())
    rng = np.random.default_rng(9)
    ang, off = random_pose(rng, E)
    first = np.arange(E) % S
    second = np.where(np.arange(E) % 2 == 0, (np.arange(E) + 3) % S, -1)       # half the envs take a posed shape, half keep
    sched = {0: first, 3: dict(index=second, angle=ang, offset=off)}
    sb, mb = shape_batch(shapes, E, N, dtype), shape_batch(shapes, E, N, dtype)
    ring = ChainedReplay(steps, n, sb.obs_dim, 2, sb.device, obs_dtype=dtype)
    obs, tr = rollout_eval(sb, policy, steps, reset=(5, 0), replay=ring, switch=sched, trace_state=True)
    # the eager loop: trace, switch, metrics, actor (noise 0) on the observation the previous step returned, step
    twin = ChainedReplay(steps, n, mb.obs_dim, 2, mb.device, obs_dtype=dtype)
    o = mb.reset(5).clone()
    met, ps, dps = [], [], []
    for t in range(steps):
        p, dp = mb.get_state()
        ps.append(p.clone()); dps.append(dp.clone())
        if t == 0:
            mb.select_shapes(first)
        elif t == 3:
            mb.select_shapes(second, angle=ang, offset=off)
        met.append(mb.metrics().clone())
        act = policy(o.reshape(n, -1), noise_scale=0).clone()
        nobs, rew, done, pri = mb.step(act.view(E, N, 2))
        twin.obs[t] = o.reshape(n, -1); twin.obs[t + 1] = nobs.reshape(n, -1)
        twin.act[t] = act; twin.rew[t] = rew.reshape(n, 1); twin.done[t] = done.reshape(n, 1); twin.act_prior[t] = pri.reshape(n, 2)
        o = nobs.clone()
    torch.cuda.synchronize()
    for k in RING:
        assert torch.equal(getattr(ring, k), getattr(twin, k)), k
    assert ring.cur == steps and ring.count == steps and torch.equal(obs, o)
    assert np.array_equal(tr.metrics.cpu().numpy(), torch.stack(met).cpu().numpy(), equal_nan=True)
    assert torch.equal(tr.p, torch.stack(ps)) and torch.equal(tr.dp, torch.stack(dps))
    same_handle(sb, mb)
    held = np.where(second >= 0, second, first)
    assert tr.shape_env.dtype == np.int64 and tr.shape_env.tolist() == [first.tolist()] * 3 + [held.tolist()] * 3
    assert tr.shape.tolist() == [-1] * steps
    assert sb.get_shape_index().tolist() == held.tolist() and sb.shape_env_in_force.tolist() == held.tolist()
    assert tr.reward_stats is not None and tr.reward_stats.shape == (steps, 2)
    rs = tr.reward_stats.cpu().numpy()
    assert np.array_equal(rs[:, 0], twin.rew[:steps].double().mean(dim=(1, 2)).cpu().numpy())
    # a device index: the schedule runs the same, and the host no longer knows who holds what
    db = shape_batch(shapes, E, N, dtype)
    dring = ChainedReplay(steps, n, db.obs_dim, 2, db.device, obs_dtype=dtype)
    _, dtr = rollout_eval(db, policy, steps, reset=(5, 0), replay=dring,
                          switch={0: torch.from_numpy(first.astype(np.int32)).to(db.device), 3: sched[3]})
    torch.cuda.synchronize()
    assert all(torch.equal(getattr(dring, k), getattr(ring, k)) for k in RING) and dtr.shape_env is None
    # a schedule of ints is still the single library call
    ints = {0: 4, 3: 5}
    ib, ab = shape_batch(shapes, E, N, dtype), shape_batch(shapes, E, N, dtype)
    iring = ChainedReplay(steps, n, ib.obs_dim, 2, ib.device, obs_dtype=dtype)
    aring = ChainedReplay(steps, n, ab.obs_dim, 2, ab.device, obs_dtype=dtype)
    _, itr = rollout_eval(ib, policy, steps, reset=(5, 0), replay=iring, switch=ints)
    ab.reset(5, 0, out=aring.obs[0])
    sw = np.array([4, -1, -1, 5, -1, -1], np.int32)
    am = torch.empty((steps, E, 3), dtype=torch.float64, device=ab.device)
    r = _ring_struct(ab, aring)
    rc = ab.lib.swarm_rollout_eval(ab.handle, policy.handle, ctypes.byref(r), steps, sw.ctypes.data_as(ctypes.c_void_p),
                                   ctypes.byref(_lib.SwarmEvalOut(am.data_ptr(), None, None, None)),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, ab.lib.swarm_rollout_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(getattr(iring, k), getattr(aring, k)) for k in RING)
    assert np.array_equal(itr.metrics.cpu().numpy(), am.cpu().numpy(), equal_nan=True)
    assert itr.shape.tolist() == [4] * 3 + [5] * 3 and itr.shape_env.tolist() == [[4] * E] * 3 + [[5] * E] * 3
    assert ib.shape_in_force == 5
    for b in (sb, mb, db, ib, ab):
        b.close()
