"""New weights for an existing fused-actor handle, from device tensors, in stream order: swarm_policy_load_device /
swarm_policy_read_packed (include/swarm_policy.h) and FusedPolicy.sync().

1. Same bytes: the blob the device packer leaves equals, byte for byte, the blob swarm_policy_create packs on the host from
   the same fp32 values -- at the smallest shape, both edges of the padding and the one-column at index 191, on values that
   hold every rounding class of the contract (the test asserts that from numpy alone).
2. Same outputs: after sync() the handle answers bit for bit like a fresh FusedPolicy of the module.
3. Stream order, no host wait: behind a delay on a side stream, forward / parameter update / sync() / forward are all
   enqueued while the delay still runs; the first forward used the old weights, the second the new ones.
4. Refusals leave the handle as it was.
5. A device rollout with a sync()ed policy fills the ring exactly as one with a policy created from those weights."""
import ctypes

import numpy as np
import pytest

from helpers import shape_batch

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DELAY_MS = 150.0
SHAPES = [(4, 1, 1), (8, 7, 2), (24, 33, 3), (188, 180, 2), (192, 180, 2), (192, 191, 4)]

# fp32 bit patterns of the rounding classes the same-bytes contract names
SPECIALS = np.array([
    0x3F800000, 0xBE9A0000,                             # exact bf16 values
    0x3F808000, 0xBF808000,                             # halfway, even upper half: rounds down to it
    0x3F818000,                                         # halfway, odd upper half: rounds up
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,     # one ulp either side of the two halfway cases
    0x00000001, 0x807FFFFF, 0x00008000, 0x00012345,     # fp32 denormals (the smallest, the largest, a halfway one, any)
    0x00000000, 0x80000000,                             # +0, -0
    0x7F7F7FFF, 0xFF7F7FFF,                             # the largest magnitudes whose bf16 rounding is finite (0x7F7F)
], dtype=np.uint32)


def classes(u):
    """Which classes the uint32 patterns `u` hold: {name: bool}.  numpy only."""
    u = np.asarray(u, np.uint32)
    low, odd = u & 0xFFFF, ((u >> 16) & 1).astype(bool)
    expo, mant = (u >> 23) & 0xFF, u & 0x7FFFFF
    return {
        "exact bf16": bool(((low == 0) & (expo > 0) & (expo < 255)).any()),
        "halfway, even upper half": bool(((low == 0x8000) & ~odd & (expo > 0)).any()),
        "halfway, odd upper half": bool(((low == 0x8000) & odd & (expo > 0)).any()),
        "one ulp below halfway (even)": bool(((low == 0x7FFF) & ~odd).any()),
        "one ulp above halfway (even)": bool(((low == 0x8001) & ~odd).any()),
        "one ulp below halfway (odd)": bool(((low == 0x7FFF) & odd & (expo < 254)).any()),
        "one ulp above halfway (odd)": bool(((low == 0x8001) & odd).any()),
        "denormal": bool(((expo == 0) & (mant != 0)).any()),
        "+0": bool((u == 0).any()),
        "-0": bool((u == 0x80000000).any()),
        "largest finite rounding, +": bool((u == 0x7F7F7FFF).any()),
        "largest finite rounding, -": bool((u == 0xFF7F7FFF).any()),
    }


def inside_contract(u):
    """Finite, and the bf16 rounding (nearest-even on the bit pattern) is finite."""
    u = np.asarray(u, np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return bool((((u >> 23) & 0xFF) != 255).all() and (((r >> 7) & 0xFF) != 255).all())


def sizes(shape):
    i, h, a = shape
    return [(h, i), (h,), (h, h), (h,), (h, h), (h,), (a, h), (a,)]


def weights(shape, seed, rot=0):
    """Eight fp32 arrays of `shape`: normal values with SPECIALS (rotated by `rot`) scattered over them -- one position in
    every array first, then random positions of the concatenation, up to three copies of the list."""
    rng = np.random.default_rng([seed, *shape])
    n_el = [int(np.prod(s)) for s in sizes(shape)]
    off = np.concatenate([[0], np.cumsum(n_el)])
    n = int(off[-1])
    flat = (rng.standard_normal(n) * 0.3).astype(np.float32)
    first = np.array([off[k] + rng.integers(n_el[k]) for k in range(8)])
    rest = rng.permutation(np.setdiff1d(np.arange(n), first))
    pos = np.concatenate([first, rest])[:min(n, 3 * len(SPECIALS))]
    flat.view(np.uint32)[pos] = np.resize(np.roll(SPECIALS, rot), len(pos))
    return [flat[off[k]:off[k + 1]].reshape(s).copy() for k, s in enumerate(sizes(shape))]


def bits(ws):
    return np.concatenate([w.reshape(-1).view(np.uint32) for w in ws])


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd import _lib
    return _lib.load()


def create(lib, ws, shape):
    h = ctypes.c_void_p()
    rc = lib.swarm_policy_create(*[ctypes.c_void_p(w.ctypes.data) for w in ws], *shape, 0, ctypes.byref(h))
    assert rc == 0, lib.swarm_policy_last_error()
    return h


def read_packed(lib, h):
    n = lib.swarm_policy_read_packed(h, None, 0, None)
    assert n > 0
    buf = np.full(n, 0xA5, np.uint8)
    assert lib.swarm_policy_read_packed(h, ctypes.c_void_p(buf.ctypes.data), n - 1, None) == n and (buf == 0xA5).all()
    assert lib.swarm_policy_read_packed(h, ctypes.c_void_p(buf.ctypes.data), n, None) == n
    return buf


def load_device(lib, h, ws):
    dev = [torch.from_numpy(w).cuda() for w in ws]
    rc = lib.swarm_policy_load_device(h, *[ctypes.c_void_p(t.data_ptr()) for t in dev],
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.swarm_policy_last_error()
    blob = read_packed(lib, h)              # waits for the stream: `dev` may go
    return blob


# ------------------------------------------------------------------------------------------------------------------------
# 1. same bytes
# ------------------------------------------------------------------------------------------------------------------------
def test_inputs_hold_every_class():
    """From numpy alone.  The smallest shape has 11 weights, fewer than the list: there B and C together hold every class
    (C takes the list rotated by 8); every other shape's B holds all of them, and every one of its eight arrays a special."""
    assert all(classes(SPECIALS).values()) and inside_contract(SPECIALS)
    for shape in SHAPES:
        B, C = weights(shape, 2), weights(shape, 3, rot=8)
        assert inside_contract(bits(B)) and inside_contract(bits(C)), shape
        both = classes(np.concatenate([bits(B), bits(C)]))
        assert all(both.values()), (shape, both)
        if shape != (4, 1, 1):
            assert all(classes(bits(B)).values()), (shape, classes(bits(B)))
        for w in B:
            assert np.isin(w.reshape(-1).view(np.uint32), SPECIALS).any(), shape


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_same_bytes_as_the_host_packer(lib, shape):
    A, B, C = weights(shape, 1), weights(shape, 2), weights(shape, 3, rot=8)
    handles = [create(lib, ws, shape) for ws in (A, B, C)]
    try:
        want_a, want_b, want_c = [read_packed(lib, h) for h in handles]
        assert not np.array_equal(want_a, want_b) and not np.array_equal(want_b, want_c)
        h = handles[0]
        for ws, want, name in ((B, want_b, "B"), (C, want_c, "C"), (A, want_a, "A again")):
            got = load_device(lib, h, ws)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, f"{shape} {name}: {bad.size} bytes differ from the host packer's, first at {bad[:4]}"
    finally:
        for h in handles:
            lib.swarm_policy_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------
# 2. same outputs
# ------------------------------------------------------------------------------------------------------------------------
def module(seed, obs_dim=192, hidden=180, device="cuda:0"):
    from marl_llm_amd.rollout import PolicyMLP
    torch.manual_seed(seed)
    return PolicyMLP(obs_dim, 2, hidden).to(device)


def put(dst, src):
    """The learner's update: src's parameters into dst's, in place, on the current stream."""
    with torch.no_grad():
        for p, q in zip(dst.parameters(), src.parameters()):
            p.copy_(q)


def same(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_sync_answers_like_a_fresh_handle(precision):
    from marl_llm_amd.rollout import FusedPolicy
    m, mb = module(1), module(2)
    pol = FusedPolicy(m, precision=precision)
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand((257, 192), device="cuda", generator=gen) * 2 - 1
    old = pol(x).clone()
    put(m, mb)
    pol.sync()
    fresh = FusedPolicy(mb, precision=precision)
    try:
        assert not torch.equal(pol(x), old)
        for rows in (1, 31, 32, 33, 257):
            for obs in (x[:rows].contiguous(), x[:rows].to(torch.bfloat16)):
                assert same(pol(obs), fresh(obs)), (rows, obs.dtype)
                got = pol(obs, noise_scale=0.3, seed=5, step=2, log_pi=True)
                want = fresh(obs, noise_scale=0.3, seed=5, step=2, log_pi=True)
                assert same(got[0], want[0]) and same(got[1], want[1]), (rows, obs.dtype)
    finally:
        pol.close(); fresh.close()


def test_sync_converts_other_dtypes_on_the_device():
    """bfloat16 parameters and a non-contiguous weight: sync() stages fp32 copies on the device; same handle as refresh()'s."""
    from marl_llm_amd.rollout import FusedPolicy
    m, mb = module(4).to(torch.bfloat16), module(5).to(torch.bfloat16)
    pol = FusedPolicy(m)
    put(m, mb)
    with torch.no_grad():
        m.fc2.weight.data = m.fc2.weight.data.t().contiguous().t()          # same values, column-major
    assert not m.fc2.weight.is_contiguous()
    pol.sync()
    fresh = FusedPolicy(m)
    try:
        x = torch.rand((33, 192), device="cuda") * 2 - 1
        assert same(pol(x), fresh(x))
        n = pol.lib.swarm_policy_read_packed(pol.handle, None, 0, None)
        blobs = [np.empty(n, np.uint8) for _ in range(2)]
        for p, b in zip((pol, fresh), blobs):
            assert p.lib.swarm_policy_read_packed(p.handle, ctypes.c_void_p(b.ctypes.data), n, None) == n
        assert np.array_equal(*blobs)
    finally:
        pol.close(); fresh.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. stream order, no host wait
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond, measured once with two events."""
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 50_000_000
    a.record(); torch.cuda._sleep(n); b.record(); b.synchronize()
    return n / a.elapsed_time(b)


def delay(stream, cpm):
    """DELAY_MS of sleep on `stream` and a guard event right behind it: guard.query() is False while the delay runs."""
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(DELAY_MS * cpm))
        guard = torch.cuda.Event()
        guard.record(stream)
    return guard


def test_sync_is_stream_ordered_and_does_not_wait(cycles_per_ms):
    from marl_llm_amd.rollout import FusedPolicy
    m, ma, mb = module(6), module(6), module(7)
    pol = FusedPolicy(m)
    fresh_a, fresh_b = FusedPolicy(ma), FusedPolicy(mb)
    try:
        x = torch.rand((77, 192), device="cuda") * 2 - 1
        out1, out2 = torch.zeros((77, 2), device="cuda"), torch.zeros((77, 2), device="cuda")
        pol(x, out=out1); pol.sync(); put(m, ma)                # warm-up: code objects; the weights stay A
        want_a, want_b = fresh_a(x).clone(), fresh_b(x).clone()
        assert not torch.equal(want_a, want_b)
        out1.zero_()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        guard = delay(side, cycles_per_ms)
        with torch.cuda.stream(side):
            pol(x, out=out1)                                    # weights A
            put(m, mb)                                          # the learner's update, behind the delay
            pol.sync()
            pol(x, out=out2)                                    # weights B
            running = not guard.query()
        side.synchronize()
        assert running, "sync waited for the stream, or the delay is too short"
        assert torch.equal(out1, want_a), "the forward enqueued before sync() did not use the old weights"
        assert torch.equal(out2, want_b), "the forward enqueued after sync() did not use the new weights"
    finally:
        pol.close(); fresh_a.close(); fresh_b.close()


# ------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cpu parameter", "other hidden"])
def test_sync_refuses_and_leaves_the_handle(case):
    from marl_llm_amd.rollout import FusedPolicy
    m = module(8)
    pol = FusedPolicy(m)
    try:
        x = torch.rand((33, 192), device="cuda") * 2 - 1
        before = pol(x).clone()
        if case == "cpu parameter":
            put(m, module(9))
            m.fc3.cpu()
        else:
            pol.module = module(9, hidden=64)
        with pytest.raises(ValueError, match=r"refresh\(\)"):
            pol.sync()
        assert torch.equal(pol(x), before)
    finally:
        pol.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. the device rollout
# ------------------------------------------------------------------------------------------------------------------------
class Coins:
    """host_rng of rollout_device: with epsilon 0.5 the second of three steps is an epsilon step."""
    def __init__(self):
        self.seq = iter((0.9, 0.1, 0.9))

    def random(self):
        return next(self.seq)


def test_rollout_after_sync_fills_the_ring_like_a_created_policy(shapes):
    from marl_llm_amd.rollout import ChainedReplay, FusedPolicy, rollout_device
    E, N, K = 2, 8, 3
    runs = {}
    for name in ("synced", "created", "stale"):
        sb = shape_batch(shapes, E, N)
        m = module(10, obs_dim=sb.obs_dim)
        mb = module(11, obs_dim=sb.obs_dim)
        pol = FusedPolicy(mb if name == "created" else m)
        if name == "synced":
            put(m, mb)
            pol.sync()
        ring = ChainedReplay(K, E * N, sb.obs_dim, 2, sb.device)
        try:
            _, stats = rollout_device(sb, pol, K, replay=ring, reset=(5, 0), noise_scale=0.2, epsilon=0.5, host_rng=Coins(), seed=7)
            torch.cuda.synchronize()
            runs[name] = dict(stats=stats.clone(), **{k: getattr(ring, k).clone() for k in ("obs", "act", "rew", "done", "act_prior")})
        finally:
            pol.close(); sb.close()
    for k, v in runs["created"].items():
        assert torch.equal(runs["synced"][k], v), k
    assert not torch.equal(runs["stale"]["act"], runs["created"]["act"])        # the weights matter to this rollout
