"""The actor bank (swarm_policy_bank_create, include/swarm_policy.h "Actor bank"; FusedPolicyBank) held to the code that is
already held to the float64 model: M plain FusedPolicy handles, one per member.  Handle m is called on the rows
[m R, (m + 1) R) with row_offset + m R and the same seed and step, and the bank must give the SAME BITS in act and log_pi -- no
tolerance anywhere in this file but in the one test that checks a segment against the float64 model itself.

R sits either side of a 32-row tile, of the bf16 workgroup's 128 rows and of the bf16x3 workgroup's 256, so a member's last
tile ends inside a workgroup: a kernel that bounded that tile by the CALL's rows would compute rows of member m + 1 with member
m's weights and overwrite them -- the members are drawn from different seeds, and every segment is also required to DIFFER
from what the next member's handle gives there, so serving one member everywhere cannot pass either.

The whole module runs in well under a minute on one MI355X."""
import ctypes

import numpy as np
import pytest

from test_gpu_policy_contract import _check_against_model, _module

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ALL_R = [1, 30, 32, 33, 127, 128, 129, 257, 300]
SOME_R = [1, 33, 129, 300]
PRECISIONS = ["bf16", "bf16x3"]
# (wide, shape, M, the R values)
CASES = [(False, (192, 180, 2), 3, ALL_R),
         (False, (192, 180, 2), 1, SOME_R), (False, (192, 180, 2), 2, ALL_R), (False, (192, 180, 2), 5, ALL_R),
         (False, (8, 16, 1), 2, [30, 129, 257]), (False, (64, 100, 3), 5, [32, 127, 300]),
         (True, (192, 256, 2), 3, ALL_R), (True, (384, 256, 2), 2, [30, 128, 257]),
         (True, (192, 180, 2), 3, ALL_R)]                                # a narrow shape forced wide (the MT = 6 geometry)
SEED, STEP, OFFSET = 7, 3, 12345 + (1 << 33)


def _members(shape, M, seed0=100):
    return [_module(shape, seed0 + 17 * k) for k in range(M)]


def _bank(modules, precision, wide=None):
    from marl_llm_amd.rollout import FusedPolicyBank
    return FusedPolicyBank(modules, precision=precision, wide=wide)


def _plain(module, precision, wide=None):
    from marl_llm_amd.rollout import FusedPolicy
    return FusedPolicy(module, precision=precision, wide=wide)


_cache = {}


def _setup(wide, shape, M, precision):
    """(bank, its modules, one plain handle per member), built once per configuration."""
    key = (wide, shape, M, precision)
    if key not in _cache:
        mods = _members(shape, M)
        _cache[key] = (_bank(mods, precision, wide or None), mods, [_plain(m, precision, wide or None) for m in mods])
    return _cache[key]


def _rows(n, in_dim, dtype, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(n, in_dim, device="cuda", generator=g) * 0.7).to(dtype).contiguous()


def _by_handles(handles, x, R, **kw):
    """What the parent commit offers: handle m on its segment, the noise keyed by the call's rows.  (act, log_pi or None)"""
    off = kw.pop("row_offset", 0)
    outs = [f(x[m * R:(m + 1) * R], row_offset=off + m * R, **kw) for m, f in enumerate(handles)]
    if kw.get("log_pi") is None:
        return torch.cat(outs), None
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


MODES = [dict(), dict(noise_scale=0.3, seed=SEED, step=STEP, row_offset=OFFSET),
         dict(noise_scale=0.3, seed=SEED, step=STEP, row_offset=OFFSET, log_pi=True)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("wide,shape,M,Rs", CASES, ids=["%s-%d-%d-%d-M%d" % (("wide" if c[0] else "narrow",) + c[1] + (c[2],)) for c in CASES])
def test_bank_equals_one_handle_per_member(wide, shape, M, Rs, precision):
    bank, mods, handles = _setup(wide, shape, M, precision)
    assert bank.members == M and bank.wide == wide and bank.lib.swarm_policy_bank_members(bank.handle) == M
    assert all(bank.lib.swarm_policy_bank_members(f.handle) == 1 for f in handles)
    for R in Rs:
        for dtype in (torch.float32, torch.bfloat16):
            x = _rows(M * R, shape[0], dtype, seed=R)
            for mode in MODES:
                want, want_lp = _by_handles(handles, x, R, **mode)
                got = bank(x, **mode)
                got, got_lp = got if mode.get("log_pi") else (got, None)
                assert got.shape == (M * R, shape[2]) and torch.equal(got, want), (R, dtype, mode)
                if want_lp is not None:
                    assert got_lp.shape == (M * R,) and torch.equal(got_lp, want_lp), (R, dtype)
            # the members differ: segment m is NOT what member m + 1's handle gives on those rows
            if M > 1:
                plain = bank(x)
                for m in range(M):
                    other = handles[(m + 1) % M](x[m * R:(m + 1) * R])
                    assert not torch.equal(plain[m * R:(m + 1) * R], other), (R, dtype, m)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_noise_does_not_depend_on_the_members(wide, precision):
    """Zero weights: the action is the clamped noise alone, keyed by row_offset + the CALL's row -- a bank of 4 gives what a
    plain handle gives over all rows (a noise keyed by the member-local row would repeat every R rows)."""
    from marl_llm_amd.rollout import PolicyMLP
    mods = [PolicyMLP(192, 2, 180).cuda() for _ in range(4)]
    with torch.no_grad():
        for m in mods:
            for p in m.parameters():
                p.zero_()
    bank, plain = _bank(mods, precision, wide or None), _plain(mods[0], precision, wide or None)
    x = _rows(4 * 129, 192, torch.float32)
    kw = dict(noise_scale=0.125, seed=SEED, step=STEP, row_offset=OFFSET, log_pi=True)
    (a, lp), (b, lq) = bank(x, **kw), plain(x, **kw)
    assert torch.equal(a, b) and torch.equal(lp, lq)
    assert not torch.equal(a[:129], a[129:258])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_one_member_and_identical_members_equal_the_plain_handle(wide, precision):
    m = _module((192, 180, 2), 31)
    plain = _plain(m, precision, wide or None)
    for M in (1, 4):
        bank = _bank([m] * M, precision, wide or None)
        for rows in (M * 1, M * 33, M * 129, M * 300):
            for dtype in (torch.float32, torch.bfloat16):
                x = _rows(rows, 192, dtype, seed=rows)
                for mode in MODES:
                    a, b = bank(x, **mode), plain(x, **mode)
                    if mode.get("log_pi"):
                        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (M, rows, dtype)
                    else:
                        assert torch.equal(a, b), (M, rows, dtype, mode)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_segment_against_the_float64_model(precision):
    """Member 1's segment of a bank of 3 (R = 300: its last tile ends inside a workgroup) within test_gpu_policy_contract.py's
    derived bounds of the float64 model of member 1."""
    bank, mods, _ = _setup(False, (192, 180, 2), 3, precision)
    R = 300
    x = _rows(3 * R, 192, torch.float32, seed=2)
    got = bank(x)[R:2 * R]
    ratio, frac = _check_against_model(got, mods[1], x[R:2 * R], precision)
    print("%s: worst ratio %.3g, decided %s" % (precision, ratio, frac))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_out_and_log_pi_inside_larger_buffers_write_only_the_calls_rows(wide, precision):
    bank, mods, handles = _setup(wide, (192, 180, 2), 3, precision)
    R, pre, post = 129, 77, 300
    x = _rows(3 * R, 192, torch.float32, seed=4)
    kw = dict(noise_scale=0.3, seed=SEED, step=STEP, row_offset=OFFSET)
    want, want_lp = _by_handles(handles, x, R, log_pi=True, **kw)
    big = torch.full((pre + 3 * R + post, 2), float("nan"), device="cuda")
    big_lp = torch.full((pre + 3 * R + post,), float("nan"), device="cuda")
    bank(x, out=big[pre:pre + 3 * R], log_pi=big_lp[pre:pre + 3 * R], **kw)
    assert torch.equal(big[pre:pre + 3 * R], want) and torch.equal(big_lp[pre:pre + 3 * R], want_lp)
    for t in (big[:pre], big[pre + 3 * R:], big_lp[:pre], big_lp[pre + 3 * R:]):
        assert torch.isnan(t).all()
    big.fill_(float("nan"))
    bank(x, out=big[pre:pre + 3 * R])
    assert torch.equal(big[pre:pre + 3 * R], _by_handles(handles, x, R)[0])
    assert torch.isnan(big[:pre]).all() and torch.isnan(big[pre + 3 * R:]).all()


def _slice(f, member):
    """member's packed slice of a bank (or, member None, a plain handle's whole blob) as bytes"""
    lib, st = f.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = lib.swarm_policy_read_packed(f.handle, None, 0, None) if member is None else lib.swarm_policy_bank_read_packed(f.handle, member, None, 0, None)
    assert n > 0, lib.swarm_policy_last_error()
    buf = np.full(n, 0xA5, np.uint8)
    got = (lib.swarm_policy_read_packed(f.handle, buf.ctypes.data, n, st) if member is None
           else lib.swarm_policy_bank_read_packed(f.handle, member, buf.ctypes.data, n, st))
    assert got == n, lib.swarm_policy_last_error()
    return buf


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_every_slice_is_the_plain_handles_blob(wide):
    bank, mods, handles = _setup(wide, (192, 180, 2), 3, "bf16")
    for k in range(3):
        assert np.array_equal(_slice(bank, k), _slice(handles[k], None)), k
    assert not np.array_equal(_slice(bank, 0), _slice(bank, 1))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_sync_of_one_member_in_stream_order(wide, precision):
    mods = _members((192, 180, 2), 3, seed0=500)
    bank = _bank(mods, precision, wide or None)
    old = [_plain(m, precision, wide or None) for m in mods]            # host copies: they keep the old weights
    before = [_slice(bank, j) for j in range(3)]
    R, k = 129, 1
    x = _rows(3 * R, 192, torch.float32, seed=6)
    # no host wait from here to the comparison: forward, the update of module k, its sync, forward -- all on one stream
    a = bank(x)
    with torch.no_grad():
        for p in mods[k].parameters():
            p.mul_(-1.25).add_(0.01)
    bank.sync(member=k)
    b = bank(x)
    new_k = _plain(mods[k], precision, wide or None)
    assert torch.equal(a, _by_handles(old, x, R)[0])
    assert torch.equal(b, _by_handles([old[0], new_k, old[2]], x, R)[0])
    assert not torch.equal(a[R:2 * R], b[R:2 * R])
    assert np.array_equal(_slice(bank, k), _slice(new_k, None))
    for j in (0, 2):
        assert np.array_equal(_slice(bank, j), before[j]), j
    # sync() of all members: every slice again the host packer's
    with torch.no_grad():
        for m in mods:
            for p in m.parameters():
                p.mul_(0.5)
    bank.sync()
    for j in range(3):
        assert np.array_equal(_slice(bank, j), _slice(_plain(mods[j], precision, wide or None), None)), j
    with pytest.raises(ValueError):
        bank.sync(member=3)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_refusals_leave_outputs_and_weights_untouched(wide):
    bank, mods, handles = _setup(wide, (192, 180, 2), 3, "bf16")
    lib, st = bank.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = _rows(3 * 40 + 1, 192, torch.float32)
    out = torch.full((3 * 40 + 1, 2), float("nan"), device="cuda")
    lp = torch.full((3 * 40 + 1,), float("nan"), device="cuda")
    # rows % M != 0, through every forward entry point
    calls = [lambda n: lib.swarm_policy_forward(bank.handle, x.data_ptr(), n, out.data_ptr(), st),
             lambda n: lib.swarm_policy_forward_bf16(bank.handle, x.data_ptr(), n, out.data_ptr(), st),
             lambda n: lib.swarm_policy_forward_explore(bank.handle, x.data_ptr(), 0, n, out.data_ptr(), 0.1, 1, 2, st),
             lambda n: lib.swarm_policy_forward_explore_at(bank.handle, x.data_ptr(), 0, n, out.data_ptr(), 0.1, 1, 2, 3, st),
             lambda n: lib.swarm_policy_forward_explore_logpi(bank.handle, x.data_ptr(), 0, n, out.data_ptr(), lp.data_ptr(), 0.1, 1, 2, 3, st)]
    for call in calls:
        for n in (121, 1, 2):
            assert call(n) == 1
            msg = lib.swarm_policy_last_error()
            assert b"rows %d" % n in msg and b"members 3" in msg
    with pytest.raises(ValueError, match="no multiple of the 3 members"):
        bank(x)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(lp).all()
    # member -1 and M, and the plain-handle calls on a bank: nothing is enqueued, every slice keeps its bytes
    before = [_slice(bank, j) for j in range(3)]
    ps = [ctypes.c_void_p(t.data_ptr()) for t in (mods[0].fc1.weight, mods[0].fc1.bias, mods[0].fc2.weight, mods[0].fc2.bias,
                                                  mods[0].fc3.weight, mods[0].fc3.bias, mods[0].fc4.weight, mods[0].fc4.bias)]
    for member in (-1, 3):
        assert lib.swarm_policy_bank_load_device(bank.handle, member, *ps, st) == 1
        assert lib.swarm_policy_last_error().startswith(b"swarm_policy_bank_load_device: member %d outside" % member)
        host = np.full(before[0].size, 0xA5, np.uint8)
        assert lib.swarm_policy_bank_read_packed(bank.handle, member, host.ctypes.data, host.size, st) == -1
        assert lib.swarm_policy_last_error().startswith(b"swarm_policy_bank_read_packed: member %d outside" % member)
        assert (host == 0xA5).all()
    assert lib.swarm_policy_load_device(bank.handle, *ps, st) == 1
    assert b"swarm_policy_bank_load_device" in lib.swarm_policy_last_error() and b"bank of 3" in lib.swarm_policy_last_error()
    host = np.full(before[0].size, 0xA5, np.uint8)
    assert lib.swarm_policy_read_packed(bank.handle, host.ctypes.data, host.size, st) == -1
    assert b"swarm_policy_bank_read_packed" in lib.swarm_policy_last_error() and (host == 0xA5).all()
    assert lib.swarm_policy_bank_load_device(bank.handle, 1, ps[0], None, *ps[2:], st) == 1
    torch.cuda.synchronize()
    for j in range(3):
        assert np.array_equal(_slice(bank, j), before[j]), j
    # the bank calls serve a plain handle as its only member
    assert np.array_equal(_slice(handles[0], None), before[0])
    n = lib.swarm_policy_bank_read_packed(handles[0].handle, 0, None, 0, None)
    assert n == before[0].size and lib.swarm_policy_bank_read_packed(handles[0].handle, 1, None, 0, None) == -1


def test_bf16_rows_need_in_dim_a_multiple_of_8():
    mods = _members((188, 180, 2), 2)
    bank = _bank(mods, "bf16")
    x = torch.zeros(2 * 33, 188, device="cuda", dtype=torch.bfloat16)
    out = torch.full((2 * 33, 2), float("nan"), device="cuda")
    rc = bank.lib.swarm_policy_forward_bf16(bank.handle, x.data_ptr(), 2 * 33, out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 1 and b"multiple of 8" in bank.lib.swarm_policy_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    xf = _rows(2 * 33, 188, torch.float32)
    assert torch.equal(bank(xf), _by_handles([_plain(m, "bf16") for m in mods], xf, 33)[0])
