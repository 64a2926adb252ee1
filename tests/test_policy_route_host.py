"""CPU-side checks of the actor bank's routing by env (include/swarm_policy.h "Routing by env", DESIGN.md "Actor bank: routing by
env"): swarm_policy_bank_route checks its arguments before it looks at the handle, so every refusal that needs no device is
decided here with SWARM_POLICY_ERR_INVALID and a message that starts "swarm_policy_bank_route:"; FusedPolicyBank.assign's
ValueErrors come before any library call (a bank without a handle, whose library refuses every call); the grid the host launches,
floor(rows / T) + min(members, n_env), is held above the tiles a count vector needs by brute force; and the header, the symbol
list and the ctypes prototypes agree.  With a device: tests/test_gpu_policy_route.py."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1                  # SWARM_POLICY_ERR_INVALID
PREFIX = b"swarm_policy_bank_route:"


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


# --------------------------------------------------------------------------------------------------- swarm_policy_bank_route
def test_argument_refusals_need_no_handle(lib):
    """The arguments are checked before the handle: each of these is refused the same way with a NULL handle (here) and with a
    bank (tests/test_gpu_policy_route.py), and none touches the table."""
    table = (ctypes.c_int32 * 4)(0, 0, 0, 0)                 # a HOST array: a call that read it on the device would fault
    t = ctypes.cast(table, ctypes.c_void_p)
    cases = [((t, -1, 30), b"n_env -1 < 0"),
             ((None, 4, 30), b"null member_of_env with n_env 4"),
             ((t, 0, 0), b"n_env 0 with a table"),
             ((t, 0, 30), b"n_env 0 with a table"),
             ((t, 4, 0), b"rows_per_env 0 < 1"),
             ((t, 4, -3), b"rows_per_env -3 < 1"),
             ((t, 1 << 16, 1 << 15), b"reaches 2^31"),
             ((t, 2147483647, 1), None),                      # 2^31 - 1 rows pass the size check: the NULL handle is what is refused
             ((t, 2147483647, 2), b"reaches 2^31")]
    for (tab, n_env, rpe), what in cases:
        assert lib.swarm_policy_bank_route(None, tab, n_env, rpe, None) == ERR_INVALID, (n_env, rpe)
        msg = lib.swarm_policy_last_error()
        assert msg.startswith(PREFIX), msg
        assert (what or b"null handle") in msg, msg
    assert b"2147483647 * 2" in lib.swarm_policy_last_error()          # the message names both numbers


def test_a_null_handle_is_refused_also_when_it_would_end_the_route(lib):
    assert lib.swarm_policy_bank_route(None, None, 0, 0, None) == ERR_INVALID
    assert lib.swarm_policy_last_error().startswith(PREFIX + b" null handle")
    table = (ctypes.c_int32 * 4)(0, 1, 0, 1)
    assert lib.swarm_policy_bank_route(None, ctypes.cast(table, ctypes.c_void_p), 4, 30, None) == ERR_INVALID
    assert lib.swarm_policy_last_error().startswith(PREFIX + b" null handle")


def test_route_read_of_a_null_handle(lib):
    counts, uns = (ctypes.c_int32 * 4)(7, 7, 7, 7), ctypes.c_int32(7)
    rc = lib.swarm_policy_bank_route_read(None, ctypes.cast(counts, ctypes.c_void_p), ctypes.addressof(uns), None, None)
    assert rc == -ERR_INVALID and lib.swarm_policy_last_error().startswith(b"swarm_policy_bank_route_read: null handle")
    assert list(counts) == [7, 7, 7, 7] and uns.value == 7


# ------------------------------------------------------------------------------------------------------ FusedPolicyBank.assign
class _NoLibrary:
    """Every library call is a failure of the test: assign() must have raised before."""

    def __getattr__(self, name):
        raise AssertionError("library call %s before the check" % name)


def _bank_without_a_handle(M=3):
    torch = pytest.importorskip("torch")
    from marl_llm_amd.rollout import FusedPolicyBank
    b = object.__new__(FusedPolicyBank)
    b.members, b.lib, b._ctypes, b.handle, b._route = M, _NoLibrary(), ctypes, None, None
    b.device = torch.device("cuda", 0)
    return b, torch


def test_assign_value_errors_come_before_any_library_call():
    b, torch = _bank_without_a_handle(3)
    ok = np.array([0, 2, 1, -1, 2], np.int64)
    bad = [(ok, dict(rows_per_env=30, n_env=4)),                           # wrong length
           (ok.reshape(5, 1), dict(rows_per_env=30)), (np.zeros(0, np.int64), dict(rows_per_env=30)),
           (np.array([0, 3, 1]), dict(rows_per_env=30)),                   # an entry M
           (np.array([0, -2, 1]), dict(rows_per_env=30)),                  # an entry -2
           ([0, 1, 3], dict(rows_per_env=30)),
           (ok.astype(np.float64), dict(rows_per_env=30)),                 # a float array
           (torch.tensor([0.0, 1.0]), dict(rows_per_env=30)),
           (ok, dict()), (ok, dict(rows_per_env=0)), (ok, dict(rows_per_env=1.5)),
           (np.zeros(1 << 16, np.int32), dict(rows_per_env=1 << 15)),      # 2^31 rows
           ("member", dict(rows_per_env=30))]
    for table, kw in bad:
        with pytest.raises(ValueError):
            b.assign(table, **kw)
    # a device table of the wrong dtype, shape or device (a meta tensor stands for "not on the host" where there is no GPU)
    for t in (torch.empty(5, dtype=torch.int64, device="meta"), torch.empty(5, dtype=torch.float32, device="meta"),
              torch.empty((5, 1), dtype=torch.int32, device="meta"), torch.empty(5, dtype=torch.int32, device="meta"),
              torch.empty(0, dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="contiguous int32 tensor"):
            b.assign(t, 30)
    assert b._route is None and b.routing() is None
    with pytest.raises(ValueError, match="entries must lie in \\[-1, 3\\)"):
        b.assign([0, 1, 3], 30)


def test_call_keeps_its_rows_check_without_an_assignment():
    b, torch = _bank_without_a_handle(3)
    b.in_dim = 8
    with pytest.raises(ValueError, match="no multiple of the 3 members"):
        b(torch.zeros(4, 8))
    assert np.array_equal(b.member_of_env(6), [0, 0, 1, 1, 2, 2])
    with pytest.raises(ValueError):
        b.member_of_env(5)


# -------------------------------------------------------------------------------------------------------------- the grid's bound
def test_tile_count_bound_against_brute_force():
    """grid = floor(rows / T) + min(M, E) >= sum_m ceil(c_m N / T) for every count vector with sum c_m <= E: each member wastes
    less than one tile, and at most min(M, E) members hold an env."""
    rng = np.random.default_rng(26)
    worst = 0
    for _ in range(4000):
        T = int(rng.choice([128, 256]))
        M = int(rng.integers(1, 257))
        E = int(rng.integers(1, 3000))
        N = int(rng.choice([1, 2, 30, 33, 64, 65, 127, 128, 129, 255, 256, 257, 1024]))
        kind = rng.integers(0, 4)
        if kind == 0:
            a = rng.integers(-1, M + 1, E)                     # with unserved envs
        elif kind == 1:
            a = rng.integers(0, M, E)
        elif kind == 2:
            a = np.full(E, M - 1)
        else:
            a = np.where(rng.random(E) < 0.5, 0, rng.integers(0, M, E))
        c = np.bincount(a[(a >= 0) & (a < M)], minlength=M)
        need = int(sum(-(-int(cm) * N // T) for cm in c))
        grid = (E * N) // T + min(M, E)
        assert need <= grid, (T, M, E, N, need, grid)
        worst = max(worst, grid - need)
    # the bound is tight: one env of one row per member wastes a whole tile each
    assert (5 * 1) // 128 + min(5, 5) == sum(-(-1 // 128) for _ in range(5)) == 5
    assert worst > 0


# ---------------------------------------------------------------------------------------------------- header, symbols, prototypes
def _declared_args(src, name):
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_symbols_and_prototypes_agree(lib):
    from marl_llm_amd._lib import ABI_VERSION, POLICY_SYMBOLS
    src = open(os.path.join(ROOT, "include", "swarm_policy.h")).read()
    assert ABI_VERSION == 5
    route = _declared_args(src, "swarm_policy_bank_route")
    assert [a.split()[-1].lstrip("*") for a in route] == ["p", "member_of_env", "n_env", "rows_per_env", "stream"]
    read = _declared_args(src, "swarm_policy_bank_route_read")
    assert [a.split()[-1].lstrip("*") for a in read] == ["p", "counts", "unserved", "env_order", "stream"]
    for n, args in (("swarm_policy_bank_route", route), ("swarm_policy_bank_route_read", read)):
        f = getattr(lib, n)
        assert n in POLICY_SYMBOLS and f.restype is ctypes.c_int and len(f.argtypes) == len(args)
        for a, t in zip(args, f.argtypes):
            assert t is (ctypes.c_int32 if a.startswith("int32_t ") and "*" not in a else ctypes.c_void_p), (n, a, t)
    ro = open(os.path.join(ROOT, "include", "swarm_rollout.h")).read()
    assert "swarm_policy_bank_route" in ro and "keep whatever" in ro
