"""CPU-side checks of the device rollout loop's C ABI (include/swarm_rollout.h): every declared function is exported and
bound, the ring struct matches the header, and a call with a null handle or ring is rejected with a message (it never
reaches a device)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "swarm_rollout.h")


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def test_rollout_header_symbols_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(swarm_rollout[a-z0-9_]*)\s*\(", src)))
    from marl_llm_amd._lib import ROLLOUT_SYMBOLS
    assert names and set(names) == set(ROLLOUT_SYMBOLS), names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/swarm_rollout.h but not exported"


def test_ring_struct_matches_header():
    from marl_llm_amd._lib import SwarmRing
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct swarm_ring \{(.*?)\} swarm_ring_t;", src, flags=re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*;", body)
    assert [f[0] for f in SwarmRing._fields_] == fields
    assert ctypes.sizeof(SwarmRing) == 5 * 8 + 8 + 4 * 4


def test_null_handles_are_rejected_with_a_message(lib):
    from marl_llm_amd._lib import SwarmRing
    ring = SwarmRing()
    ring.n_slots, ring.rows = 2, 1
    args = (1, None, 0.0, 0, 0, 0, None, None)
    assert lib.swarm_rollout(None, None, ctypes.byref(ring), *args) == 1                 # SWARM_ERR_INVALID
    assert b"null env, policy or ring" in lib.swarm_rollout_last_error()
    lib.swarm_rollout_last_error()                                                       # wired up: a bytes message, callable twice
    fake = ctypes.c_void_p(8)                                                            # never dereferenced: the ring check comes first
    assert lib.swarm_rollout(fake, fake, None, *args) == 1
    assert lib.swarm_rollout_last_error().startswith(b"swarm_rollout:")


def test_policy_explore_at_is_bound(lib):
    f = lib.swarm_policy_forward_explore_at
    assert len(f.argtypes) == 10 and f.argtypes[8] is ctypes.c_uint64
    assert lib.swarm_policy_forward_explore_at(None, None, 0, 0, None, 0.0, 0, 0, 0, None) == 1     # SWARM_POLICY_ERR_INVALID
    assert b"bad argument" in lib.swarm_policy_last_error()
