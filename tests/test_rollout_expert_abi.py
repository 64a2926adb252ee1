"""CPU-side checks of swarm_rollout_expert (include/swarm_rollout.h): the entry point is exported and bound, and a call with
a bad source, a null handle or a null ring is rejected with a message before it could reach a device."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def test_expert_entry_point_is_exported_and_bound(lib):
    from marl_llm_amd import _lib
    assert "swarm_rollout_expert" in _lib.ROLLOUT_SYMBOLS
    f = lib.swarm_rollout_expert
    assert f.restype is ctypes.c_int and len(f.argtypes) == 6
    assert f.argtypes[2] is ctypes.c_int32 and f.argtypes[3] is ctypes.c_int32
    assert (_lib.EXPERT_RULE, _lib.EXPERT_LLM) == (0, 1)


def test_null_env_and_ring_are_rejected_with_a_message(lib):
    from marl_llm_amd._lib import EXPERT_LLM, EXPERT_RULE, SwarmRing
    ring = SwarmRing()
    ring.n_slots, ring.rows = 2, 1
    for src in (EXPERT_RULE, EXPERT_LLM):
        assert lib.swarm_rollout_expert(None, ctypes.byref(ring), 1, src, None, None) == 1        # SWARM_ERR_INVALID
        assert lib.swarm_rollout_last_error() == b"swarm_rollout_expert: null env or ring"
    fake = ctypes.c_void_p(8)                                                                   # never dereferenced
    assert lib.swarm_rollout_expert(fake, None, 1, EXPERT_RULE, None, None) == 1
    assert lib.swarm_rollout_last_error() == b"swarm_rollout_expert: null env or ring"


@pytest.mark.parametrize("source", [-1, 2, 7])
def test_bad_source_is_rejected_with_a_message(lib, source):
    from marl_llm_amd._lib import SwarmRing
    ring = SwarmRing()
    ring.n_slots, ring.rows = 2, 1
    fake = ctypes.c_void_p(8)                                                                   # the source check comes first
    assert lib.swarm_rollout_expert(fake, ctypes.byref(ring), 1, source, None, None) == 1
    msg = lib.swarm_rollout_last_error()
    assert msg.startswith(b"swarm_rollout_expert: source must be") and b"SWARM_EXPERT_RULE" in msg
