"""CPU-side checks of swarm_policy_load_device / swarm_policy_read_packed (include/swarm_policy.h): both are exported, and a
null handle is refused before any device call -- with the message the header promises, or a negative size."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def test_symbols_exported(lib):
    from marl_llm_amd._lib import POLICY_SYMBOLS
    for n in ("swarm_policy_load_device", "swarm_policy_read_packed"):
        assert n in POLICY_SYMBOLS
        assert hasattr(lib, n), f"{n} not exported"


def test_load_device_refuses_a_null_handle(lib):
    w = (ctypes.c_float * 4)()
    ptr = ctypes.cast(w, ctypes.c_void_p)
    assert lib.swarm_policy_load_device(None, *[ptr] * 8, None) == 1
    assert lib.swarm_policy_last_error().startswith(b"swarm_policy_load_device:")


def test_read_packed_refuses_a_null_handle(lib):
    buf = (ctypes.c_ubyte * 16)()
    assert lib.swarm_policy_read_packed(None, None, 0, None) < 0
    assert lib.swarm_policy_read_packed(None, ctypes.cast(buf, ctypes.c_void_p), 16, None) < 0
    assert lib.swarm_policy_last_error().startswith(b"swarm_policy_read_packed:")
