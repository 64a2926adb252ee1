"""CPU-side checks of the fused policy's C ABI (include/swarm_policy.h): swarm_policy_create validates its shapes and pointers
before it looks for a device, and swarm_policy_set_precision validates its argument, so every rejection below is decided
here, without a GPU, with SWARM_POLICY_ERR_INVALID and a message."""
import ctypes

import numpy as np
import pytest

ERR_INVALID = 1      # SWARM_POLICY_ERR_INVALID


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def _create(lib, in_dim, hidden, act_dim, null=None):
    """swarm_policy_create on fp32 host weights of the given shape (argument `null` of the eight passed as NULL)."""
    shapes = [(hidden, in_dim), (hidden,), (hidden, hidden), (hidden,), (hidden, hidden), (hidden,), (act_dim, hidden), (act_dim,)]
    ws = [np.zeros(max(1, int(np.prod(s))), np.float32) for s in shapes]
    ptrs = [None if i == null else ctypes.c_void_p(w.ctypes.data) for i, w in enumerate(ws)]
    h = ctypes.c_void_p()
    rc = lib.swarm_policy_create(*ptrs, in_dim, hidden, act_dim, -1, ctypes.byref(h))
    return rc, h, lib.swarm_policy_last_error()


@pytest.mark.parametrize("in_dim,hidden,act_dim", [
    (192, 192, 2),          # hidden 192: the padded feature that carries the constant one has no room
    (2, 180, 2), (6, 180, 2), (196, 180, 2), (0, 180, 2),        # in_dim: 4..192, multiple of 4
    (192, 180, 0), (192, 180, 5),                                 # act_dim: 1..4
    (192, 0, 2),
])
def test_unsupported_shapes_are_rejected_with_a_message(lib, in_dim, hidden, act_dim):
    rc, h, msg = _create(lib, in_dim, hidden, act_dim)
    assert rc == ERR_INVALID and not h.value
    assert msg.startswith(b"swarm_policy_create:") and b"hidden <= 191" in msg and b"act_dim <= 4" in msg


@pytest.mark.parametrize("null", range(8))
def test_null_weight_is_rejected_with_a_message(lib, null):
    rc, h, msg = _create(lib, 192, 180, 2, null=null)
    assert rc == ERR_INVALID and not h.value and msg == b"swarm_policy_create: null weight pointer"


def test_null_out_is_rejected(lib):
    w = np.zeros(192 * 192, np.float32)
    p = ctypes.c_void_p(w.ctypes.data)
    assert lib.swarm_policy_create(*([p] * 8), 192, 180, 2, -1, None) == ERR_INVALID


@pytest.mark.parametrize("precision", [-1, 2, 3, 1 << 30])
def test_set_precision_rejects_unknown_values(lib, precision):
    lib.swarm_policy_set_precision(None, 0)                         # reset the message
    assert lib.swarm_policy_set_precision(None, precision) == ERR_INVALID
    assert lib.swarm_policy_last_error() == b"swarm_policy_set_precision: bad argument"


@pytest.mark.parametrize("precision", [0, 1])
def test_set_precision_rejects_a_null_handle(lib, precision):
    assert lib.swarm_policy_set_precision(None, precision) == ERR_INVALID
    assert lib.swarm_policy_last_error() == b"swarm_policy_set_precision: bad argument"


def test_header_states_the_accepted_shapes():
    """The header, the code and the message agree: hidden <= 191."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "swarm_policy.h")).read()
    assert "hidden <= 191" in src and "hidden <= 192" not in src
