"""CPU-side checks of swarm_policy_create_wide (include/swarm_policy.h): shapes and pointers are validated before the call looks
for a device, so every rejection below is decided here, without a GPU, with SWARM_POLICY_ERR_INVALID, a null handle and a
message that starts "swarm_policy_create_wide:" and names the three limits; a shape that passes validation fails here with
"no HIP device" (on a machine with a device the same call succeeds: tests/test_gpu_policy_wide.py)."""
import ctypes

import numpy as np
import pytest

ERR_INVALID, ERR_HIP = 1, 2      # SWARM_POLICY_ERR_INVALID, SWARM_POLICY_ERR_HIP


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def _create_wide(lib, in_dim, hidden, act_dim, null=None):
    """swarm_policy_create_wide on fp32 host weights of the given shape (argument `null` of the eight passed as NULL)."""
    shapes = [(hidden, in_dim), (hidden,), (hidden, hidden), (hidden,), (hidden, hidden), (hidden,), (act_dim, hidden), (act_dim,)]
    ws = [np.zeros(max(1, int(np.prod(s))), np.float32) for s in shapes]
    ptrs = [None if i == null else ctypes.c_void_p(w.ctypes.data) for i, w in enumerate(ws)]
    h = ctypes.c_void_p()
    rc = lib.swarm_policy_create_wide(*ptrs, in_dim, hidden, act_dim, -1, ctypes.byref(h))
    return rc, h, lib.swarm_policy_last_error()


def _has_device():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


@pytest.mark.parametrize("in_dim,hidden,act_dim", [
    (388, 180, 2), (386, 180, 2), (2, 180, 2), (0, 180, 2),       # in_dim: 4..384, multiple of 4
    (192, 257, 2), (192, 0, 2),                                   # hidden: 1..256
    (192, 180, 0), (192, 180, 5),                                 # act_dim: 1..4
])
def test_unsupported_shapes_are_rejected_with_a_message(lib, in_dim, hidden, act_dim):
    rc, h, msg = _create_wide(lib, in_dim, hidden, act_dim)
    assert rc == ERR_INVALID and not h.value
    assert msg.startswith(b"swarm_policy_create_wide:")
    assert b"in_dim <= 384" in msg and b"hidden <= 256" in msg and b"act_dim <= 4" in msg


@pytest.mark.parametrize("null", range(8))
def test_null_weight_is_rejected_with_a_message(lib, null):
    rc, h, msg = _create_wide(lib, 384, 256, 2, null=null)
    assert rc == ERR_INVALID and not h.value and msg == b"swarm_policy_create_wide: null weight pointer"


def test_null_out_is_rejected(lib):
    w = np.zeros(384 * 256, np.float32)
    p = ctypes.c_void_p(w.ctypes.data)
    assert lib.swarm_policy_create_wide(*([p] * 8), 384, 256, 2, -1, None) == ERR_INVALID


@pytest.mark.parametrize("in_dim,hidden,act_dim", [(384, 256, 4), (196, 180, 2), (192, 192, 2)])
def test_shapes_past_the_narrow_limits_pass_validation(lib, in_dim, hidden, act_dim):
    """Both maxima and the first shape past each narrow limit: without a device the call gets as far as looking for one."""
    rc, h, msg = _create_wide(lib, in_dim, hidden, act_dim)
    if _has_device():
        assert rc == 0 and h.value
        lib.swarm_policy_destroy(h)
    else:
        assert rc == ERR_HIP and not h.value
        assert msg.startswith(b"swarm_policy_create_wide:") and b"no HIP device" in msg


def test_the_narrow_create_keeps_its_limits(lib):
    """swarm_policy_create still refuses what only the wide kernel serves, with its own message."""
    shapes = [(180, 196), (180,), (180, 180), (180,), (180, 180), (180,), (2, 180), (2,)]
    ws = [np.zeros(int(np.prod(s)), np.float32) for s in shapes]
    h = ctypes.c_void_p()
    rc = lib.swarm_policy_create(*[ctypes.c_void_p(w.ctypes.data) for w in ws], 196, 180, 2, -1, ctypes.byref(h))
    assert rc == ERR_INVALID and not h.value and lib.swarm_policy_last_error().startswith(b"swarm_policy_create:")


def test_header_declares_the_symbol_and_its_limits():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "swarm_policy.h")).read()
    assert "swarm_policy_create_wide(" in src and "in_dim <= 384" in src and "hidden <= 256" in src
