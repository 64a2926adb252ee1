"""CPU-side checks of the evaluation loop's C ABI (include/swarm_rollout.h swarm_rollout_eval, include/swarm_env.h
swarm_select_shape): declared, exported and bound with the headers' argument counts, the output struct matches the header,
and calls with null handles are rejected with a message (they never reach a device)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def declared_args(src, fn):
    """Number of parameters of `fn` as the header declares it."""
    args = re.search(r"\b%s\s*\((.*?)\)\s*;" % fn, src, flags=re.S).group(1)
    return len([a for a in args.split(",") if a.strip()])


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from marl_llm_amd import _lib
    ro, env = header("swarm_rollout.h"), header("swarm_env.h")
    assert "swarm_rollout_eval" in _lib.ROLLOUT_SYMBOLS and "swarm_select_shape" in _lib.BATCHED_SYMBOLS
    f, g = lib.swarm_rollout_eval, lib.swarm_select_shape
    assert f.restype is ctypes.c_int and len(f.argtypes) == declared_args(ro, "swarm_rollout_eval") == 7
    assert f.argtypes[3] is ctypes.c_int32
    assert g.restype is ctypes.c_int and len(g.argtypes) == declared_args(env, "swarm_select_shape") == 3
    assert g.argtypes[1] is ctypes.c_int32


def test_eval_out_struct_matches_header():
    from marl_llm_amd._lib import SwarmEvalOut
    body = re.search(r"typedef struct swarm_eval_out \{(.*?)\} swarm_eval_out_t;", header("swarm_rollout.h"), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        fields += re.findall(r"\*\s*(\w+)", decl)
    assert [f[0] for f in SwarmEvalOut._fields_] == fields == ["metrics", "p", "dp", "reward_stats"]
    assert ctypes.sizeof(SwarmEvalOut) == 4 * 8


def test_null_handles_are_rejected_with_a_message(lib):
    from marl_llm_amd._lib import SwarmEvalOut, SwarmRing
    ring = SwarmRing()
    ring.n_slots, ring.rows = 2, 1
    out = SwarmEvalOut()
    fake = ctypes.c_void_p(8)                                   # never dereferenced: the null checks come first
    for env, pol, r in ((None, fake, ctypes.byref(ring)), (fake, None, ctypes.byref(ring)), (fake, fake, None)):
        assert lib.swarm_rollout_eval(env, pol, r, 1, None, ctypes.byref(out), None) == 1      # SWARM_ERR_INVALID
        msg = lib.swarm_rollout_last_error()
        assert msg.startswith(b"swarm_rollout_eval:") and b"null env, policy or ring" in msg


def test_select_shape_rejects_a_null_handle(lib):
    assert lib.swarm_select_shape(None, 0, None) == 1               # SWARM_ERR_INVALID
