"""CPU-side checks of the per-workgroup cell path's public surface: swarm_path_envs is declared, bound and exported, a NULL
handle is an error, both sides of the ctypes boundary carry ABI version 5, and appending KP::path_filter moved none of the
kernel argument's existing fields -- the lattice launches' LDS map, which env_layout writes into those fields and
swarm_debug_lds_map reads back out of them, still answers as before."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "swarm_env.h")
# swarm_debug_lds_map(npad, half, 80): smem_lat, smem_lat_export, g_stride, off_orow, as they stood before KP grew
LDS_AT_G80 = {(8, 0): (31040, 35136, 82, 31040), (16, 1): (24128, 28224, 82, 24128), (32, 0): (24128, 28224, 82, 24128),
              (64, 0): (22976, 27072, 82, 22976), (128, 0): (46848, 55040, 82, 46848), (256, 0): (96640, 113024, 82, 96640)}


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def test_path_envs_is_declared_bound_and_exported(lib):
    from marl_llm_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+swarm_path_envs\s*\(\s*swarm_env_t\s*\*\s*h\s*,\s*int32_t\s*\*\s*walk_envs\s*,\s*int32_t\s*\*\s*scan_envs\s*\)", src)
    assert "swarm_path_envs" in _lib.BATCHED_SYMBOLS
    assert hasattr(lib, "swarm_path_envs")
    from marl_llm_amd.batched import SwarmBatch
    assert callable(getattr(SwarmBatch, "path_envs", None))


def test_null_handle_is_an_error(lib):
    w, s = ctypes.c_int32(-7), ctypes.c_int32(-7)
    assert lib.swarm_path_envs(None, ctypes.byref(w), ctypes.byref(s)) == 1          # SWARM_ERR_INVALID
    assert (w.value, s.value) == (-7, -7)
    assert lib.swarm_path_envs(None, None, None) == 1


def test_abi_version_is_5_on_both_sides(lib):
    from marl_llm_amd import _lib
    assert _lib.ABI_VERSION == 5
    assert lib.swarm_abi_version() == 5
    assert re.search(r"#define\s+SWARM_ABI_VERSION\s+5\b", open(HEADER).read())


@pytest.mark.parametrize("npad,half", sorted(LDS_AT_G80))
def test_kp_fields_keep_their_places(lib, npad, half):
    f = lib.swarm_debug_lds_map
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    out = (ctypes.c_int * 32)()
    assert f(npad, half, 80, out) == 0
    assert (out[0], out[1], out[2], out[3]) == LDS_AT_G80[(npad, half)]
    assert list(out[16:28]) == list(out[4:16])          # KP's run-time offsets are the kernel's compile-time map
