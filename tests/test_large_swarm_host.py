"""CPU-side checks of the large-swarm switch (include/swarm_env.h: swarm_config_t.large_swarm): the field sits where the
reserved int32 sat, the struct's size and the ABI version are what they were, the default is off, and swarm_create's
validation -- which runs before it looks for a device -- accepts n_agents in [1, 1024] with the switch and [1, 256] without."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    return _lib.load()


def _create(lib, **fields):
    """swarm_create of the default config with `fields` set -> (rc, message); a handle that was created is destroyed."""
    from marl_llm_amd._lib import SwarmConfig
    cfg = SwarmConfig()
    lib.swarm_default_config(ctypes.byref(cfg))
    for k, v in fields.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    rc = lib.swarm_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = lib.swarm_last_error(None).decode() if rc else ""
    if h.value:
        lib.swarm_destroy(h)
    return rc, msg


def test_struct_field_replaces_the_reserved_one(lib):
    from marl_llm_amd._lib import ABI_VERSION, SwarmConfig
    names = [f[0] for f in SwarmConfig._fields_]
    assert names[-1] == "large_swarm" and names[-2] == "llm_action" and "reserved_" not in names
    assert SwarmConfig.large_swarm.offset == SwarmConfig.llm_action.offset + 4 and SwarmConfig.large_swarm.size == 4
    assert ctypes.sizeof(SwarmConfig) == 12 * 4 + 12 * 8 + 4 * 8 + 2 * 4           # tests/test_abi.py's figure
    assert ABI_VERSION == 5 and lib.swarm_abi_version() == 5
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "swarm_env.h")).read(), flags=re.S)
    body = header[header.index("typedef struct swarm_config {"): header.index("} swarm_config_t;")]
    members = re.findall(r"\b(?:int32_t|double)\s+([^;]+);", body)
    assert members[-1].strip() == "large_swarm" and members[-2].strip() == "llm_action" and "reserved_" not in body


def test_default_is_off(lib):
    from marl_llm_amd._lib import SwarmConfig
    cfg = SwarmConfig()
    cfg.large_swarm = 7
    lib.swarm_default_config(ctypes.byref(cfg))
    assert cfg.large_swarm == 0


def test_large_swarm_passes_validation_above_256(lib):
    """n_agents = 300 with the switch gets past validation: to a handle on a machine with a device, to SWARM_ERR_HIP without."""
    for n in (300, 1024, 1, 256):
        rc, msg = _create(lib, n_agents=n, large_swarm=1)
        assert rc in (0, 2), (n, rc, msg)
        if rc == 2:
            assert "no CPU path" in msg, msg


def test_default_handle_still_refuses_above_256(lib):
    rc, msg = _create(lib, n_agents=300, large_swarm=0)
    assert rc == 1 and msg == "n_agents must be in [1, 256]"
    rc, msg = _create(lib, n_agents=257)
    assert rc == 1 and msg == "n_agents must be in [1, 256]"


def test_large_swarm_names_its_own_range(lib):
    for n in (1025, 0, 4096):
        rc, msg = _create(lib, n_agents=n, large_swarm=1)
        assert rc == 1 and "[1, 1024]" in msg and "n_agents" in msg, (n, rc, msg)


def test_switch_takes_zero_or_one(lib):
    rc, msg = _create(lib, n_agents=30, large_swarm=2)
    assert rc == 1 and "large_swarm" in msg
