"""marl_llm_amd.build decides by unit what to compile (CPU only; nothing is compiled here beyond the build_lib() that the
other CPU tests call too): the decision, stale_units(), on file times moved with os.utime and put back."""
import contextlib
import glob
import os
import time

import pytest

from marl_llm_amd import build

CSRC = os.path.join(build.PKG, "csrc")
ALL = [name for name, _, _ in build.UNITS]


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_lib()


@contextlib.contextmanager
def newer(path):
    """`path` modified a minute from now, for the length of the block"""
    st = os.stat(path)
    try:
        os.utime(path, (st.st_atime, time.time() + 60))
        yield
    finally:
        os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns))


def test_nothing_changed_nothing_stale():
    assert build.stale_units() == []


def test_newer_source_makes_its_unit_stale():
    with newer(os.path.join(CSRC, "env_api.hip")):
        assert build.stale_units() == ["env_api"]
    with newer(os.path.join(CSRC, "swarm_env.hip")):
        assert build.stale_units() == [n for n in ALL if n.startswith("swarm_env_")]
    assert build.stale_units() == []


@pytest.mark.parametrize("header", [os.path.join(CSRC, "env_types.h"), os.path.join(build.INC, "swarm_policy.h")])
def test_newer_header_makes_every_unit_stale(header):
    with newer(header):
        assert build.stale_units() == ALL
    assert build.stale_units() == []


def test_other_defines_make_every_unit_stale():
    assert build.stale_units(defines=["-DSWARM_WPS=6"]) == ALL
    # ... also where the objects are the same files: the command line kept beside each object no longer matches
    flags = list(build.HIPCC_FLAGS)
    try:
        build.HIPCC_FLAGS.append("-DSWARM_WPS=6")
        assert build.stale_units() == ALL
    finally:
        build.HIPCC_FLAGS[:] = flags
    assert build.stale_units() == []


def test_units_name_every_source():
    sources = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")))
    assert sorted(set(src for _, src, _ in build.UNITS)) == sources
    assert len(set(ALL)) == len(ALL)
    cuts = [d for _, src, d in build.UNITS if src == "swarm_env.hip"]
    assert sorted(cuts) == sorted(["-DSWARM_ENV_UNIT=%d" % n] for n in (0, 8, 16, 32, 64, 128, 256))
    assert all(d == [] for _, src, d in build.UNITS if src != "swarm_env.hip")


def test_variants_have_their_own_objects_and_library():
    plain, stamps, exp = build.variant(), build.variant(stamps=True), build.variant(["-DSWARM_WPS=6"])
    assert plain[1] == build.LIB and stamps[1] == os.path.join(build.LIB_DIR, "libswarmenv_stamps.so")
    assert len(set([plain[0], stamps[0], exp[0]])) == 3 and len(set([plain[1], stamps[1], exp[1]])) == 3
    assert "-DSWARM_STAMPS" in build.unit_cmd("env_api", stamps=True) and "-DSWARM_STAMPS" not in build.unit_cmd("env_api")
    assert build.unit_cmd("swarm_env_n64", ["-DSWARM_WPS=6"])[-3:] == ["-DSWARM_WPS=6", "-DSWARM_ENV_UNIT=64", os.path.join(CSRC, "swarm_env.hip")]
