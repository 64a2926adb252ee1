"""CPU-side check of the lattice launches' LDS map.  The kernel addresses its LDS regions through compile-time offsets
(LatMap in csrc/swarm_env.hip) and the host sizes the launches from the same struct, so the two cannot drift from each other;
what CAN move is the map itself.  This file restates the layout independently -- region sizes from the geometry, 16-byte
alignment, the sensed lists last -- and holds every lattice instantiation's offsets and totals to it, with the dynamic LDS
of every instantiation at the reference's list length written out as literals."""
import ctypes

import pytest

GEOMETRIES = [(8, 0), (8, 1), (16, 0), (16, 1), (32, 0), (32, 1), (64, 0), (128, 0), (256, 0)]
G_MAX = [1, 7, 80, 81, 240]          # the reference's list length, odd / tiny ones, the longest a 15-row window can hold
REGIONS = ["sp", "hdr", "srow", "pcr", "partc", "partd", "lat", "cov", "flag", "snei", "sncf", "sidx"]
# (smem_lat, smem_lat_export) at g_max = 80, as the layout stood before the map became compile-time
AT_G80 = {(8, 0): (31040, 35136), (8, 1): (26432, 30528), (16, 0): (26432, 30528), (16, 1): (24128, 28224),
          (32, 0): (24128, 28224), (32, 1): (22976, 27072), (64, 0): (22976, 27072), (128, 0): (46848, 55040),
          (256, 0): (96640, 113024)}


@pytest.fixture(scope="module")
def fn():
    from marl_llm_amd.build import build_lib
    from marl_llm_amd import _lib
    build_lib()
    f = _lib.load().swarm_debug_lds_map
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return f


def g_stride(g_max):
    half = (g_max + 1) // 2
    if half % 2 == 0:
        half += 1                      # odd dword stride
    return 2 * half


def restated(npad, half, g_max):
    """The layout from the geometry alone: (offsets by region, smem_lat, off_orow, smem_lat_export)."""
    ag = max(64, npad)
    epb = (64 // npad) // (2 if half else 1) if npad < 64 else 1
    nw, wpe, nrc, nei_stride = ag // 64, 4, 16, 8
    pm = (wpe * 4 if nw == 1 else 5) * nw * ag * 8
    sizes = [("sp", 4 * ag * 8), ("hdr", ag * 16), ("srow", max((nrc - 1) * ag * 4, nw * 1536)), ("pcr", ag * nrc),
             ("partc", wpe * ag * 2), ("partd", (wpe - 1) * ag * 8), ("lat", epb * 64 * 10), ("cov", epb * 64 * 8),
             ("flag", ag), ("snei", ag * nei_stride * 2), ("sncf", ag * 4), ("snear", nw * ag * 8 if nw > 1 else 0),
             ("sidx", max(ag * g_stride(g_max) * 2, pm))]
    off, offs = 0, {}
    for name, size in sizes:
        offs[name] = off
        off = (off + size + 15) & ~15
    return offs, off, off, off + nrc * ag * 4


@pytest.mark.parametrize("npad,half", GEOMETRIES)
def test_map_equals_restated_layout(fn, npad, half):
    for g in G_MAX:
        out = (ctypes.c_int * 32)()
        assert fn(npad, half, g, out) == 0
        offs, smem_lat, off_orow, smem_exp = restated(npad, half, g)
        assert out[2] == g_stride(g)
        assert (out[0], out[1], out[3]) == (smem_lat, smem_exp, off_orow)
        assert {r: out[4 + q] for q, r in enumerate(REGIONS)} == {r: offs[r] for r in REGIONS}
        # the run-time copy of the map, read by the geometries that do not take the constants (full-occupancy N < 64)
        assert {r: out[16 + q] for q, r in enumerate(REGIONS)} == {r: offs[r] for r in REGIONS}
        assert out[28] == (1 if (npad >= 64 or half) else 0)
        # aliasing: the wave permutations (T bytes) fit part_d, the exact reward's scratch fits the window rows
        ag = max(64, npad)
        assert 4 * ag <= offs["lat"] - offs["partd"] and (ag // 64) * 1536 <= offs["pcr"] - offs["srow"]


@pytest.mark.parametrize("npad,half", GEOMETRIES)
def test_dynamic_lds_at_reference_list_length(fn, npad, half):
    out = (ctypes.c_int * 32)()
    assert fn(npad, half, 80, out) == 0
    assert (out[0], out[1]) == AT_G80[(npad, half)]
    assert out[1] <= 160 * 1024


def test_no_instantiation_is_refused(fn):
    out = (ctypes.c_int * 32)()
    assert fn(48, 0, 80, out) == -1 and fn(64, 1, 80, out) == -1 and fn(64, 0, 0, out) == -1
