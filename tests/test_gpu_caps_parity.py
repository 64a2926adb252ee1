"""The fused env step against the oracle across the LIST CAPS (topo, g_max, occ_max) and the OBSERVATION DTYPES, and the
host export beside it.  The other GPU files leave the caps at (6, 80, 200) for every step they compare and run every path-,
geometry- and edge-oriented comparison at obs_dtype float64; here

  a. every non-default row of helpers.CAPS_ROWS steps at float64 on the lattice, generic, forced-exact and full-geometry
     launches, walls and periodic, with and without the own-state block;
  b. float32 and bfloat16 handles step at the rows that reach each writer of the observation rows: the two-slots-per-lane
     sensed writer (g_max == 80), the wave-per-row one (every other g_max), the 4-value and the 2-value head stores
     (even / odd pairs per row);
  c. swarm_observe_host / swarm_step_host export rows shorter than, and no multiple of, k_export's 32-feature tile, in all
     three dtypes, with E N below, across and on its 64-row tile.

Tolerances are test_gpu_parity.py's and include/swarm_env.h's, none new: p, dp, the four index arrays, reward and done
bit-equal to the oracle; obs / a_prior equal to the oracle's double as helpers.as_obs_dtype rounds it -- float64 itself,
float32 cast once, bfloat16 cast to float32 and then to bfloat16 (both nearest-even; NOT double -> bfloat16 in one step).

Pattern of test_gpu_config_parity.py: the oracle's trajectory of a case (helpers.caps_trajectory: observe, then steps
alternating random float32 actions with the fed-back prior as a handle of that dtype returns it) is computed once and shared
by the debug-flag variants.  What the inputs reach -- capped and uncapped sensed lists, capped occupied lists, both rewards,
list lengths at which the integer cap and the reference's fp64 round() part ways, values on which one and two roundings to
bfloat16 differ -- is asserted without a GPU by test_oracle_vs_reference.py::test_caps_inputs_reach_the_caps on these same
calls.  The oracle is pinned to the reference at every row by test_step_matches_reference_across_list_caps there.
"""
import numpy as np
import pytest

from helpers import CAPS_DTYPE_NS, CAPS_DTYPE_ROWS, CAPS_NS, CAPS_ROWS, caps_trajectory, make_case, pad_cells
from lockstep import hold

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TORCH_DT = dict(f64=torch.float64, f32=torch.float32, bf16=torch.bfloat16)
FLAG_IDS = {0: "lattice", 1: "forced", 2: "generic", 4: "fullgeo"}
_REF = {}


def _shared(oracle, shapes, row, n_a, dtype="f64", periodic=False, with_self=True):
    """The oracle side of a case, computed once per session and never modified."""
    key = (row, n_a, dtype, periodic, with_self)
    if key not in _REF:
        _REF[key] = caps_trajectory(oracle, shapes, row, n_a, dtype, periodic, with_self)
    return _REF[key]


def _hold(cases, ref, ra, row, dtype="f64", flags=0, periodic=False, with_self=True):
    """lockstep.hold at the row's caps; returns its state, reward and index arrays (for the float64 twin of a narrower handle)."""
    topo, g_max, occ_max = CAPS_ROWS[row]
    return hold(cases, ref, lattice=0 if flags & 2 else len(cases), r_avoid=ra, is_boundary=not periodic, with_self=with_self,
                topo=topo, g_max=g_max, occ_max=occ_max, obs_dtype=TORCH_DT[dtype], debug_flags=flags)


# ---- a. the caps matrix, float64 ----
ROWS_A = [r for r in CAPS_ROWS if r != "default"]
MATRIX = [(r, n, f, False, True) for r in ROWS_A for n in CAPS_NS for f in (0, 2)]
MATRIX += [(r, n, 1, False, True) for r in ROWS_A for n in (8, 30, 64)]                               # forced exact
MATRIX += [(r, n, 4, False, True) for r in ("t1_g5", "t6_g33_o33", "t6_g79_o64") for n in CAPS_NS if n < 64]      # full geometry
MATRIX += [(r, n, f, True, True) for r in ("t3_g10_o7", "t6_g79_o64") for n in (8, 30, 64) for f in (0, 2)]        # periodic
MATRIX += [(r, n, f, False, False) for r in ("t3_g10_o7", "t6_g79_o64") for n in (8, 30, 64) for f in (0, 2)]      # NB = 7


def _id(c):
    return "%s-n%d-%s%s%s" % (c[0], c[1], FLAG_IDS[c[2]], "-periodic" if c[3] else "", "" if c[4] else "-noself")


@pytest.mark.parametrize("row,n_a,flags,periodic,with_self", MATRIX, ids=[_id(c) for c in MATRIX])
def test_caps_matrix(oracle, shapes, row, n_a, flags, periodic, with_self):
    """observe and four steps at non-default caps, obs_dtype float64, everything bit-equal to the oracle: the reward's walk
    over the capped and sub-sampled sensed list, the prior over a neighbour list cut to topo, the generic scan, the forced
    exact paths, the full geometry of N < 64, periodic, and no own-state block (seven head blocks: the head writer's
    division by a non-power-of-two)."""
    cases, ref, ra = _shared(oracle, shapes, row, n_a, "f64", periodic, with_self)
    _hold(cases, ref, ra, row, "f64", flags, periodic, with_self)


# ---- b. the dtype matrix ----
DTYPES = [(d, r, n, f, False, True) for d in ("f32", "bf16") for r in CAPS_DTYPE_ROWS for n in CAPS_DTYPE_NS for f in (0, 2)]
# the two-slot writer's "own rows" form deals different agents to a wave in the two geometries
DTYPES += [(d, "default", n, 4, False, True) for d in ("f32", "bf16") for n in CAPS_DTYPE_NS if n < 64]
DTYPES += [(d, "t6_g33_o33", 30, 0, True, True) for d in ("f32", "bf16")]
DTYPES += [(d, "default", 30, 0, False, False) for d in ("f32", "bf16")]


@pytest.mark.parametrize("dtype,row,n_a,flags,periodic,with_self", DTYPES, ids=[c[0] + "-" + _id(c[1:]) for c in DTYPES])
def test_dtype_matrix(oracle, shapes, dtype, row, n_a, flags, periodic, with_self):
    """float32 and bfloat16 handles at the rows of both sensed writers and both head stores: obs and a_prior equal the
    oracle's double rounded as as_obs_dtype states (the fed-back actions are the handle's own rounded priors, which the
    oracle was given), unused sensed slots are exactly zero, and the float64 twin run on the same inputs and actions gives
    the same state, reward and indices -- the obs dtype does not leak into the fp64 bits.  N = 100 and 200 on the generic
    path leave the two-slot writer a partial last 8-row group per wave."""
    cases, ref, ra = _shared(oracle, shapes, row, n_a, dtype, periodic, with_self)
    narrow = _hold(cases, ref, ra, row, dtype, flags, periodic, with_self)
    twin = _hold(cases, ref, ra, row, "f64", flags, periodic, with_self)
    for t, (a, b) in enumerate(zip(narrow, twin)):
        for k in a:
            assert np.array_equal(a[k], b[k]), (t, k)


# ---- c. the host export ----
EXPORT = [(d, r, ws, n, e, wp) for d in ("f64", "f32", "bf16")
          for r, ws in (("t1_g5", False), ("t6_g33_o33", True), ("default", True))         # D = 18, 98 = 3 * 32 + 2, 192
          for n, e in ((5, 3), (30, 3), (64, 2), (65, 2))                                   # E N = 15, 90, 128, 130 rows
          for wp in (True, False)]


@pytest.mark.parametrize("dtype,row,with_self,n_a,n_env,with_prior", EXPORT,
                         ids=["%s-%s-n%dx%d-%s" % (c[0], c[1], c[3], c[4], "prior" if c[5] else "noprior") for c in EXPORT])
def test_host_export(shapes, dtype, row, with_self, n_a, n_env, with_prior):
    """observe_host / step_host on one handle, observe / step on a twin with the same inputs, two steps (both pinned
    slots): the host block is the twin's tensors widened to float64 and transposed -- obs (D, E N) with column e N + i,
    a_prior (2, E N), reward (1, E N), done (1, E N), include/swarm_env.h swarm_host_out_t -- exactly.  Without with_prior
    the slot's a_prior array keeps what the caller put there."""
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.shapes import r_avoid_for
    topo, g_max, occ_max = CAPS_ROWS[row]
    rng = np.random.default_rng([list(CAPS_ROWS).index(row), n_a, n_env, 3])
    ra = r_avoid_for(n_a, shapes)
    cases = [make_case(rng, shapes, n_a, 1) for _ in range(n_env)]
    cells, n_g = pad_cells([c[2] for c in cases], max(c[2].shape[1] for c in cases) + 3)
    EN = n_env * n_a
    D = 4 * (topo + 1 + int(with_self)) + 2 * g_max
    pair = [SwarmBatch(n_env=n_env, n_agents=n_a, n_cells_max=cells.shape[2], r_avoid=ra, with_self=with_self, with_prior=with_prior,
                       topo=topo, g_max=g_max, occ_max=occ_max, obs_dtype=TORCH_DT[dtype]) for _ in range(2)]
    try:
        for sb in pair:
            sb.set_cells(cells, n_g, [c[3] for c in cases])
            sb.set_state(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]))
        host, twin = pair
        assert host.obs_dim == D == twin.obs_dim
        wide = lambda t, w: np.ascontiguousarray(t.reshape(EN, w).to(torch.float64).cpu().numpy().T)
        views = host.host_views()
        if not with_prior:
            for s, v in enumerate(views):
                v["a_prior"][:] = 7.0 + s
        o_h = host.observe_host()
        assert o_h.shape == (D, EN) and o_h.dtype == np.float64
        assert np.array_equal(o_h, wide(twin.observe(), D))
        slots = []
        for t in range(2):
            act = torch.from_numpy(rng.uniform(-1, 1, (n_env, n_a, 2)).astype(np.float32)).to(host.device)
            h = host.step_host(act)
            obs, rew, done, pri = twin.step(act)
            assert np.array_equal(h["obs"], wide(obs, D)), t
            assert h["reward"].shape == (1, EN) and np.array_equal(h["reward"][0], rew.reshape(EN).cpu().numpy().astype(np.float64)), t
            assert h["done"].shape == (1, EN) and h["done"].dtype == np.bool_ and not h["done"].any(), t
            assert h["a_prior"].shape == (2, EN)
            if with_prior:
                assert np.array_equal(h["a_prior"], wide(pri, 2)), t
            slots.append(h)
        assert not np.shares_memory(slots[0]["obs"], slots[1]["obs"])
        if not with_prior:
            for s, v in enumerate(views):
                assert (v["a_prior"] == 7.0 + s).all(), s
    finally:
        for sb in pair:
            sb.close()
