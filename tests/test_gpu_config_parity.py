"""The fused env step against the oracle AWAY from the reference's constants: every field of swarm_config_t that the other
GPU files only ever run at its default -- size_a, k_ball, k_wall, c_wall, vel_max, dt, boundary, d_sen, r_avoid beyond
r_avoid_for, prior_gain -- and with them what swarm_create derives: the squared cut-offs, the pre-selection radii and their
cap at c_sen, the fp32 bands sized from the arena, the lattice gate, the wraps' w_half / h_half.

Pattern of test_gpu_parity.test_batched_trajectories_vs_oracle: E envs, obs_dtype float64, observe, then free-running steps
that alternate random float32 actions with the fed-back prior; after every step p, dp, obs, a_prior, reward and the four
index arrays equal E sequential oracle steps given the same constants.  Tolerance: none (include/swarm_env.h: exact), with
test_gpu_parity.py's caveat about the reward's cos().  The oracle is pinned to the reference at these values by
test_oracle_vs_reference.py.

The oracle's trajectory of a set of envs is computed once (helpers.oracle_run) and shared by the debug-flag variants; it
also counts what the inputs reached -- contacts, each wall, velocity clips, each edge's wrap, wrap-only neighbours -- and
every test asserts those counts, from the oracle alone, before it looks at the device.  The seeds in the parametrisations
are ones for which they hold.

Not here: llm_repulsion.  The 'llm' twin is the oracle's prior with another repulsion gain only up to np.linalg.norm's
rounding (the recorded g10_llm_n32 actions differ from orc_action_prior_g(2, 1, 2) by an ulp in 33 of 384 components), so
there is no exact reference to hold a non-default gain to; test_gpu_llm.py keeps its 1e-12 at the default.
"""
import copy

import numpy as np
import pytest

from helpers import BIG_BOX, DEFAULT_BOX, DYNAMICS_ROWS, OFF_BOX, adversarial_case, config_case, oracle_run, physics, random_actions
from lockstep import hold

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_REF = {}


def _ra(n_a, shapes):
    from marl_llm_amd.shapes import r_avoid_for
    return r_avoid_for(n_a, shapes)


def _shared(key, make):
    """The oracle side of a parametrisation, computed once per session and never modified."""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _hold(cases, ref, ra, *, d_sen=0.4, boundary=DEFAULT_BOX, periodic=False, prior_gain=(2.0, 3.0, 2.0), flags=0, lattice=None, **phys):
    """lockstep.hold with the given constants at obs_dtype float64."""
    hold(cases, ref, lattice=lattice, r_avoid=ra, d_sen=d_sen, boundary=boundary, is_boundary=not periodic,
         obs_dtype=torch.float64, debug_flags=flags, prior_gain=prior_gain, **physics(**phys))


def _free_run(oracle, shapes, seed, n_a, *, boundary=DEFAULT_BOX, periodic=False, d_sen=0.4, r_avoid=None, prior_gain=(2.0, 3.0, 2.0),
              far=False, **phys):
    """config_case envs, their action schedule and the oracle's trajectory with its counts, conditions asserted."""
    ph = physics(**phys)
    rng = np.random.default_rng(seed)
    E, T = (4, 5) if n_a <= 64 else (3, 4)
    ra = _ra(n_a, shapes) if r_avoid is None else r_avoid
    cases = [config_case(rng, shapes, n_a, boundary, ph["size_a"], ph["vel_max"], ph["dt"]) for _ in range(E)]
    if far:                 # beyond coord_lim = 1.5 max|boundary| + 1 = 4.6: the lanes that take the exact path outright
        for p, dp, g, l in cases:
            p[:, 8:13] = [[11.0, -40.0, 3.0, 11.5, 40.0], [0.5, 1.0, 40.0, -11.0, 40.25]]
    ref = oracle_run(oracle, cases, random_actions(rng, T, E, n_a), ra, d_sen=d_sen, boundary=boundary, periodic=periodic,
                     prior_gain=prior_gain, **ph)
    c = ref[2]
    assert c["contact"] >= 1 and c["clip"] >= 1, c
    if periodic:
        assert (c["wrap"] >= 1).all() and c["wrap_only"] >= 1, c
        for o in ref[0]:    # 0-2 are neighbours through the x wrap alone, 1-3 through the y wrap alone
            assert 2 in o["neighbor_index"][0] and 3 in o["neighbor_index"][1]
    else:
        assert (c["wall"] >= 1).all(), c
    if ph["size_a"] != 0.035:          # a pair that is a contact for exactly one of this size_a and the default one
        b = np.array(boundary, np.float64)
        for p, dp, g, l in cases:
            assert (oracle.dist_b2b(p, b, periodic, ph["size_a"])[2] != oracle.dist_b2b(p, b, periodic, 0.035)[2]).any()
    return cases, ref, ra


# ---- a. dynamics: one constant at a time, then all together (lattice path: dynamics do not touch the cell scan) ----
DYNAMICS = [(name, mode, n_a, 1) for name, _ in DYNAMICS_ROWS for mode in ("walls", "periodic") for n_a in (8, 30, 64)]
DYNAMICS += [("all", mode, n_a, 1) for mode in ("walls", "periodic") for n_a in (100, 256)]


@pytest.mark.parametrize("name,mode,n_a,seed", DYNAMICS, ids=["%s-%s-n%d-s%d" % r for r in DYNAMICS])
def test_dynamics_constants(oracle, shapes, name, mode, n_a, seed):
    """size_a (c_ball and both wall terms), k_ball, k_wall, c_wall, vel_max and dt (used twice) away from their defaults:
    every env set has an agent-agent contact, a contact with each of the four walls (walls mode) or a wrap at each edge
    (periodic), a clipped velocity component, and for size_a a pair whose contact a defaulted c_ball would flip."""
    phys = dict(DYNAMICS_ROWS)[name]
    periodic = mode == "periodic"
    cases, ref, ra = _shared(("dyn", name, mode, n_a, seed), lambda: _free_run(oracle, shapes, [seed, n_a, periodic], n_a, periodic=periodic, **phys))
    _hold(cases, ref, ra, periodic=periodic, lattice=len(cases), **phys)


# ---- b. arena ----
OFF = [(mode, name, n_a, 1) for mode in ("walls", "periodic") for name in ("default", "all") for n_a in (8, 30, 64)]
OFF += [(mode, "all", n_a, 1) for mode in ("walls", "periodic") for n_a in (100, 256)]


@pytest.mark.parametrize("mode,name,n_a,seed", OFF, ids=["%s-%s-n%d-s%d" % r for r in OFF])
def test_off_centre_box(oracle, shapes, mode, name, n_a, seed):
    """boundary = (-1.5, 2.0, 3.0, -1.0): w_half = 2.25, h_half = 1.5, no edge pair symmetric about the origin.  Walls: a
    contact with each wall.  Periodic: an absolute wrap at each of the four edges, neighbour pairs that exist only through
    the x wrap and only through the y wrap (the entry disappears from the oracle's list with is_periodic=False), and
    agent 0 in contact through the wrap (the one row the reference's distance matrix wraps)."""
    phys = dict(DYNAMICS_ROWS)[name] if name != "default" else {}
    periodic = mode == "periodic"
    cases, ref, ra = _shared(("off", name, mode, n_a, seed),
                             lambda: _free_run(oracle, shapes, [seed, n_a, periodic, 7], n_a, boundary=OFF_BOX, periodic=periodic, **phys))
    _hold(cases, ref, ra, boundary=OFF_BOX, periodic=periodic, lattice=len(cases), **phys)


def _threshold_run(oracle, shapes, seed, n_a, n_env, *, d_sen=0.4, r_avoid=None, size_a=0.035, boundary=DEFAULT_BOX, reach=None):
    """adversarial_case envs (test_gpu_parity.test_threshold_adversarial_inputs' inputs, thresholds at this d_sen, r_avoid
    and 2 size_a) with the oracle's observation and one zero-action step: the agents stay near the thresholds.
    reach: the shape is first moved into a corner of the arena so that its cells reach |coordinate| = reach."""
    rng = np.random.default_rng(seed)
    ra = _ra(n_a, shapes) if r_avoid is None else r_avoid
    cases = []
    for e in range(n_env):
        shift = None
        if reach is not None:
            g = adversarial_case(copy.deepcopy(rng), shapes, n_a, ra, d_sen, 2 * size_a)[2]          # preview of the shape's pose
            sx, sy = [(-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0), (1.0, 1.0)][e % 4]
            shift = np.array([[sx * reach - (g[0].max() if sx > 0 else g[0].min())], [sy * reach - (g[1].max() if sy > 0 else g[1].min())]])
        p, dp, g, l_cell = adversarial_case(rng, shapes, n_a, ra, d_sen, 2 * size_a, shift)
        if reach is not None:
            assert abs(np.abs(g).max() - reach) < 1e-9
        # Two agents sent to the same lattice vertex +- 1e-16 are the same doubles out here (an ulp of 5 is 9e-16).  Which of
        # two coincident agents the reference drops as "self" is its std::sort's choice among ties (deviation 1:
        # the oracle drops the lower index, the kernel the agent itself), so nothing exact can be asked there: the later one
        # moves 1e-9 aside -- still one of the placements' own offsets from the vertex.
        for j in range(1, n_a):
            while (p[:, :j] == p[:, [j]]).all(axis=0).any():
                p[0, j] += 1e-9
        cases.append((p, dp, g, l_cell))
    ref = oracle_run(oracle, cases, [np.zeros((n_env, n_a, 2), np.float32)], ra, d_sen=d_sen, boundary=boundary, size_a=size_a)
    return cases, ref, ra


@pytest.mark.parametrize("flags", [0, 1, 2], ids=["lattice", "forced", "generic"])
@pytest.mark.parametrize("n_a,n_env", [(30, 8), (64, 8), (256, 4)])
def test_big_box_thresholds(oracle, shapes, n_a, n_env, flags):
    """boundary = (-6, 6, 6, -6): the fp32 bands are sized from S = 1.5 * 6 + 1 = 10 instead of 4.6.  The threshold
    placements of test_threshold_adversarial_inputs on shapes pushed into the four corners, cells out to |coordinate| =
    5.5, where an fp32 coordinate carries 2.3 times the rounding error it has inside the default arena (a scratch build with
    bands a fiftieth as wide fails the generic rows here).  Fast, forced-exact and generic paths all equal the oracle."""
    cases, ref, ra = _shared(("big", n_a), lambda: _threshold_run(oracle, shapes, 600 + n_a, n_a, n_env, boundary=BIG_BOX, reach=5.5))
    _hold(cases, ref, ra, boundary=BIG_BOX, flags=flags, lattice=0 if flags & 2 else n_env)


@pytest.mark.parametrize("flags", [0, 2], ids=["lattice", "generic"])
@pytest.mark.parametrize("n_a,seed", [(30, 1), (64, 1)])
def test_agents_beyond_the_band_limit(oracle, shapes, n_a, seed, flags):
    """Walls, default box: five agents at coordinates 11 and 40, beyond coord_lim = 4.6, for which the bands were not
    derived -- those lanes must take the exact path (and the wall spring, thousands of units, clips them at vel_max);
    everyone else stays inside."""
    cases, ref, ra = _shared(("far", n_a, seed), lambda: _free_run(oracle, shapes, [seed, n_a, 11], n_a, far=True))
    assert all((np.abs(s["p"]) > 4.6).any(axis=0).sum() == 5 for row in ref[1] for s in row)
    _hold(cases, ref, ra, flags=flags, lattice=0 if flags & 2 else len(cases))


# ---- c. sensing ----
SENSING = [(0.25, None), (0.6, None), (1.0, None), (0.25, 0.30), (0.4, 0.08)]        # (d_sen, r_avoid; None = r_avoid_for)


@pytest.mark.parametrize("flags", [0, 2], ids=["lattice", "generic"])
@pytest.mark.parametrize("n_a", [8, 30, 64, 100, 256])
@pytest.mark.parametrize("d_sen,r_avoid", SENSING, ids=["d%g-r%s" % s for s in SENSING])
def test_sensing_radii(oracle, shapes, d_sen, r_avoid, n_a, flags):
    """d_sen and r_avoid away from 0.4 / r_avoid_for.  (0.25, 0.30): r_avoid > d_sen, so c_close and c_close2 are capped by
    c_sen and d_sen + r_avoid / 2 is mostly r_avoid.  (1.0, .): the sensing window is taller than 15 lattice rows -- the
    handle must decline the row walk and still be exact -- and far more than 80 cells are in range, so the lists that the
    occupied-cell filter leaves long are sub-sampled (asserted: every env has full lists at every step).  Nothing is asserted about lattice_envs() (the header promises the walk only within 15 rows)."""
    cases, ref, ra = _shared(("sen", d_sen, r_avoid, n_a),
                             lambda: _free_run(oracle, shapes, [3, n_a, int(1000 * d_sen)], n_a, d_sen=d_sen, r_avoid=r_avoid))
    if d_sen == 1.0:
        assert all((s["sensed_index"][:, -1] >= 0).any() for row in ref[1] for s in row)     # full lists: sub-sampled
    _hold(cases, ref, ra, d_sen=d_sen, flags=flags)


@pytest.mark.parametrize("flags", [0, 2], ids=["lattice", "generic"])
@pytest.mark.parametrize("n_a,n_env", [(8, 8), (64, 8), (256, 3)])
@pytest.mark.parametrize("d_sen,r_avoid", [(0.25, 0.30), (0.6, None)], ids=["d0.25-r0.3", "d0.6-rNone"])
def test_sensing_thresholds(oracle, shapes, d_sen, r_avoid, n_a, n_env, flags):
    """The threshold placements at another d_sen, r_avoid and size_a = 0.05: cells at d_sen and r_avoid / 2 to within an
    ulp, agent pairs at d_sen, r_avoid, 2 size_a = 0.10 and d_sen + r_avoid / 2."""
    cases, ref, ra = _shared(("thr", d_sen, r_avoid, n_a),
                             lambda: _threshold_run(oracle, shapes, [5, n_a, int(1000 * d_sen)], n_a, n_env, d_sen=d_sen, r_avoid=r_avoid, size_a=0.05))
    _hold(cases, ref, ra, d_sen=d_sen, size_a=0.05, flags=flags)


# ---- d. prior gains ----
@pytest.mark.parametrize("n_a,seed", [(8, 1), (64, 1)])
def test_prior_gains(oracle, shapes, n_a, seed):
    """prior_gain = (1.5, 4.0, 0.75): the carried prior of observe (returned by the first step) and of every step equals
    the oracle's with those gains; each of the three gains changes some returned component that the clamp leaves alone."""
    gains = (1.5, 4.0, 0.75)
    cases, ref, ra = _shared(("gain", n_a, seed), lambda: _free_run(oracle, shapes, [seed, n_a, 23], n_a, prior_gain=gains))
    states = [(c[0], c[1], c[2], c[3], o["neighbor_index"]) for c, o in zip(cases, ref[0])]
    states += [(s["p"], s["dp"], c[2], c[3], s["neighbor_index"]) for row in ref[1][:-1] for c, s in zip(cases, row)]
    for k in range(3):      # the states whose prior the steps return: the first observation's and every step's but the last
        g1 = list(gains); g1[k] = (2.0, 3.0, 2.0)[k]
        moved = sum(int((oracle.action_prior(p, dp, g, nei, l, ra, prior_gain=gains) != oracle.action_prior(p, dp, g, nei, l, ra, prior_gain=g1)).sum())
                    for p, dp, g, l, nei in states)
        assert moved > 0, k
    _hold(cases, ref, ra, prior_gain=gains, lattice=len(cases))
