"""The observation heads and the prior policy of the lattice step kernel at 64 agents, where the target comes from LDS.

In those kernels the split whose nearest-cell candidate wins the merge publishes `cell - own position` once per agent
(csrc/swarm_env.hip, TGT_LDS / `tgt`); the head writer (head_blocks_tgt) and the prior policy read it from there and gather
no cell.  The head writer picks a block's minuend by ADDRESS (neighbour or own state) and writes the reference's zeros as
own - own.  A slip shows as a target block or an attraction vector of another cell (a lost tie, a stale or foreign `tgt`
entry), a zero of the wrong sign, a block of the wrong kind where a row has fewer than eight blocks, or a head that is not
stored at all.

Every call writes into CALLER-OWNED tensors filled with NaN (obs, prior, reward) and 255 (done) before the call, and every
field is compared bit for bit with the oracle (lockstep.compare): observe, then three steps.  Each case ASSERTS what it
exists for from what the device exported (in_flags, neighbour lists); a case whose inputs stop reaching it fails.

  n64x3     64 x 3 (one env clustered on the shape, two scattered), float32: agents inside and outside the shape, an agent
            with no neighbour, with 1 - 5 and with all 6
  n50x2     50 x 2: fourteen agent threads hold no agent (their lanes store nothing, their `tgt` entries are never read)
  bf16      64 x 2, bfloat16 rows
  periodic  64 x 2 in a periodic arena, a neighbour pair across the seam (the relative position is wrapped)
  topo3     64 x 2 with three neighbour slots: five blocks to a row, the writer's general form
  noself    64 x 2 without the own-state block: seven blocks to a row
  observe   the observation-only kernel, twice in a row, no step in between
  tie       an unrotated lattice with dyadic coordinates and agents exactly midway between two cells: two cells of adjacent
            lattice rows (they fall to different walking splits) from inside and from beyond the sensing range, and two
            cells of one row.  The lower cell index wins: the head's target block is that cell's offset, and the prior the
            first step returns points at it.  (The nearest-cell index has no export of its own on the Python side; the
            target block names the cell.)
  zeros     velocity components of -0.0, observed without a step, obs compared as int32 bit patterns
  no cells  an env with zero cells is refused by set_cells, so the kernels never see one
"""
import numpy as np
import pytest

from helpers import config_case, lattice, make_case, obs_feedback, oracle_run, pad_cells, random_actions
from lockstep import FIELDS, OBSERVE, compare, device_layout, host_copy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G_MAX, STEPS = 80, 3
#        name        n_a  envs (cluster flag per env)  dtype  seed  SwarmBatch / oracle options
CASES = {
    "n64x3":    (64, (1, 0, 0), "f32", 2, {}),
    "n50x2":    (50, (1, 0), "f32", 1, {}),
    "bf16":     (64, (1, 0), "bf16", 0, {}),
    "periodic": (64, (1, 0), "f32", 3, dict(periodic=True)),
    "topo3":    (64, (1, 0), "f32", 4, dict(topo=3)),
    "noself":   (64, (1, 0), "f32", 5, dict(with_self=False)),
}


def torch_dtype(dtype):
    return dict(f32=torch.float32, bf16=torch.bfloat16)[dtype]


def build(oracle, shapes, name):
    """The inputs of a case and the oracle's trajectory of them: (cases, oracle_run's result, r_avoid).  Deterministic."""
    from marl_llm_amd.shapes import r_avoid_for
    n_a, envs, dtype, seed, opt = CASES[name]
    rng = np.random.default_rng([n_a, len(envs), G_MAX, seed, 16])
    ra = r_avoid_for(n_a, shapes)
    cases = [config_case(rng, shapes, n_a, cluster=cl) if opt.get("periodic") else make_case(rng, shapes, n_a, cl) for cl in envs]
    ref = oracle_run(oracle, cases, random_actions(rng, STEPS, len(envs), n_a), ra, g_max=G_MAX, feedback=obs_feedback(dtype), **opt)
    return cases, ref, ra


class Poisoned:
    """A SwarmBatch over `cases` whose every call writes into the same caller-owned tensors, poisoned before each call."""

    def __init__(self, cases, ra, dtype, periodic=False, **kw):
        from marl_llm_amd.batched import SwarmBatch
        cells, n_g = pad_cells([c[2] for c in cases], max(c[2].shape[1] for c in cases) + 3)
        E, N = len(cases), cases[0][0].shape[1]
        self.sb = sb = SwarmBatch(n_env=E, n_agents=N, n_cells_max=cells.shape[2], r_avoid=ra, g_max=G_MAX, obs_dtype=torch_dtype(dtype),
                                  is_boundary=not periodic, **kw)
        self.dtype = dtype
        try:
            sb.set_cells(cells, n_g, [c[3] for c in cases])
            assert sb.lattice_envs() == E, sb.lattice_envs()
            self.out = dict(obs=torch.empty((E, N, sb.obs_dim), dtype=sb.obs_dtype, device=sb.device),
                            rew=torch.empty((E, N), dtype=torch.float32, device=sb.device),
                            done=torch.empty((E, N), dtype=torch.uint8, device=sb.device),
                            prior=torch.empty((E, N, 2), dtype=sb.obs_dtype, device=sb.device))
            sb.set_state(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]))
        except BaseException:
            sb.close()
            raise

    def poison(self):
        for k, t in self.out.items():
            t.fill_(255 if k == "done" else float("nan"))

    def observe(self, first, tag="observe"):
        self.poison()
        self.sb.observe(out=self.out["obs"])
        dev = host_copy(self.sb, self.out["obs"], state=False, indices=True)
        compare(dev, device_layout(first, self.dtype), tag, fields=OBSERVE)
        return dev

    def step(self, step, tag):
        want = device_layout(step, self.dtype)
        self.poison()
        self.sb.step(torch.from_numpy(want["act"]).to(self.sb.device), out=self.out)
        dev = host_copy(self.sb, self.out, indices=True)
        compare(dev, want, tag, fields=FIELDS)
        return dev

    def close(self):
        self.sb.close()


def reached(calls):
    """What the calls of a case reached, from the device's exported in_flags [E, N] and neighbour lists [E, N, topo]."""
    inf = np.concatenate([d["in_flags"].ravel() for d in calls])
    nn = np.concatenate([(d["neighbor_index"] >= 0).sum(axis=2).ravel() for d in calls])
    topo = calls[0]["neighbor_index"].shape[2]
    return {"inside the shape": bool((inf != 0).any()), "outside the shape": bool((inf == 0).any()),
            "no neighbour": bool((nn == 0).any()), "some neighbours": bool(((nn > 0) & (nn < topo)).any()),
            "every neighbour slot": bool((nn == topo).any())}


@pytest.mark.parametrize("name", list(CASES))
def test_heads_and_prior_in_lockstep(oracle, shapes, name):
    """observe and three steps into poisoned caller-owned tensors, every field bit-equal to the oracle, and the coverage."""
    n_a, envs, dtype, _, opt = CASES[name]
    cases, (first, steps, counts), ra = build(oracle, shapes, name)
    run = Poisoned(cases, ra, dtype, **opt)
    try:
        calls = [run.observe(first)]
        for t, step in enumerate(steps):
            calls.append(run.step(step, t))
    finally:
        run.close()
    got = reached(calls)
    print(name, got, counts)
    assert all(got.values()), got
    blocks = opt.get("topo", 6) + 1 + int(opt.get("with_self", True))
    assert calls[0]["head"] == 4 * blocks and (blocks == 8) == (name not in ("topo3", "noself"))
    if name == "periodic":
        assert counts["wrap_only"] > 0, counts                                 # a neighbour that exists only through the wrap


def test_observe_only(oracle, shapes):
    """The observation-only kernel, twice over the same state: the second pass writes the same heads over poison."""
    cases, (first, _, _), ra = build(oracle, shapes, "n64x3")
    run = Poisoned(cases, ra, "f32")
    try:
        a = run.observe(first, "observe 1")
        b = run.observe(first, "observe 2")
    finally:
        run.close()
    assert np.array_equal(a["obs"].view(np.int32), b["obs"].view(np.int32))


# ---- ties: an unrotated 24 x 16 lattice of spacing 2^-4, cell (ix, iy) = index iy * NX + ix, every coordinate dyadic ----
NX, NY, L_CELL = 24, 16, 0.0625
#   agent: (position in cell units, the two tied cells as (ix, iy); the lower index first)
TIES = {
    0: ((26.0, 5.5), ((23, 5), (23, 6))),         # two lattice rows, inside the sensing range: the row walk, two walking splits
    1: ((39.0, 9.5), ((23, 9), (23, 10))),        # the same from beyond the sensing range: the exact search
    2: ((3.5, 17.0), ((3, 15), (4, 15))),         # two cells of one row: one split's own tie
}


def tie_case(n_a=64):
    """(p, dp, grid, l_cell): the tie agents alone at their places (no agent within d_sen of them, so their prior is the
    attraction alone), every other agent over the lower left part of the shape."""
    rng = np.random.default_rng([n_a, 7, 16])
    g = lattice(NX, NY, L_CELL, centre=(-0.5, 0.0))
    org = g[:, 0]
    p = org[:, None] + L_CELL * np.stack([rng.uniform(0, 12, n_a), rng.uniform(0, 7, n_a)])
    for i, (at, _) in TIES.items():
        p[:, i] = org + L_CELL * np.array(at)
    dp = rng.uniform(-0.5, 0.5, (2, n_a))
    return np.ascontiguousarray(p), np.ascontiguousarray(dp), g, L_CELL


def test_nearest_cell_tie_takes_the_lower_index(oracle):
    p, dp, g, l_cell = tie_case()
    for i, (_, (lo, hi)) in TIES.items():
        c0, c1 = lo[1] * NX + lo[0], hi[1] * NX + hi[0]
        d = ((g - p[:, [i]]) ** 2).sum(axis=0)
        assert c0 < c1 and d[c0] == d[c1] == d.min() and (d == d.min()).sum() == 2, (i, c0, c1)      # an exact two-way tie
        assert d.min() > 0.5 * l_cell ** 2                                                        # outside the shape: the target block is not zero
        others = np.delete(np.arange(p.shape[1]), i)
        assert np.sqrt(((p[:, others] - p[:, [i]]) ** 2).sum(axis=0)).min() > 0.45                # alone: no neighbour
    ra = 0.1
    acts = [np.zeros((1, p.shape[1], 2), np.float32)]
    first, steps, _ = oracle_run(oracle, [(p, dp, g, l_cell)], acts, ra, g_max=G_MAX)
    run = Poisoned([(p, dp, g, l_cell)], ra, "f32")
    try:
        obs = run.observe(first)
        st = run.step(steps[0], 0)
    finally:
        run.close()
    head = obs["head"]
    for i, (_, (lo, hi)) in TIES.items():
        c0, c1 = lo[1] * NX + lo[0], hi[1] * NX + hi[0]
        assert obs["in_flags"][0, i] == 0 and (obs["neighbor_index"][0, i] < 0).all()
        want = (g[:, c0] - p[:, i]).astype(np.float32)
        other = (g[:, c1] - p[:, i]).astype(np.float32)
        assert not np.array_equal(want, other)
        assert np.array_equal(obs["obs"][0, i, head - 4: head - 2], want), (i, obs["obs"][0, i, head - 4: head], want, other)
        # the prior the first step returns is the one of the observed state: the attraction alone, 2 (cell - p) / |cell - p|
        t = g[:, c0] - p[:, i]
        q = np.clip(2.0 * t / np.sqrt((t * t).sum()), -1.0, 1.0).astype(np.float32)
        k = 1 if lo[0] == hi[0] else 0                                         # the component in which the two cells differ
        assert -1 < q[k] < 0 and st["a_prior"][0, i, k] == q[k], (i, st["a_prior"][0, i], q)         # (the other cell: -q[k])


def test_signed_zero_velocities(oracle, shapes):
    """Velocity components of -0.0 (own block own - 0 = -0; every other block of the row a difference that is +0 or the
    neighbour's value), observed without a step; obs compared as bit patterns."""
    from marl_llm_amd.shapes import r_avoid_for
    n_a = 64
    rng = np.random.default_rng([n_a, 2, 9, 16])
    ra = r_avoid_for(n_a, shapes)
    cases = []
    for cl in (1, 0):
        p, dp, g, l_cell = make_case(rng, shapes, n_a, cl)
        dp[0, 0::4] = -0.0; dp[1, 1::4] = -0.0; dp[:, 2::8] = -0.0; dp[1, 3::8] = 0.0
        cases.append((p, dp, g, l_cell))
    first, _, _ = oracle_run(oracle, cases, [], ra, g_max=G_MAX)
    run = Poisoned(cases, ra, "f32")
    try:
        dev = run.observe(first)
    finally:
        run.close()
    want = device_layout(first, "f32")["obs"]
    assert np.signbit(want[want == 0]).any() and (~np.signbit(want[want == 0])).any()      # zeros of both signs to tell apart
    assert np.array_equal(dev["obs"].view(np.int32), want.view(np.int32))
    got = reached([dev])
    assert got["inside the shape"] and got["outside the shape"] and got["no neighbour"] and got["every neighbour slot"], got


def test_an_env_without_cells_is_refused(shapes):
    """swarm_set_cells takes n_g in [1, n_cells_max]: no kernel ever runs an env with zero cells."""
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd._lib import SwarmError
    sb = SwarmBatch(n_env=1, n_agents=64, n_cells_max=8, r_avoid=0.1)
    try:
        with pytest.raises(SwarmError):
            sb.set_cells(np.zeros((1, 2, 8)), [0], [0.1])
    finally:
        sb.close()
