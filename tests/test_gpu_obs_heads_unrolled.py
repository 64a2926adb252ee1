"""The observation heads of the lattice step kernels at 64 agent threads, written as straight-line chunks.

Without the ablation hooks (csrc/swarm_env.hip, DIAG) the head writer of those kernels (head_blocks_tgt) has two forms.  An
env of 64 agents in a bounded arena with eight blocks to a row takes the unrolled one: split A writes chunks 0 - 4 and
split C chunks 5 - 7 as straight-line code, the index words of all of a wave's chunks read first.  Every other env takes the
rolled loop over the chunks, each behind its owner test, where `it_ < n_it` and `r < rows` decide what is stored.  A slip
shows as a chunk that nobody owns or two waves own (rows of poison, or rows written twice with different values), a chunk
whose index words are another chunk's (a neighbour block or a target block of another row), rows past the last agent
stored, or the rolled form's rows lost where the unrolled form's condition is tested wrongly.

Every call writes into CALLER-OWNED tensors filled with NaN (obs, prior, reward) and 255 (done) before the call, and every
field is compared bit for bit with the oracle (lockstep.compare): observe, then three steps.  Each case ASSERTS, from the
in_flags and neighbour lists the device exported, that agents inside and outside the shape and agents with no neighbour,
with some and with every neighbour slot filled occurred; the seeds were chosen on the CPU, with the oracle, so that they do.

  n64x3      64 x 3, float32: the unrolled form (n64x3 and every 64-agent case below but periodic, topo3 and noself)
  n57x2      57 x 2: eight chunks, the last with one row
  n56x2      56 x 2: exactly seven chunks, C's last chunk is past the end
  n50x2      50 x 2: seven chunks, the last with two rows
  n33x2      33 x 2: five chunks, all of them A's -- C owns nothing
  bf16, f64  64 x 2 at the other row dtypes
  noself     64 x 2 without the own-state block: seven blocks to a row, the writer's general arm
  topo3      64 x 2 with three neighbour slots: five blocks
  periodic   64 x 2 in a periodic arena: the rolled form with the wrap
  mixed      64 x 3 with one env on a jittered (off-lattice) cell set: two launches over the grid, the lattice one with
             the mixed-batch filter (the FILT twins of the kernels above)
  observe    the observation-only kernel, twice in a row
"""
import numpy as np
import pytest

from helpers import config_case, make_case, obs_feedback, oracle_run, pad_cells, random_actions
from lockstep import FIELDS, OBSERVE, compare, device_layout, host_copy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G_MAX, STEPS = 80, 3
TORCH_DT = dict(f64=torch.float64, f32=torch.float32, bf16=torch.bfloat16)
#        name        n_a  envs (cluster flag per env; 2: clustered, jittered cells)  dtype  seed  SwarmBatch / oracle options
CASES = {
    "n64x3":    (64, (1, 0, 0), "f32", 0, {}),
    "n57x2":    (57, (1, 0), "f32", 0, {}),
    "n56x2":    (56, (1, 0), "f32", 0, {}),
    "n50x2":    (50, (1, 0), "f32", 0, {}),
    "n33x2":    (33, (1, 0), "f32", 0, {}),
    "bf16":     (64, (1, 0), "bf16", 0, {}),
    "f64":      (64, (1, 0), "f64", 0, {}),
    "noself":   (64, (1, 0), "f32", 0, dict(with_self=False)),
    "topo3":    (64, (1, 0), "f32", 0, dict(topo=3)),
    "periodic": (64, (1, 0), "f32", 0, dict(periodic=True)),
    "mixed":    (64, (1, 2, 0), "f32", 0, {}),
}
_REF = {}


def build(oracle, shapes, name, seed=None):
    """The inputs of a case and the oracle's trajectory of them: (cases, oracle_run's result, r_avoid).  Deterministic, and
    computed once per case."""
    from marl_llm_amd.shapes import r_avoid_for
    key = (name, seed)
    if key not in _REF:
        n_a, envs, dtype, seed0, opt = CASES[name]
        rng = np.random.default_rng([n_a, len(envs), G_MAX, seed0 if seed is None else seed, 17])
        ra = r_avoid_for(n_a, shapes)
        cases = []
        for cl in envs:
            p, dp, g, l_cell = config_case(rng, shapes, n_a, cluster=cl) if opt.get("periodic") else make_case(rng, shapes, n_a, min(cl, 1))
            if cl == 2:
                g = np.ascontiguousarray(g + rng.normal(0, 0.004, g.shape))          # off-lattice: this env takes the generic launch
            cases.append((p, dp, g, l_cell))
        ref = oracle_run(oracle, cases, random_actions(rng, STEPS, len(envs), n_a), ra, g_max=G_MAX, feedback=obs_feedback(dtype), **opt)
        _REF[key] = (cases, ref, ra)
    return _REF[key]


def reached(calls, lattice_envs):
    """What the calls of a case reached in its lattice envs, from in_flags [E, N] and neighbour lists [E, N, topo] (the
    device's exports, or the oracle's in the device's layout)."""
    inf = np.concatenate([d["in_flags"][lattice_envs].ravel() for d in calls])
    nn = np.concatenate([(d["neighbor_index"][lattice_envs] >= 0).sum(axis=2).ravel() for d in calls])
    topo = calls[0]["neighbor_index"].shape[2]
    return {"inside the shape": bool((inf != 0).any()), "outside the shape": bool((inf == 0).any()),
            "no neighbour": bool((nn == 0).any()), "some neighbours": bool(((nn > 0) & (nn < topo)).any()),
            "every neighbour slot": bool((nn == topo).any())}


class Poisoned:
    """A SwarmBatch over `cases` whose every call writes into the same caller-owned tensors, poisoned before each call."""

    def __init__(self, cases, ra, dtype, lattice, periodic=False, **kw):
        from marl_llm_amd.batched import SwarmBatch
        cells, n_g = pad_cells([c[2] for c in cases], max(c[2].shape[1] for c in cases) + 3)
        E, N = len(cases), cases[0][0].shape[1]
        self.sb = sb = SwarmBatch(n_env=E, n_agents=N, n_cells_max=cells.shape[2], r_avoid=ra, g_max=G_MAX, obs_dtype=TORCH_DT[dtype],
                                  is_boundary=not periodic, **kw)
        self.dtype = dtype
        try:
            sb.set_cells(cells, n_g, [c[3] for c in cases])
            assert sb.lattice_envs() == lattice, (sb.lattice_envs(), lattice)
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


def lattice_envs_of(name):
    return np.array([cl != 2 for cl in CASES[name][1]])


@pytest.mark.parametrize("name", list(CASES))
def test_heads_in_lockstep(oracle, shapes, name):
    """observe and three steps into poisoned caller-owned tensors, every field bit-equal to the oracle, and the coverage."""
    n_a, envs, dtype, _, opt = CASES[name]
    cases, (first, steps, counts), ra = build(oracle, shapes, name)
    lat = lattice_envs_of(name)
    run = Poisoned(cases, ra, dtype, int(lat.sum()), **opt)
    try:
        calls = [run.observe(first)]
        for t, step in enumerate(steps):
            calls.append(run.step(step, t))
    finally:
        run.close()
    got = reached(calls, lat)
    print(name, got, counts)
    assert all(got.values()), got
    blocks = opt.get("topo", 6) + 1 + int(opt.get("with_self", True))
    assert calls[0]["head"] == 4 * blocks and (blocks == 8) == (name not in ("topo3", "noself"))
    assert calls[0]["obs"].shape[1] == n_a and (n_a + 7) // 8 == dict(n57x2=8, n56x2=7, n50x2=7, n33x2=5).get(name, 8)      # chunks
    if name == "periodic":
        assert counts["wrap_only"] > 0, counts                                 # a neighbour that exists only through the wrap


def test_observe_only_twice(oracle, shapes):
    """The observation-only kernel, twice over the same state: the second pass writes the same heads over poison."""
    cases, (first, _, _), ra = build(oracle, shapes, "n64x3")
    run = Poisoned(cases, ra, "f32", len(cases))
    try:
        a = run.observe(first, "observe 1")
        b = run.observe(first, "observe 2")
    finally:
        run.close()
    assert np.array_equal(a["obs"].view(np.int32), b["obs"].view(np.int32))
    assert all(reached([a, b], lattice_envs_of("n64x3")).values())
