"""Shared test helpers: seeded synthetic states in the reference's layouts, golden-fixture loading."""
import glob
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_files(pattern=None):
    """Recorded reference episodes: g2_* (synthetic shape set), g6_* (the reference's own fig/*.png shapes) and g11_* (three
    episodes each of N = 30 / 100 / 200, also run as 3-env batches)."""
    pats = [pattern] if pattern else ["g2_*.npz", "g6_*.npz", "g11_*.npz"]
    return sorted(f for p in pats for f in glob.glob(os.path.join(GOLDEN_DIR, p)))


def fig_shapes():
    """The reference's seven target shapes (fig/*.png) as tiled by marl_llm_amd.shape_images; results.pkl layout."""
    from marl_llm_amd.shape_images import unpack_cells_npz
    return unpack_cells_npz(os.path.join(GOLDEN_DIR, "fig_cells.npz"))


def load_golden(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def make_case(rng, shapes, n_a, cluster, shape=None):
    """One env: rotated/offset target shape + agents either scattered over the arena or clustered on the
    shape (the latter exercises in-shape flags, the occupied-cell filter, collisions)."""
    s = int(rng.integers(0, len(shapes["l_cell"]))) if shape is None else shape
    g = shapes["grid_coords"][s].T.copy()
    l_cell = float(shapes["l_cell"][s])
    th = rng.uniform(-np.pi, np.pi)
    rot = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]])
    g = np.ascontiguousarray(rot @ g + rng.uniform(-1.4, 1.4, (2, 1)))
    if cluster:
        p = g[:, rng.integers(0, g.shape[1], n_a)] + rng.normal(0, 0.05, (2, n_a))
    else:
        p = rng.uniform(-2.4, 2.4, (2, n_a))
    dp = rng.uniform(-0.5, 0.5, (2, n_a))
    return np.ascontiguousarray(p), np.ascontiguousarray(dp), g, l_cell


def adversarial_case(rng, shapes, n_a, ra, d_sen=0.4, contact=0.07, shift=None):
    """Agents placed (almost) exactly ON the decision thresholds the fp32 pre-filter has to resolve:
    distance to a cell ~ d_sen and ~ r_avoid/2 (sensed / occupied bits), the midpoint between two cells
    (nearest-cell ties), the in-shape radius, and agent pairs ~ d_sen, r_avoid and `contact` (= 2 size_a) apart.
    shift (2, 1): the whole case is translated by it BEFORE the placements, so they sit on the thresholds at that offset."""
    p, dp, g, l_cell = make_case(rng, shapes, n_a, 1)
    if shift is not None:
        g = np.ascontiguousarray(g + shift); p = p + shift
    eps = [0.0, 1e-16, -1e-16, 1e-13, -1e-13, 1e-10, -1e-10, 1e-8, -1e-8, 3e-7, -3e-7, 2e-6, -2e-6]
    k = 0
    for i in range(n_a):
        c = int(rng.integers(0, g.shape[1]))
        th = rng.uniform(0, 2 * np.pi)
        u = np.array([np.cos(th), np.sin(th)])
        mode = i % 6
        e = eps[k % len(eps)]; k += 1
        if mode == 0:
            p[:, i] = g[:, c] + u * d_sen * (1 + e)
        elif mode == 1:
            p[:, i] = g[:, c] + u * (ra / 2) * (1 + e)
        elif mode == 2:
            c2 = (c + 1) % g.shape[1]
            mid = 0.5 * (g[:, c] + g[:, c2]); d = g[:, c2] - g[:, c]
            p[:, i] = mid + d * e + np.array([-d[1], d[0]]) * rng.uniform(-0.3, 0.3)
        elif mode == 3:
            p[:, i] = g[:, c] + u * (np.sqrt(2) * l_cell / 2) * (1 + e)
        elif mode == 4 and i > 0:
            p[:, i] = p[:, i - 1] + u * [d_sen, ra, contact, d_sen + ra / 2][k % 4] * (1 + e)
        elif mode == 5:
            # nearest-cell ties across lattice rows: the midpoint of two vertically adjacent cells, the common vertex
            # of a 2x2 block (four-way tie -> lowest index wins), and the same from far outside the shape
            dd = np.linalg.norm(g - g[:, [c]], axis=0)
            nb = np.where((dd > 0) & (dd < 1.01 * l_cell))[0]
            if len(nb):
                d = g[:, nb[int(rng.integers(0, len(nb)))]] - g[:, c]
                perp = np.array([-d[1], d[0]])
                sub = k % 3
                if sub == 0:
                    p[:, i] = g[:, c] + 0.5 * d + d * e
                elif sub == 1:
                    p[:, i] = g[:, c] + 0.5 * d + 0.5 * perp + u * abs(e)
                else:
                    p[:, i] = g[:, c] + 0.5 * d + perp * (rng.integers(3, 12) + 0.5) + d * e
    return np.ascontiguousarray(p), dp, g, l_cell


# ---- non-default configurations of the env step (test_gpu_config_parity.py, test_oracle_vs_reference.py) ----
DEFAULT_BOX = (-2.4, 2.4, 2.4, -2.4)            # [x_min, y_max, x_max, y_min]
OFF_BOX = (-1.5, 2.0, 3.0, -1.0)                # non-square, off-centre: w_half = 2.25, h_half = 1.5
BIG_BOX = (-6.0, 6.0, 6.0, -6.0)
DEFAULT_PHYS = dict(size_a=0.035, k_ball=30.0, k_wall=100.0, c_wall=5.0, vel_max=0.8, dt=0.1)
# one constant at a time, then all together; none a power-of-two multiple of its default, no two fields equal
DYNAMICS_ROWS = [("size_a", dict(size_a=0.05)), ("size_a_small", dict(size_a=0.02)), ("k_ball", dict(k_ball=45.0)),
                 ("k_wall", dict(k_wall=60.0)), ("c_wall", dict(c_wall=2.5)), ("vel_max", dict(vel_max=0.5)),
                 ("dt", dict(dt=0.05)), ("dt_long", dict(dt=0.13)),
                 ("all", dict(size_a=0.05, k_ball=45.0, k_wall=60.0, c_wall=2.5, vel_max=0.5, dt=0.13))]


def physics(**over):
    """The six dynamics constants, the reference's values unless overridden."""
    d = dict(DEFAULT_PHYS); d.update(over)
    return d


def config_case(rng, shapes, n_a, boundary=DEFAULT_BOX, size_a=0.035, vel_max=0.8, dt=0.1, cluster=1):
    """One env (n_a >= 8) whose state reaches every term of the dynamics in the box `boundary`.  make_case's shape and
    agents, translated so that the shape's bounding box is centred in the box, then
      agents 0..3  at the left, top, right and bottom edge, closer than size_a (a wall contact) and closer than one step
                   (a periodic wrap), moving outward = into the wall; 0 and 2 share their y, 1 and 3 their x, so in periodic
                   mode each pair is a neighbour pair through the wrap of one axis only, and 0 -- the one row the
                   reference's numpy distance matrix wraps -- is in contact with 2 through it;
      agents 4, 5  1.2 size_a apart: in contact for this size_a;
      agents 6, 7  between 2 size_a and the default 0.07 apart (0.08 at the default size): a contact for exactly one of
                   this size_a and the default one;
      agents 4..7  move at 0.995 vel_max per component, so a small push clips them.
    Returns p, dp, grid, l_cell."""
    p, dp, g, l_cell = make_case(rng, shapes, n_a, cluster)
    x0, y1, x2, y3 = boundary
    shift = np.array([[0.5 * (x0 + x2)], [0.5 * (y1 + y3)]]) - 0.5 * (g.min(axis=1, keepdims=True) + g.max(axis=1, keepdims=True))
    g = np.ascontiguousarray(g + shift); p = p + shift
    if not cluster:
        p = np.stack([rng.uniform(x0, x2, n_a), rng.uniform(y3, y1, n_a)])
    v = 0.6 * vel_max
    gap = min(0.4 * size_a, 0.4 * v * dt)
    ym, xm = rng.uniform(y3 + 0.3, y1 - 0.3), rng.uniform(x0 + 0.3, x2 - 0.3)
    p[:, 0] = (x0 + gap, ym); dp[:, 0] = (-v, 0.01)
    p[:, 1] = (xm, y1 - gap); dp[:, 1] = (0.02, v)
    p[:, 2] = (x2 - gap, ym); dp[:, 2] = (v, -0.015)
    p[:, 3] = (xm, y3 + gap); dp[:, 3] = (-0.025, -v)
    th = rng.uniform(0, 2 * np.pi, 2)
    u = np.stack([np.cos(th), np.sin(th)])
    p[:, 5] = p[:, 4] + u[:, 0] * 1.2 * size_a
    band = 0.08 if size_a == 0.035 else 0.5 * (2 * size_a + 0.07)
    p[:, 7] = p[:, 6] + u[:, 1] * band
    dp[:, 4:8] = 0.995 * vel_max * rng.choice([-1.0, 1.0], (2, 4))
    return np.ascontiguousarray(p), np.ascontiguousarray(dp), g, l_cell


def pad_cells(grids, ng_max):
    """[E] lists of (2, n_g) cells -> SwarmBatch.set_cells' cells [E, 2, ng_max] and n_g [E]."""
    cells = np.zeros((len(grids), 2, ng_max))
    n_g = np.zeros(len(grids), np.int32)
    for e, g in enumerate(grids):
        n_g[e] = g.shape[1]
        cells[e, :, : g.shape[1]] = g
    return cells, n_g


def shape_batch(shapes, E, N, dtype=None, upload=True, **kw):
    """A SwarmBatch of E envs x N agents with room for any shape of `shapes`, the set uploaded (set_shapes) unless upload is
    False.  dtype: the obs dtype, default torch.float32."""
    import torch
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.shapes import r_avoid_for
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    sb = SwarmBatch(n_env=E, n_agents=N, n_cells_max=ng_max, r_avoid=r_avoid_for(N, shapes), obs_dtype=dtype or torch.float32, **kw)
    if upload:
        sb.set_shapes(shapes)
    return sb


def lat_nrs(cells, n_g, d_sen=0.4):
    """The window-row count of lattice cell sets (csrc/env_api.hip: detect_lattice fits the step as the closest pair of
    consecutive cells, stored as float; R = d_sen / step; window_rows takes floor(2 (R + 0.01)) + 1 in float).  The row walk
    serves a cell set while this is <= 15."""
    rmax = np.float32(0)
    for c, n in zip(cells, n_g):
        d = np.diff(c[:, :n], axis=1)
        step = np.float32(np.sqrt(np.min(d[0] * d[0] + d[1] * d[1])))
        rmax = max(rmax, np.float32(d_sen / np.float64(step)))
    return int(np.floor(np.float32(2) * (rmax + np.float32(0.01)))) + 1


def oracle_run(oracle, cases, acts, r_avoid, d_sen=0.4, boundary=DEFAULT_BOX, periodic=False, prior_gain=(2.0, 3.0, 2.0), *,
               topo=None, g_max=None, occ_max=None, with_self=True, feedback=None, **phys):
    """The oracle's trajectory of every case (p, dp, grid, l_cell) of `cases`: get_observation, then one step per entry of
    `acts` ([E, N, 2] float32 actions; None = the previous step's prior rounded to float32, as a float32 policy would feed it
    back).  Returns (first [E] observation dicts, steps [T][E] oracle.step dicts each with the float32 action it took under
    "act" ([N, 2]), counts) where counts holds what the trajectory reached, from the oracle's own functions: agent-agent
    contacts, contacts with each wall [left, top, right, bottom], velocity components clipped at +-vel_max, absolute wraps
    at each edge [left, top, right, bottom] and neighbour-list entries that exist only through the periodic wrap.
    topo, g_max, occ_max: the list caps (default: the oracle's constants); with_self: the own-state block.  feedback: what a
    None entry of `acts` feeds back, a function of the previous step's a_prior (2, N) float64 returning the [N, 2] float32
    action (default: the prior rounded once to float32; obs_feedback gives a float32 / bfloat16 handle's)."""
    from oracle.oracle_py import G_MAX, OCC_MAX, TOPO
    ph = physics(**phys)
    cap = dict(topo=TOPO if topo is None else topo, g_max=G_MAX if g_max is None else g_max, occ_max=OCC_MAX if occ_max is None else occ_max)
    if feedback is None:
        feedback = lambda prior: prior.T.astype(np.float32)
    b = np.array(boundary, np.float64)
    w_half, h_half = (b[2] - b[0]) / 2, (b[1] - b[3]) / 2
    first = [oracle.get_observation(p, dp, g, l, r_avoid, d_sen=d_sen, boundary=b, is_periodic=periodic, with_self=with_self, **cap)
             for p, dp, g, l in cases]
    state = [(c[0], c[1], o["neighbor_index"]) for c, o in zip(cases, first)]
    counts = dict(contact=0, wall=np.zeros(4, int), clip=0, wrap=np.zeros(4, int), wrap_only=0)

    def wrap_only(p, dp, g, l, nei):
        plain = oracle.get_observation(p, dp, g, l, r_avoid, d_sen=d_sen, boundary=b, is_periodic=False, **cap)["neighbor_index"]
        return sum(len(set(a[a >= 0]) - set(q[q >= 0])) for a, q in zip(nei, plain))

    if periodic:
        counts["wrap_only"] += sum(wrap_only(c[0], c[1], c[2], c[3], o["neighbor_index"]) for c, o in zip(cases, first))
    steps = []
    for t, act in enumerate(acts):
        row = []
        for e, (p, dp, nei) in enumerate(state):
            a = np.ascontiguousarray(act[e] if act is not None else feedback(steps[-1][e]["a_prior"]))
            g, l = cases[e][2], cases[e][3]
            counts["contact"] += int(oracle.dist_b2b(p, b, periodic, ph["size_a"])[2].sum())
            if not periodic:
                counts["wall"] += oracle.dist_b2w(p, b, ph["size_a"])[1].sum(axis=1)
            s = oracle.step(p, dp, np.ascontiguousarray(a.T), g, nei, l, r_avoid, d_sen=d_sen, boundary=b, is_boundary=not periodic,
                            with_self=with_self, prior_gain=prior_gain, **cap, **ph)
            counts["clip"] += int((np.abs(s["dp"]) == ph["vel_max"]).sum())
            if periodic:
                d = s["p"] - p
                counts["wrap"] += [int((d[0] > w_half).sum()), int((d[1] < -h_half).sum()), int((d[0] < -w_half).sum()), int((d[1] > h_half).sum())]
                counts["wrap_only"] += wrap_only(s["p"], s["dp"], g, l, s["neighbor_index"])
            s["act"] = a
            row.append(s)
            state[e] = (s["p"], s["dp"], s["neighbor_index"])
        steps.append(row)
    return first, steps, counts


def random_actions(rng, steps, n_env, n_a):
    """The action schedule of the free-running parity tests: random float32 actions alternating with the fed-back prior."""
    return [rng.uniform(-1, 1, (n_env, n_a, 2)).astype(np.float32) if t % 2 == 0 else None for t in range(steps)]


def oracle_threads(n_items=None):
    """Worker count of the threaded oracle: at most 16 and at most the CPUs this process may run on (the machine's CPU count
    can be many times that), and no more than there are items to share out."""
    n = min(16, len(os.sched_getaffinity(0)))
    return max(1, min(n, int(n_items))) if n_items is not None else n


class ThreadedOracle:
    """The oracle stepped over a whole batch of envs on a thread pool.  ctypes releases the GIL for the length of each C
    call, and assembly_oracle.c keeps no mutable static state (it allocates per call), so threads run it in parallel.
    Every worker takes one contiguous chunk of envs through Oracle.step_batch (one C call per chunk).

    cells [E,2,NG_MAX], n_g [E], l_cell [E] are the batch's target cells in SwarmBatch.set_cells' layout."""

    def __init__(self, oracle, cells, n_g, l_cell, r_avoid, is_boundary=True, with_self=True, workers=None):
        from concurrent.futures import ThreadPoolExecutor
        self.oracle = oracle
        self.r_avoid, self.is_boundary, self.with_self = float(r_avoid), bool(is_boundary), bool(with_self)
        self.set_cells(cells, n_g, l_cell)
        self.workers = oracle_threads(len(self.n_g)) if workers is None else int(workers)
        self.pool = ThreadPoolExecutor(max_workers=self.workers)

    def set_cells(self, cells, n_g, l_cell):
        self.cells = np.array(cells, np.float64, order="C")
        self.n_g = np.array(n_g, np.int32)
        self.l_cell = np.array(l_cell, np.float64)

    def close(self):
        self.pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chunks(self, n):
        return [c for c in np.array_split(np.arange(n), min(self.workers, n)) if len(c)]

    def _map(self, fn, n):
        for f in [self.pool.submit(fn, int(c[0]), int(c[-1]) + 1) for c in self._chunks(n)]:
            f.result()

    def step(self, p, dp, a, neighbor_index, envs=None):
        """One oracle step of envs `envs` (default: all, in order) from p, dp, a [len,2,N] (float64 or float32 action, taken
        to float64 exactly) and the previous step's neighbor_index [len,N,topo].  Inputs are not modified.  Returns a dict
        of [len, ...] arrays in the oracle's layouts: p, dp, obs [.,od,N], reward [.,N], a_prior [.,2,N], neighbor_index,
        in_flags, sensed_index, occupied_index."""
        from oracle.oracle_py import G_MAX, OCC_MAX, obs_dim
        envs = np.arange(len(self.n_g)) if envs is None else np.asarray(envs)
        n, n_a = len(envs), p.shape[2]
        out = dict(p=np.array(p, np.float64, order="C"), dp=np.array(dp, np.float64, order="C"),
                   neighbor_index=np.array(neighbor_index, np.int32, order="C"),
                   obs=np.empty((n, obs_dim(self.with_self), n_a)), reward=np.empty((n, n_a)), a_prior=np.empty((n, 2, n_a)),
                   in_flags=np.empty((n, n_a), np.int32), sensed_index=np.empty((n, n_a, G_MAX), np.int32),
                   occupied_index=np.empty((n, n_a, OCC_MAX), np.int32))
        a = np.ascontiguousarray(a, np.float64)
        cells, n_g, l_cell = self.cells[envs], self.n_g[envs], self.l_cell[envs]

        def work(b, e):            # step_batch advances p, dp, neighbor_index in place: the chunk's rows of the copies
            res = self.oracle.step_batch(out["p"][b:e], out["dp"][b:e], a[b:e], cells[b:e], n_g[b:e], l_cell[b:e],
                                         out["neighbor_index"][b:e], self.r_avoid, is_boundary=self.is_boundary,
                                         with_self=self.with_self, indices=True)
            for k, v in zip(("obs", "reward", "a_prior", "in_flags", "sensed_index", "occupied_index"), res):
                out[k][b:e] = v
        self._map(work, n)
        return out

    def observe(self, p, dp, envs=None):
        """Oracle.get_observation of every env (the tail of reset()): obs [.,od,N] and the four index arrays."""
        envs = np.arange(len(self.n_g)) if envs is None else np.asarray(envs)
        res = [None] * len(envs)

        def work(b, e):
            for k in range(b, e):
                en = envs[k]
                res[k] = self.oracle.get_observation(p[k], dp[k], self.cells[en][:, : self.n_g[en]], float(self.l_cell[en]),
                                                     self.r_avoid, is_periodic=not self.is_boundary, with_self=self.with_self)
        self._map(work, len(envs))
        return {k: np.stack([r[k] for r in res]) for k in res[0]}


# ---- list caps and observation dtypes of the env step (test_gpu_caps_parity.py, test_oracle_vs_reference.py) ----
# id -> (topo, g_max, occ_max)
CAPS_ROWS = {
    "default": (6, 80, 200),        # the two-slots-per-lane sensed writer; used by the dtype matrix only
    "t1_g5": (1, 5, 200),           # G - 1 even: the reference's fp64 round(); almost every list capped; D = 18 / 22 < one export tile
    "t3_g10_o7": (3, 10, 7),        # G - 1 odd: the integer cap arithmetic; binding occupied cap
    "t2_g16_o20": (2, 16, 20),
    "t6_g33_o33": (6, 33, 33),      # odd pairs per row; lists capped for some agents and not for others
    "t6_g79_o64": (6, 79, 64),      # odd pairs per row, one below the two-slot form, slot loop past lane 63
    "t5_g81": (5, 81, 200),         # one above it
    "t4_g128_o11": (4, 128, 11),    # the longest list the rule expert accepts; the sensed cap never binds
    "t6_g80_o20": (6, 80, 20),      # two-slot writer with a binding occupied cap
}
CAPS_NS = (5, 8, 16, 17, 30, 32, 64, 65, 128, 200, 256)          # the caps matrix (float64)
CAPS_DTYPE_NS = (5, 8, 30, 32, 64, 100, 200, 256)                # the dtype matrix (float32, bfloat16)
CAPS_DTYPE_ROWS = ("default", "t6_g80_o20", "t6_g33_o33", "t5_g81", "t1_g5")
CAPS_STEPS = 4


def caps_envs(n_a):
    """Env count of a caps case: small, and no multiple of the envs per workgroup."""
    return 11 if n_a <= 16 else 5 if n_a <= 64 else 3


def as_obs_dtype(x, dtype):
    """What a handle of obs dtype `dtype` ("f64", "f32", "bf16") has to return for the oracle's float64 array x, widened back
    exactly to a numpy array (float64 for "f64", else float32) so that == compares values of the narrow format.
      f64   x itself
      f32   x rounded once to float32
      bf16  x rounded to float32 and THEN to bfloat16, both to nearest-even (include/swarm_env.h: "the f32 value rounded to
            nearest-even"; the kernel's to_out<__bf16> is (__bf16)(float)v).
    Rounding the double to bfloat16 directly (bf16_direct) is NOT the contract, even where the two agree: they differ where
    the float32 rounding lands exactly on the midpoint of two bfloat16 values the double was not on -- about one value in
    2^17 -- and there the contract is the twice-rounded one, the value a float32 handle's output gives when cast."""
    import torch
    if dtype == "f64":
        return np.asarray(x, np.float64)
    t = torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(torch.float32)
    if dtype == "bf16":
        t = t.to(torch.bfloat16).to(torch.float32)
    elif dtype != "f32":
        raise ValueError(dtype)
    return t.numpy()


def bf16_direct(x):
    """float64 -> bfloat16 in ONE nearest-even rounding (8 significant bits), widened back; normal range only.  Not the
    contract (as_obs_dtype): the tests use it to count the values on which a kernel rounding this way would be caught."""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.rint(m * 256.0) / 256.0, e).astype(np.float32)


def obs_feedback(dtype):
    """oracle_run's `feedback` for a handle of obs dtype `dtype`: the prior as that handle returns it, widened to float32."""
    return lambda prior: np.ascontiguousarray(as_obs_dtype(prior.T, dtype).astype(np.float32))


def caps_trajectory(oracle, shapes, row, n_a, dtype="f64", periodic=False, with_self=True):
    """The inputs of one caps case and the oracle's trajectory of them: caps_envs(n_a) envs -- two thirds make_case envs
    clustered on the shape, every third an adversarial_case (thresholds meeting the capped lists) -- observe, then
    CAPS_STEPS steps alternating random float32 actions with the fed-back prior as a handle of `dtype` returns it.
    Deterministic in its arguments.  Returns (cases, oracle_run's result, r_avoid)."""
    from marl_llm_amd.shapes import r_avoid_for
    topo, g_max, occ_max = CAPS_ROWS[row]
    rng = np.random.default_rng([list(CAPS_ROWS).index(row), n_a, int(periodic), int(with_self), 41])
    ra = r_avoid_for(n_a, shapes)
    n_env = caps_envs(n_a)
    cases = []
    for e in range(n_env):
        if e % 3 != 2:
            cases.append(make_case(rng, shapes, n_a, 1))
            continue
        p, dp, g, l_cell = adversarial_case(rng, shapes, n_a, ra)
        for j in range(1, n_a):             # coincident agents: the reference's choice of "self" among them is its sort's
            while (p[:, :j] == p[:, [j]]).all(axis=0).any():
                p[0, j] += 1e-9
        cases.append((p, dp, g, l_cell))
    ref = oracle_run(oracle, cases, random_actions(rng, CAPS_STEPS, n_env, n_a), ra, periodic=periodic, topo=topo, g_max=g_max,
                     occ_max=occ_max, with_self=with_self, feedback=obs_feedback(dtype))
    return cases, ref, ra


def cap_round_parts_ways(g_max, n):
    """Does a sensed list of uncapped length n > g_max have a slot q whose rank round(q * ((n - 1) / (g_max - 1))) in the
    reference's fp64 (std::round: half away from zero, of the rounded product of the rounded quotient) differs from the
    exact quotient rounded half up, floor((2 q (n - 1) + g_max - 1) / (2 (g_max - 1)))?  Only exact ties can, so only even
    g_max - 1, and only where the fp64 product lands below the tie (never for g_max - 1 a power of two).  These are the
    lengths at which a kernel taking the integer form at the wrong parity of g_max - 1 selects another cell."""
    q = np.arange(g_max)
    v = q * ((n - 1) / (g_max - 1))
    fp = np.floor(v) + (v - np.floor(v) >= 0.5)
    return bool((fp != (2 * q * (n - 1) + g_max - 1) // (2 * (g_max - 1))).any())


def caps_reach(oracle, cases, row, ref, r_avoid, periodic=False):
    """What a caps trajectory reached, from the oracle alone, over every observation of it (the first and each step's), in
    agent-steps: sensed_over / sensed_under -- the UNCAPPED filtered sensed list (the oracle's observation with g_max =
    occ_max = n_g) longer / shorter than g_max; occ_over -- the uncapped occupied list longer than occ_max; nei_full /
    nei_part -- neighbour lists with all topo entries / fewer; rew1 / rew0 -- rewards of 1 / 0; tie_below -- capped sensed lists
    of a length at which cap_round_parts_ways."""
    topo, g_max, occ_max = CAPS_ROWS[row]
    first, steps, _ = ref
    c = dict(sensed_over=0, sensed_under=0, occ_over=0, nei_full=0, nei_part=0, rew1=0, rew0=0, tie_below=0, agent_steps=0)
    for e, (p0, dp0, g, l) in enumerate(cases):
        n_g = g.shape[1]
        states = [(p0, dp0, first[e]["neighbor_index"])] + [(row_[e]["p"], row_[e]["dp"], row_[e]["neighbor_index"]) for row_ in steps]
        for p, dp, nei in states:
            o = oracle.get_observation(p, dp, g, l, r_avoid, is_periodic=periodic, topo=topo, g_max=n_g, occ_max=n_g)
            n_s, n_o = (o["sensed_index"] >= 0).sum(axis=1), (o["occupied_index"] >= 0).sum(axis=1)
            c["sensed_over"] += int((n_s > g_max).sum()); c["sensed_under"] += int((n_s < g_max).sum())
            c["occ_over"] += int((n_o > occ_max).sum())
            c["tie_below"] += sum(cap_round_parts_ways(g_max, int(n)) for n in n_s[n_s > g_max])
            full = (nei >= 0).all(axis=1)
            c["nei_full"] += int(full.sum()); c["nei_part"] += int((~full).sum())
            c["agent_steps"] += p.shape[1]
        for row_ in steps:
            c["rew1"] += int((row_[e]["reward"] == 1).sum()); c["rew0"] += int((row_[e]["reward"] == 0).sum())
    return c


# ---- counter-based generators of the policy and rollout kernels (include/swarm_policy.h, include/swarm_rollout.h) ----
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def mix64(z):
    """pmix64 (splitmix64's finaliser) on a Python int, mod 2^64."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix64_np(z):
    """pmix64 elementwise on a uint64 array (numpy's uint64 arithmetic wraps mod 2^64)."""
    z = np.asarray(z).astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise_key(seed, step):
    """swarm_noise_key: the key of a (seed, step)'s exploration generators."""
    return mix64(mix64(seed + GOLD) ^ ((0xD1B54A32D192ED03 * (step + 1)) & M64))


def policy_normals(seed, step, rows, act_dim, row_offset=0):
    """include/swarm_policy.h 'Gaussian noise', restated: the normals z [rows, act_dim] of global rows row_offset + row, in
    float64 from the kernel's float32 uniforms (u1, u2 and the argument 2 pi u2 are formed exactly as the kernel forms them),
    and the Box-Muller radius [rows, act_dim] of each component (the scale of its rounding error)."""
    g = np.arange(rows, dtype=np.uint64) + np.uint64(row_offset)
    h = mix64_np(np.uint64(noise_key(seed, step)) ^ g)
    z = np.empty((rows, act_dim)); rad = np.empty((rows, act_dim))
    for k in range(0, act_dim, 2):
        u1 = ((h >> np.uint64(40)) + np.uint64(1)).astype(np.float32) * np.float32(2.0 ** -24)          # (0, 1], exact
        u2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)   # [0, 1), exact
        arg = np.float32(6.283185307179586) * u2                                                        # rounded in fp32
        r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
        z[:, k] = r * np.cos(arg.astype(np.float64)); rad[:, k] = r
        if k + 1 < act_dim:
            z[:, k + 1] = r * np.sin(arg.astype(np.float64)); rad[:, k + 1] = r
        h = mix64_np(h + np.uint64(GOLD))
    return z, rad


# ---- float64 model of the fused policy kernel's arithmetic (csrc/policy_mlp.hip, include/swarm_policy.h) ----
U32 = 2.0 ** -24            # unit roundoff of fp32
SLOPE = 0.01                # leaky-ReLU slope, applied as the fp32 product 0.01f * v


def _bf(t):
    """Round float32-representable values (held in float64) to bfloat16, nearest-even, and widen back."""
    import torch
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _lrelu32(h):
    """The kernel's activation of a float64 pre-activation h: v = fp32(h), r = fmaxf(v, 0.01f * v) (product rounded in
    fp32).  Returns r in float64.  Monotone non-decreasing in h."""
    import torch
    v = h.to(torch.float32)
    return torch.maximum(v, v * torch.tensor(SLOPE, dtype=torch.float32, device=h.device)).to(torch.float64)


def _split(t):
    """hi = bf(v), lo = bf(v - hi) of float32-representable values (v - hi is exact in fp32)."""
    hi = _bf(t)
    return hi, _bf(t - hi)


def _lowbit(t):
    """Exponent of the lowest set bit of every nonzero element (float64, exact); +inf for zeros."""
    import torch
    a = t.abs()
    m, e = torch.frexp(a)
    mi = (m * 2.0 ** 53).to(torch.int64)
    low = torch.log2((mi & -mi).to(torch.float64)) + e.to(torch.float64) - 53.0
    return torch.where(a > 0, low, torch.full_like(low, float("inf")))


def policy_weights(module):
    """fc1..fc4 weights and biases of a PolicyMLP-like module as fp32 values held in float64 (what swarm_policy_create
    reads)."""
    import torch
    return [t.detach().to("cpu", torch.float32).to(torch.float64) for fc in (module.fc1, module.fc2, module.fc3, module.fc4)
            for t in (fc.weight, fc.bias)]


def policy_model(module, x, precision, device=None, quantum=False):
    """csrc/policy_mlp.hip restated in float64 (include/swarm_policy.h 'Arithmetic').  x [rows, in_dim] float32 or bfloat16
    (the values the kernel reads); precision "bf16" or "bf16x3".

    bf16:   layer 1  h = bf(W1) . bf(x) + b1                  (b1 fp32: it initialises the accumulators)
            layer l  h = bf(Wl) . a + bf(bl)                   (the bias rides in the constant-one column), l = 2..4
            a = bf(fp32(max(v, 0.01f * v))), v = fp32(h);    output tanh(h4)
    bf16x3: every operand v split as hi = bf(v), lo = bf(v - hi); a product is Whi.xhi + Whi.xlo + Wlo.xhi (lo.lo dropped);
            biases of layers 2-4 are hi + lo, layer 1's fp32; bf16 input rows have lo = 0; a = hi + lo of the activation r.

    The sums h are exact up to float64 rounding.  Returns a dict (float64 tensors on `device`, default x's):
      out [rows, act]    tanh(h4)
      h   list of the four pre-activations [rows, width]
      r   list of the three fp32 activations r (before the bf16 rounding / split)
      S   list of the four sums of |terms| (the bias included) per row and feature
      n   list of the four term counts per sum (bias included)
      q   (quantum=True) list of the four per-row exponents q such that every term of the row's sums is a multiple of 2^q
    """
    import torch
    dev = torch.device(device) if device is not None else x.device
    x3 = precision == "bf16x3"
    if precision not in ("bf16", "bf16x3"):
        raise ValueError(precision)
    w1, b1, w2, b2, w3, b3, w4, b4 = [t.to(dev) for t in policy_weights(module)]
    xin = x.to(dev).to(torch.float64)
    res = dict(h=[], r=[], S=[], n=[], q=[])
    # layer inputs: a list of (operand, weight part) pairs whose products are the terms
    if x3:
        if x.dtype == torch.bfloat16:
            ah, al = xin, torch.zeros_like(xin)
        else:
            ah, al = _split(xin)
    else:
        ah, al = _bf(xin), None
    layers = ((w1, b1, True), (w2, b2, False), (w3, b3, False), (w4, b4, False))
    for li, (w, b, first) in enumerate(layers):
        if x3:
            wh, wl = _split(w)
            pairs = [(ah, wh), (al, wh), (ah, wl)]
            bias_terms = [b] if first else list(_split(b))
        else:
            pairs = [(ah, _bf(w))]
            bias_terms = [b] if first else [_bf(b)]
        h = sum(a @ wt.T for a, wt in pairs) + sum(bias_terms)
        S = sum(a.abs() @ wt.abs().T for a, wt in pairs) + sum(t.abs() for t in bias_terms)
        res["h"].append(h); res["S"].append(S)
        res["n"].append(len(pairs) * w.shape[1] + len(bias_terms))
        if quantum:
            qa = torch.stack([_lowbit(a).amin(dim=1) for a, _ in pairs], 1)             # [rows, pairs]
            qw = torch.stack([_lowbit(wt).amin() for _, wt in pairs])                    # [pairs]
            qb = torch.stack([_lowbit(t).amin() for t in bias_terms]).amin()
            res["q"].append(torch.minimum((qa + qw).amin(dim=1), qb))
        if li < 3:
            r = _lrelu32(h)
            res["r"].append(r)
            if x3:
                ah, al = _split(r)
            else:
                ah = _bf(r)
    res["out"] = torch.tanh(res["h"][3])
    return res


def gamma(n):
    """Rigorous relative factor of an fp32 sum of n exact terms in any order, against the exact sum rounded once:
    |fl(sum) - sum| <= n 2^-24 sum|terms| (first order; n u covers the (n - 1) u of the additions and the model's own
    float64 rounding with room to spare)."""
    return n * U32


def decided_rows(model, slack=1.0):
    """bf16 mode: rows whose every hidden activation is the same bf16 value for any pre-activation within gamma(n) S of the
    model's (the rounding function is monotone in h, so comparing both ends of the interval decides it).  On such a row the
    kernel's bf16 activations equal the model's whatever its summation order.  Returns a bool [rows] tensor."""
    ok = None
    for h, S, n in zip(model["h"][:3], model["S"][:3], model["n"][:3]):
        rho = slack * gamma(n) * S
        same = (_bf(_lrelu32(h - rho)) == _bf(_lrelu32(h + rho))).all(dim=1)
        ok = same if ok is None else ok & same
    return ok


def output_bound(model, precision, module):
    """Bound on |kernel pre-tanh - model h4| per output.  bf16: gamma(n4) S4, valid on decided rows (identical activations).
    bf16x3: propagated through the layers -- the sum's own gamma(n) S, plus the effect of the previous layer's activation
    error on this layer's terms (fp32 rounding of v and of 0.01f v, the re-split of a moved activation into hi + lo)."""
    import torch
    if precision == "bf16":
        return gamma(model["n"][3]) * model["S"][3]
    ws = [t.to(model["h"][0].device) for t in policy_weights(module)][0::2]
    E = gamma(model["n"][0]) * model["S"][0]
    for li in range(1, 4):
        h, r = model["h"][li - 1], model["r"][li - 1]
        Dr = E * (1 + 2 * SLOPE * U32) + 2 * U32 * h.abs()              # |r' - r|: the kernel's fp32 v and the product 0.01f v
        Da = Dr * (1 + 2.0 ** -18) + 2.0 ** -17 * r.abs()               # |(hi + lo)' - (hi + lo)|, each within 2^-18 |r| of r
        Dhi = Dr * (1 + 2.0 ** -8) + 2.0 ** -8 * r.abs()                # |hi' - hi|
        wh, wl = _split(ws[li])
        prop = Da @ wh.abs().T + Dhi @ wl.abs().T
        E = prop + gamma(model["n"][li]) * (model["S"][li] + prop + 2 * Dhi @ wh.abs().T)      # the kernel's own S
    return E


def tanh_tol(y):
    """Accuracy of the kernel's tanhf (device libm: within 2 ulp) plus the fp32 rounding of the result: 4 ulp."""
    return 8 * U32 * y.abs() + 2.0 ** -30


# ---- inputs and bookkeeping of the rule-expert contract tests (test_gpu_rule_contract.py, test_rule_contract_host.py) ----
def calm_case(rng, shapes, n_a, r_avoid, shape=None, off_shape=0.125, jitter=0.1, speed=0.05, spacing=1.0, away=0.0):
    """One env on which the rule expert's sum mostly stays inside (-1, 1): a rotated / offset target shape as in make_case,
    the agents on cells picked greedily at pairwise distance >= spacing * r_avoid (when the shape runs out of such cells the
    rest go on any free cell), a jitter of `jitter` * l_cell, `off_shape` of the agents pushed 1 to 3 cells outside the
    shape's nearest cell (so in_flag == 0 and v_ent acts) and velocities within +-speed.  `away` of the agents are taken off
    the shape altogether (>= 0.8 from every cell where the arena has room): the others then keep long sensed lists, so the
    n_s > g_max subsample runs.  Returns p, dp, grid, l_cell."""
    s = int(rng.integers(0, len(shapes["l_cell"]))) if shape is None else shape
    g = np.asarray(shapes["grid_coords"][s], np.float64).T.copy()
    l_cell = float(shapes["l_cell"][s])
    th = rng.uniform(-np.pi, np.pi)
    rot = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]])
    g = np.ascontiguousarray(rot @ g + rng.uniform(-1.4, 1.4, (2, 1)))
    n_g = g.shape[1]
    order = rng.permutation(n_g)
    chosen = []
    for c in order:                                                    # greedy packing at the avoidance distance
        if len(chosen) == n_a:
            break
        if not chosen or np.linalg.norm(g[:, chosen] - g[:, [c]], axis=0).min() >= spacing * r_avoid:
            chosen.append(int(c))
    if len(chosen) < n_a:
        rest = [int(c) for c in order if int(c) not in set(chosen)]
        chosen += rest[: n_a - len(chosen)]
    chosen += [int(c) for c in rng.integers(0, n_g, max(0, n_a - len(chosen)))]           # n_a > n_g: share cells
    p = g[:, chosen] + rng.uniform(-jitter, jitter, (2, n_a)) * l_cell
    centre = g.mean(axis=1, keepdims=True)
    for i in rng.permutation(n_a)[: int(round(off_shape * n_a))]:      # off the shape: outward, beyond its nearest cell
        out = p[:, [i]] - centre
        out = out / (np.linalg.norm(out) + 1e-12)
        for k in range(1, 400):
            q = p[:, [i]] + out * k * 0.5 * l_cell
            if np.linalg.norm(g - q, axis=0).min() > rng.uniform(1.0, 3.0) * l_cell:
                break
        p[:, [i]] = q
    for i in rng.permutation(n_a)[: int(round(away * n_a))]:
        for _ in range(200):
            q = rng.uniform(-2.3, 2.3, (2, 1))
            if np.linalg.norm(g - q, axis=0).min() >= 0.8:
                break
        p[:, [i]] = q
    dp = rng.uniform(-speed, speed, (2, n_a))
    return np.ascontiguousarray(p), np.ascontiguousarray(dp), g, l_cell


def rule_details(cases, r_avoid, g_max=80, d_sen=0.4, workers=None):
    """oracle_py.rule_action(detail=True) of every (p, dp, grid, l_cell) of `cases` on a pool of oracle_threads() processes
    (the restatement is Python loops: threads would share one interpreter lock).  Returns (a [E,2,N], info dict of stacked
    per-env arrays, RULE_DETAIL_KEYS)."""
    jobs = [(np.asarray(p), np.asarray(dp), np.asarray(g), float(l), float(r_avoid), float(d_sen), int(g_max)) for p, dp, g, l in cases]
    n = oracle_threads() if workers is None else int(workers)
    if n <= 1 or len(jobs) == 1:
        res = [_rule_detail_job(j) for j in jobs]
    else:
        res = list(_rule_pool(n).map(_rule_detail_job, jobs, chunksize=max(1, len(jobs) // (4 * n))))
    a = np.stack([r[0] for r in res])
    return a, {k: np.stack([r[1][k] for r in res]) for k in res[0][1]}


_RULE_POOL = {}


def _rule_pool(n):
    """One pool of spawned workers per process (spawn: the parent may hold a GPU context, which must not be forked), shut
    down at exit."""
    if n not in _RULE_POOL:
        import atexit
        import multiprocessing as mp
        from concurrent.futures import ProcessPoolExecutor
        _RULE_POOL[n] = ProcessPoolExecutor(max_workers=n, mp_context=mp.get_context("spawn"))
        atexit.register(_RULE_POOL[n].shutdown)
    return _RULE_POOL[n]


def _rule_detail_job(job):
    import os as _os
    import sys as _sys
    root = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    if root not in _sys.path:
        _sys.path.insert(0, root)
    from oracle.oracle_py import rule_action
    p, dp, g, l_cell, r_avoid, d_sen, g_max = job
    with np.errstate(all="ignore"):
        return rule_action(p, dp, g, l_cell, r_avoid, d_sen=d_sen, g_max=g_max, detail=True)


def rule_branch_counts(info):
    """Of the agents with at least one component of |raw| < 1 (NaN excluded): how many have a neighbour in d_sen, one inside
    r_avoid, in_flag == 0, a non-empty filtered sensed list, a subsampled list; and the share of components with |raw| < 1."""
    with np.errstate(invalid="ignore"):
        free = np.abs(info["raw"]) < 1                                 # [E, 2, N]
    ag = free.any(axis=1)                                              # [E, N]
    return dict(share=float(free.mean()), near=int((ag & (info["n_near"] >= 1)).sum()), avoid=int((ag & (info["n_avoid"] >= 1)).sum()),
                outside=int((ag & (info["in_flag"] == 0)).sum()), sensed=int((ag & (info["n_filtered"] >= 1)).sum()),
                subsampled=int((ag & (info["subsampled"] != 0)).sum()), agents=int(ag.size))


RULE_NS = (1, 2, 7, 8, 9, 30, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 255, 256)
RULE_SUBSAMPLE_NS = tuple(n for n in RULE_NS if n >= 30)    # below, an agent's own r_avoid / 2 disc leaves <= g_max cells


def calm_batch(shapes, n_a, r_avoid, seed=0, agents=6144):
    """The calm envs of one agent count: a third packed on the shape (neighbours inside r_avoid, the occupied-cell filter),
    two thirds with most agents away from it (v_ent, and long filtered lists: the subsample), about `agents` agents in all."""
    rng = np.random.default_rng([seed, n_a])
    n_env = max(6, -(-agents // n_a)) if n_a >= 8 else 64
    return [calm_case(rng, shapes, n_a, r_avoid) if e % 3 == 0 else
            calm_case(rng, shapes, n_a, r_avoid, away=0.7, off_shape=0.05, spacing=2.0) for e in range(n_env)]


def assert_calm_conditions(n_a, info):
    """The conditions the unsaturated comparison puts on its inputs, from the restatement's detail output alone; returns
    the counts (rule_branch_counts)."""
    c = rule_branch_counts(info)
    if n_a < 8:
        assert c["share"] > 0, (n_a, c)
        return c
    assert c["share"] >= 1 / 3, (n_a, c)
    for k in ("near", "avoid", "outside", "sensed") + (("subsampled",) if n_a in RULE_SUBSAMPLE_NS else ()):
        assert c[k] >= 100, (n_a, k, c)
    return c


# ---- hand-built inputs of the five legacy symbols (test_gpu_legacy_contract.py, test_oracle_vs_reference.py) ----
# A case is dict(id, fn, kw, meta): fn the RefLib / Oracle method, kw its keyword arguments (what the caller hands the symbol),
# meta what the builder placed on purpose.  legacy_call() runs one through any of the three libraries with the outputs
# pre-filled with junk; the restatements below (legacy_reward_v, ...) say from the inputs alone what a case reaches.
LEGACY_NS = (1, 2, 5, 63, 64, 65, 256)          # _get_observation stops at 256 agents; the four small symbols have no cap
LEGACY_L = 0.0625                               # lattice spacing 2^-4: cell coordinates and their differences are exact
LEGACY_NX, LEGACY_NY = 24, 16
OBS_JUNK, IDX_JUNK = 7.0, -7


def lattice(nx, ny, l, centre=None, theta=0.0):
    """(2, nx * ny) cell centres, index = iy * nx + ix, cell (0, 0) at the origin; or rotated by theta about the lattice's
    middle and moved so that the middle lies at `centre`."""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    g = np.stack([ix.ravel() * l, iy.ravel() * l]).astype(np.float64)
    if centre is not None:
        g = g - g.mean(axis=1, keepdims=True)
        rot = np.array([[np.cos(theta), np.sin(theta)], [-np.sin(theta), np.cos(theta)]])
        g = rot @ g + np.asarray(centre, np.float64).reshape(2, 1)
    return np.ascontiguousarray(g)


def legacy_obs_case(n_a, topo, g_max, d_sen, with_self, periodic, box, occ_max=None, vel_max=0.8, n_g=324, seed=0):
    """_get_observation: an 18 x 18 rotated lattice (cut to its first n_g cells) whose spacing puts about 1.5 g_max cells
    (at least; the spacing is capped at 0.08) inside d_sen, agent 0 in its middle, 60 % of the others scattered over it and
    the rest over the box; in periodic mode up to four pairs straddle an edge (x and y alternating), 0.02 to 0.1 apart through
    the wrap and a box apart without it.  With two agents in periodic mode the lattice sits on the left edge instead and the
    two agents straddle it.  meta: pairs."""
    rng = np.random.default_rng([seed, n_a, topo, g_max, int(d_sen * 10), periodic])
    x0, y1, x2, y3 = box
    l = min(0.08, d_sen * np.sqrt(np.pi / (1.5 * g_max)))
    mid = np.array([0.5 * (x0 + x2), 0.5 * (y1 + y3)]) + rng.uniform(-0.2, 0.2, 2)
    two = periodic and n_a == 2
    if two:
        mid = np.array([x0 + 0.04, 0.5 * (y1 + y3)])
    g = lattice(18, 18, l, mid, rng.uniform(-np.pi, np.pi))[:, :n_g]
    g = np.ascontiguousarray(g)
    p = np.empty((2, n_a))
    k_cl = int(round(0.6 * n_a))
    p[:, :k_cl] = g[:, rng.integers(0, g.shape[1], k_cl)] + rng.normal(0, 0.4 * l, (2, k_cl))
    p[:, k_cl:] = np.stack([rng.uniform(x0 + 0.25, x2 - 0.25, n_a - k_cl), rng.uniform(y3 + 0.25, y1 - 0.25, n_a - k_cl)])
    p[:, 0] = mid + rng.uniform(-0.3, 0.3, 2) * l
    pairs = 0
    if two:
        p[:, 1] = (x2 - 0.04, mid[1] + 0.01); pairs = 1
    elif periodic:
        pairs = min((n_a - 1) // 2, 4)
        for k in range(pairs):
            d1, d2, off = rng.uniform(0.01, 0.04), rng.uniform(0.01, 0.04), rng.uniform(-0.02, 0.02)
            if k % 2 == 0:
                ym = y3 + (k + 1) * (y1 - y3) / (pairs + 1) + 0.013
                p[:, 1 + 2 * k] = (x0 + d1, ym); p[:, 2 + 2 * k] = (x2 - d2, ym + off)
            else:
                xm = x0 + (k + 1) * (x2 - x0) / (pairs + 1) + 0.017
                p[:, 1 + 2 * k] = (xm, y3 + d1); p[:, 2 + 2 * k] = (xm + off, y1 - d2)
    dp = rng.uniform(-0.5, 0.5, (2, n_a))
    kw = dict(p=np.ascontiguousarray(p), dp=dp, grid=g, l_cell=float(l), r_avoid=float(2 * l), d_sen=d_sen,
              boundary=np.array(box, np.float64), is_periodic=periodic, with_self=with_self, topo=topo, g_max=g_max,
              occ_max=g.shape[1] if occ_max is None else occ_max, vel_max=vel_max)
    return dict(fn="get_observation", kw=kw, meta=dict(pairs=pairs))


_NEI_PATTERNS = ("MNFFMF", "FMNDMM", "FFMFMF", "SMMMMM", "MMMMMM", "FNSDFM")
_SYM_OFFSETS = sorted(((a, b) for a in range(-3, 4) for b in range(0, 4) if (b > 0 or a > 0)), key=lambda o: (o[0] ** 2 + o[1] ** 2, o))


def legacy_hand_state(n_a, topo, g_max, d_sen, box=OFF_BOX, seed=0):
    """The caller-built inputs of _get_reward and calculateActionPrior; nothing here is any library's output.

    Cells: the 24 x 16 lattice of spacing 2^-4 with cell (0, 0) at the origin, plus (n_a >= 16) two cells either side of each
    of the four edge agents.  Agent i sits on interior cell (1 + i % 22, 1 + i // 22), odd i 0.0036 off it, so agent i + 1 is
    one cell away and agent i + 3 three.  Placed on purpose:
      agent 3 (n_a >= 5)     half a cell off in x: two cells equidistant;
      agent 4 (n_a >= 5)     half a cell off in x and y: four cells at sqrt(2) * 2^-4 / 2 exactly;
      agents 6..11 (n_a >= 16)  three pairs along x from x = 0: 0.125 apart, one step of nextafter less, one more;
      agents 12..15 (n_a >= 16) one pair straddling the x edges of `box`, one the y edges, 0.06 apart through the wrap.
    neighbor_index rows cycle through _NEI_PATTERNS (rotated by i // 6, cut to topo): M = -1, N = agent i + 1, F = agents
    i + 3 + 2 k, S = i itself, D = the entry before repeated; so -1 comes first, in the middle and last, a far agent before a
    near one, duplicates and the own index all occur.  in_flags cycles through (1, 1, 0, 1, 2, 1, -1).  sensed_index rows
    cycle through five kinds: 0 pairs of cells mirrored about the agent with -1 between them (|v| ~ the agent's offset);
    1 cells on the +x side only; 2 all -1; 3 only cells at z >= d_sen (den == 0); 4 -1, then the agent's own cell (z == 0
    for even i).  The placed agents get in_flag 1 and kind 0.  Returns dict(p, grid, neighbor_index, in_flags, sensed_index,
    r_avoid = 0.125, l_cell = 2^-4, boundary)."""
    l, nx, ny = LEGACY_L, LEGACY_NX, LEGACY_NY
    g = lattice(nx, ny, l)
    x0, y1, x2, y3 = box
    p = np.empty((2, n_a)); base = np.empty(n_a, np.int64)
    for i in range(n_a):
        ix, iy = 1 + i % 22, 1 + (i // 22) % 14
        base[i] = iy * nx + ix
        p[:, i] = g[:, base[i]] + ((0.003, -0.002) if i % 2 else (0.0, 0.0))
    placed = {}
    if n_a >= 5:
        p[:, 3] = g[:, base[3]] + (l / 2, 0.0)
        p[:, 4] = g[:, base[4]] + (l / 2, l / 2)
    extra = []
    if n_a >= 16:
        for k, d in enumerate((0.125, np.nextafter(0.125, 0.0), np.nextafter(0.125, 1.0))):
            row = 8 + 2 * k
            a, b = 6 + 2 * k, 7 + 2 * k
            p[:, a] = (0.0, row * l); base[a] = row * nx
            p[:, b] = (d, row * l); base[b] = row * nx + 2
            placed[a] = b; placed[b] = a
        edge = [(x0 + 0.03, 0.5), (x2 - 0.03, 0.5), (0.75, y3 + 0.03), (0.75, y1 - 0.03)]
        for k, q in enumerate(edge):
            a = 12 + k
            p[:, a] = q; base[a] = -1
            extra += [(q[0] + l, q[1]), (q[0] - l, q[1])]
            placed[a] = 12 + (k ^ 1)
        g = np.ascontiguousarray(np.concatenate([g, np.array(extra).T], axis=1))
    nei = np.full((n_a, topo), -1, np.int32)
    for i in range(n_a):
        pat = _NEI_PATTERNS[i % 6]
        r = (i // 6) % 6
        pat = (pat[r:] + pat[:r])[:topo]
        for k, t in enumerate(pat):
            nei[i, k] = {"M": -1, "N": (i + 1) % n_a, "F": (i + 3 + 2 * k) % n_a, "S": i, "D": nei[i, k - 1] if k else (i + 1) % n_a}[t]
    for a, b in placed.items():
        nei[a] = -1
        nei[a, min(1, topo - 1)] = b                   # after a leading -1 where topo allows
    inf = np.array([(1, 1, 0, 1, 2, 1, -1)[i % 7] for i in range(n_a)], np.int32)
    sen = np.full((n_a, g_max), -1, np.int32)

    def fit(cells, gap):
        """cells with a -1 after every `gap` of them, as many whole groups of `gap` as g_max holds"""
        row = []
        for k in range(0, len(cells) - gap + 1, gap):
            grp = list(cells[k:k + gap]) + ([-1] if g_max >= 7 else [])
            if len(row) + gap > g_max:
                break
            row += grp
        return row[:g_max]

    for i in range(n_a):
        kind = 0 if i in placed else i % 5
        if i in placed:
            inf[i] = 1
        if base[i] < 0:                                 # an edge agent: its own two cells
            c = nx * ny + 2 * (i - 12)
            row = [c, c + 1]
        else:
            ix, iy = base[i] % nx, base[i] // nx
            ok = lambda a, b: 0 <= ix + a < nx and 0 <= iy + b < ny
            cid = lambda a, b: (iy + b) * nx + ix + a
            if kind == 0:
                row = fit([c for a, b in _SYM_OFFSETS if ok(a, b) and ok(-a, -b) for c in (cid(a, b), cid(-a, -b))], 2)
            elif kind == 1:
                row = fit([cid(a, b) for a in (1, 2, 3) for b in (0, 1, -1) if ok(a, b)], 1)
            elif kind == 2:
                row = []
            elif kind == 3:
                z = np.linalg.norm(g[:, :nx * ny] - p[:, [i]], axis=0)
                far = np.argsort(-z, kind="stable")[:5]
                row = fit([int(c) for c in far if z[c] >= d_sen + 1e-6], 1)
            else:
                row = ([-1] + [int(base[i])] + ([cid(1, 0), cid(-1, 0)] if g_max >= 4 else []))[:g_max]
        sen[i, :len(row)] = row
    return dict(p=np.ascontiguousarray(p), grid=g, neighbor_index=nei, in_flags=inf, sensed_index=sen, r_avoid=0.125,
                l_cell=l, boundary=np.array(box, np.float64))


def legacy_reward_case(n_a, topo, g_max, d_sen, periodic, cond3, cond4, r_avoid=0.125):
    s = legacy_hand_state(n_a, topo, g_max, d_sen)
    kw = dict(p=s["p"], grid=s["grid"], neighbor_index=s["neighbor_index"], in_flags=s["in_flags"], sensed_index=s["sensed_index"],
              r_avoid=r_avoid, d_sen=d_sen, boundary=s["boundary"], is_periodic=periodic,
              occupied_index=np.full((n_a, 3), -1, np.int32), cond3=cond3, cond4=cond4, coef=0.05)
    return dict(fn="get_reward", kw=kw, meta={})


def legacy_reward_v(kw):
    """|v| of AssemblyEnv.cpp:506-545 restated in numpy float64 for every agent that reaches it (in_flag == 1 and a sensed
    cell), NaN for the others; and the agents whose list is non-empty but has den == 0."""
    p, g, d_sen = kw["p"], kw["grid"], kw["d_sen"]
    n_a = p.shape[1]
    v = np.full(n_a, np.nan); den0 = np.zeros(n_a, bool)
    for i in range(n_a):
        cells = kw["sensed_index"][i][kw["sensed_index"][i] != -1]
        if kw["in_flags"][i] != 1 or len(cells) == 0:
            continue
        rel = g[:, cells] - p[:, [i]]
        z = np.sqrt(rel[0] ** 2 + rel[1] ** 2)
        psi = np.where(z < d_sen, 0.5 * (1.0 + np.cos(np.pi * (z / d_sen))), 0.0)
        den = psi.sum()
        den0[i] = den == 0
        den = 1e-8 if den == 0 else den
        v[i] = np.hypot((psi * rel[0]).sum() / den, (psi * rel[1]).sum() / den)
    return v, den0


def legacy_collisions(kw, wrap):
    """Per agent: does any listed neighbour lie inside r_avoid (AssemblyEnv.cpp:459-491), with or without the periodic wrap;
    and the distance of every listed neighbour (NaN for -1), for the tests that need one to sit exactly at r_avoid."""
    p, nei, b = kw["p"], kw["neighbor_index"], kw["boundary"]
    wh, hh = (b[2] - b[0]) / 2, (b[1] - b[3]) / 2
    hit = np.zeros(p.shape[1], bool); dist = np.full(nei.shape, np.nan)
    for i in range(p.shape[1]):
        for k, j in enumerate(nei[i]):
            if j == -1:
                continue
            x, y = p[0, j] - p[0, i], p[1, j] - p[1, i]
            if wrap:
                x = x + 2 * wh if x < -wh else (x - 2 * wh if x > wh else x)
                y = y + 2 * hh if y < -hh else (y - 2 * hh if y > hh else y)
            dist[i, k] = np.sqrt(x * x + y * y)
            hit[i] |= kw["r_avoid"] > dist[i, k]
    return hit, dist


def legacy_prior_case(n_a, topo, r_avoid, dp_scale, l_cell=LEGACY_L, one_cell=False, coincide=False, seed=0):
    """calculateActionPrior on legacy_hand_state's positions and neighbour lists.  l_cell is the caller's number: below the
    lattice's own spacing it puts agents outside the in-shape threshold sqrt(2) l_cell / 2 without moving anything.
    one_cell: n_g = 1.  coincide (n_a >= 6): agent 5 lies exactly on agent 2 and each lists the other first."""
    s = legacy_hand_state(n_a, topo, 2, 0.4)
    rng = np.random.default_rng([seed, n_a, topo])
    p, nei = s["p"].copy(), s["neighbor_index"].copy()
    if coincide:
        p[:, 5] = p[:, 2]; nei[5, 0] = 2; nei[2, 0] = 5
    g = s["grid"][:, [LEGACY_NX * 3 + 5]].copy() if one_cell else s["grid"]
    kw = dict(p=p, dp=rng.uniform(-1, 1, (2, n_a)) * dp_scale, grid=np.ascontiguousarray(g), neighbor_index=nei, l_cell=l_cell,
              r_avoid=r_avoid, d_sen=0.4)
    return dict(fn="action_prior", kw=kw, meta={})


def legacy_sf_case(n_a, k_ball, periodic, mode, box=OFF_BOX, seed=0):
    """_sf_b2b_all on matrices that are nobody's function of p: d_edge normal (negatives included), d_center uniform in
    [0.05, 1], collide 0/1 bytes, all three asymmetric.  mode "rand": a third of the pairs collide; "dense": all of them;
    "coincident": rand, with agent 1 on agent 0 and d_center[1][0] = 0."""
    rng = np.random.default_rng([seed, n_a, int(k_ball * 10), periodic])
    x0, y1, x2, y3 = box
    p = np.stack([rng.uniform(x0, x2, n_a), rng.uniform(y3, y1, n_a)])
    d_edge = rng.normal(0, 0.05, (n_a, n_a))
    d_center = rng.uniform(0.05, 1.0, (n_a, n_a))
    collide = np.ones((n_a, n_a), bool) if mode == "dense" else rng.random((n_a, n_a)) < 1 / 3
    if mode == "coincident":
        p[:, 1] = p[:, 0]; d_center[1, 0] = 0.0; collide[1, 0] = True
    kw = dict(p=p, d_edge=d_edge, collide=collide, d_center=d_center, boundary=np.array(box, np.float64), is_periodic=periodic,
              k_ball=k_ball)
    return dict(fn="sf_b2b_all", kw=kw, meta=dict(mode=mode))


def legacy_sf_terms(kw):
    """Per agent, the number of nonzero terms its sum has, from the inputs: pairs (a > b) with collide[a][b] set, d_edge[a][b]
    nonzero and the two agents apart."""
    n_a = kw["p"].shape[1]
    lo = np.tril(np.ones((n_a, n_a), bool), -1)
    apart = (kw["p"][:, :, None] != kw["p"][:, None, :]).any(axis=0)
    live = lo & kw["collide"].astype(bool) & (kw["d_edge"] != 0) & apart
    return (live | live.T).sum(axis=1)


def legacy_b2w_case(n_a, box=OFF_BOX, seed=0):
    """_get_dist_b2w with a radius of its own for every agent, agents inside the box, and (n_a >= 8) agents 0..3 with their
    edge exactly on the left, top, right and bottom wall (radius 0.25; d == 0 in exact arithmetic) and 4..7 beyond them."""
    rng = np.random.default_rng([seed, n_a])
    x0, y1, x2, y3 = box
    p = np.stack([rng.uniform(x0 + 0.2, x2 - 0.2, n_a), rng.uniform(y3 + 0.2, y1 - 0.2, n_a)])
    r = 0.02 + 0.1 * (rng.permutation(n_a) + 1) / (n_a + 1)
    if n_a >= 8:
        p[:, 0] = (x0 + 0.25, 0.3); p[:, 1] = (0.4, y1 - 0.25); p[:, 2] = (x2 - 0.25, 0.6); p[:, 3] = (0.9, y3 + 0.25)
        r[:4] = 0.25
        p[:, 4] = (x0 - 0.3, 0.1); p[:, 5] = (0.2, y1 + 0.3); p[:, 6] = (x2 + 0.3, 0.7); p[:, 7] = (1.1, y3 - 0.3)
    elif n_a == 1:
        p[:, 0] = (x0 + 0.25, y1 + 0.5); r[0] = 0.25            # on the left wall, beyond the top one
    return dict(fn="dist_b2w", kw=dict(p=p, boundary=np.array(box, np.float64), radius=r), meta={})


def legacy_call(lib, case, **over):
    """Run a case through RefLib, a RefLib bound to libswarmenv.so, or Oracle, the caller's output buffers pre-filled with
    junk (doubles 7.0, indices -7, bools True).  Returns {name: array}."""
    from oracle.oracle_py import obs_out_arrays
    kw = dict(case["kw"]); kw.update(over)
    fn, n_a = case["fn"], case["kw"]["p"].shape[1]
    if fn == "get_observation":
        out = obs_out_arrays(n_a, kw["topo"], kw["g_max"], kw["occ_max"], kw["with_self"], fill=(OBS_JUNK, IDX_JUNK))
        return lib.get_observation(**kw, out=out)
    if fn == "dist_b2w":
        d, c = lib.dist_b2w(**kw, out=(np.full((4, n_a), OBS_JUNK), np.ones((4, n_a), bool)))
        return dict(d_b2w=d, collide=c)
    rows = 1 if fn == "get_reward" else 2
    return {fn: getattr(lib, fn)(**kw, out=np.full((rows, n_a), OBS_JUNK))}


def assert_same(a, b, what=""):
    """Every output of two legacy_call results equal bit for bit (NaN == NaN)."""
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (what, k, int((a[k] != b[k]).sum()))


# the rows of each symbol: every n_a, topo, g_max, d_sen and flag value the contract names occurs in at least one
LEGACY_OBS_ROWS = [                       # n_a, topo, g_max, d_sen, with_self, periodic, box, occ_max, vel_max
    (1, 1, 2, 0.2, True, False, OFF_BOX, None, 0.8), (2, 3, 7, 0.4, False, True, OFF_BOX, None, 0.8),
    (5, 6, 45, 0.7, True, False, DEFAULT_BOX, None, 0.3), (5, 3, 80, 0.4, True, True, OFF_BOX, None, 0.8),
    (63, 6, 80, 0.4, True, True, OFF_BOX, None, 0.8), (64, 3, 45, 0.4, False, False, OFF_BOX, None, 0.8),
    (65, 1, 7, 0.7, True, True, OFF_BOX, None, 2.5), (256, 6, 80, 0.7, True, False, OFF_BOX, None, 0.8),
    (256, 3, 2, 0.2, False, True, OFF_BOX, None, 0.8), (64, 6, 45, 0.7, True, True, OFF_BOX, 20, 0.8)]
LEGACY_REWARD_ROWS = [                    # n_a, topo, g_max, d_sen, periodic, cond3, cond4
    (1, 1, 2, 0.2, False, True, True), (2, 3, 7, 0.4, True, True, True), (5, 6, 80, 0.7, False, False, True),
    (63, 6, 128, 0.4, True, True, True), (64, 3, 7, 0.4, False, True, False), (65, 1, 2, 0.7, True, False, False),
    (256, 6, 80, 0.2, False, True, True), (300, 6, 128, 0.4, True, True, True), (300, 3, 7, 0.7, False, False, True),
    (64, 6, 80, 0.4, True, False, True)]
LEGACY_SF_ROWS = [                        # n_a, k_ball, periodic, mode
    (1, 30.0, False, "rand"), (2, 7.5, True, "rand"), (5, 30.0, True, "dense"), (5, 30.0, False, "coincident"),
    (63, 7.5, False, "rand"), (64, 30.0, True, "dense"), (65, 7.5, True, "rand"), (256, 30.0, False, "rand"),
    (300, 7.5, True, "dense")]
LEGACY_B2W_ROWS = [(n,) for n in LEGACY_NS + (300,)]
LEGACY_PRIOR_ROWS = [                     # n_a, topo, r_avoid, dp_scale, l_cell, one_cell, coincide, calm
    (5, 6, 0.07, 0.05, LEGACY_L, False, False, True), (64, 3, 0.07, 0.05, LEGACY_L, False, False, True),
    (300, 6, 0.07, 0.05, LEGACY_L, False, False, True), (256, 1, 0.07, 0.05, LEGACY_L, False, False, True),
    (1, 1, 0.125, 0.5, LEGACY_L, False, False, False), (2, 3, 0.125, 0.5, 0.03, False, False, False),
    (63, 6, 0.125, 0.5, LEGACY_L, False, True, False), (65, 6, 0.125, 0.5, 0.03, False, True, False),
    (256, 6, 0.125, 0.5, LEGACY_L / 2, False, False, False), (300, 3, 0.125, 0.5, 0.03, True, False, False),
    (5, 6, 0.125, 0.05, float(np.nextafter(LEGACY_L, 0.0)), False, False, False),
    (5, 6, 0.125, 0.05, float(np.nextafter(LEGACY_L, 1.0)), False, False, False),
    (5, 3, 0.125, 0.05, 0.0, False, False, False), (64, 6, 0.07, 0.05, LEGACY_L, True, False, False)]


def legacy_specs():
    """[(id, builder, args)] of every case; legacy_case(spec) builds one."""
    def tag(*a):
        return "-".join("%g" % x if isinstance(x, (int, float)) and not isinstance(x, bool) else ("T" if x is True else "F" if x is False
                        else "off" if x == OFF_BOX else "def" if x == DEFAULT_BOX else "n" if x is None else str(x)) for x in a)
    s = [("obs-" + tag(*r), "obs", r) for r in LEGACY_OBS_ROWS]
    s += [("reward-" + tag(*r), "reward", r) for r in LEGACY_REWARD_ROWS]
    s += [("reward-ravoid-%s" % k, "reward", (64, 6, 7, 0.4, True, True, True, v)) for k, v in
          (("below", float(np.nextafter(0.125, 0.0))), ("above", float(np.nextafter(0.125, 1.0))))]
    s += [("sf-" + tag(*r), "sf", r) for r in LEGACY_SF_ROWS]
    s += [("b2w-" + tag(*r), "b2w", r) for r in LEGACY_B2W_ROWS]
    s += [("prior%d-" % k + tag(*r[:4]), "prior", r) for k, r in enumerate(LEGACY_PRIOR_ROWS)]
    return s


_LEGACY_CACHE = {}


def legacy_case(spec):
    """The case of one legacy_specs() entry, built once per process; the arrays are shared, so nobody writes to them."""
    cid, kind, r = spec
    if cid not in _LEGACY_CACHE:
        if kind == "obs":
            c = legacy_obs_case(*r)
        elif kind == "reward":
            c = legacy_reward_case(*r)
        elif kind == "sf":
            c = legacy_sf_case(*r)
        elif kind == "b2w":
            c = legacy_b2w_case(*r)
        else:
            c = legacy_prior_case(*r[:7])
            c["meta"]["calm"] = r[7]
        c["id"] = cid
        for v in c["kw"].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _LEGACY_CACHE[cid] = c
    return _LEGACY_CACHE[cid]


def legacy_reach(case, ref):
    """What a case has to reach, asserted from its inputs and from `ref`'s outputs alone (ref: the reference library, or the
    oracle where that was not built); never from the library under test.  Returns the counts."""
    kw, fn, meta = case["kw"], case["fn"], case["meta"]
    n_a = kw["p"].shape[1]
    c = {}
    if fn == "get_observation":
        n_g = kw["grid"].shape[1]
        full = legacy_call(ref, case, g_max=max(n_g, 2), occ_max=n_g)
        c["over_g_max"] = int(((full["sensed_index"] >= 0).sum(axis=1) > kw["g_max"]).sum())
        assert c["over_g_max"] >= 1, c
        c["occupied_max"] = int((full["occupied_index"] >= 0).sum(axis=1).max())
        if kw["occ_max"] < n_g:              # the reference bounds the list by the same round(i * step) pick (AssemblyEnv.cpp:218-228)
            assert c["occupied_max"] > kw["occ_max"], c
        got = legacy_call(ref, case)
        if n_a - 1 < kw["topo"]:
            assert (got["neighbor_index"][:, n_a - 1:] == -1).all()
        if kw["is_periodic"]:
            plain = legacy_call(ref, case, is_periodic=False)["neighbor_index"]
            c["wrap_only"] = sum(len(set(a[a >= 0]) - set(q[q >= 0])) for a, q in zip(got["neighbor_index"], plain))
            assert meta["pairs"] >= 1 and c["wrap_only"] >= 2 * meta["pairs"], (c, meta)
        if kw["vel_max"] != 0.8:             # the Cartesian branch never reads Vel_max
            assert_same(got, legacy_call(ref, case, vel_max=0.8), "vel_max")
    elif fn == "get_reward":
        v, den0 = legacy_reward_v(kw)
        c["margin"] = float(np.nanmin(np.abs(v - 0.05))) if np.isfinite(v).any() else np.inf
        assert c["margin"] >= 1e-9, c
        c["uniform"], c["not_uniform"], c["den0"] = int((v < 0.05).sum()), int((v >= 0.05).sum()), int(den0.sum())
        hit_w, dist = legacy_collisions(kw, True)
        hit_p, _ = legacy_collisions(kw, False)
        c["wrap_only_collisions"] = int((hit_w & ~hit_p).sum())
        nei = kw["neighbor_index"]
        first = np.array([np.argmax(kw["r_avoid"] > np.nan_to_num(d, nan=np.inf)) if h else -1 for d, h in zip(dist, hit_p)])
        c["hit_after_gap"] = int(sum(f > 0 and (nei[i, :f] == -1).any() for i, f in enumerate(first)))
        c["hit_after_far"] = int(sum(f > 0 and (nei[i, :f] >= 0).any() for i, f in enumerate(first)))
        if n_a >= 16:
            k = min(1, nei.shape[1] - 1)
            assert (dist[6, k], dist[8, k], dist[10, k]) == (0.125, np.nextafter(0.125, 0.0), np.nextafter(0.125, 1.0))
            assert c["wrap_only_collisions"] == 4
            assert c["den0"] >= 1 and c["uniform"] >= 8 and c["not_uniform"] >= 1, c
            if nei.shape[1] >= 3:
                assert c["hit_after_gap"] >= 1 and c["hit_after_far"] >= 1, c
            sen = kw["sensed_index"]
            if sen.shape[1] >= 7:
                inner = [(r[:np.max(np.nonzero(r >= 0)[0])] == -1).any() for r in sen if (r >= 0).any()]
                assert sum(inner) >= n_a // 4
            assert ((sen == -1).all(axis=1) & (kw["in_flags"] == 1)).any()
            assert set(np.unique(kw["in_flags"])) == {-1, 0, 1, 2}
            own = [i for i in range(n_a) if any((kw["grid"][:, s] == kw["p"][:, i]).all() for s in sen[i][sen[i] >= 0])]
            assert len(own) >= 1                     # a sensed cell exactly at the agent: z == 0
    elif fn == "sf_b2b_all":
        terms = legacy_sf_terms(kw)
        c["three_terms"] = float((terms >= 3).mean())
        if meta["mode"] == "dense":
            assert c["three_terms"] >= 0.9, c
        if n_a >= 5:                                 # nothing here is symmetric, and d_edge has both signs
            assert not np.array_equal(kw["d_edge"], kw["d_edge"].T) and not np.array_equal(kw["d_center"], kw["d_center"].T)
            assert (kw["d_edge"] < 0).any() and (kw["d_edge"] > 0).any()
            assert meta["mode"] == "dense" or not np.array_equal(kw["collide"], kw["collide"].T)
        assert set(np.unique(kw["collide"].view(np.uint8))) <= {0, 1}
    elif fn == "dist_b2w":
        d, col = legacy_call(ref, case).values()
        assert len(np.unique(kw["radius"])) >= min(n_a, max(1, n_a - 3))
        if n_a >= 8:
            for w in range(4):
                assert d[w, w] == 0 and not col[w, w] and col[w, 4 + w], w
        c["collisions"] = int(col.sum())
    else:
        out = legacy_call(ref, case)["action_prior"]
        if n_a >= 5 and kw["grid"].shape[1] > 1:     # agent 3: two cells equidistant; agent 4: four at sqrt(2) 2^-4 / 2 exactly
            z = [np.sort(np.sqrt(((kw["grid"] - kw["p"][:, [i]]) ** 2).sum(axis=0))) for i in (3, 4)]
            assert z[0][0] == z[0][1] == LEGACY_L / 2 and z[1][0] == z[1][3] == np.sqrt(2) * LEGACY_L / 2
            assert np.sqrt(2) * np.nextafter(LEGACY_L, 0.0) / 2 < z[1][0] < np.sqrt(2) * np.nextafter(LEGACY_L, 1.0) / 2
        c["free_share"] = float((np.abs(out) < 1).mean())
        if meta.get("calm"):
            assert c["free_share"] >= 0.4, c
        elif n_a >= 5:
            assert (np.abs(out) == 1).any(), c
    return c


def legacy_cache_configs():
    """The _get_observation calls of the cache test: A, then B (A with seven cells fewer), C (A in a box 0.3 wider on every
    side, so the pairs straddling A's edges are no neighbours), D (A without the self state).  Each differs from A in
    exactly one argument."""
    a = legacy_obs_case(64, 6, 45, 0.4, True, True, OFF_BOX)
    def variant(**over):
        kw = dict(a["kw"]); kw.update(over)
        return dict(fn="get_observation", kw=kw, meta=a["meta"])
    b = variant(grid=np.ascontiguousarray(a["kw"]["grid"][:, :-7]))
    b["kw"]["occ_max"] = a["kw"]["occ_max"]
    c = variant(boundary=np.array(OFF_BOX) + np.array([-0.3, 0.3, 0.3, -0.3]))
    d = variant(with_self=False)
    return dict(A=a, B=b, C=c, D=d)
