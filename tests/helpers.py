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
