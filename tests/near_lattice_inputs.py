"""Cell sets at the edge of detect_lattice's fit (csrc/env_api.hip), agents on the decision thresholds of such cells, and the
cases test_near_lattice_host.py (CPU) and test_gpu_near_lattice.py (GPU) share.

detect_lattice accepts a cell set whose fitted coordinates lie within 1e-6 lattice steps of integers; the lattice kernels
then decide from the fitted frame -- the MODEL, here the exact parent lattice -- and read the stored cell only inside guard
bands that budget for that 1e-6 (lat_m, lat_dlt in csrc/swarm_env.hip, rew_ga_lat in set_lattice_mode).  near_lattice builds
sets whose fit residual is a chosen delta in both coordinates, lattice_fit restates the acceptance in numpy so that a test
knows the classification before a kernel runs, threshold_case puts agents where the model's cells and the stored cells give
different answers, and reach counts them.
"""
import numpy as np

from helpers import CAPS_ROWS, lat_nrs, lattice

FIT_TOL = 1e-6
D_SEN = 0.4
DYADIC = 0.0625                  # 2^-4: d_sen = 6.4 steps, 13 window rows
# offsets from a threshold, in lattice steps
EPS_STEPS = (0.0, 2e-7, -2e-7, 6e-7, -6e-7, 1.2e-6, -1.2e-6, 3e-6, -3e-6, 1e-5, -1e-5)
CATEGORIES = ("row_mid", "cross_mid", "vertex", "sense", "cover", "inshape")
REACH = ("nearest", "sensed", "covered", "inshape")
OUT = 0.52                       # steps outside the shape, on the bisector of a boundary pair: sqrt(0.25 + 0.52^2) = 0.7214 > sqrt(2) / 2


def lattice_fit(g, tol=FIT_TOL):
    """detect_lattice's acceptance of one (2, n_g) cell array, restated: the step is the closest pair of consecutive cells;
    the row direction is one of up to four distinct directions of consecutive cells within (1 + 1e-6) of that step; every
    cell gets coordinates (a, b) relative to cell 0, which must lie within `tol` of integers; the order must be row-major
    (columns increase inside a row, rows never decrease), with one retry with the row axis mirrored when rows decrease; the
    extent is at most 64 x 64 and no column repeats in a row.  The library is built without contraction, so the float64
    expressions below are the library's.
    Returns (accepted, max |a - rint a|, max |b - rint b|, ncols, nrows): of the accepted candidate; of a candidate that
    fitted and ordered but was refused for its extent or a repeated column; else the residuals of the candidate whose
    larger residual is smallest, with ncols = nrows = 0 (n_g < 2 or a zero step: nan)."""
    gx, gy = np.asarray(g[0], np.float64), np.asarray(g[1], np.float64)
    n = len(gx)
    none = (False, float("nan"), float("nan"), 0, 0)
    if n < 2:
        return none
    dx, dy = np.diff(gx), np.diff(gy)
    d2 = dx * dx + dy * dy
    l2 = d2.min()
    if not l2 > 0:
        return none
    cand = []
    for c in range(n - 1):
        if len(cand) == 4:
            break
        if d2[c] > l2 * (1.0 + 1e-6):
            continue
        if not any(abs(q[0] - dx[c]) + abs(q[1] - dy[c]) < 1e-6 * np.sqrt(l2) for q in cand):
            cand.append((dx[c], dy[c]))
    rx, ry = gx - gx[0], gy - gy[0]
    best = (np.inf, np.inf)
    for ux, uy in cand:
        vx, vy = -uy, ux
        for attempt in range(2):
            a, b = (rx * ux + ry * uy) / l2, (rx * vx + ry * vy) / l2
            ar, br = np.rint(a), np.rint(b)
            res = (float(np.abs(a - ar).max()), float(np.abs(b - br).max()))
            if max(res) < max(best):
                best = res
            if res[0] > tol or res[1] > tol or np.abs(ar).max() > 4096 or np.abs(br).max() > 4096:
                break
            ai, bi = ar.astype(np.int64), br.astype(np.int64)
            down = bool((bi[1:] < bi[:-1]).any())
            back = bool(((bi[1:] == bi[:-1]) & (ai[1:] <= ai[:-1])).any())
            if not down and not back:
                ncols, nrows = int(ai.max() - ai.min() + 1), int(bi.max() - bi.min() + 1)
                ok = ncols <= 64 and nrows <= 64 and len(set(zip(ai.tolist(), bi.tolist()))) == n
                return (ok,) + res + (ncols, nrows)
            if attempt == 0 and down:
                vx, vy = -vx, -vy
                continue
            break
    return (False,) + best + (0, 0)


def window_rows(radius, step):
    """csrc/env_api.hip window_rows for a radius `radius` on a lattice of step `step` (both as the library forms them: the
    step a float, the quotient a float)."""
    r = np.float32(radius / np.float64(np.float32(step)))
    return int(np.floor(np.float32(2) * (r + np.float32(0.01)))) + 1


def fit_path(g, n_a, r_avoid, d_sen=D_SEN):
    """("walk" | "scan", is a lattice): what classify_cells decides for one cell set -- a lattice subset walks when its
    sensing window is at most 15 rows (helpers.lat_nrs) and, at 64 agent threads, its covered window at most 29."""
    ok = lattice_fit(g)[0]
    if not ok:
        return "scan", False
    step = np.sqrt(np.min(np.sum(np.diff(g, axis=1) ** 2, axis=0)))
    walks = lat_nrs([g], [g.shape[1]], d_sen) <= 15 and not (32 < n_a <= 64 and window_rows(r_avoid / 2.0, step) > 29)
    return ("walk" if walks else "scan"), True


def lattice_frame(g):
    """Row direction u, row normal v (unit vectors), step and integer coordinates (a, b) of a (near-)lattice set whose cells 0
    and 1 are neighbours in a row."""
    d = g[:, 1] - g[:, 0]
    step = float(np.linalg.norm(d))
    u = d / step
    v = np.array([-u[1], u[0]])
    rel = g - g[:, [0]]
    return u, v, step, np.rint(u @ rel / step).astype(int), np.rint(v @ rel / step).astype(int)


def near_lattice(g, l, delta, rng):
    """From an exact row-major lattice subset g (2, n_g) of step l: a cell set whose fit residuals are `delta` steps in both
    coordinates.  The row of cells 0 and 1 stays; every other row is shifted as a whole along the row direction by
    +-delta l (one sign per row), and every cell of those rows is moved across its row by +-delta l (one sign per cell).
    In-row pairs only get longer, at second order, so the closest consecutive pair -- the fitted step and direction -- stays
    the exact lattice's."""
    u, v, step, _, b = lattice_frame(g)
    assert abs(step - l) < 1e-9 * l and (b != 0).any(), "cells 0 and 1 must be row neighbours, and the set needs a second row"
    rows = np.unique(b)
    sign = dict(zip(rows.tolist(), rng.choice([-1.0, 1.0], len(rows))))
    sign[0] = 0.0
    across = rng.choice([-1.0, 1.0], g.shape[1]) * (b != 0)
    # consecutive cells one step apart ACROSS rows (a one-cell row under the next row's first cell) move together: such a
    # pair must not get shorter either, or it becomes the fitted step and scales every column
    for c in np.nonzero((np.diff(b) != 0) & (np.linalg.norm(np.diff(g, axis=1), axis=0) < 1.01 * l))[0]:
        sign[int(b[c + 1])] = sign[int(b[c])]
        across[b == b[c + 1]] = across[c]
    along = np.array([sign[r] for r in b.tolist()])
    return np.ascontiguousarray(g + delta * l * (u[:, None] * along + v[:, None] * across))


def rotated_parent(rng, shapes, shape=None):
    """A shipped shape in a random pose (helpers.make_case's rotation, the offset kept inside the arena): exact to rounding."""
    s = int(rng.integers(0, len(shapes["l_cell"]))) if shape is None else shape
    g = np.asarray(shapes["grid_coords"][s], np.float64).T
    th = rng.uniform(-np.pi, np.pi)
    rot = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]])
    return np.ascontiguousarray(rot @ g + rng.uniform(-0.9, 0.9, (2, 1))), float(shapes["l_cell"][s])


def dyadic_parent():
    """An axis-aligned lattice subset of step 2^-4 at dyadic coordinates (every coordinate and difference exact): a 24 x 22
    block without its upper right 8 x 8 corner, its lower right 3 x 2 one and the first two cells of its first row, 456 cells,
    several convex corners.  Columns 0 and 1 of the second row -- a row near_lattice moves -- are open from below at the
    fitted frame's origin (threshold_case: the floor of the tie band)."""
    g = lattice(24, 22, DYADIC)
    ix, iy = np.rint(g[0] / DYADIC), np.rint(g[1] / DYADIC)
    keep = ~((ix >= 16) & (iy >= 14)) & ~((ix >= 21) & (iy < 2)) & ~((ix < 2) & (iy < 1))
    return np.ascontiguousarray(g[:, keep] + np.array([[-0.75], [-0.6875]])), DYADIC


def threshold_case(rng, g, l_cell, n_a, ra, d_sen=D_SEN, eps_steps=EPS_STEPS, parent=None):
    """One env on the cells g: three quarters of the agents (a multiple of six) hand-placed on the thresholds of g's cells, one
    category of CATEGORIES after the other, the rest clustered on the shape as in helpers.make_case (rewards of both values,
    the occupied filter).  Offsets e from the threshold cycle through eps_steps (lattice steps, not relative to the radius;
    the first three categories take +-5e-8 in place of 0).
      row_mid, cross_mid  on the bisector of two boundary cells adjacent in a row / across rows, OUT = 0.52 steps outside the
                          shape (0.7214 steps from both: beyond the in-shape radius, so the nearest cell is the target the
                          observation and the prior show; inside the shape no output names it), moved along the pair by e
      vertex              the common vertex of a 2 x 2 block, moved by |e| in a random direction
      sense, cover        at distance d_sen + e / r_avoid / 2 + e from a cell (cover: from a cell with all eight neighbours,
                          so the agent stands inside the shape and senses it)
      inshape             at distance sqrt(2) l_cell / 2 + e from a convex corner cell, outward on its diagonal: anywhere else
                          another cell is nearer and the in-shape radius decides nothing
    Every second placement of the first three categories goes to the fitted frame's origin (see near0 below), the sign of e
    there chosen like that too.
    parent: the exact lattice g was perturbed from (same cell order).  Every second placement of sense / cover then looks
    along the cell's displacement, and every second one of the three takes the sign of e against it, so that the model's
    cell lies on the other side of the threshold whenever |e| is below the displacement's projection.
    Cells of the row of cell 0 (which near_lattice leaves alone) are not used.  Returns p, dp, kind [n_a] (index into
    CATEGORIES, -1: clustered)."""
    u, v, step, a, b = lattice_frame(g)
    at = {ab: c for c, ab in enumerate(zip(a.tolist(), b.tolist()))}
    has = lambda c, da, db: (a[c] + da, b[c] + db) in at
    cells = [c for c in range(g.shape[1]) if b[c] != 0]
    pick = lambda ok: [c for c in cells if ok(c)]
    sides = lambda ok: [(c, sd) for c in cells for sd in (-1, 1) if ok(c, sd)]
    pools = dict(row_mid=sides(lambda c, sd: has(c, 1, 0) and not (has(c, 0, sd) or has(c, 1, sd))),
                 cross_mid=sides(lambda c, sd: has(c, 0, 1) and b[c] + 1 != 0 and not (has(c, sd, 0) or has(c, sd, 1))),
                 vertex=pick(lambda c: has(c, 1, 0) and has(c, 0, 1) and has(c, 1, 1) and b[c] + 1 != 0), sense=cells,
                 cover=pick(lambda c: all(has(c, i, j) for i in (-1, 0, 1) for j in (-1, 0, 1))),
                 inshape=[(c, i, j) for c in cells for i in (-1, 1) for j in (-1, 1)
                          if not (has(c, i, 0) or has(c, 0, j) or has(c, i, j))])
    # the nearest-cell tie band lat_dlt grows with the agent's lattice coordinates from the frame's origin (column 0 of the
    # first stored row): only within a few steps of it is the band at its floor, so every second tie placement goes there
    cell_of = lambda x: x[0] if isinstance(x, tuple) else x
    near0 = {cat: [x for x in pools[cat] if a[cell_of(x)] - a.min() <= 1 and abs(b[cell_of(x)]) <= 2]
             for cat in ("row_mid", "cross_mid", "vertex")}
    n = g.shape[1]
    p = g[:, rng.integers(0, n, n_a)] + rng.normal(0, 0.05, (2, n_a))
    dp = rng.uniform(-0.5, 0.5, (2, n_a))
    kind = np.full(n_a, -1)
    per = (3 * n_a // 4) // len(CATEGORIES)
    tie_eps = [5e-8, -5e-8] + [x for x in eps_steps if x != 0]

    def place(cat, pool, q, attempt):
        # (the tie categories take +-5e-8 steps for the zero offset: exactly on a midpoint the two squared distances differ by
        # rounding alone, where the kernels' nearest cell, taken by d^2, and the reference's, taken by sqrt(d^2), may part --
        # DESIGN.md deviation 2; at 5e-8 steps the squares differ by 1e-7 of themselves)
        e = (tie_eps[q % len(tie_eps)] if cat in near0 else eps_steps[q % len(eps_steps)]) * step
        origin = q % 2 == 1 and bool(near0.get(cat)) and attempt < 20
        if origin:
            pool, e = near0[cat], tie_eps[(q // 2) % len(tie_eps)] * step
        c = pool[int(rng.integers(0, len(pool)))]
        th = rng.uniform(0, 2 * np.pi)
        w = np.array([np.cos(th), np.sin(th)])
        if cat in ("row_mid", "cross_mid"):
            c, sd = c
            c2 = at[(a[c] + 1, b[c])] if cat == "row_mid" else at[(a[c], b[c] + 1)]
            d = g[:, c2] - g[:, c]
            d = d / np.linalg.norm(d)
            if origin and parent is not None:                 # the model's midpoint lies on the other side of the agent if |e| is small enough
                proj = 0.5 * (g[:, c] + g[:, c2] - parent[:, c] - parent[:, c2]) @ d
                e = -np.sign(proj) * abs(e) if proj else e
            return 0.5 * (g[:, c] + g[:, c2]) + d * e + (v if cat == "row_mid" else u) * sd * OUT * step
        if cat == "vertex":
            four = [c, at[(a[c] + 1, b[c])], at[(a[c], b[c] + 1)], at[(a[c] + 1, b[c] + 1)]]
            return g[:, four].mean(axis=1) + w * abs(e)
        if cat == "inshape":
            c, i_, j_ = c
            w = (i_ * u + j_ * v) / np.sqrt(2)
        disp = g[:, c] - parent[:, c] if parent is not None else np.zeros(2)
        if q % 2 == 0 and disp.any():
            if cat != "inshape":
                w = disp / np.linalg.norm(disp)
            if w @ disp != 0:
                e = -np.sign(w @ disp) * abs(e)
        r = d_sen if cat == "sense" else ra / 2 if cat == "cover" else np.sqrt(2) * l_cell / 2
        # (a sideways 1e-6 steps changes the distance by 1e-12: the few convex corners then serve any number of agents)
        side = np.array([-w[1], w[0]]) * rng.uniform(-1e-6, 1e-6) * step if cat == "inshape" else 0.0
        return g[:, c] + w * (r + e) + side

    for k, cat in enumerate(CATEGORIES):
        for q in range(per if pools[cat] else 0):
            i = k * per + q
            for attempt in range(100):  # no two agents in one place: which of them the reference calls "self" is its sort's choice
                p[:, i] = place(cat, pools[cat], q, attempt)
                if not (p[:, :i] == p[:, [i]]).all(axis=0).any():
                    break
            else:
                raise AssertionError("no free placement for %s %d" % (cat, q))
            kind[i] = k
    return np.ascontiguousarray(p), np.ascontiguousarray(dp), kind


def answers(p, g, l_cell, ra, d_sen=D_SEN):
    """What the oracle decides per agent from the cells g, in its own float64 expressions (assembly_oracle.c
    target_grid_state and the occupied filter): nearest cell (first minimum), sensed matrix d < d_sen [N, n_g], covered
    matrix !(d > r_avoid / 2) [N, n_g], in-shape flag."""
    rx, ry = g[0][None, :] - p[0][:, None], g[1][None, :] - p[1][:, None]
    d = np.sqrt(rx * rx + ry * ry)
    return dict(nearest=d.argmin(axis=1), sensed=d < d_sen, covered=~(d > ra / 2), inshape=d.min(axis=1) < np.sqrt(2) * l_cell / 2)


def reach(p, parent, g, l_cell, ra, d_sen=D_SEN):
    """Per category of REACH, the agents [N] bool whose answer from the exact parent lattice (the model) differs from the
    answer from the cells g (the truth).  A nearest cell counts only for an agent outside the shape by one of the two: inside,
    the target is the agent itself and no output names the cell.  A covered cell counts only where it can change an output:
    where an in-shape agent i (by the truth) senses it and the covering agent j is within d_sen + r_avoid / 2 of i, the pairs
    the oracle's occupied filter looks at."""
    m, t = answers(p, parent, l_cell, ra, d_sen), answers(p, g, l_cell, ra, d_sen)
    dx, dy = p[0][:, None] - p[0][None, :], p[1][:, None] - p[1][None, :]
    close = np.sqrt(dx * dx + dy * dy) < d_sen + ra / 2.0                                  # [i, j]
    looked = (close.T.astype(int) @ (t["sensed"] & t["inshape"][:, None]).astype(int)) > 0     # [j, c]
    return dict(nearest=(m["nearest"] != t["nearest"]) & ~(m["inshape"] & t["inshape"]), sensed=(m["sensed"] != t["sensed"]).any(axis=1),
                covered=((m["covered"] != t["covered"]) & looked).any(axis=1), inshape=m["inshape"] != t["inshape"])


# ---- the cases: name -> agents, options of the handle, envs as (parent, delta) ----
R, D = "rot", "dya"
CASES = {
    "n64": dict(n_a=64, envs=[(R, 0.0), (R, 5e-7), (R, 9e-7), (D, 5e-7), (D, 9e-7)]),
    "n64_f64": dict(n_a=64, dtype="f64", envs=[(R, 9e-7), (D, 9e-7), (R, 9e-7)]),
    "n64_bf16": dict(n_a=64, dtype="bf16", envs=[(R, 9e-7), (D, 9e-7), (R, 9e-7)]),
    "n57": dict(n_a=57, envs=[(R, 9e-7), (D, 9e-7), (R, 5e-7)]),
    "n30": dict(n_a=30, envs=[(R, 9e-7), (D, 9e-7), (R, 5e-7), (D, 5e-7), (R, 9e-7)]),            # two envs per workgroup, a tail
    "n16": dict(n_a=16, envs=[(R, 9e-7), (D, 9e-7), (R, 5e-7), (D, 5e-7), (R, 9e-7), (R, 0.0)]),  # four, a tail of two
    "n100": dict(n_a=100, envs=[(R, 9e-7), (D, 9e-7), (R, 5e-7)]),
    "n256": dict(n_a=256, envs=[(R, 9e-7), (D, 9e-7), (R, 5e-7)]),
    "periodic": dict(n_a=64, periodic=True, envs=[(R, 9e-7), (D, 9e-7), (R, 5e-7)]),
    "caps": dict(n_a=64, caps="t6_g33_o33", envs=[(R, 9e-7), (D, 9e-7), (R, 9e-7)]),
    "mixed64": dict(n_a=64, envs=[(R, 0.0), (R, 9e-7), (R, 1.5e-6), (D, 3e-6), (D, 9e-7)]),
    "mixed16": dict(n_a=16, envs=[(R, 0.0), (R, 9e-7), (R, 1.5e-6), (D, 3e-6), (D, 9e-7), (R, 5e-7)]),   # [0..3] mixed, [4 5] walk
}
STEPS = 3


def build_case(name, shapes):
    """The inputs of case `name`, deterministic: dict(cases [(p, dp, g, l_cell)], parents [E] (the exact lattices), deltas [E],
    kinds [E][N], r_avoid, caps (topo, g_max, occ_max), and the spec's own entries)."""
    from marl_llm_amd.shapes import r_avoid_for
    spec = CASES[name]
    n_a = spec["n_a"]
    rng = np.random.default_rng([list(CASES).index(name), n_a, 28])
    ra = r_avoid_for(n_a, shapes)
    out = dict(spec, cases=[], parents=[], deltas=[], kinds=[], r_avoid=ra, caps=CAPS_ROWS[spec.get("caps", "default")])
    cornered = [1 + list(CASES).index(name) % 2]         # "rect" / "L": shapes with cells at the fitted frame's origin, for one env
    for kind, delta in spec["envs"]:
        parent, l_cell = rotated_parent(rng, shapes, cornered.pop() if cornered and delta else None) if kind == R else dyadic_parent()
        g = near_lattice(parent, l_cell, delta, rng) if delta else parent
        p, dp, k = threshold_case(rng, g, l_cell, n_a, ra, parent=parent if delta else None)
        out["cases"].append((p, dp, g, l_cell)); out["parents"].append(parent); out["deltas"].append(delta); out["kinds"].append(k)
    return out


def expected_paths(case):
    """(lattice envs, scanning envs as a set) of a built case, from lattice_fit."""
    fits = [fit_path(c[2], case["n_a"], case["r_avoid"]) for c in case["cases"]]
    return sum(ok for _, ok in fits), {e for e, (path, _) in enumerate(fits) if path == "scan"}


# ---- structural edges of detect_lattice: dyadic lattices inside the default arena ----
def _block(nx, ny, x0=None, y0=None):
    g = lattice(nx, ny, DYADIC)
    x0 = -DYADIC * (nx // 2) if x0 is None else x0
    y0 = -DYADIC * (ny // 2) if y0 is None else y0
    return np.ascontiguousarray(g + np.array([[x0], [y0]]))


def edge_sets():
    """name -> (cells (2, n_g), the path the issue expects or None where lattice_fit is to say)."""
    b = _block(12, 10)
    iy = np.rint((b[1] - b[1].min()) / DYADIC).astype(int)
    top_down = np.concatenate([np.nonzero(iy == r)[0] for r in range(9, -1, -1)])
    col_major = np.lexsort((b[1], b[0]))                           # x outer, y inner
    swapped = np.arange(b.shape[1]); swapped[[40, 41]] = [41, 40]
    return {
        "rows64": (_block(6, 64), "walk"),
        "rows65": (_block(6, 65), "scan"),
        "cols65": (_block(65, 6), "scan"),
        "empty_row": (np.ascontiguousarray(b[:, iy != 4]), "walk"),
        "top_down": (np.ascontiguousarray(b[:, top_down]), "walk"),
        "col_major": (np.ascontiguousarray(b[:, col_major]), None),
        "duplicate": (np.ascontiguousarray(np.insert(b, 30, b[:, 29], axis=1)), "scan"),
        "one_column": (_block(1, 20), None),
        "two_cells": (_block(2, 1), None),
        "one_cell": (_block(1, 1), "scan"),
        "swapped": (np.ascontiguousarray(b[:, swapped]), "scan"),
    }


def edge_case(name, n_a, shapes, n_env=2):
    """n_env envs on edge set `name`: agents clustered on the cells; on the 64- and 65-row sets agents 0..5 stand in rows 0, 62
    and 63 (the last entries of the kernels' 64-entry row tables) and one and five steps beyond both ends.  Returns (cases,
    expected path from lattice_fit, is a lattice, the issue's expectation or None, r_avoid)."""
    from marl_llm_amd.shapes import r_avoid_for
    g, want = edge_sets()[name]
    ra = r_avoid_for(n_a, shapes)
    rng = np.random.default_rng([list(edge_sets()).index(name), n_a, 29])
    cases = []
    for _ in range(n_env):
        p = g[:, rng.integers(0, g.shape[1], n_a)] + rng.normal(0, 0.05, (2, n_a))
        if name in ("rows64", "rows65"):
            x, y0 = rng.uniform(g[0].min(), g[0].max(), 6), g[1].min()
            p[:, :6] = np.stack([x, y0 + DYADIC * (np.array([0, 62, 63, -1.3, 64.2, 68.7]) + rng.uniform(-0.3, 0.3, 6))])
        dp = rng.uniform(-0.5, 0.5, (2, n_a))
        cases.append((np.ascontiguousarray(p), dp, g, DYADIC))
    path, ok = fit_path(g, n_a, ra)
    return cases, path, ok, want, ra
