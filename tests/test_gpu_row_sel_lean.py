"""The window rows of the lattice walk in the step kernels of 64 agent threads (csrc/swarm_env.hip, row_sel_lean).

Those kernels work out, per agent and lattice row, the set columns within the sensing radius (the window rows) and within
r_avoid / 2 (the covered columns) as a 32-bit word relative to the pass's first possible column c0: the row mask is shifted
down to c0 once, the interval [ceil(ax - ho), floor(ax + ho)] is formed in fp32 from the agent's column coordinate relative
to c0 and clamped to 0 and to the lattice's last column, an interval wholly beside the lattice is empty, and an end column
whose model distance lies inside the margin around the radius goes to the reference's fp64 test on the stored cell.  The
covered words are shifted back to lattice columns for the OR into the env's covered rows.  A slip shows in sensed_index,
occupied_index and the observation rows, the reward and the prior.

The nearest-cell walk of the same kernels is held here too where two candidates tie or nearly tie: two sides of one row,
two adjacent rows (two walking waves), two rows of one trip of a wave (rows r and r + 3), two rows in different trips
(rows 9 and 12) -- the lower cell index wins -- and an agent forty steps from the shape whose two best candidates differ
only in the last three bits of the fp32 squared distance.

Every case is small lattices: TALL (20 rows x 12 columns, cut by hand) and cut(nc) (12 rows of 32, 33, 39, 40 or 64
columns: full rows with two holes each, a left third, a right third, a row of one cell), each with cells in its last
column.  The first agents of an env stand at chosen lattice coordinates (chosen()), the others are scattered around and
beyond the lattice.  Every call writes into caller-owned tensors filled with NaN / 255 before the call
and every field is compared bit for bit with the oracle (lockstep.compare): observe, then three steps.  Each case ASSERTS
that its situations occurred, from the positions of the oracle's trajectory and a numpy restatement of the fp32 interval
model (facts); seed 0 of every case was checked on the CPU to reach them.

  tall       TALL alone: the ties, the near tie far out, agents on every side of the lattice, uncertain end columns for both
             radii, free and at the lattice's edge
  c32 .. c64 one env of 32 / 33 / 39 / 40 / 64 columns: 32-bit and 64-bit row masks, a window across bit 32 of the mask,
             c0 clamped at 0 and (64 columns) at 63, a sensed cell in column 63
  n57        57 agents: inactive lanes walk along and must leave nothing behind
  periodic   a periodic arena, agents at the arena's edges too
  exact      force_exact
  bf16, f64  the other row dtypes
  mixed      one env on jittered cells takes the generic launch, the lattice envs the kernels with the mixed-batch filter
  widths     a 40-column env beside a 12-column one: the batch's masks are 64-bit, each env walks by its own width
  ra_wide    r_avoid = 1.25 on 64 columns: the covered radius is 10 steps, a covered window of 21 rows and columns -- covered
             columns up to 21 behind the pass's first column, past the 17 a sensed row can hold; the covered pass's first
             column clamped at 63
  ra_huge    r_avoid = 1.9: 15.2 steps, a covered window of 31 rows, more than the 32-bit covered word takes -- the set must
             take the generic scan (recognised as a lattice, not walked) and still equal the oracle
"""
import numpy as np
import pytest

from helpers import obs_feedback, oracle_run, pad_cells, random_actions
from lockstep import FIELDS, OBSERVE, compare, device_layout, host_copy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

G_MAX = 80
TORCH_DT = dict(f64=torch.float64, f32=torch.float32, bf16=torch.bfloat16)

STEPS, D_SEN, L = 3, 0.4, 0.0625                   # step 2^-4: the cells and the chosen positions are exact in binary
EPS = 3e-5                                         # steps inside a radius: within the model's margin (>= 1e-4), outside its error
# 20 rows x 12 columns ('#' = cell), row 0 first.  Rows 4, 5 lie right and rows 10, 11 left: an agent at their empty end
# has its nearest cells in the rows around them, three rows apart.
TALL = ["############",
        "############",
        "############",
        "############",
        "........####",
        "........####",
        "############",
        "############",
        "############",
        "############",
        "####........",
        "####........",
        "############",
        "############",
        "############",
        "#####..#####",
        "############",
        "############",
        "##...##...##",
        "############"]


def cut(nc):
    """12 rows x nc columns: full rows with two holes each, row 4 the left third, row 5 the right third, row 9 one cell in
    the last column."""
    rows = []
    for r in range(12):
        row = ["#"] * nc
        row[(5 * r + 3) % (nc - 1)] = "."
        row[(11 * r + 7) % (nc - 1)] = "."
        if r == 4:
            row = ["#" if c < nc // 3 else "." for c in range(nc)]
        if r == 5:
            row = ["#" if c >= nc - nc // 3 else "." for c in range(nc)]
        if r == 9:
            row = ["."] * (nc - 1) + ["#"]
        rows.append("".join(row))
    return rows


def chosen(kind, nc, rho, rho_c):
    """Lattice coordinates (column a, row b) of the first agents of an env.  rho, rho_c: the sensed and the covered radius
    in steps."""
    if kind in "TJ":
        return [(2.0, 4.5),                    # (2, 3) and (2, 6) tie: rows 0 mod 3, one trip
                (9.0, 10.5),                   # (9, 9) and (9, 12) tie: rows 0 mod 3, trips 0 and 1
                (5.0, 7.5),                    # (5, 7) and (5, 8) tie: adjacent rows, two waves
                (5.5, 14.0),                   # (5, 14) and (6, 14) tie: two sides of one row
                (7.0, 2.0),                    # on a lattice point
                (52.0 + 2.0 ** -18, 16.5 + 2.0 ** -12),   # 41 steps right: (11, 16) and (11, 17) differ by 2^-11 in d2, four ulp
                (-9.0, 5.0),                   # left of the lattice by more than the radius
                (20.0, 8.0),                   # right of it
                (5.0, -9.0),                   # below
                (5.0, 28.0),                   # above
                (rho - EPS, 2.0),              # column 0 of row 2 at the sensed radius, from inside
                (-rho + EPS, 3.0),             # the same from the left: column 0 is the clamped first and the last column
                (11.0 + rho - EPS, 6.0),       # column 11 of row 6: the clamped last and the first column
                (4.0 + rho_c - EPS, 12.0),     # column 4 of row 12 at the covered radius
                (-rho_c + EPS, 13.0),          # column 0 of row 13 at the covered radius, the clamped first column
                (rho + EPS, 1.0),              # column 0 of row 1 just outside the sensed radius: the first column, uncertain, out
                (8.0 - rho - EPS, 0.0),        # column 8 of row 0 just outside it: the last column
                (8.0 - rho + EPS, 19.0),       # column 8 of row 19 just inside it: the last column
                (4.0 + rho_c + EPS, 16.0),     # column 4 of row 16 just outside the covered radius: the first column
                (8.0 - rho_c - EPS, 19.0),     # column 8 of row 19 just outside it: the last column
                (3.25, 17.5)]                  # inside, c0 clamped at 0
    return [(nc - 1.5, 5.25),                  # senses the last column
            (nc - 1.0 + rho - EPS, 2.0),       # the last column of row 2 at the sensed radius: the clamped last column
            (2.5, 7.25),                       # c0 clamped at 0
            (31.5, 6.0),                       # window columns 26 .. 37: across bit 32 of a 64-bit row mask
            (nc - 1.0, 9.0),                   # on the single cell of row 9, in the last column
            (nc - 1.0 + rho - 0.3, 3.0),       # c0 = the last column (63 of 64: the upper clamp's edge, not clamped)
            (nc + 7.0, 5.0),                   # c0 behind the last column (64 columns: clamped at 63), nothing in range
            (min(nc - 1.0 + rho_c + 0.2, nc + 9.2), 4.0),   # the covered pass's first column behind the last column
            (nc / 2.0, 6.5)]


def lattice_env(rng, kind, n_a, periodic, ra):
    """One env of kind T (TALL), J (TALL, jittered off the lattice) or an int nc (cut(nc)): its description for facts() and
    (p, dp, cells, l_cell).  Cells in row-major order, index = the device's."""
    rows = TALL if kind in ("T", "J") else cut(kind)
    mask = np.array([[ch == "#" for ch in r] for r in rows])
    nr, nc = mask.shape
    o = np.array([-1.5, -0.625]) if kind in ("T", "J") else np.array([-2.25, -0.375])
    rc = np.argwhere(mask)                                        # (row, column), row-major
    g = np.stack([o[0] + L * rc[:, 1], o[1] + L * rc[:, 0]]).astype(np.float64)
    sp = chosen("T" if kind in ("T", "J") else "C", nc, D_SEN / L, ra / 2 / L)
    ab = np.stack([rng.uniform(-3.0, nc + 2.0, n_a), rng.uniform(-3.0, nr + 2.0, n_a)])
    near = rng.integers(0, len(rc), n_a // 3)                     # a third of them on the shape
    ab[:, : len(near)] = rc[near][:, ::-1].T + rng.normal(0, 0.4, (2, len(near)))
    ab = np.roll(ab, len(sp), axis=1)
    p = np.clip(np.stack([o[0] + L * ab[0], o[1] + L * ab[1]]), -2.3, 2.3)
    p[:, : len(sp)] = (o[:, None] + L * np.array(sp).T)
    assert np.abs(p).max() < 2.39
    dp = rng.uniform(-0.3, 0.3, (2, n_a))
    dp[:, : len(sp)] *= 0.02                                      # the chosen ones stay close to their places
    if periodic:                                                  # the last four at the arena's edges, moving out
        p[:, -4:] = [[-2.39, 0.3, 2.395, -0.7], [0.1, 2.39, -0.4, -2.395]]
        dp[:, -4:] = [[-0.5, 0.02, 0.5, 0.01], [0.03, 0.5, -0.02, -0.5]]
    if kind == "J":
        g = g + rng.normal(0, 0.004, g.shape)
    spec = None if kind == "J" else dict(mask=mask, o=o, g=np.ascontiguousarray(g))
    return spec, (np.ascontiguousarray(p), np.ascontiguousarray(dp), np.ascontiguousarray(g), L)


def facts(spec, p, ra):
    """What the agents at p (2, n) meet in the lattice `spec`.  The window rows: the fp32 interval model restated -- first
    column c0, relative coordinate, the margin lat_m, the clamped ends and the end columns inside the margin -- for the
    sensed ("sen") and the covered ("cov") radius.  The nearest cell: the two best cells by the reference's distance, and
    the fp32 squared distances of the model in lattice units."""
    f32 = np.float32
    mask, g, o = spec["mask"], spec["g"], spec["o"]
    nr, nc = mask.shape
    rowstart = np.concatenate([[0], np.cumsum(mask.sum(axis=1))])
    row_of = np.argwhere(mask)[:, 0]
    col_of = np.argwhere(mask)[:, 1]
    got = {"cols_%d" % nc}
    if mask[:, nc - 1].any():
        got.add("cell_in_last_column")
    for x, y in p.T:
        a, b = (x - o[0]) / L, (y - o[1]) / L
        apf, bpf = f32(a), f32(b)
        m = max(f32(1e-4), f32(8e-7) * max(abs(apf), abs(bpf)))
        if a == np.floor(a) and b == np.floor(b) and 0 <= a < nc and 0 <= b < nr and mask[int(b), int(a)]:
            got.add("on_point")
        for name, rho, cut in (("sen", f32(D_SEN / L), D_SEN * D_SEN), ("cov", f32(ra / 2 / L), (ra / 2) * (ra / 2))):
            raw0 = int(np.ceil(apf - (rho + f32(2) * m)))
            c0 = min(max(raw0, 0), 63)
            ax = f32(a - c0)
            cmax = min(nc - 1 - c0, 30)
            ro, ri = rho + m, rho - m
            ro2, ri2 = ro * ro, (ri * ri if ri > 0 else f32(0))
            b0 = int(np.ceil(bpf - (rho + f32(2) * m)))
            seen, rows_in, rows_out = False, 0, 0
            for bb in range(b0, b0 + 16):
                dy = f32(bb) - bpf
                dy2 = dy * dy
                ho2 = ro2 - dy2
                if not ho2 > 0:
                    continue
                if not 0 <= bb < nr:
                    rows_out += 1
                    continue
                rows_in += 1
                ho = np.sqrt(ho2)
                f0, f1 = np.ceil(ax - ho), np.floor(ax + ho)
                lo, hi = max(f0, f32(0)), min(f1, f32(cmax))
                if hi < lo:
                    if name == "sen":
                        got |= {"left_empty"} if f1 < 0 else set()
                        got |= {"right_empty"} if f0 > nc - 1 - c0 else set()
                    continue
                cols = [c for c in range(c0 + int(lo), c0 + int(hi) + 1) if mask[bb, c]]
                if name == "cov" and cols and cols[-1] - c0 > 17:
                    got.add("cov_past_17")
                for which, end, raw in (("lo", lo, f0), ("hi", hi, f1)):
                    e = float(end) - float(ax)
                    d2 = f32(e * e + float(dy2))
                    if not d2 < ri2 and mask[bb, c0 + int(end)]:      # an uncertain end column: the exact test decides
                        c = rowstart[bb] + int(mask[bb, : c0 + int(end)].sum())
                        ex, ey = g[0, c] - x, g[1, c] - y
                        inside = ex * ex + ey * ey < cut
                        got.add("band_" + name)
                        got.add("band_%s_%s_%s" % ("in" if inside else "out", which, name))
                        if end != raw:
                            got.add("band_clamped_" + name)
                if name == "sen" and cols:
                    seen = True
                    if 20 <= c0 <= 31 and cols[0] < 32 <= cols[-1]:
                        got.add("straddle_32")
                    if cols[-1] == 63:
                        got.add("col_63_sensed")
                    if cols[-1] == nc - 1:
                        got.add("last_column_sensed")
                    if c0 == nc - 1:
                        got.add("c0_last_column")
            if name == "cov":
                got |= {"c0_clamped_63_cov"} if raw0 > 63 else set()
            if name == "sen":
                got |= {"c0_clamped_0"} if raw0 < 0 and seen else set()
                got |= {"c0_clamped_63"} if raw0 > 63 else set()
                if rows_in == 0 and rows_out > 0:
                    got.add("below" if b < 0 else "above")
        d2 = (g[0] - x) ** 2 + (g[1] - y) ** 2
        first, second = np.argsort(d2, kind="stable")[:2]
        r1, r2 = sorted((row_of[first], row_of[second]))
        if d2[first] == d2[second]:
            got.add("tie_one_row" if r1 == r2 else "tie_adjacent_rows" if r2 == r1 + 1 else
                    "tie_one_trip" if r1 % 3 == r2 % 3 and r1 // 12 == r2 // 12 else
                    "tie_two_trips" if r1 % 3 == r2 % 3 else "tie_other")
        else:
            k = []
            for c in (first, second):
                dx, dy = f32(col_of[c]) - apf, f32(row_of[c]) - bpf
                k.append(f32(float(dx) * float(dx) + float(dy * dy)).view(np.uint32))
            if np.sqrt(d2[first]) / L >= 40 and k[0] != k[1] and (k[0] & ~np.uint32(7)) == (k[1] & ~np.uint32(7)):
                got.add("far_low_bits")
    assert rowstart[-1] == g.shape[1]
    return got


TIES = ("tie_one_row", "tie_adjacent_rows", "tie_one_trip", "tie_two_trips")
SIDES = ("left_empty", "right_empty", "below", "above")
BANDS = ("band_sen", "band_cov", "band_clamped_sen", "band_clamped_cov", "band_in_lo_sen", "band_in_hi_sen", "band_out_lo_sen",
         "band_out_hi_sen", "band_in_lo_cov", "band_out_lo_cov", "band_out_hi_cov")
TALL_REQ = TIES + SIDES + BANDS + ("far_low_bits", "on_point", "c0_clamped_0", "cols_12", "cell_in_last_column")
CUT_REQ = ("band_sen", "band_clamped_sen", "c0_clamped_0", "last_column_sensed", "c0_last_column", "right_empty", "on_point",
           "cell_in_last_column")
WIDE_REQ = CUT_REQ + ("straddle_32",)
#        name       n_a  envs  dtype  SwarmBatch / oracle options  required
CASES = {
    "tall":     (64, ("T",), "f32", {}, TALL_REQ),
    "c32":      (64, (32,), "f32", {}, CUT_REQ + ("cols_32",)),
    "c33":      (64, (33,), "f32", {}, WIDE_REQ + ("cols_33",)),
    "c39":      (64, (39,), "f32", {}, WIDE_REQ + ("cols_39",)),
    "c40":      (64, (40,), "f32", {}, WIDE_REQ + ("cols_40",)),
    "c64":      (64, (64,), "f32", {}, WIDE_REQ + ("cols_64", "col_63_sensed", "c0_clamped_63", "c0_clamped_63_cov")),
    "n57":      (57, ("T", 40), "f32", {}, TALL_REQ + WIDE_REQ),
    "periodic": (64, ("T", 40), "f32", dict(periodic=True), TALL_REQ + WIDE_REQ),
    "exact":    (64, ("T", 40), "f32", dict(debug_flags=1), TALL_REQ + WIDE_REQ),
    "bf16":     (64, ("T", 40), "bf16", {}, TALL_REQ + WIDE_REQ),
    "f64":      (64, ("T", 40), "f64", {}, TALL_REQ + WIDE_REQ),
    "mixed":    (64, ("T", "J", 40), "f32", {}, TALL_REQ + WIDE_REQ),
    "widths":   (64, (40, "T"), "f32", {}, TALL_REQ + WIDE_REQ + ("cols_12", "cols_40")),
    "ra_wide":  (64, (64,), "f32", dict(ra=1.25), ("cols_64", "cov_past_17", "c0_clamped_63_cov", "col_63_sensed")),
    "ra_huge":  (64, (64,), "f32", dict(ra=1.9, walks=0), ("cols_64",)),
}
_REF = {}


def build(oracle, shapes, name, seed=0):
    """The inputs of a case and the oracle's trajectory of them, once per case: (specs, cases, oracle_run's result, r_avoid)."""
    from marl_llm_amd.shapes import r_avoid_for
    key = (name, seed)
    if key not in _REF:
        n_a, envs, dtype, opt, _ = CASES[name]
        rng = np.random.default_rng([n_a, len(envs), seed, 59])
        ra = opt.get("ra", r_avoid_for(n_a, shapes))
        made = [lattice_env(rng, kind, n_a, bool(opt.get("periodic")), ra) for kind in envs]
        cases = [m[1] for m in made]
        oopt = {k: v for k, v in opt.items() if k not in ("debug_flags", "ra", "walks")}
        ref = oracle_run(oracle, cases, random_actions(rng, STEPS, len(envs), n_a), ra, g_max=G_MAX, feedback=obs_feedback(dtype), **oopt)
        _REF[key] = ([m[0] for m in made], cases, ref, ra)
    return _REF[key]


def reached(specs, cases, ref, ra):
    """The situations the oracle's trajectory reaches in the lattice envs: the first state and the state after each step."""
    got = set()
    for e, spec in enumerate(specs):
        if spec is not None:
            for p in [cases[e][0]] + [step[e]["p"] for step in ref[1]]:
                got |= facts(spec, p, ra)
    return got


class Poisoned:
    """A SwarmBatch over `cases` whose every call writes into the same caller-owned tensors, poisoned before each call.
    lattice: the number of envs that must be recognised as lattices; walks: the number the row walk must step."""

    def __init__(self, cases, ra, dtype, lattice, walks, periodic=False, **kw):
        from marl_llm_amd.batched import SwarmBatch
        cells, n_g = pad_cells([c[2] for c in cases], max(c[2].shape[1] for c in cases) + 3)
        E, N = len(cases), cases[0][0].shape[1]
        self.sb = sb = SwarmBatch(n_env=E, n_agents=N, n_cells_max=cells.shape[2], r_avoid=ra, g_max=G_MAX, obs_dtype=TORCH_DT[dtype],
                                  is_boundary=not periodic, d_sen=D_SEN, **kw)
        self.dtype = dtype
        try:
            sb.set_cells(cells, n_g, [c[3] for c in cases])
            assert sb.lattice_envs() == lattice, (sb.lattice_envs(), lattice)
            assert sb.path_envs() == (walks, E - walks), (sb.path_envs(), walks)
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

    def observe(self, first):
        self.poison()
        self.sb.observe(out=self.out["obs"])
        dev = host_copy(self.sb, self.out["obs"], state=False, indices=True)
        compare(dev, device_layout(first, self.dtype), "observe", fields=OBSERVE)
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


@pytest.mark.parametrize("name", list(CASES))
def test_window_rows_in_lockstep(oracle, shapes, name):
    """observe and three steps into poisoned caller-owned tensors, every field bit-equal to the oracle; the case's situations
    occurred."""
    n_a, envs, dtype, opt, required = CASES[name]
    specs, cases, ref, ra = build(oracle, shapes, name)
    first, steps, counts = ref
    got = reached(specs, cases, ref, ra)
    print(name, sorted(got), counts)
    assert not set(required) - got, sorted(set(required) - got)
    for spec in specs:
        if spec is not None:
            assert spec["mask"].shape[0] <= 20
    n_lat = sum(s is not None for s in specs)
    run = Poisoned(cases, ra, dtype, n_lat, opt.get("walks", n_lat),
                   **{k: v for k, v in opt.items() if k not in ("ra", "walks")})
    try:
        calls = [run.observe(first)]
        for t, step in enumerate(steps):
            calls.append(run.step(step, t))
    finally:
        run.close()
    assert calls[0]["obs"].shape[1] == n_a
    inf = np.concatenate([c["in_flags"].ravel() for c in calls])
    assert (inf != 0).any() and (inf == 0).any()                                 # agents inside and outside the shape
    assert any((c["occupied_index"] >= 0).any() for c in calls)                  # the covered pass had something to say
    if name == "periodic":
        assert counts["wrap"].sum() > 0, counts                                  # an agent left through an edge
