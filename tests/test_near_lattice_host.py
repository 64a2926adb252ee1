"""The inputs of test_gpu_near_lattice.py are what they claim, judged by numpy and the oracle alone (no GPU): the
classification near_lattice_inputs.lattice_fit predicts for every cell set, the fit residuals the construction reaches, and
per accepted case the agents that the exact parent lattice -- the model the lattice kernels decide from -- and the stored
cells decide differently.  Without those agents a kernel that evaluated the model alone would pass the GPU file.
"""
import numpy as np
import pytest

from near_lattice_inputs import (CASES, REACH, build_case, dyadic_parent, edge_case, edge_sets, expected_paths, fit_path, lattice_fit,
                                 near_lattice, reach, rotated_parent)


@pytest.mark.parametrize("name", list(CASES))
def test_cases_classify_as_they_say(shapes, name):
    """Every exact parent is accepted with residuals < 1e-10 steps; a set of delta 5e-7 or 9e-7 is accepted with both
    residual maxima >= 0.9 delta and walks; one of delta 1.5e-6 or 3e-6 is rejected and scans."""
    case = build_case(name, shapes)
    for (p, dp, g, l), parent, delta in zip(case["cases"], case["parents"], case["deltas"]):
        ok, ra_, rb_, ncols, nrows = lattice_fit(parent)
        assert ok and max(ra_, rb_) < 1e-10 and 2 <= ncols <= 64 and 2 <= nrows <= 64, (name, delta, ra_, rb_)
        ok, ra_, rb_, _, _ = lattice_fit(g)
        path = fit_path(g, case["n_a"], case["r_avoid"])[0]
        if delta <= 1e-6:
            assert ok and path == "walk" and (delta == 0 or min(ra_, rb_) >= 0.9 * delta) and max(ra_, rb_) <= 1e-6, (name, delta, ra_, rb_)
        else:
            assert not ok and path == "scan" and max(ra_, rb_) > 1e-6, (name, delta, ra_, rb_)


def test_boundary_of_the_construction(shapes):
    """Accepted up to 9.5e-7 and rejected from 1.05e-6, on a rotated shipped shape and on the dyadic lattice: the window
    between the two is decided by rounding, and no case stands in it."""
    rng = np.random.default_rng(5)
    for parent, l in (rotated_parent(rng, shapes, 0), rotated_parent(rng, shapes, 3), dyadic_parent()):
        for delta, want in ((5e-7, True), (9e-7, True), (9.5e-7, True), (1.05e-6, False), (1.5e-6, False), (3e-6, False)):
            assert lattice_fit(near_lattice(parent, l, delta, rng))[0] == want, delta


def test_what_cell_files_meet(shapes):
    """A float32 round trip of a rotated shipped shape and independent per-cell noise of 2e-7 steps are both rejected (a
    shortened in-row pair becomes the fitted step and scales every column): a cell file that is not exact to double
    rounding scans, so tightening the fit's tolerance would move no real file off the row walk."""
    rng = np.random.default_rng(6)
    for s in range(len(shapes["l_cell"])):
        g, l = rotated_parent(rng, shapes, s)
        assert lattice_fit(g)[0]
        assert not lattice_fit(g.astype(np.float32).astype(np.float64))[0], s
        assert not lattice_fit(g + rng.uniform(-2e-7, 2e-7, g.shape) * l)[0], s


@pytest.mark.parametrize("name", list(CASES))
def test_reach(shapes, oracle, name, capsys):
    """Per case, over its accepted perturbed envs: at least one agent per category of REACH whose answer from the model
    differs from the answer from the stored cells, and the oracle's observation of those envs on the parent cells differs
    from its observation on the stored cells in sensed_index, in_flags (for exactly the agents of the in-shape category) and
    obs.  The counts are printed; profiles/r28/README.md has a copy."""
    case = build_case(name, shapes)
    topo, g_max, occ_max = case["caps"]
    total = dict.fromkeys(REACH, 0)
    differs = dict.fromkeys(("sensed_index", "in_flags", "obs"), 0)
    placed = 0
    for (p, dp, g, l), parent, delta, kind in zip(case["cases"], case["parents"], case["deltas"], case["kinds"]):
        if delta == 0 or not lattice_fit(g)[0]:
            continue
        r = reach(p, parent, g, l, case["r_avoid"])
        for k in REACH:
            total[k] += int(r[k].sum())
        placed += int((kind >= 0).sum())
        kw = dict(is_periodic=case.get("periodic", False), topo=topo, g_max=g_max, occ_max=occ_max)
        model = oracle.get_observation(p, dp, parent, l, case["r_avoid"], **kw)
        truth = oracle.get_observation(p, dp, g, l, case["r_avoid"], **kw)
        assert np.array_equal(model["in_flags"] != truth["in_flags"], r["inshape"]), (name, delta)
        for k in differs:
            differs[k] += int((model[k] != truth[k]).sum())
    with capsys.disabled():
        print("\nreach %-9s placed %4d  " % (name, placed) + "  ".join("%s %3d" % (k, total[k]) for k in REACH))
    for k in REACH:
        assert total[k] >= 1, (name, k, total)
    for k, n in differs.items():
        assert n >= 1, (name, k)


@pytest.mark.parametrize("n_a", [16, 64])
@pytest.mark.parametrize("name", list(edge_sets()))
def test_edge_sets_classify_as_the_issue_expects(shapes, name, n_a):
    """Where the issue names the path of a structural edge set, lattice_fit agrees; the sets it leaves open are accepted: a
    column-major set is the row-major set of the transposed frame, one column is one row of the fitted frame, and two
    cells are a row of two."""
    cases, path, ok, want, ra = edge_case(name, n_a, shapes)
    assert want is None or path == want, (name, path, want)
    if want is None:
        assert ok and path == "walk", name
    if name in ("rows65", "cols65"):                 # refused for the extent alone: the fit itself is exact
        fit = lattice_fit(cases[0][2])
        assert not fit[0] and max(fit[1:3]) < 1e-10 and max(fit[3:]) == 65
