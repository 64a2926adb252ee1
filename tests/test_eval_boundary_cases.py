"""Inputs on the decision boundaries of the evaluation metrics (coverage_rate, distribution_uniformity,
voronoi_based_uniformity), built and checked on the CPU with the oracle's restatement of the wrapper
(oracle_py.wrapper_metrics) so that the expected values are known before any kernel sees them.
tests/test_gpu_rollout_eval.py feeds the same inputs to the evaluation loop's metrics kernel and to swarm_metrics."""
import numpy as np


def boundary_cases(r_avoid):
    """Per env (p [2, 4], cells [2, n_g]) on the decision boundaries of the metrics: the coverage threshold r_avoid / 2 and
    one ulp to either side, Voronoi ties (equal distances; different squared distances whose rounded norms coincide),
    coincident agents (distance 0 is skipped), all minimum distances equal, n_g = 1."""
    h = r_avoid / 2
    far = np.array([[2.0, -2.0, 2.0], [2.0, 2.0, -2.0]])
    one = np.zeros((2, 1))
    cases = []
    for x in (h, np.nextafter(h, 0.0), np.nextafter(h, 1.0)):                  # exactly at, just inside, just outside
        cases.append((np.concatenate([[[x], [0.0]], far], 1), one))
    # two agents equidistant from cell 0: np.argmin gives it to agent 0, which also owns cell 1 -> counts (2, 0, 0, 0)
    cases.append((np.array([[0.3, -0.3, 2.0, -2.0], [0.0, 0.0, 2.0, 2.0]]), np.array([[0.0, 0.35], [0.0, 0.0]])))
    # agent 0 at squared distance 1 + 2^-52 (its norm rounds to 1.0), agent 1 at exactly 1.0: np.argmin picks agent 0
    a, b = None, None
    base = np.array([0.6, 0.8])
    for i in range(-40, 41):
        for j in range(-40, 41):
            x = base[0] + i * 2.0 ** -53; y = base[1] + j * 2.0 ** -53
            if x * x + y * y == 1.0 + 2.0 ** -52 and np.sqrt(x * x + y * y) == 1.0:
                a, b = x, y
    assert a is not None
    cases.append((np.array([[a, 1.0, 2.0, -2.0], [b, 0.0, 2.0, 2.0]]), np.array([[0.0, 0.6], [0.0, 0.9]])))
    cases.append((np.array([[0.5, 0.5, -0.5, 1.5], [0.5, 0.5, 0.5, 0.5]]), np.array([[0.5, -0.5], [0.5, 0.5]])))   # coincident
    cases.append((np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]]),                                          # a square:
                  np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]])))                                         # all minima equal
    return cases


def test_boundary_cases_are_what_they_claim():
    """The oracle's restatement on the constructed inputs: they sit where they are meant to sit."""
    from oracle.oracle_py import wrapper_metrics
    ra = 0.37
    c = boundary_cases(ra)
    m = [wrapper_metrics(p, g, ra) for p, g in c]
    assert [x[0] for x in m[:3]] == [0.0, 1.0, 0.0]
    for k in (3, 4):                                               # the tie goes to agent 0: counts (2, 0, 0, 0), not (1, 1, 0, 0)
        assert m[k][2] == (np.var([2.0, 0, 0, 0]) - 0.0) / 2.0 != (np.var([1.0, 1, 0, 0]) - 0.0) / 1.0
    assert m[5][0] == 1.0 and m[5][1] == -np.inf                   # the coincident pair's next distance equals the others'
    assert m[6][0] == 1.0 and m[6][1] == -np.inf and m[6][2] == -np.inf      # max == min: a division by zero




def near_tie_states(r_avoid, E=3, N=6, G=256, seed=0):
    """p [E, 2, N], cells [E, 2, G]: every cell has two agents at nearly the same distance -- agent b is agent a mirrored
    through the cell and moved by k ulps, k in -3..3, so their squared distances agree to a few 2^-52 (equal, or different
    with equal or different rounded norms) -- and cells at r_avoid / 2 +- a few ulps from an agent."""
    rs = np.random.RandomState(seed)
    p = rs.uniform(-2.0, 2.0, (E, 2, N))
    cells = np.zeros((E, 2, G))
    for e in range(E):
        for c in range(G):
            a = rs.randint(N)
            if c % 4 == 3:                                         # a cell a few ulps around r_avoid / 2 from agent a
                x = r_avoid / 2
                for _ in range(abs(c // 4 % 7 - 3)):
                    x = np.nextafter(x, 0.0 if c // 4 % 7 < 3 else 1.0)
                cells[e, :, c] = p[e, :, a] + (np.array([x, 0.0]) if c % 8 == 3 else np.array([0.0, -x]))
            else:                                                  # midway between agents a and b, nudged by ulps
                b = (a + 1 + rs.randint(N - 1)) % N
                mid = (p[e, :, a] + p[e, :, b]) / 2
                for _ in range(abs(c % 7 - 3)):
                    mid[0] = np.nextafter(mid[0], -9.0 if c % 7 < 3 else 9.0)
                cells[e, :, c] = mid
    return p, cells


def test_near_tie_states_contain_ties_after_rounding():
    """Among the constructed cells some have a unique smallest squared distance whose rounded norm is shared by another
    agent (the case a squared-distance argmin would get wrong when the other agent has the lower index)."""
    p, cells = near_tie_states(0.37)
    rounded_only, exact = 0, 0
    for e in range(p.shape[0]):
        for c in range(cells.shape[2]):
            d2 = ((p[e] - cells[e][:, [c]]) ** 2).sum(axis=0)
            d = np.sqrt(d2)
            exact += (d2 == d2.min()).sum() > 1
            rounded_only += (d == d.min()).sum() > (d2 == d2.min()).sum()
    assert rounded_only > 0 and exact > 0, (rounded_only, exact)
