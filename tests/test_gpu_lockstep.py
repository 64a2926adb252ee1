"""lockstep.hold wired to the device and not to itself: with the oracle's own trajectory it passes, and with a copy of that
trajectory in which one element of step 1 of env 1 is changed by the least amount it raises Mismatch naming the step, the env
and the field -- for every field the reference carries.  `done` and the unused-slot rule are properties of the device's
output alone (the reference has nothing to change for them); tests/test_lockstep_host.py holds those on the CPU."""
import copy

import numpy as np
import pytest

from helpers import make_case, oracle_run, random_actions
from lockstep import IDX, Mismatch, hold

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, E = 8, 3
PATHS = pytest.mark.parametrize("flags", [0, 2], ids=["lattice", "generic"])


@pytest.fixture(scope="module")
def run(oracle, shapes):
    """E envs, the oracle's observation and two steps of them (never modified), and r_avoid."""
    from marl_llm_amd.shapes import r_avoid_for
    rng = np.random.default_rng(21)
    ra = r_avoid_for(N, shapes)
    cases = [make_case(rng, shapes, N, 1) for _ in range(E)]
    return cases, oracle_run(oracle, cases, random_actions(rng, 2, E, N), ra), ra


def _hold(cases, ref, ra, flags):
    return hold(cases, ref, lattice=0 if flags & 2 else E, r_avoid=ra, obs_dtype=torch.float64, debug_flags=flags)


@PATHS
def test_the_oracles_trajectory_passes(run, flags):
    cases, ref, ra = run
    seen = _hold(cases, ref, ra, flags)
    assert len(seen) == 3 and np.array_equal(seen[2]["p"], np.stack([s["p"] for s in ref[1][1]]))


@PATHS
@pytest.mark.parametrize("field", ("p", "dp", "obs", "a_prior", "reward") + IDX)
def test_a_changed_reference_is_caught(run, field, flags):
    cases, ref, ra = run
    steps = copy.deepcopy(ref[1])
    x = steps[1][1][field]
    last = (-1,) * x.ndim
    x[last] = x[last] + 1 if field in IDX else np.nextafter(x[last], np.inf)
    with pytest.raises(Mismatch) as ex:
        _hold(cases, (ref[0], steps), ra, flags)
    assert (ex.value.field, ex.value.tag, list(ex.value.envs)) == (field, 1, [1])
