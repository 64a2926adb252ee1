"""Lifetime of what a handle owns on the device (csrc/swarm_internal.h: DevBuf): a shape set that replaces another must
leave no trace of the one it replaced, and a handle that has allocated every lazily allocated group (the export lists, the
expert's action scratch, the host-output block with its pinned slots) must close cleanly and leave the next handle of the
same configuration computing the same bits.  Neither test makes an allocation fail."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sets():
    from marl_llm_amd.shapes import SHAPE_NAMES, synthetic_shape_set
    two, three = synthetic_shape_set(SHAPE_NAMES[:2]), synthetic_shape_set(SHAPE_NAMES[:3])
    ng_max = max(np.asarray(g).shape[0] for s in (two, three) for g in s["grid_coords"])
    return two, three, ng_max


def hip_last_error(lib):
    """hipPeekAtLastError of the runtime the library itself is linked to (dlsym through the library's handle)."""
    return int(lib.hipPeekAtLastError())


def test_replacing_a_shape_set(sets):
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.shapes import r_avoid_for
    two, three, ng_max = sets
    E, N = 4, 8
    mk = lambda: SwarmBatch(n_env=E, n_agents=N, n_cells_max=ng_max, r_avoid=r_avoid_for(N, three), obs_dtype=torch.float64)
    sb, fresh = mk(), mk()
    try:
        sb.set_shapes(two)
        sb.reset(seed=3)
        assert set(sb.get_shape_index()) <= {0, 1}
        act = torch.rand((E, N, 2), device=sb.device, generator=torch.Generator(device=sb.device).manual_seed(1)) * 2 - 1
        got = {}
        for name, b in (("replaced", sb), ("fresh", fresh)):
            b.set_shapes(three)
            r = {"obs0": b.reset(seed=7).clone()}            # seed 7 draws shapes (2, 1, 0, 1): every shape of the new set
            r["shape_index"] = b.get_shape_index()
            r["obs"], r["reward"], r["done"], r["a_prior"] = [t.clone() for t in b.step(act)]
            r["p"], r["dp"] = b.get_state()
            r["cells"], r["n_g"] = b.get_cells()
            r["obs_sel"] = b.select_shape(2).clone()         # the shape only the new set has, through the other reader of the set
            got[name] = r
        assert got["fresh"]["shape_index"].tolist() == [2, 1, 0, 1]
        for k, want in got["fresh"].items():
            have = got["replaced"][k]
            same = torch.equal(have, want) if isinstance(want, torch.Tensor) else np.array_equal(have, want)
            assert same, k
        for b in (sb, fresh):
            assert b.lib.swarm_last_error(b.handle) == b""
    finally:
        sb.close(); fresh.close()


def test_every_lazy_buffer_then_destroy(sets):
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.rollout import rollout_expert
    from marl_llm_amd.shapes import r_avoid_for
    two, _, ng_max = sets
    E, N = 2, 8
    a_host = np.random.default_rng(2).uniform(-1, 1, (2, E * N))

    def life():
        """One handle's whole life; everything it computed, as host copies."""
        sb = SwarmBatch(n_env=E, n_agents=N, n_cells_max=ng_max, r_avoid=r_avoid_for(N, two), llm_action=True, with_prior=True)
        try:
            sb.set_shapes(two)
            r = {"obs0": sb.reset(seed=5).clone()}
            r.update(sb.indices())                                           # the export lists
            r["rule"] = sb.rule_action()
            r["host_obs"] = sb.observe_host().copy()                         # the host-output block: slot 1 ...
            for k, v in sb.step_host(a_host).items():                        # ... slot 0, the action through the pinned staging buffer
                r["host_step_" + k] = v.copy()
            for k, v in sb.step_host(None).items():                          # ... slot 1 again, the 'llm' action
                r["host_llm_" + k] = v.copy()
            r["llm"] = sb.llm_action()
            r["expert_obs"], r["expert_stats"] = rollout_expert(sb, 1, reset=(9, 0))   # the expert's fp64 action scratch
            r["expert_act"] = sb._rollout_ring.act                          # the private ring: the rule action's f32 rounding
            r["p"], r["dp"] = sb.get_state()
            r = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.array(v) for k, v in r.items()}
            assert sb.lib.swarm_last_error(sb.handle) == b""
            return r, sb.lib
        finally:
            sb.close()

    from marl_llm_amd import _lib
    _lib.load().hipGetLastError()                # clear what earlier tests of this process left (it returns and resets)
    first, lib = life()
    assert hip_last_error(lib) == 0
    second, _ = life()
    assert hip_last_error(lib) == 0
    assert first.keys() == second.keys()
    for k in first:
        assert first[k].dtype == second[k].dtype and np.array_equal(first[k], second[k], equal_nan=True), k
    assert np.abs(first["rule"]).max() > 0 and first["host_step_reward"].shape == (1, E * N)
