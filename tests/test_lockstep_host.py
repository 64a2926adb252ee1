"""lockstep.compare held to its own claim, without a GPU: the oracle's result restated in the device's layout passes, and one
element of one env changed by the smallest representable amount -- in every field the comparator says it checks -- raises
Mismatch naming that field and exactly that env."""
import numpy as np
import pytest

from helpers import make_case
from lockstep import FIELDS, IDX, Mismatch, compare, device_layout

torch = pytest.importorskip("torch")

N, E, ENV, ENV0 = 8, 3, 1, 40


@pytest.fixture(scope="module")
def stepped(oracle, shapes):
    """One oracle.step of E make_case envs: the [E] result dicts."""
    from marl_llm_amd.shapes import r_avoid_for
    rng = np.random.default_rng(12)
    ra = r_avoid_for(N, shapes)
    res = []
    for _ in range(E):
        p, dp, g, l_cell = make_case(rng, shapes, N, 1)
        nei = oracle.get_observation(p, dp, g, l_cell, ra)["neighbor_index"]
        res.append(oracle.step(p, dp, rng.uniform(-1, 1, (2, N)), g, nei, l_cell, ra))
    return res


def _device_side(res, dtype):
    """What a handle of obs dtype `dtype` would hand host_copy for `res`, restated here and not taken from lockstep."""
    rows = lambda k: torch.from_numpy(np.stack([r[k].T for r in res]))                  # [E, D, N] -> [E, N, D]
    cast = {"f64": lambda t: t, "f32": lambda t: t.float(), "bf16": lambda t: t.float().bfloat16().float()}[dtype]
    dev = dict(obs=cast(rows("obs")).numpy(), a_prior=cast(rows("a_prior")).numpy(), head=32, done=np.zeros((E, N), np.uint8))
    dev.update({k: np.stack([r[k] for r in res]) for k in ("p", "dp") + IDX})
    dev["reward"] = np.stack([r["reward"][0] for r in res])
    assert dev["obs"].dtype == (np.float64 if dtype == "f64" else np.float32) and dev["obs"].shape == (E, N, 192)
    return dev


def _corrupt(dev, field, env):
    """One element of env `env` of `field` changed by the least amount."""
    if field == "unused":
        i, s = np.argwhere(dev["sensed_index"][env] < 0)[0]
        dev["obs"][env, i, dev["head"] + 2 * s + 1] = np.finfo(dev["obs"].dtype).tiny
    elif field == "done":
        dev["done"][env, N - 1] = 1
    elif field in IDX:
        dev[field][env][(-1,) * (dev[field].ndim - 1)] += 1
    else:
        x = dev[field][env]
        x[(-1,) * x.ndim] = np.nextafter(x[(-1,) * x.ndim], np.asarray(np.inf, x.dtype))


@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_the_restated_device_side_passes(stepped, dtype):
    ref = device_layout(stepped, dtype)
    compare(_device_side(stepped, dtype), ref, "step")
    if dtype != "f64":          # the narrow formats are really narrower: the float64 layout does not pass for them
        with pytest.raises(Mismatch):
            compare(_device_side(stepped, dtype), device_layout(stepped, "f64"), "step")


@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
@pytest.mark.parametrize("field", FIELDS)
def test_one_changed_element_is_named(stepped, field, dtype):
    dev = _device_side(stepped, dtype)
    _corrupt(dev, field, ENV)
    with pytest.raises(Mismatch) as ex:
        compare(dev, device_layout(stepped, dtype), 7, env0=ENV0)
    # an unused slot is part of obs too: obs comes first in FIELDS, so the rule itself is named only once obs is left out
    if field == "unused":
        assert ex.value.field == "obs"
        with pytest.raises(Mismatch) as ex:
            compare(dev, device_layout(stepped, dtype), 7, env0=ENV0, fields=[f for f in FIELDS if f != "obs"])
    assert (ex.value.field, ex.value.tag, list(ex.value.envs)) == (field, 7, [ENV + ENV0])
    assert isinstance(ex.value, AssertionError)


def test_a_field_left_out_is_not_compared_and_missing_indices_are_skipped(stepped):
    ref = device_layout(stepped)
    dev = _device_side(stepped, "f64")
    _corrupt(dev, "a_prior", ENV)
    compare(dev, ref, fields=[f for f in FIELDS if f != "a_prior"])
    dev = {k: v for k, v in _device_side(stepped, "f64").items() if k not in IDX}
    compare(dev, ref, indices=False)
    with pytest.raises(KeyError):
        compare(dev, ref)


@pytest.mark.parametrize("field", ["dp", "obs", "sensed_index", "done"])
def test_env_subset(stepped, field):
    """envs = [0, 2] with the oracle's rows for those two: env 1 is not looked at, env 2 is, and is named as env 2."""
    ref = device_layout([stepped[0], stepped[2]])
    dev = _device_side(stepped, "f64")
    _corrupt(dev, field, 1)
    compare(dev, ref, envs=[0, 2])
    _corrupt(dev, field, 2)
    with pytest.raises(Mismatch) as ex:
        compare(dev, ref, "sample", envs=[0, 2], env0=ENV0)
    assert (ex.value.field, list(ex.value.envs)) == (field, [2 + ENV0])


def test_both_reference_forms_give_the_same_layout(stepped):
    """A list of per-env dicts and ThreadedOracle's dict of [E, ...] arrays (reward [E, N], no done)."""
    stacked = {k: np.stack([r[k] for r in stepped]) for k in stepped[0] if k != "done"}
    stacked["reward"] = stacked["reward"][:, 0]
    a, b = device_layout(stepped, "bf16"), device_layout(stacked, "bf16")
    for k in stacked:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
