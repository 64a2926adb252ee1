"""The five legacy drop-in symbols of libswarmenv.so (csrc/legacy_shim.hip) held, call for call, to the library they replace.

Every case of helpers.legacy_specs() goes through the shim and through the witnesses with the same wrapper method and the
same arguments (helpers.legacy_call: caller buffers pre-filled with junk), and every output array has to be equal bit for
bit, NaN == NaN.  The witnesses are the C oracle, always, and the reference's own libAssemblyEnv.so (oracle/_ref) wherever
it was built; tests/test_oracle_vs_reference.py holds the two to each other on the same cases without a GPU.

All five symbols are fp64 in the reference's operation order with contraction off, so bit for bit is the bar.  _get_reward
is no exception in what is compared -- its output is 0.0 or 1.0 -- but the device cos may differ from libm's by ulps, and the
value it feeds is only compared with 0.05: helpers.legacy_reach restates |v| in numpy float64 and asserts that every agent
of every reward case is at least 1e-9 away from 0.05 (the closest is 0.0095 away).

The inputs of _get_reward, _sf_b2b_all, _get_dist_b2w and calculateActionPrior are built by hand (helpers.legacy_hand_state,
legacy_sf_case, legacy_b2w_case), not taken from _get_observation: -1 anywhere in a list, duplicates, the own index, far
before near, asymmetric matrices, a radius per agent, an off-centre non-square box.  legacy_reach asserts what each case
reaches from the inputs and the witness's outputs alone.

occupied_index: the reference bounds that list itself (AssemblyEnv.cpp:218-228 picks num_occupied_grid_max entries by
round(i * step) when there are more), so one _get_observation row runs with occ_max = 20 below the 66 occupied cells its
fullest agent has; the other rows give the list room for every cell.
"""
import threading

import numpy as np
import pytest

from helpers import (IDX_JUNK, OBS_JUNK, assert_same, legacy_cache_configs, legacy_call, legacy_case, legacy_reach,
                     legacy_specs)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SPECS = legacy_specs()
SYMBOL = dict(get_observation="_get_observation", get_reward="_get_reward", sf_b2b_all="_sf_b2b_all", dist_b2w="_get_dist_b2w",
              action_prior="calculateActionPrior")


@pytest.fixture(scope="module")
def legacy():
    """RefLib-style caller bound to OUR library instead of libAssemblyEnv.so."""
    from marl_llm_amd import _lib
    from oracle.oracle_py import RefLib
    r = RefLib.__new__(RefLib)
    r.lib = _lib.load()
    return r


@pytest.fixture(scope="module")
def witnesses(oracle):
    """[(name, library)]: the oracle always, the reference's own binary where oracle/_ref holds it."""
    from oracle.oracle_py import RefLib
    w = [("oracle", oracle)]
    if RefLib.available():
        w.append(("reference", RefLib()))
    return w


def held(legacy, witnesses, case, **over):
    got = legacy_call(legacy, case, **over)
    assert legacy.lib.swarm_legacy_status() == 0, legacy.lib.swarm_legacy_last_error()
    for name, w in witnesses:
        assert_same(legacy_call(w, case, **over), got, (case.get("id"), name))
    return got


@pytest.mark.parametrize("spec", SPECS, ids=[s[0] for s in SPECS])
def test_symbol_matches_the_library_it_replaces(legacy, witnesses, spec):
    case = legacy_case(spec)
    legacy_reach(case, witnesses[-1][1])
    got = held(legacy, witnesses, case)
    for k, v in got.items():                     # the reference overwrites every element of every buffer: no junk is left
        assert v.dtype == bool or not (v == (OBS_JUNK if v.dtype.kind == "f" else IDX_JUNK)).any(), k


def test_observation_cache_follows_every_argument(legacy, witnesses):
    """_get_observation keeps one private handle keyed by the whole configuration.  A, B, A, C, A, D, A: each call has to be
    that configuration's own result (the witness's, computed with no cache at all), whatever was cached before it; and the
    witness's results of B, C, D differ from A's, so a handle kept too long could not pass."""
    cfg = legacy_cache_configs()
    ref = {k: legacy_call(witnesses[-1][1], c) for k, c in cfg.items()}
    for k in "BCD":
        assert ref[k]["obs"].shape != ref["A"]["obs"].shape or not np.array_equal(ref[k]["obs"], ref["A"]["obs"]), k
    assert not np.array_equal(ref["C"]["neighbor_index"], ref["A"]["neighbor_index"])      # the box alone changed the neighbours
    for k in "ABACADA":
        held(legacy, witnesses, dict(cfg[k], id="cache-" + k))


FIRST64 = {kind: next(s for s in SPECS if s[1] == kind and s[2][0] == 64) for kind in ("obs", "reward", "sf", "b2w", "prior")}
REFUSALS = [(FIRST64[kind], dict(dim=3)) for kind in FIRST64] + [(FIRST64["obs"], dict(cartesian=False))]


@pytest.mark.parametrize("spec,over", REFUSALS, ids=[s[1] + "-" + "-".join(o) for s, o in REFUSALS])
def test_refusal_is_reported_and_the_next_call_is_good(legacy, witnesses, spec, over):
    """A call the shim refuses (dim = 3 for each symbol; condition[1] false for _get_observation): every double output NaN,
    swarm_legacy_status() == 1, a message that names the symbol; the next good call of the same symbol (for _get_observation:
    through a cache the refusal may have dropped) is held to the witnesses again and reports status 0."""
    case = legacy_case(spec)
    held(legacy, witnesses, case)                                # a cached handle exists before the refusal
    bad = legacy_call(legacy, case, **over)
    assert legacy.lib.swarm_legacy_status() == 1
    assert legacy.lib.swarm_legacy_last_error().startswith(SYMBOL[case["fn"]].encode() + b":")
    for k, v in bad.items():
        if v.dtype.kind == "f":
            assert np.isnan(v).all(), k
    held(legacy, witnesses, case)
    assert legacy.lib.swarm_legacy_last_error() == b""


def test_two_threads_share_the_shim(legacy, witnesses):
    """ctypes releases the lock of the interpreter, the shim serialises on one mutex and shares one device scratch area and
    one cached handle: 30 _get_observation calls on one thread (three configurations in turn, so the handle is rebuilt)
    against 30 calls cycling the other four symbols on another.  Every result equals the same call made alone before."""
    pick = lambda kind, n: [s for s in SPECS if s[1] == kind and s[2][0] in n]
    obs = [legacy_case(s) for s in pick("obs", (63, 64, 65))][:3]
    rest = [legacy_case(pick(kind, (63, 64, 65, 300))[k]) for k in (0, 1) for kind in ("reward", "sf", "b2w", "prior")]
    jobs = {"obs": [obs[k % len(obs)] for k in range(30)], "rest": [rest[k % len(rest)] for k in range(30)]}
    serial = {c["id"]: held(legacy, witnesses, c) for c in obs + rest}
    out, err = {"obs": [], "rest": []}, []

    def work(name):
        try:
            for c in jobs[name]:
                out[name].append((c["id"], legacy_call(legacy, c), legacy.lib.swarm_legacy_status()))
        except Exception as e:                                   # noqa: BLE001 - reported by the main thread
            err.append(repr(e))

    ts = [threading.Thread(target=work, args=(n,)) for n in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not err, err
    for name in jobs:
        assert len(out[name]) == 30
        for cid, got, status in out[name]:
            assert status == 0
            assert_same(serial[cid], got, (name, cid))
