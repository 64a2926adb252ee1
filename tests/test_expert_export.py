"""save_expert_data (marl_llm_amd/rollout.py): a ChainedReplay's transitions as the reference's expert_data.npz
(ReplayBufferExpert.save in buffer_expert.py: keys obs_buffs / ac_buffs / next_obs_buffs / done_buffs, float64), oldest step
first, sealed slots skipped.  CPU only: the ring is filled by ChainedReplay.push on CPU tensors."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

KEYS = ("obs_buffs", "ac_buffs", "next_obs_buffs", "done_buffs")


class ExpertPushes:
    """ReplayBufferExpert.push as collect_expert_data.py drives it, restated: per step the numpy API's (D, n_a) obs,
    (2, n_a) action, (D, n_a) next_obs and (1, n_a) done; every block is transposed into n_a rows, appended in order."""

    def __init__(self):
        self.rows = {k: [] for k in KEYS}

    def push(self, obs, act, next_obs, done):
        for k, a in zip(KEYS, (obs, act, next_obs, done)):
            self.rows[k].append(np.asarray(a, np.float64)[:, slice(0, a.shape[1])].T)

    def arrays(self):
        return {k: np.concatenate(v, 0) for k, v in self.rows.items()}


def episode(E, N, D, T, gen):
    """T steps of one episode as device-shaped tensors: obs_0..obs_T [E,N,D], act [E,N,2], done [E,N]."""
    obs = [torch.randn((E, N, D), generator=gen) for _ in range(T + 1)]
    act = [torch.rand((E, N, 2), generator=gen) * 2 - 1 for _ in range(T)]
    done = [torch.randint(0, 2, (E, N), generator=gen).to(torch.uint8) for _ in range(T)]
    return obs, act, done


def numpy_api(t):
    """[E, N, X] -> the reference's (X, E * N) layout: envs side by side on the agent axis."""
    t = t.double().numpy()
    return t.reshape(-1, t.shape[-1]).T if t.ndim == 3 else t.reshape(1, -1)


def fill(ring, obs, act, done, ref, new_chain=False):
    for t in range(len(act)):
        rew = torch.zeros(act[t].shape[:2])
        if t == 0 and new_chain:
            ring.new_chain(obs[0])
        ring.push(obs[t], act[t], rew, obs[t + 1], done[t])
        if ref is not None:
            ref.push(numpy_api(obs[t]), numpy_api(act[t]), numpy_api(obs[t + 1]), numpy_api(done[t]))


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_keys_dtypes_and_shapes(tmp_path):
    from marl_llm_amd.rollout import ChainedReplay, save_expert_data
    E, N, D, T = 2, 3, 5, 4
    ring = ChainedReplay(10, E * N, D, 2, "cpu")
    fill(ring, *episode(E, N, D, T, torch.Generator().manual_seed(0)), None)
    path = save_expert_data(ring, str(tmp_path / "out"))
    assert path == os.path.join(str(tmp_path / "out"), "expert_data.npz")
    z = load(path)
    assert sorted(z) == sorted(KEYS)
    L = T * E * N
    assert z["obs_buffs"].shape == (L, D) and z["next_obs_buffs"].shape == (L, D)
    assert z["ac_buffs"].shape == (L, 2) and z["done_buffs"].shape == (L, 1)
    assert all(a.dtype == np.float64 for a in z.values())
    z32 = load(save_expert_data(ring, str(tmp_path / "f32"), dtype=np.float32))
    assert all(a.dtype == np.float32 for a in z32.values())
    for k in KEYS:
        assert np.array_equal(z32[k], z[k].astype(np.float32))


def test_rows_equal_the_reference_push_sequence(tmp_path):
    from marl_llm_amd.rollout import ChainedReplay, save_expert_data
    E, N, D, T = 3, 4, 6, 7
    ring, ref = ChainedReplay(T, E * N, D, 2, "cpu"), ExpertPushes()
    fill(ring, *episode(E, N, D, T, torch.Generator().manual_seed(1)), ref)
    got, want = load(save_expert_data(ring, str(tmp_path))), ref.arrays()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k


def test_chronological_after_wrap_around(tmp_path):
    from marl_llm_amd.rollout import ChainedReplay, save_expert_data
    E, N, D, K, T = 2, 2, 3, 4, 11                  # 11 steps through a ring of 4: the last 4 steps, oldest first
    ring, ref = ChainedReplay(K, E * N, D, 2, "cpu"), ExpertPushes()
    obs, act, done = episode(E, N, D, T, torch.Generator().manual_seed(2))
    fill(ring, obs, act, done, None)
    for t in range(T - K, T):
        ref.push(numpy_api(obs[t]), numpy_api(act[t]), numpy_api(obs[t + 1]), numpy_api(done[t]))
    assert ring.cur != 0                            # the ring did wrap: slot order is not step order
    got, want = load(save_expert_data(ring, str(tmp_path))), ref.arrays()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k


def test_sealed_slots_are_excluded(tmp_path):
    from marl_llm_amd.rollout import ChainedReplay, save_expert_data
    E, N, D = 2, 3, 4
    ring, ref = ChainedReplay(12, E * N, D, 2, "cpu"), ExpertPushes()
    g = torch.Generator().manual_seed(3)
    first, second = episode(E, N, D, 3, g), episode(E, N, D, 5, g)
    fill(ring, *first, ref)
    fill(ring, *second, ref, new_chain=True)        # an episode boundary: the first episode's last next_obs slot is sealed
    assert ring._sealed
    got, want = load(save_expert_data(ring, str(tmp_path))), ref.arrays()
    assert got["obs_buffs"].shape[0] == 8 * E * N
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    # no row pairs the first episode's last observation with the second's first
    last = numpy_api(first[0][3]).T
    rows = np.flatnonzero((got["next_obs_buffs"][:, None, :] == last[None]).all(-1).any(-1))
    assert len(rows) == E * N and np.all(rows < 3 * E * N)


def test_bfloat16_ring_and_np_load_round_trip(tmp_path):
    from marl_llm_amd.rollout import ChainedReplay, save_expert_data
    E, N, D, T = 2, 2, 8, 3
    ring = ChainedReplay(T, E * N, D, 2, "cpu", obs_dtype=torch.bfloat16)
    obs, act, done = episode(E, N, D, T, torch.Generator().manual_seed(4))
    obs = [o.to(torch.bfloat16) for o in obs]
    fill(ring, obs, act, done, None)
    z = load(save_expert_data(ring, str(tmp_path)))
    want = np.concatenate([o.float().numpy().reshape(-1, D) for o in obs[:T]]).astype(np.float64)
    assert np.array_equal(z["obs_buffs"], want)
    # what ReplayBufferExpert.load + sample do with the file: np.load, then torch.Tensor rows (fp32)
    with np.load(os.path.join(str(tmp_path), "expert_data.npz")) as f:
        assert torch.equal(torch.Tensor(f["next_obs_buffs"]),
                           torch.cat([o.float().reshape(-1, D) for o in obs[1:]]))
        assert torch.equal(torch.Tensor(f["done_buffs"]), torch.cat([d.float().reshape(-1, 1) for d in done]))


def test_empty_ring_writes_empty_arrays(tmp_path):
    from marl_llm_amd.rollout import ChainedReplay, save_expert_data
    z = load(save_expert_data(ChainedReplay(3, 4, 5, 2, "cpu"), str(tmp_path)))
    assert z["obs_buffs"].shape == (0, 5) and z["done_buffs"].shape == (0, 1)
