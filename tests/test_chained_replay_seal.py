"""ChainedReplay.new_chain (host logic, CPU tensors): an episode boundary seals the slot that holds the previous chain's last
next_obs instead of overwriting it, sample() and len() skip sealed slots, and a ring that was never sealed samples exactly
as before."""
import pytest

torch = pytest.importorskip("torch")


def episode(ep, steps, n, d):
    """Observations ep*1000 + t (t = 0 .. steps) so that every (obs, next_obs) pair tells where it comes from."""
    obs = [torch.full((1, n, d), float(ep * 1000 + t)) for t in range(steps + 1)]
    act = [torch.full((1, n, 2), float(ep * 1000 + t)) for t in range(steps)]
    return obs, act


def fill(ring, eps, n, d, seal):
    for ep, steps in eps:
        obs, act = episode(ep, steps, n, d)
        if seal:
            ring.new_chain(obs[0])
        else:
            ring.break_chain()
        for t in range(steps):
            ring.push(obs[t], act[t], torch.zeros(1, n), obs[t + 1], torch.zeros(1, n), torch.zeros(1, n, 2))


@pytest.mark.parametrize("K", [4, 6, 20])
def test_sampled_transitions_never_cross_an_episode_boundary(K):
    from marl_llm_amd.rollout import ChainedReplay
    n, d = 3, 2
    ring = ChainedReplay(K, n, d, 2, "cpu")
    fill(ring, [(1, 3), (2, 2), (3, 4), (4, 1)], n, d, seal=True)
    g = torch.Generator().manual_seed(0)
    o, a, r, no, dn, pr = ring.sample(4000, generator=g)
    assert torch.equal(no[:, 0] - o[:, 0], torch.ones(4000))            # next_obs is always the same episode's t + 1
    assert torch.equal(a[:, 0], o[:, 0])                                 # and the action is the one taken on obs
    eps = set((o[:, 0] // 1000).tolist())
    assert 4.0 in eps and (len(eps) > 1 or K < 6)
    assert len(ring) // n == len(set(o[:, 0].tolist()))                  # every stored transition drawn, nothing else


def test_new_chain_keeps_the_last_next_obs():
    from marl_llm_amd.rollout import ChainedReplay
    n, d = 2, 2
    ring = ChainedReplay(8, n, d, 2, "cpu")
    fill(ring, [(1, 3)], n, d, seal=True)
    assert ring.cur == 3 and ring.count == 3
    slot = ring.new_chain(torch.full((1, n, d), 2000.0))
    assert slot == 4 and ring.cur == 4 and ring.count == 4 and len(ring) == 3 * n
    assert torch.equal(ring.obs[3], torch.full((n, d), 1003.0))          # episode 1's last next_obs survives
    assert torch.equal(ring.obs[4], torch.full((n, d), 2000.0))
    assert ring.new_chain(torch.full((1, n, d), 3000.0)) == 4            # nothing stored since: no second seal
    # break_chain() (unchanged) has the hazard new_chain() avoids: it overwrites the stored next_obs
    old = ChainedReplay(8, n, d, 2, "cpu")
    fill(old, [(1, 3), (2, 1)], n, d, seal=False)
    assert torch.equal(old.obs[3], torch.full((n, d), 2000.0))


def test_unsealed_ring_samples_as_before():
    from marl_llm_amd.rollout import ChainedReplay
    n, d, K = 4, 3, 5
    a, b = ChainedReplay(K, n, d, 2, "cpu"), ChainedReplay(K, n, d, 2, "cpu")
    fill(a, [(1, 7)], n, d, seal=False)
    fill(b, [(1, 7)], n, d, seal=True)                                  # new_chain on an empty ring seals nothing
    assert not b._sealed and a.cur == b.cur and len(a) == len(b) == K * n
    sa = a.sample(64, generator=torch.Generator().manual_seed(3))
    sb = b.sample(64, generator=torch.Generator().manual_seed(3))
    assert all(torch.equal(x, y) for x, y in zip(sa, sb))
    # the same draws as the sampling rule of the parent implementation
    g = torch.Generator().manual_seed(3)
    back = torch.randint(0, a.count, (64,), generator=g)
    j = (a.cur - 1 - back) % a.S
    r = torch.randint(0, a.n, (64,), generator=g)
    assert torch.equal(sa[0], a.obs[j, r]) and torch.equal(sa[3], a.obs[(j + 1) % a.S, r])
