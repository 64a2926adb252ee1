"""The episode ledger's host half without a GPU: the numpy model of the ledger's contract (tests/ledger_model.py) gives
hand-computed values; the decoding of the episode log (marl_llm_amd/ledger.py), the cursor that hands out every finished
episode once and the grouping are plain numpy, fed here with the model's arrays."""
import numpy as np
import pytest

import ledger_model as model

S3_4 = 0.4330127018922193          # sqrt(3) / 4: the population std of one 1 among four


# ---- the model against values computed by hand (N = 4: a step with one 1 has std sqrt(3)/4, with two 1s 0.5, with none or four 0)

def _rows(*counts):
    """one step's rewards [E, 4] with counts[e] ones in env e"""
    return np.array([[1.0] * c + [0.0] * (4 - c) for c in counts], np.float32)


def test_model_std_term():
    assert model.step_std(np.array([0, 1, 2, 3, 4]), 4).tolist() == [0.0, S3_4, 0.5, S3_4, 0.0]
    assert S3_4 == np.sqrt(0.1875)
    # 2 of 5: m = 0.4, (2 * 0.36 + 3 * 0.16) / 5 in that order
    assert model.step_std(np.array([2]), 5)[0] == np.sqrt((2.0 * (0.6 * 0.6) + 3.0 * (0.4 * 0.4)) / 5.0)


def test_model_env_reset_twice_without_a_step():
    m = model.LedgerModel(1, 4, 3)
    m.cut(0); m.cut(1)                                        # the first reset, then one more with no step between
    assert (m.n_log[0], m.episode[0], m.len[0]) == (0, 1, 0)
    m.step(_rows(2)); m.step(_rows(1))
    assert (m.ret[0], m.len[0], m.std_sum[0]) == (3, 2, 0.5 + S3_4)
    m.cut(2)
    assert m.n_log[0] == 1 and (m.log_episode[0, 0], m.log_ret[0, 0], m.log_std_sum[0, 0], m.log_len[0, 0]) == (1, 3, 0.5 + S3_4, 2)
    assert (m.ret[0], m.std_sum[0], m.len[0], m.episode[0]) == (0, 0.0, 0, 2)
    m.cut(3)
    assert m.n_log[0] == 1 and m.episode[0] == 3 and not m.log_len[0, 1:].any()


def test_model_cap_wrap():
    m = model.run([_rows(4), _rows(1), _rows(1), _rows(2), _rows(0)], {0: 7, 1: 8, 3: 9, 4: 10}, 1, 4, cap=2)
    # episodes 7 (one step, 4), 8 (two steps, 1 + 1), 9 (one step, 2) are finished; 10 runs.  Entry k sits in slot k % 2.
    assert m.n_log[0] == 3
    assert m.log_episode[0].tolist() == [9, 8] and m.log_ret[0].tolist() == [2, 2] and m.log_len[0].tolist() == [1, 2]
    assert m.log_std_sum[0].tolist() == [0.5, S3_4 + S3_4]
    assert (m.episode[0], m.ret[0], m.len[0], m.std_sum[0]) == (10, 0, 1, 0.0)


def test_model_kept_env_across_another_envs_cut():
    m = model.run([_rows(1, 2), _rows(3, 4), _rows(2, 2)], {0: 0, 1: np.array([-1, 5])}, 2, 4, cap=2)
    assert m.n_log.tolist() == [0, 1] and m.episode.tolist() == [0, 5]
    assert (m.ret[0], m.len[0], m.std_sum[0]) == (6, 3, S3_4 + S3_4 + 0.5)             # env 0 never cut: three steps in one episode
    assert (m.ret[1], m.len[1], m.std_sum[1]) == (6, 2, 0.0 + 0.5)
    assert (m.log_episode[1, 0], m.log_ret[1, 0], m.log_std_sum[1, 0], m.log_len[1, 0]) == (0, 2, 0.5, 1)
    assert not m.log_len[0].any()


# ---- decoding, drain, grouping

def _synthetic():
    """3 envs, cap 2: env 0 finished 3 episodes (entry 0 overwritten), env 1 none, env 2 one"""
    n_log = np.array([3, 0, 1], np.int32)
    log_episode = np.array([[12, 11], [0, 0], [4, 0]], np.int64)        # env 0: entry 2 in slot 0, entry 1 in slot 1
    log_ret = np.array([[30, 8], [0, 0], [5, 0]], np.int64)
    log_std_sum = np.array([[1.5, 0.25], [0, 0], [0.75, 0]], np.float64)
    log_len = np.array([[3, 2], [0, 0], [5, 0]], np.int32)
    return n_log, log_episode, log_ret, log_std_sum, log_len


def test_decode_log_orders_by_env_then_oldest_first():
    from marl_llm_amd.ledger import EPISODE_DTYPE, decode_log
    ep = decode_log(*_synthetic(), cap=2, n_agents=4)
    assert ep.dtype == EPISODE_DTYPE and ep.dtype.names == ("env", "episode", "ret", "std_sum", "len", "mean")
    assert ep["env"].tolist() == [0, 0, 2] and ep["episode"].tolist() == [11, 12, 4]
    assert ep["ret"].tolist() == [8, 30, 5] and ep["len"].tolist() == [2, 3, 5] and ep["std_sum"].tolist() == [0.25, 1.5, 0.75]
    assert ep["mean"].tolist() == [8 / (4 * 2), 30 / (4 * 3), 5 / (4 * 5)]
    empty = decode_log(np.zeros(3, np.int32), *_synthetic()[1:], cap=2, n_agents=4)
    assert empty.shape == (0,) and empty.dtype == EPISODE_DTYPE


def test_decode_log_since_seen_and_overflow():
    from marl_llm_amd.ledger import LedgerOverflow, decode_log
    ep = decode_log(*_synthetic(), cap=2, n_agents=4, seen=np.array([2, 0, 0]))
    assert ep["env"].tolist() == [0, 2] and ep["episode"].tolist() == [12, 4]
    assert decode_log(*_synthetic(), cap=2, n_agents=4, seen=np.array([3, 0, 1])).shape == (0,)
    with pytest.raises(LedgerOverflow, match=r"env 0 finished 3 episodes .* cap = 2"):
        decode_log(*_synthetic(), cap=2, n_agents=4, seen=np.zeros(3))
    with pytest.raises(ValueError):
        decode_log(*_synthetic(), cap=2, n_agents=4, seen=np.array([4, 0, 0]))


def test_drain_returns_each_episode_once_and_names_an_overflow():
    from marl_llm_amd.ledger import LedgerOverflow, LogCursor
    m = model.LedgerModel(2, 4, cap=2)
    cur = LogCursor(2, cap=2, n_agents=4)
    read = lambda: [np.array(a) for a in (m.n_log, m.log_episode, m.log_ret, m.log_std_sum, m.log_len)]
    m.cut(0); m.step(_rows(1, 2)); m.cut(np.array([1, -1])); m.step(_rows(3, 3))
    first = cur.drain(*read())
    assert first["env"].tolist() == [0] and first["episode"].tolist() == [0] and first["mean"].tolist() == [0.25]
    assert cur.drain(*read()).shape == (0,)                             # nothing new
    m.cut(np.array([2, 1])); m.step(_rows(4, 4)); m.cut(np.array([3, -1]))
    second = cur.drain(*read())
    assert second["env"].tolist() == [0, 0, 1] and second["episode"].tolist() == [1, 2, 0] and second["len"].tolist() == [1, 1, 2]
    assert second["mean"].tolist() == [0.75, 1.0, 5 / 8]
    assert cur.finished(*read())["episode"].tolist() == [1, 2, 0]       # env 0's entry 0 is overwritten (cap 2)
    for ep in (4, 5, 6):                                         # env 0 finishes three more: one more than the log holds
        m.step(_rows(1, 1)); m.cut(np.array([ep, -1]))
    with pytest.raises(LedgerOverflow, match=r"env 0 finished 3 episodes since the last drain, the log holds cap = 2"):
        cur.drain(*read())
    with pytest.raises(LedgerOverflow):                          # the failed drain did not move the cursor
        cur.drain(*read())
    assert cur.finished(*read())["episode"].tolist() == [4, 5, 0]


def test_by_group_five_envs_three_groups_one_unserved():
    from marl_llm_amd.ledger import EPISODE_DTYPE, GROUP_DTYPE, by_group
    ep = np.zeros(6, EPISODE_DTYPE)
    ep["env"] = [0, 0, 1, 2, 3, 4]
    ep["len"] = [2, 4, 6, 8, 10, 12]
    ep["mean"] = [0.5, 0.25, 1.0, 0.125, 0.75, 0.0]
    group_of_env = np.array([1, 1, -1, 0, 0])                    # env 2 is unserved; nobody is in group 2
    g = by_group(ep, group_of_env, 3)
    assert g.dtype == GROUP_DTYPE and g["episodes"].tolist() == [2, 3, 0]
    assert g["mean"][:2].tolist() == [(0.75 + 0.0) / 2, (0.5 + 0.25 + 1.0) / 3] and np.isnan(g["mean"][2])
    assert g["len"][:2].tolist() == [11.0, 4.0] and np.isnan(g["len"][2])
    assert by_group(ep[:0], group_of_env, 3)["episodes"].tolist() == [0, 0, 0]


def test_drained_episodes_are_the_uncapped_log_of_a_random_schedule():
    """Random rewards, random per-env and whole-batch resets, a drain after every reset: what the cursor hands out over a small
    log is, env by env and in order, the log of a ledger large enough never to wrap."""
    from marl_llm_amd.ledger import LogCursor, decode_log
    rng = np.random.default_rng(7)
    E, N, cap = 6, 5, 2
    small, big = model.LedgerModel(E, N, cap), model.LedgerModel(E, N, 64)
    cur, drained, episode = LogCursor(E, cap, N), [], 0
    for t in range(60):
        if t == 0 or rng.random() < 0.35:
            vec = episode if t == 0 or rng.random() < 0.2 else np.where(rng.random(E) < 0.4, episode, -1)
            episode += 1
            small.cut(vec); big.cut(vec)
            a = small.arrays()
            drained.append(cur.drain(a["n_log"], a["log_episode"], a["log_ret"], a["log_std_sum"], a["log_len"]))
        r = (rng.random((E, N)) < 0.3).astype(np.float32)
        small.step(r); big.step(r)
    b = big.arrays()
    want = decode_log(b["n_log"], b["log_episode"], b["log_ret"], b["log_std_sum"], b["log_len"], 64, N)
    got = np.concatenate(drained)
    got = got[np.argsort(got["env"], kind="stable")]
    assert len(want) > 3 * E and (b["n_log"] > cap).all() and got.tobytes() == want.tobytes()
    for k in ("ret", "std_sum", "len", "episode", "n_log"):            # the running entries do not depend on cap
        assert model.same_bits(small.arrays()[k], b[k]), k
