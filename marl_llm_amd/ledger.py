"""The host half of a per-env episode ledger: the layout of the episode log, its decoding and the grouping of episodes.

The reference prints and logs one figure per episode, episode_reward_mean_bar / episode_length
(train_assembly_airl.py:146-148, 203-215).  With staggered episodes (EpisodeClock, reset_envs), per-env exploration, an actor
bank or per-env shapes, the batch figure reward_stats[t] mixes what should be told apart: the per-episode figure belongs to an
ENV.  A ledger keeps, per env, the sums of the episode in progress and a log of the episodes a reset has ended:

    ret [E] int64       reward-1 agent-steps of the current episode (the env's rewards are in {0, 1}: an integer count)
    std_sum [E] f64     sum over the episode's steps of that step's population std over the env's N agents
    len [E] int32       steps taken in the current episode
    episode [E] int64   the episode number the last reset gave the env (-1: never reset)
    n_log [E] int32     episodes the env has FINISHED (may exceed cap)
    log_episode, log_ret, log_std_sum, log_len [E, cap]
                        entry k of env e lives in slot k % cap: the last cap episodes survive

A step adds (c, std(c), 1) for every env, c = its number of nonzero rewards; a reset of env e with len[e] > 0 writes
(episode, ret, std_sum, len) into slot n_log[e] % cap, counts it, and zeroes the running entries (an env with len == 0 logs
nothing: its first reset, two resets without a step between).  tests/ledger_model.py restates this in numpy float64.

This module is plain numpy -- no GPU, no library: decode_log turns the arrays into one record per episode, LogCursor hands
out each finished episode once, by_group averages them per bank member, epsilon class or shape.  The arrays are filled by
whoever keeps the ledger; nothing in the library fills them on the device yet (DESIGN.md "Episode ledger: the host half").
"""
import numpy as np

EPISODE_DTYPE = np.dtype([("env", np.int32), ("episode", np.int64), ("ret", np.int64), ("std_sum", np.float64),
                          ("len", np.int32), ("mean", np.float64)])
GROUP_DTYPE = np.dtype([("episodes", np.int64), ("mean", np.float64), ("len", np.float64)])


class LedgerOverflow(RuntimeError):
    """An env finished more episodes between two reads than the log holds: the oldest are overwritten."""


def decode_log(n_log, log_episode, log_ret, log_std_sum, log_len, cap, n_agents, seen=None):
    """The log as one record per episode (EPISODE_DTYPE), by env, oldest first.

    n_log [E]: episodes every env has finished; log_* [E, cap]: entry k of env e sits in slot k % cap, so the last
    min(n_log[e], cap) survive.  seen [E] (None: zeros): the n_log a previous call saw; only entries k >= seen[e] are
    returned, and LedgerOverflow raises -- naming the env, its new episodes and cap -- if more than cap of them were
    finished since, because the oldest are then gone.  Without seen the surviving entries are returned, however many were
    overwritten.  mean = ret / (n_agents * len): the episode's reward mean per agent-step -- the reference's
    episode_reward_mean_bar / episode_length for that env's episode, exact in double."""
    n_log = np.asarray(n_log, dtype=np.int64)
    E, cap = n_log.shape[0], int(cap)
    logs = [np.asarray(a).reshape(E, cap) for a in (log_episode, log_ret, log_std_sum, log_len)]
    if seen is None:
        first = np.maximum(n_log - cap, 0)
    else:
        first = np.asarray(seen, dtype=np.int64)
        if first.shape != (E,) or (first > n_log).any() or (first < 0).any():
            raise ValueError("decode_log: seen must be [E] with 0 <= seen[e] <= n_log[e]")
        over = np.nonzero(n_log - first > cap)[0]
        if over.size:
            e = int(over[0])
            raise LedgerOverflow("env %d finished %d episodes since the last drain, the log holds cap = %d: the oldest are "
                                 "overwritten (drain more often or raise cap)" % (e, int(n_log[e] - first[e]), cap))
    count = n_log - first
    env = np.repeat(np.arange(E, dtype=np.int64), count)
    k = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(np.cumsum(count) - count, count) + np.repeat(first, count)
    slot = k % cap
    out = np.zeros(env.shape[0], EPISODE_DTYPE)
    out["env"] = env
    for name, a in zip(("episode", "ret", "std_sum", "len"), logs):
        out[name] = a[env, slot]
    out["mean"] = out["ret"].astype(np.float64) / (np.float64(n_agents) * out["len"].astype(np.float64))
    return out


class LogCursor:
    """Hands out every finished episode once: the host keeps the n_log it has seen.

        cursor = LogCursor(E, cap, N)
        done = cursor.drain(n_log, log_episode, log_ret, log_std_sum, log_len)      # the episodes finished since the last drain

    drain raises LedgerOverflow if an env finished more than cap episodes in between, and then leaves the cursor where it was;
    finished() is decode_log without a cursor: every logged episode still in the log."""

    def __init__(self, n_env, cap, n_agents):
        self.cap, self.n_agents = int(cap), int(n_agents)
        if self.cap < 1:
            raise ValueError("LogCursor: cap must be >= 1")
        self.seen = np.zeros(int(n_env), np.int64)

    def drain(self, n_log, log_episode, log_ret, log_std_sum, log_len):
        out = decode_log(n_log, log_episode, log_ret, log_std_sum, log_len, self.cap, self.n_agents, seen=self.seen)
        self.seen = np.array(n_log, dtype=np.int64)
        return out

    def finished(self, n_log, log_episode, log_ret, log_std_sum, log_len):
        return decode_log(n_log, log_episode, log_ret, log_std_sum, log_len, self.cap, self.n_agents)


def by_group(episodes, group_of_env, G):
    """Per group g in [0, G): the number of episodes, the mean of their `mean` and their mean length (GROUP_DTYPE [G]) over
    `episodes` (decode_log's records).  group_of_env [E]: the group of env e -- FusedPolicyBank.member_of_env(E) for the
    members of a bank, SwarmBatch.get_shape_index() for the shapes of the set, any labelling for an exploration spectrum; an env
    with an entry outside [0, G) (an unserved env of a bank, cells set by hand) is left out.  A group without episodes has NaN
    means."""
    group_of_env = np.asarray(group_of_env, dtype=np.int64)
    G = int(G)
    g = group_of_env[episodes["env"]]
    keep = (g >= 0) & (g < G)
    g, ep = g[keep], episodes[keep]
    out = np.zeros(G, GROUP_DTYPE)
    out["episodes"] = np.bincount(g, minlength=G)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["mean"] = np.bincount(g, weights=ep["mean"], minlength=G) / out["episodes"]
        out["len"] = np.bincount(g, weights=ep["len"].astype(np.float64), minlength=G) / out["episodes"]
    return out
