"""The per-env episode ledger (marl_llm_amd/ledger.py describes its arrays) restated in numpy float64: what a step and a reset
do to them.  The yardstick of tests/test_ledger_host.py, and of any implementation that fills the arrays on the device: every
quantity is an integer or an fp64 sum in step order (numpy rounds every elementwise operation on its own: no fused
multiply-add), so such values can be compared bit for bit."""
import numpy as np


def step_std(c, n_agents):
    """k_reward_stats' population std (csrc/rollout.hip) of a {0, 1} row with c ones among n_agents, in its operation order."""
    nd = np.float64(n_agents)
    cd = np.asarray(c).astype(np.float64)
    m = cd / nd
    a = 1.0 - m
    return np.sqrt((cd * (a * a) + (nd - cd) * (m * m)) / nd)


class LedgerModel:
    def __init__(self, n_env, n_agents, cap):
        E, self.N, self.cap = int(n_env), int(n_agents), int(cap)
        self.ret = np.zeros(E, np.int64)
        self.std_sum = np.zeros(E, np.float64)
        self.len = np.zeros(E, np.int32)
        self.episode = np.full(E, -1, np.int64)
        self.n_log = np.zeros(E, np.int32)
        self.log_episode = np.zeros((E, cap), np.int64)
        self.log_ret = np.zeros((E, cap), np.int64)
        self.log_std_sum = np.zeros((E, cap), np.float64)
        self.log_len = np.zeros((E, cap), np.int32)

    def step(self, reward):
        """one step's rewards [E, N] (any layout with E * N elements, env-major)"""
        c = (np.asarray(reward).reshape(self.ret.shape[0], self.N) != 0).sum(axis=1).astype(np.int64)
        self.ret += c
        self.len += 1
        self.std_sum += step_std(c, self.N)

    def cut(self, episode):
        """a reset: an int (every env starts that episode) or a vector [E] (a negative entry keeps the env)"""
        E = self.ret.shape[0]
        ep = np.full(E, int(episode), np.int64) if np.ndim(episode) == 0 else np.asarray(episode, np.int64)
        for e in np.nonzero(ep >= 0)[0]:
            if self.len[e] > 0:
                s = int(self.n_log[e]) % self.cap
                self.log_episode[e, s], self.log_ret[e, s] = self.episode[e], self.ret[e]
                self.log_std_sum[e, s], self.log_len[e, s] = self.std_sum[e], self.len[e]
                self.n_log[e] += 1
            self.ret[e], self.std_sum[e], self.len[e], self.episode[e] = 0, 0.0, 0, ep[e]

    def arrays(self):
        return dict(ret=self.ret, std_sum=self.std_sum, len=self.len, episode=self.episode, n_log=self.n_log,
                    log_episode=self.log_episode, log_ret=self.log_ret, log_std_sum=self.log_std_sum, log_len=self.log_len)


def run(rewards, resets, n_env, n_agents, cap):
    """The ledger after T steps: rewards [T][E][N] (or [T][E * N]); resets {t: episode} -- the reset of step t comes before
    step t, as in the device loops' resets= (an int: every env; a vector [E]: -1 keeps)."""
    m = LedgerModel(n_env, n_agents, cap)
    for t, r in enumerate(rewards):
        if t in resets:
            m.cut(resets[t])
        m.step(r)
    return m


NAMES = ("ret", "std_sum", "len", "episode", "n_log", "log_episode", "log_ret", "log_std_sum", "log_len")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def mismatches(got, want):
    """names of the arrays (dicts by NAMES) that are not the same bits"""
    return [k for k in NAMES if not same_bits(np.asarray(got[k]), np.asarray(want[k]))]
