#!/usr/bin/env python3
"""How full are the observation rows' passes on the bench workload?  CPU only (the oracle); no GPU.

    python3 tools/row_tile_stats.py [--envs 24] [--steps 100] [--agents 64] [--seed 226]

The lattice step kernel of 64 agents writes the 80 sensed-cell slots of a wave's sixteen rows -- the env's agents ranked by
list length, sixteen per wave -- as two groups of eight rows x five passes of 16 slots (csrc/swarm_env.hip,
sensed_rows_live).  A pass none of whose eight rows reaches into it only stores zeros.  This prints, for the bench's two
states, the share of empty slots, the share of 8 x 16 tiles that are entirely empty (= dead passes), the mean number of live
passes per wave (of ten) and the longest list of every quartile of the ranking.

  assembled   bench.py's headline: synthetic_batch(seed), zero first action, then `--steps` prior-policy steps with the prior
              fed back as float32; the lists of the last step
  scatter     the reset distribution: the lists after one step (zero action)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G_MAX, SLOTS, GROUP = 80, 16, 8


def tiles(n):
    """n: [N] list lengths of one env -> (empty slots, slots, dead tiles, tiles, [N / 16] longest list per wave)."""
    s = np.sort(np.minimum(np.asarray(n), G_MAX), kind="stable")
    top = s.reshape(-1, GROUP).max(axis=1)
    live = (top + SLOTS - 1) // SLOTS
    per = G_MAX // SLOTS
    return G_MAX * len(s) - int(s.sum()), G_MAX * len(s), int((per - live).sum()), per * len(live), s.reshape(-1, 2 * GROUP).max(axis=1)


def report(name, counts):
    t = [tiles(n) for n in counts]
    es, sl, dt, tl = (sum(x[k] for x in t) for k in range(4))
    q = np.stack([x[4] for x in t])
    print("%-10s empty slots %4.1f %%   dead tiles %4.1f %%   live passes per wave %.2f of %d   quartile longest list: mean %s, max %s"
          % (name, 100.0 * es / sl, 100.0 * dt / tl, (tl - dt) / q.size, 2 * G_MAX // SLOTS,
             " / ".join("%.0f" % v for v in q.mean(axis=0)), " / ".join("%d" % v for v in q.max(axis=0))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=24)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--seed", type=int, default=226)
    a = ap.parse_args()
    from marl_llm_amd.shapes import r_avoid_for, synthetic_shape_set
    from marl_llm_amd.synth import synthetic_batch
    from oracle.oracle_py import Oracle
    oracle, shapes = Oracle(), synthetic_shape_set()
    ra = r_avoid_for(a.agents, shapes)
    sy = synthetic_batch(a.envs, a.agents, shapes, seed=a.seed)
    scatter, assembled = [], []
    for e in range(a.envs):
        g = np.ascontiguousarray(sy["cells"][e][:, : sy["n_g"][e]])
        l = float(sy["l_cell"][e])
        p, dp = np.ascontiguousarray(sy["p"][e]), np.ascontiguousarray(sy["dp"][e])
        nei = oracle.get_observation(p, dp, g, l, ra)["neighbor_index"]
        act = np.zeros((2, a.agents))
        for t in range(a.steps + 1):
            s = oracle.step(p, dp, act, g, nei, l, ra)
            p, dp, nei = s["p"], s["dp"], s["neighbor_index"]
            act = np.ascontiguousarray(s["a_prior"].astype(np.float32).astype(np.float64))
            if t == 0:
                scatter.append((s["sensed_index"] >= 0).sum(axis=1))
        assembled.append((s["sensed_index"] >= 0).sum(axis=1))
    print("%d envs x %d agents, seed %d, %d prior-policy steps" % (a.envs, a.agents, a.seed, a.steps))
    report("assembled", assembled)
    report("scatter", scatter)


if __name__ == "__main__":
    main()
