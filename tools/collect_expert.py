#!/usr/bin/env python3
"""Expert data collection on the device: the counterpart of the reference's marl_llm/eval/collect_expert_data.py (rule-based
expert, `n_episodes` episodes of `episode_length` steps, ReplayBufferExpert.save) that writes the same expert_data.npz.

Per call, E = --envs-per-call episodes run side by side: a device reset (swarm_reset keyed by (seed, 0, call * E + e), so
episode call * E + e draws its own shape and start state), then ONE rollout_expert call of episode_length steps into a
chained replay ring that holds every transition of the run; the reset seals the previous episode's last slot.  After
each call the coverage rate and distribution uniformity of the final states (metrics()) are printed, as the reference
prints them per episode.  The ring is then streamed into DIR/expert_data.npz (save_expert_data).

  python tools/collect_expert.py --n_a 30 --n_episodes 500 --episode_length 200 --envs-per-call 500 --out DIR"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from marl_llm_amd.batched import SwarmBatch
from marl_llm_amd.rollout import ChainedReplay, rollout_expert, save_expert_data
from marl_llm_amd.shapes import load_results, r_avoid_for, synthetic_shape_set


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n_a", type=int, default=30, help="agents per episode, 1 to 1024")
    ap.add_argument("--n_episodes", type=int, default=500)
    ap.add_argument("--episode_length", type=int, default=200)
    ap.add_argument("--envs-per-call", type=int, default=500, help="episodes per rollout_expert call (must divide n_episodes)")
    ap.add_argument("--seed", type=int, default=226)
    ap.add_argument("--shapes", default=None, help="a results.pkl (the reference's layout); default: the synthetic shape set")
    ap.add_argument("--obs-dtype", choices=("float32", "bfloat16"), default="float32")
    ap.add_argument("--npz-dtype", choices=("float64", "float32"), default="float64",
                    help="dtype of the file's arrays (float64: the reference's; float32 halves the file, same values)")
    ap.add_argument("--out", required=True, help="directory of expert_data.npz")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("collect_expert: no HIP device")
    E, L = args.envs_per_call, args.episode_length
    if E < 1 or args.n_episodes % E:
        raise SystemExit("--envs-per-call must divide --n_episodes")
    calls = args.n_episodes // E
    t0 = time.perf_counter()
    shapes = load_results(args.shapes) if args.shapes else synthetic_shape_set()
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    dtype = torch.float32 if args.obs_dtype == "float32" else torch.bfloat16
    # (above the step kernel's 256 agents the large-swarm kernels step the envs and k_rule_large is the expert; up to 1024)
    sb = SwarmBatch(n_env=E, n_agents=args.n_a, n_cells_max=ng_max, r_avoid=r_avoid_for(args.n_a, shapes), obs_dtype=dtype,
                    large_swarm=args.n_a > 256)
    sb.set_shapes(shapes)
    ring = ChainedReplay(calls * (L + 1) - 1, E * args.n_a, sb.obs_dim, 2, sb.device, obs_dtype=dtype)   # every transition
    print(f"expert collection: {args.n_episodes} episodes x {L} steps x {args.n_a} agents, {E} envs per call, "
          f"ring {ring.S} slots x {ring.n} rows ({ring.obs.numel() * ring.obs.element_size() / 2**30:.2f} GiB obs)", flush=True)
    for call in range(calls):
        tc = time.perf_counter()
        _, stats = rollout_expert(sb, L, replay=ring, reset=(args.seed, 0, call * E), source="rule")
        m = sb.metrics().cpu().numpy()
        r = stats[:, 0].mean().item()
        print(f"call {call + 1}/{calls} | episodes {call * E}-{call * E + E - 1} | avg reward {r:.4f} | coverage "
              f"{m[:, 0].mean():.4f} [{m[:, 0].min():.4f}, {m[:, 0].max():.4f}] | uniformity {m[:, 1].mean():.4f} | "
              f"{time.perf_counter() - tc:.2f} s", flush=True)
    tw = time.perf_counter()
    path = save_expert_data(ring, args.out, dtype=np.dtype(args.npz_dtype))
    n_rows = len(ring) if ring._sealed else ring.count * ring.n
    print(f"wrote {path}: {n_rows} transitions, {os.path.getsize(path) / 2**30:.2f} GiB, write {time.perf_counter() - tw:.1f} s")
    print(f"end to end {time.perf_counter() - t0:.1f} s")
    sb.close()


if __name__ == "__main__":
    main()
