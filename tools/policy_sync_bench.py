#!/usr/bin/env python3
"""What the weight update of the fused actor costs the training loop: FusedPolicy.refresh() (eight blocking copies to the
host, the host packer, a new handle, a synchronous upload) against FusedPolicy.sync() (swarm_policy_load_device: one packing
kernel enqueued on the stream).  One process, the two paths alternating (`--reps` times each), three measurements:

  call     host wall time of one refresh() / sync() issued right behind a pending rollout_device of `--steps` steps at
           32 x 1024 -- refresh() includes the wait for that rollout (its first copy waits for the stream): the host stall
  kernel   the packing kernel between two HIP events, enqueued behind a pending rollout so that the GPU never waits for the
           host: one sync() alone (with the events' own cost), and 50 back to back divided by 50
  episode  wall time per episode of a loop at 30 x 256, 32 x 1024 and 64 x 4096 (f32 rows): rollout_device for `--steps`
           steps, a stand-in learner (`--learner-steps` Adam steps of the PolicyMLP on `--batch` rows sampled from the ring,
           regressing on the stored actions), then the weight update.  `--episodes` episodes per timed repetition, one device
           synchronisation at its end; the policies of the two paths share the module, the ring and the env.

Output: a table (median [min, max] over the repetitions) and one JSON line per row, also written to --out
(profiles/r11/policy_sync_bench.txt is such a file)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from marl_llm_amd.batched import SwarmBatch
from marl_llm_amd.rollout import ChainedReplay, FusedPolicy, PolicyMLP, rollout_device
from marl_llm_amd.shapes import r_avoid_for, synthetic_shape_set

CONFIGS = ((30, 256), (32, 1024), (64, 4096))          # agents x envs, as tools/rollout_loop_bench.py
PATHS = ("refresh", "sync")


def mmm(v, nd=4):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def fmt(d, w=9, nd=3):
    return f"{d['median']:{w}.{nd}f} [{d['min']:.{nd}f}, {d['max']:.{nd}f}]"


class Loop:
    """Env, ring, module, optimizer and one FusedPolicy per path, at one configuration."""

    def __init__(self, n_a, E, shapes, args):
        ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
        self.sb = SwarmBatch(n_env=E, n_agents=n_a, n_cells_max=ng_max, r_avoid=r_avoid_for(n_a, shapes))
        self.sb.set_shapes(shapes)
        torch.manual_seed(0)
        self.module = PolicyMLP(self.sb.obs_dim, 2, 180).to(self.sb.device)
        self.opt = torch.optim.Adam(self.module.parameters(), lr=1e-4)
        self.pol = {p: FusedPolicy(self.module, device=self.sb.device) for p in PATHS}
        self.ring = ChainedReplay(8, E * n_a, self.sb.obs_dim, 2, self.sb.device)
        self.gen = torch.Generator(device=self.sb.device).manual_seed(1)
        self.obs, self.t, self.args = self.sb.reset(seed=226), 0, args

    def rollout(self, path):
        k = self.args.steps
        self.obs, _ = rollout_device(self.sb, self.pol[path], k, obs=self.obs, replay=self.ring, noise_scale=0.1, seed=1, step0=self.t)
        self.t += k

    def learn(self):
        for _ in range(self.args.learner_steps):
            obs, act = self.ring.sample(self.args.batch, generator=self.gen)[:2]
            loss = ((self.module(obs) - act) ** 2).mean()
            self.opt.zero_grad(set_to_none=True)
            loss.backward()
            self.opt.step()

    def update(self, path):
        getattr(self.pol[path], path)()

    def episodes(self, path, n):
        """Wall ms per episode of n episodes, the device synchronised before and after."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.rollout(path)
            self.learn()
            self.update(path)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def close(self):
        for p in self.pol.values():
            p.close()
        self.sb.close()


def measure_calls(shapes, args):
    """Host ms of one refresh() / sync() behind a pending rollout, and the packing kernel's event time (us)."""
    lp = Loop(32, 1024, shapes, args)
    for p in PATHS:                                             # warm-up: code objects, allocator
        lp.episodes(p, 1)
    host = {p: [] for p in PATHS}
    for _ in range(args.reps):
        for p in PATHS:
            torch.cuda.synchronize()
            lp.rollout(p)
            lp.learn()
            t0 = time.perf_counter()
            lp.update(p)
            host[p].append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    pol = lp.pol["sync"]
    one, many = [], []
    for _ in range(args.reps):
        for n, dst in ((1, one), (50, many)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            lp.rollout("sync")                                  # ~10 ms of pending work: the launches below queue up behind it,
            a.record()                                          # so the events see the GPU's time, not the host's enqueue rate
            for _ in range(n):
                pol.sync()
            b.record()
            b.synchronize()
            dst.append(a.elapsed_time(b) / n * 1e3)
    lp.close()
    return dict(measurement="call", agents=32, envs=1024, steps_pending=args.steps, reps=args.reps,
                refresh_host_ms=mmm(host["refresh"]), sync_host_ms=mmm(host["sync"]),
                pack_kernel_us_single=mmm(one, 2), pack_kernel_us_back_to_back_50=mmm(many, 2))


def measure_episodes(n_a, E, shapes, args):
    lp = Loop(n_a, E, shapes, args)
    for p in PATHS:
        lp.episodes(p, 1)
    ms = {p: [] for p in PATHS}
    for _ in range(args.reps):                                  # alternate the paths (measuring-on-mi355x section 5)
        for p in PATHS:
            ms[p].append(lp.episodes(p, args.episodes))
    lp.close()
    r = dict(measurement="episode", agents=n_a, envs=E, rows=n_a * E, steps=args.steps, learner_steps=args.learner_steps,
             batch=args.batch, episodes_per_rep=args.episodes, reps=args.reps,
             refresh_episode_ms=mmm(ms["refresh"]), sync_episode_ms=mmm(ms["sync"]))
    r["sync_over_refresh"] = round(r["sync_episode_ms"]["median"] / r["refresh_episode_ms"]["median"], 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="env steps per episode (train_assembly.py's episode length)")
    ap.add_argument("--reps", type=int, default=7, help="alternating repetitions of each path (at least 5)")
    ap.add_argument("--episodes", type=int, default=4, help="episodes per timed repetition")
    ap.add_argument("--learner-steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "policy_sync_bench.txt"))
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("policy_sync_bench: --reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("policy_sync_bench: no HIP device (this is a GPU measurement)")
    shapes = synthetic_shape_set()
    lines = [f"{torch.cuda.get_device_name(0)}; {args.steps} steps per episode, {args.learner_steps} Adam steps on {args.batch} rows, "
             f"{args.episodes} episodes per timed repetition, {args.reps} alternating repetitions; median [min, max]"]
    js = []
    c = measure_calls(shapes, args)
    js.append(json.dumps(c))
    lines += [f"one call behind a pending {args.steps}-step rollout at 32 x 1024, host ms:  refresh() {fmt(c['refresh_host_ms'])}   "
              f"sync() {fmt(c['sync_host_ms'], 9, 4)}",
              f"packing kernel between two HIP events, us:  one sync() {fmt(c['pack_kernel_us_single'], 7, 2)}   "
              f"50 back to back / 50 {fmt(c['pack_kernel_us_back_to_back_50'], 7, 2)}",
              f"{'config':>14} | {'episode ms, refresh()':>32} | {'episode ms, sync()':>32} | sync / refresh"]
    print("\n".join(lines), flush=True)
    for n_a, E in CONFIGS:
        r = measure_episodes(n_a, E, shapes, args)
        js.append(json.dumps(r))
        lines.append(f"{n_a:>5} x {E:<6} | {fmt(r['refresh_episode_ms'], 12):>32} | {fmt(r['sync_episode_ms'], 12):>32} | {r['sync_over_refresh']:.3f}")
        print(lines[-1], flush=True)
    print("\n".join(js))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + js) + "\n")


if __name__ == "__main__":
    main()
