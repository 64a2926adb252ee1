#!/usr/bin/env python3
"""Expert collection step: the eager loop (SwarmBatch.rule_action() + step() + ChainedReplay.push, three library calls and
a dozen host operations per step) against rollout_expert (one swarm_rollout_expert call per K steps).  Same transitions.

Per config (agents x envs) and observation dtype, the two paths alternate in one process, `--reps` times each; step_ms is
the host clock around K steps that ends in a device synchronise, per step, median [min, max] over the repetitions.
Output: a table and one JSON line per config (format of profiles/r04/rollout_loop_bench.txt)."""
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
from marl_llm_amd.rollout import ChainedReplay, rollout_expert
from marl_llm_amd.shapes import r_avoid_for, synthetic_shape_set

CONFIGS = ((30, 1), (30, 500), (64, 4096))      # agents x envs: one reference env, the reference's 500 episodes in one call, the headline


def measure(n_a, E, dtype, steps, reps, shapes):
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    sb = SwarmBatch(n_env=E, n_agents=n_a, n_cells_max=ng_max, r_avoid=r_avoid_for(n_a, shapes), obs_dtype=dtype)
    sb.set_shapes(shapes)
    n = E * n_a
    ring = ChainedReplay(8, n, sb.obs_dim, 2, sb.device, obs_dtype=dtype)
    state = {"obs": sb.reset(seed=226)}

    def eager(k):
        obs = state["obs"]
        for _ in range(k):
            u = sb.rule_action()
            nxt, rew, done, pri = sb.step(u)
            ring.push(obs, u, rew, nxt, done, pri)
            obs = nxt
        state["obs"] = obs

    def fused(k):
        state["obs"], _ = rollout_expert(sb, k, obs=state["obs"], replay=ring)

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    for fn in (eager, fused):                                   # warm-up: code objects, allocator, scratch, LDS attributes
        timed(fn, steps)
    res = {"eager": [], "fused": []}
    for _ in range(reps):                                       # alternate the paths
        res["eager"].append(timed(eager, steps))
        res["fused"].append(timed(fused, steps))
    sb.close()

    def summary(v):
        return dict(step_ms=round(statistics.median(v), 4), step_ms_min=round(min(v), 4), step_ms_max=round(max(v), 4))
    return dict(agents=n_a, envs=E, rows=n, obs_dtype=str(dtype).replace("torch.", ""), steps_per_call=steps, reps=reps,
                eager_loop=summary(res["eager"]), rollout_expert=summary(res["fused"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed call (one episode of collect_expert_data.py)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table and the JSON lines to this file")
    ap.add_argument("--only", default=None, help="one config AGENTSxENVS (e.g. 64x4096), both dtypes; e.g. under rocprofv3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("expert_bench: no HIP device (this is a GPU measurement)")
    shapes = synthetic_shape_set()
    lines = [f"{torch.cuda.get_device_name(0)}; {args.steps} steps per call, {args.reps} alternating repetitions; "
             "median [min, max] over repetitions",
             f"{'config':>16} {'dtype':>9} | {'eager loop ms/step':>26} | {'rollout_expert ms/step':>26} | {'speed-up':>8}"]
    js = []
    configs = CONFIGS if args.only is None else (tuple(int(v) for v in args.only.split("x")),)
    for n_a, E in configs:
        for dtype in (torch.bfloat16, torch.float32):
            r = measure(n_a, E, dtype, args.steps, args.reps, shapes)
            p, d = r["eager_loop"], r["rollout_expert"]
            lines.append(f"{n_a:>6} x {E:<7}  {r['obs_dtype']:>9} | "
                         f"{p['step_ms']:8.4f} [{p['step_ms_min']:.4f}, {p['step_ms_max']:.4f}] | "
                         f"{d['step_ms']:8.4f} [{d['step_ms_min']:.4f}, {d['step_ms_max']:.4f}] | {p['step_ms'] / d['step_ms']:7.2f}x")
            js.append(json.dumps(r))
            print(lines[-1], flush=True)
    text = "\n".join(lines + js) + "\n"
    print("\n".join(js))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
