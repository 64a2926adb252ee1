#!/usr/bin/env python3
"""Host cost of the rollout loop: rollout()'s fused Python loop (FusedPolicy + ChainedReplay + SwarmBatch, two library
calls and a dozen host operations per step) against rollout_device (one swarm_rollout call per K steps).  Both run the
trainer's setting: in-kernel exploration noise on, track_reward on.

Per config (agents x envs) and observation dtype, the two paths alternate in one process, `--reps` times each:
  step_ms     host clock around K steps that ends in a device synchronise, per step
  enqueue_us  host clock until the call returns (the GPU may still be working), per step
plus the policy kernel alone on the config's rows (K calls, synchronised).  Output: a table and one JSON line per config.

--log-pi: the cost of recording log-probabilities instead -- rollout_device with log_pi=False / True (epsilon 0.3, so both
kernels that write log-pi run) and the policy kernel with and without its log-pi output, alternating in one process; the
overhead is the ratio of the medians."""
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
from marl_llm_amd.rollout import ChainedReplay, FusedPolicy, PolicyMLP, rollout, rollout_device
from marl_llm_amd.shapes import r_avoid_for, synthetic_shape_set

CONFIGS = ((30, 256), (32, 1024), (64, 4096))          # agents x envs: the reference's N = 30, BASELINE config 1, the headline


def measure(n_a, E, dtype, steps, reps, shapes, module):
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    sb = SwarmBatch(n_env=E, n_agents=n_a, n_cells_max=ng_max, r_avoid=r_avoid_for(n_a, shapes), obs_dtype=dtype)
    sb.set_shapes(shapes)
    pol = FusedPolicy(module, device=sb.device)
    n = E * n_a
    ring = ChainedReplay(8, n, sb.obs_dim, 2, sb.device, obs_dtype=dtype)
    state = {"obs": sb.reset(seed=226), "t": 0}

    def python_loop(k):
        state["obs"], r = rollout(sb, pol, k, state["obs"], replay=ring, noise_scale=0.1, seed=1, step0=state["t"])
        state["t"] += k

    def device_loop(k):
        state["obs"], r = rollout_device(sb, pol, k, obs=state["obs"], replay=ring, noise_scale=0.1, seed=1, step0=state["t"])
        state["t"] += k

    x = state["obs"].reshape(n, -1)
    out = torch.empty((n, 2), device=sb.device)

    def policy_only(k):
        for t in range(k):
            pol(x, out=out, noise_scale=0.1, seed=1, step=t)

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t2 - t0) / k * 1e3, (t1 - t0) / k * 1e6

    for fn in (python_loop, device_loop, policy_only):           # warm-up: code objects, allocator, LDS attributes
        timed(fn, steps)
    res = {"python": [], "device": [], "policy": []}
    for _ in range(reps):                                       # alternate the paths (measuring-on-mi355x section 5)
        res["python"].append(timed(python_loop, steps))
        res["device"].append(timed(device_loop, steps))
        res["policy"].append(timed(policy_only, steps))
    sb.close()
    pol.close()

    def summary(v):
        ms = [a for a, _ in v]
        us = [b for _, b in v]
        return dict(step_ms=round(statistics.median(ms), 4), step_ms_min=round(min(ms), 4), step_ms_max=round(max(ms), 4),
                    enqueue_us=round(statistics.median(us), 2), enqueue_us_min=round(min(us), 2), enqueue_us_max=round(max(us), 2))
    return dict(agents=n_a, envs=E, rows=n, obs_dtype=str(dtype).replace("torch.", ""), steps_per_call=steps, reps=reps,
                python_loop=summary(res["python"]), device_loop=summary(res["device"]),
                policy_kernel_ms=summary(res["policy"])["step_ms"])


def measure_log_pi(n_a, E, dtype, steps, reps, shapes, module):
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    sb = SwarmBatch(n_env=E, n_agents=n_a, n_cells_max=ng_max, r_avoid=r_avoid_for(n_a, shapes), obs_dtype=dtype)
    sb.set_shapes(shapes)
    pol = FusedPolicy(module, device=sb.device)
    n = E * n_a
    ring = ChainedReplay(8, n, sb.obs_dim, 2, sb.device, obs_dtype=dtype, log_pi=True)
    state = {"obs": sb.reset(seed=226), "t": 0}
    rng = np.random.RandomState(0)

    def device_loop(k, lp):
        state["obs"], _ = rollout_device(sb, pol, k, obs=state["obs"], replay=ring, noise_scale=0.1, epsilon=0.3, host_rng=rng,
                                         seed=1, step0=state["t"], log_pi=lp)
        state["t"] += k

    x = state["obs"].reshape(n, -1)
    out = torch.empty((n, 2), device=sb.device)
    lp_out = torch.empty(n, device=sb.device)

    def policy_only(k, lp):
        for t in range(k):
            pol(x, out=out, noise_scale=0.1, seed=1, step=t, log_pi=lp_out if lp else None)

    def timed(fn, k, lp):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k, lp)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    cases = [("device", device_loop, False), ("device_logpi", device_loop, True), ("policy", policy_only, False),
             ("policy_logpi", policy_only, True)]
    for _, fn, lp in cases:                                     # warm-up
        timed(fn, steps, lp)
    res = {name: [] for name, _, _ in cases}
    for _ in range(reps):                                       # alternate (measuring-on-mi355x section 5)
        for name, fn, lp in cases:
            res[name].append(timed(fn, steps, lp))
    sb.close()
    pol.close()
    med = {k: statistics.median(v) for k, v in res.items()}
    return dict(agents=n_a, envs=E, rows=n, obs_dtype=str(dtype).replace("torch.", ""), steps_per_call=steps, reps=reps,
                **{k + "_ms": round(v, 5) for k, v in med.items()},
                **{k + "_ms_min": round(min(res[k]), 5) for k in res},
                **{k + "_ms_max": round(max(res[k]), 5) for k in res},
                device_overhead_pct=round(100 * (med["device_logpi"] / med["device"] - 1), 2),
                policy_overhead_pct=round(100 * (med["policy_logpi"] / med["policy"] - 1), 2))


def main_log_pi(args, shapes, module):
    lines = [f"{torch.cuda.get_device_name(0)}; --log-pi; {args.steps} steps per timed call, {args.reps} alternating repetitions; "
             "median [min, max] ms per step / per policy call",
             f"{'config':>16} {'dtype':>9} | {'device loop':>26} {'+ log-pi':>26} {'ovh %':>7} | "
             f"{'policy kernel':>26} {'+ log-pi':>26} {'ovh %':>7}"]
    js = []
    for n_a, E in CONFIGS:
        for dtype in (torch.bfloat16, torch.float32):
            r = measure_log_pi(n_a, E, dtype, args.steps, args.reps, shapes, module)
            f = lambda k: f"{r[k + '_ms']:8.4f} [{r[k + '_ms_min']:.4f}, {r[k + '_ms_max']:.4f}]"
            lines.append(f"{n_a:>6} x {E:<7}  {r['obs_dtype']:>9} | {f('device'):>26} {f('device_logpi'):>26} "
                         f"{r['device_overhead_pct']:7.2f} | {f('policy'):>26} {f('policy_logpi'):>26} {r['policy_overhead_pct']:7.2f}")
            js.append(json.dumps(r))
            print(lines[-1], flush=True)
    return lines, js


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed call (one episode of train_assembly.py)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the table and the JSON lines to this file")
    ap.add_argument("--log-pi", action="store_true", help="measure the cost of log-pi recording instead (see above)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_loop_bench: no HIP device (this is a GPU measurement)")
    shapes = synthetic_shape_set()
    torch.manual_seed(0)
    module = PolicyMLP(192, 2, 180).cuda()
    if args.log_pi:
        lines, js = main_log_pi(args, shapes, module)
        text = "\n".join(lines + js) + "\n"
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text)
        return
    lines = [f"{torch.cuda.get_device_name(0)}; {args.steps} steps per call, {args.reps} alternating repetitions; "
             "median [min, max] over repetitions",
             f"{'config':>16} {'dtype':>9} | {'python loop ms/step':>26} {'enqueue us/step':>17} | "
             f"{'device loop ms/step':>26} {'enqueue us/step':>17} | {'policy ms':>9}"]
    js = []
    for n_a, E in CONFIGS:
        for dtype in (torch.bfloat16, torch.float32):
            r = measure(n_a, E, dtype, args.steps, args.reps, shapes, module)
            p, d = r["python_loop"], r["device_loop"]
            lines.append(f"{n_a:>6} x {E:<7}  {r['obs_dtype']:>9} | "
                         f"{p['step_ms']:8.4f} [{p['step_ms_min']:.4f}, {p['step_ms_max']:.4f}] {p['enqueue_us']:17.1f} | "
                         f"{d['step_ms']:8.4f} [{d['step_ms_min']:.4f}, {d['step_ms_max']:.4f}] {d['enqueue_us']:17.1f} | "
                         f"{r['policy_kernel_ms']:9.4f}")
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
