#!/usr/bin/env python3
"""What the per-env reset costs (DESIGN.md "Per-env reset"), at 64 agents x 4096 envs with float32 observation rows.

(a) One call each, HIP events around it, alternating in one process: reset_envs with 1/8 of the envs reset, reset_envs with
    all envs reset, reset (swarm_reset), and one observe() -- the observation pass that every one of them ends with.
(b) rollout_device in stretches of --steps steps (one episode): EpisodeClock(groups=1) and EpisodeClock(groups=8) on this
    tree, and the in-phase loop `reset=(seed, episode)` on the tree given by --parent (a checkout of the parent commit with
    its library built; without it, on this tree).  Each variant runs in a process of its own, --rounds times, the variants
    alternating; inside a process --reps stretches are timed with HIP events after one warm-up stretch.

Median [min, max] over the repetitions; a table and one JSON line per part, also written to --out.  Reads nothing outside the
trees it is given."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_A, N_ENV, SEED = 64, 4096, 226


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


def fmt(s):
    return f"{s['median']:9.4f} [{s['min']:.4f}, {s['max']:.4f}]"


def make(root):
    """(torch, SwarmBatch 64 x 4096 f32 with the synthetic shape set, the rollout module) of the tree at root"""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from marl_llm_amd import rollout
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.shapes import r_avoid_for, synthetic_shape_set
    if not torch.cuda.is_available():
        raise SystemExit("reset_envs_bench: no HIP device (this is a GPU measurement)")
    shapes = synthetic_shape_set()
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    sb = SwarmBatch(n_env=N_ENV, n_agents=N_A, n_cells_max=ng_max, r_avoid=r_avoid_for(N_A, shapes), obs_dtype=torch.float32)
    sb.set_shapes(shapes)
    return torch, sb, rollout


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def part_a(reps):
    torch, sb, _ = make(ROOT)
    sb.reset(SEED, 0)
    e = torch.arange(N_ENV, device=sb.device)
    keep = torch.full((N_ENV,), -1, dtype=torch.int64, device=sb.device)
    vec = {"eighth": [torch.where(e % 8 == k % 8, torch.full_like(keep, k + 1), keep) for k in range(reps + 1)],
           "all": [torch.full_like(keep, k + 1) for k in range(reps + 1)]}
    torch.cuda.synchronize()
    cases = {"reset_envs_eighth": lambda k: sb.reset_envs(SEED, vec["eighth"][k]), "reset_envs_all": lambda k: sb.reset_envs(SEED, vec["all"][k]),
             "reset": lambda k: sb.reset(SEED, k + 1), "observe": lambda k: sb.observe()}
    for fn in cases.values():
        fn(reps)                                            # warm-up
    res = {name: [] for name in cases}
    for k in range(reps):                                   # alternate
        for name, fn in cases.items():
            res[name].append(event_ms(torch, lambda: fn(k)))
    name = torch.cuda.get_device_name(0)
    sb.close()
    return name, {k: summary(v) for k, v in res.items()}


def child(variant, root, steps, reps):
    torch, sb, R = make(root)
    torch.manual_seed(0)
    pol = R.FusedPolicy(R.PolicyMLP(sb.obs_dim, 2, 180).cuda(), device=sb.device)
    ring = R.ChainedReplay(16, N_ENV * N_A, sb.obs_dim, 2, sb.device)
    kw = dict(replay=ring, noise_scale=0.1, seed=1)
    clock = R.EpisodeClock(N_ENV, steps, groups=int(variant[5:]), seed=SEED) if variant.startswith("clock") else None
    state = {"k": 0}

    def stretch():
        k = state["k"]
        if clock is not None:
            R.rollout_device(sb, pol, steps, resets=clock.resets(steps), step0=k * steps, **kw)
        else:
            R.rollout_device(sb, pol, steps, reset=(SEED, k), step0=k * steps, **kw)
        state["k"] += 1

    stretch()                                               # warm-up: code objects, allocator, LDS attributes
    ms = [event_ms(torch, stretch) / steps for _ in range(reps)]
    print(json.dumps(dict(variant=variant, ms_per_step=ms)))
    sb.close(); pol.close()


def part_b(args):
    variants = [("clock1", ROOT), ("clock8", ROOT), ("inphase", args.parent or ROOT)]
    res = {v: [] for v, _ in variants}
    for _ in range(args.rounds):                            # alternate the variants, one process each
        for v, root in variants:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v, "--root", root, "--steps", str(args.steps),
                                  "--reps", str(args.reps)], stdout=subprocess.PIPE, universal_newlines=True, check=True, timeout=300).stdout
            res[v] += json.loads(out.strip().splitlines()[-1])["ms_per_step"]
    return {v: summary(x) for v, x in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per stretch = episode length (train_assembly.py)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: runs the in-phase loop of (b)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.root, args.steps, args.reps)
    b = part_b(args)                                        # first: this process has not opened the GPU yet
    name, a = part_a(max(args.reps, 7))
    where = "the parent commit" if args.parent else "this tree"
    lines = [f"{name}; {N_A} agents x {N_ENV} envs, float32 rows; median [min, max]",
             f"(a) one call, HIP events, {a['reset']['n']} alternating repetitions, ms"]
    lines += [f"    {k:<20} {fmt(v)}" for k, v in a.items()]
    lines += [f"(b) rollout_device, stretches of {args.steps} steps, {args.rounds} alternating processes x {args.reps} stretches, ms per step"]
    names = {"clock1": "EpisodeClock(groups=1)", "clock8": "EpisodeClock(groups=8)", "inphase": f"reset= loop on {where}"}
    lines += [f"    {names[k]:<32} {fmt(v)}   x{v['median'] / b['inphase']['median']:.4f}" for k, v in b.items()]
    lines += [json.dumps(dict(part="a", **a)), json.dumps(dict(part="b", steps=args.steps, parent=bool(args.parent), **b))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
