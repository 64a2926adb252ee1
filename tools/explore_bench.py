#!/usr/bin/env python3
"""What per-env exploration costs the device rollout: rollout_device milliseconds per step at 64 agents x 4096 envs, f32 rows,
200-step stretches timed with HIP events.

    python3 tools/explore_bench.py --compare PARENT_ROOT [--rounds 5] [--out FILE]

PARENT_ROOT is a built checkout of the parent commit.  The scalar path (one noise scale, no coin: policy kernel with noise +
env step per step) is measured there, coin="env" (epsilon 0.1, noise scale 0.1 in every env: policy kernel without noise +
k_explore_envs + env step) in this tree, each with and without the log-pi column, in interleaved fresh processes:
parent scalar, tree env, parent scalar + log-pi, tree env + log-pi, `--rounds` times over.  Every process warms up with one
stretch, times `--stretches` stretches and reports their median; the table is the median [min, max] over the processes.

    python3 tools/explore_bench.py --worker scalar|env [--log-pi] [--root ROOT]     one process of the above: a JSON line

What to expect, written before the first run: one more launch per step and one pass over the step's actions -- 262,144 rows x
8 bytes = 2 MB read and written (3 MB with log-pi) -- against about 0.178 ms per step, i.e. a few microseconds where the
launches are not the bound.  An expectation, not a bar."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_AGENTS, N_ENVS = 64, 4096


def worker(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    from marl_llm_amd.batched import SwarmBatch
    from marl_llm_amd.rollout import ChainedReplay, FusedPolicy, PolicyMLP, rollout_device
    from marl_llm_amd.shapes import r_avoid_for, synthetic_shape_set
    if not torch.cuda.is_available():
        raise SystemExit("explore_bench: no HIP device (this is a GPU measurement)")
    shapes = synthetic_shape_set()
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    sb = SwarmBatch(n_env=N_ENVS, n_agents=N_AGENTS, n_cells_max=ng_max, r_avoid=r_avoid_for(N_AGENTS, shapes), obs_dtype=torch.float32)
    sb.set_shapes(shapes)
    torch.manual_seed(0)
    pol = FusedPolicy(PolicyMLP(192, 2, 180).cuda(), device=sb.device)
    ring = ChainedReplay(8, N_ENVS * N_AGENTS, sb.obs_dim, 2, sb.device, log_pi=args.log_pi)
    kw = dict(replay=ring, seed=1, log_pi=args.log_pi)
    if args.worker == "env":
        sig = torch.full((N_ENVS,), 0.1, device=sb.device)
        kw.update(coin="env", epsilon=torch.full((N_ENVS,), 0.1, device=sb.device), noise_scale=sig)
        if args.log_pi:
            from marl_llm_amd.rollout import explore_log_c
            kw["log_c"] = torch.from_numpy(explore_log_c(sig.cpu().numpy())).to(sb.device)
    else:
        kw.update(noise_scale=0.1)
    obs, t, ms = sb.reset(seed=226), 0, []
    for rep in range(args.stretches + 1):                        # the first stretch is the warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        obs, _ = rollout_device(sb, pol, args.steps, obs=obs, step0=t, **kw)
        b.record()
        b.synchronize()
        t += args.steps
        if rep:
            ms.append(a.elapsed_time(b) / args.steps)
    sb.close()
    pol.close()
    print(json.dumps(dict(worker=args.worker, log_pi=args.log_pi, root=os.path.abspath(args.root), steps=args.steps,
                          ms_per_step=round(statistics.median(ms), 6), stretches=[round(v, 6) for v in ms],
                          device=torch.cuda.get_device_name(0))), flush=True)


def compare(args):
    cases = [("parent scalar", "scalar", False, args.compare), ("tree coin=env", "env", False, HERE),
             ("parent scalar + log-pi", "scalar", True, args.compare), ("tree coin=env + log-pi", "env", True, HERE)]
    res, device = {name: [] for name, _, _, _ in cases}, "?"
    for _ in range(args.rounds):
        for name, mode, lp, root in cases:                        # interleaved: one fresh process at a time
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--root", root, "--steps", str(args.steps),
                   "--stretches", str(args.stretches)] + (["--log-pi"] if lp else [])
            p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, timeout=args.timeout)
            if p.returncode != 0:
                raise SystemExit("explore_bench: %s exited %d" % (" ".join(cmd), p.returncode))
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res[name].append(r["ms_per_step"])
            device = r["device"]
            print("%-24s %.4f ms/step" % (name, r["ms_per_step"]), flush=True)
    lines = ["%s; %d agents x %d envs, f32 rows; %d-step stretches, %d per process after a warm-up; %d interleaved processes per case; "
             "median [min, max] ms per step" % (device, N_AGENTS, N_ENVS, args.steps, args.stretches, args.rounds)]
    med = {k: statistics.median(v) for k, v in res.items()}
    for name, _, _, _ in cases:
        v = res[name]
        lines.append("%-24s %.4f [%.4f, %.4f]" % (name, med[name], min(v), max(v)))
    lines.append("coin=env - scalar: %+.4f ms per step; with log-pi: %+.4f ms per step"
                 % (med["tree coin=env"] - med["parent scalar"], med["tree coin=env + log-pi"] - med["parent scalar + log-pi"]))
    lines.append(json.dumps(res))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--compare", metavar="PARENT_ROOT", help="a built checkout of the parent commit")
    ap.add_argument("--worker", choices=["scalar", "env"])
    ap.add_argument("--root", default=HERE, help="the tree whose package a worker imports")
    ap.add_argument("--log-pi", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--stretches", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds one worker process may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        worker(args)
    elif args.compare:
        compare(args)
    else:
        ap.error("give --compare PARENT_ROOT or --worker")


if __name__ == "__main__":
    main()
