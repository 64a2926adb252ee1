#!/usr/bin/env python3
"""Device counterpart of the reference's eval_assembly.py: one rollout_eval call evaluates a given actor on `--envs`
environments at once, with mid-episode target-shape switches, and save_eval_results writes the reference's metrics.pkl and
state_data.npz for one env plus metrics_batch.npz (mean / std of the three metrics over the envs per step).

  python tools/eval_device.py --random-actor --envs 64 --episode_length 300 --switch 0:0,150:1
  python tools/eval_device.py --model models/run/model.pt --results_file results.pkl --switch 0:4,300:5 --episode_length 600
  python tools/eval_device.py --random-actor --envs 70 --all-shapes
  python tools/eval_device.py --models run/incremental/model_ep*.pt --envs 64
  python tools/eval_device.py --random-actors 4 --envs 64

--all-shapes evaluates the actor on every shape of the set in one batch: env e takes shape e % S at step 0 (a per-env switch,
SwarmBatch.select_shapes), the final per-shape table is printed and save_eval_by_shape writes metrics_by_shape.npz.

--models A.pt B.pt ... evaluates several checkpoints of one shape in the same call (a FusedPolicyBank): env group m -- the envs
[m E / M, (m + 1) E / M) -- runs checkpoint m, --envs must be a multiple of their count, the per-member table is printed and
save_eval_by_member writes metrics_by_member.npz.  --random-actors M is that with M randomly initialised actors.

--model reads the actor's fc1..fc4 tensors from a MADDPG checkpoint (torch.save of {'init_dict', 'agent_params': [{'policy':
state_dict, ...}]}; a bare state dict works too) into a PolicyMLP.  The file is read with torch.load(weights_only=True): tensors
and plain containers only."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from marl_llm_amd.batched import SwarmBatch
from marl_llm_amd.rollout import (FusedPolicy, FusedPolicyBank, PolicyMLP, rollout_eval, save_eval_by_member, save_eval_by_shape,
                                  save_eval_results)
from marl_llm_amd.shapes import load_results, r_avoid_for, synthetic_shape_set

FC = ("fc1", "fc2", "fc3", "fc4")


def parse_switch(text):
    """'0:4,300:5' -> {0: 4, 300: 5}."""
    sched = {}
    for item in filter(None, (text or "").split(",")):
        t, s = item.split(":")
        sched[int(t)] = int(s)
    return sched


def all_shapes_switch(n_env, n_shapes):
    """The schedule of --all-shapes: at step 0 env e takes shape e % S."""
    return {0: np.arange(n_env) % n_shapes}


def by_shape_table(mean, count):
    """The per-shape table of one step: mean [S, 3], count [S] of metrics_by_shape.npz."""
    lines = ["shape | envs | coverage | distribution uniformity | voronoi uniformity"]
    for s in range(len(count)):
        lines.append("%5d | %4d | %8.4f | %23.4f | %18.4f" % (s, count[s], mean[s, 0], mean[s, 1], mean[s, 2]))
    return "\n".join(lines)


def by_member_table(mean, count, names):
    """The per-member table of one step: mean [M, 3], count [M] of metrics_by_member.npz, names [M]."""
    lines = ["member | envs | coverage | distribution uniformity | voronoi uniformity | actor"]
    for m in range(len(count)):
        lines.append("%6d | %4d | %8.4f | %23.4f | %18.4f | %s" % (m, count[m], mean[m, 0], mean[m, 1], mean[m, 2], names[m]))
    return "\n".join(lines)


def check_actor_args(args):
    """'' or what is wrong with the actor options: exactly one of --model, --random-actor, --models, --random-actors; a bank's
    member count divides --envs."""
    given = [args.model is not None, bool(args.random_actor), args.models is not None, args.random_actors is not None]
    if args.model is not None and args.models is not None:
        return "--model and --models are mutually exclusive"
    if sum(given) != 1:
        return "give exactly one of --model, --random-actor, --models and --random-actors"
    n = len(args.models) if args.models is not None else args.random_actors
    if n is not None:
        if not 1 <= n <= 256:
            return "a bank holds 1 to 256 actors, not %d" % n
        if args.envs % n != 0:
            return "--envs %d must be a multiple of the %d actors" % (args.envs, n)
    return ""


def actor_state(ckpt):
    """The fc1..fc4 weight / bias tensors of the actor in a checkpoint dict."""
    sd = ckpt
    if isinstance(sd, dict) and "agent_params" in sd:
        sd = sd["agent_params"][0]
    if isinstance(sd, dict) and "policy" in sd:
        sd = sd["policy"]
    out = {}
    for fc in FC:
        for part in ("weight", "bias"):
            keys = [k for k in sd if k == f"{fc}.{part}" or k.endswith(f".{fc}.{part}")]
            if len(keys) != 1:
                raise KeyError(f"checkpoint: expected exactly one {fc}.{part}, found {keys}")
            out[f"{fc}.{part}"] = sd[keys[0]].detach().to(torch.float32)
    return out


def load_actor(path):
    sd = actor_state(torch.load(path, map_location="cpu", weights_only=True))
    hidden, obs_dim = sd["fc1.weight"].shape
    module = PolicyMLP(obs_dim, sd["fc4.weight"].shape[0], hidden)
    module.load_state_dict(sd)
    return module


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n_a", type=int, default=30)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--episode_length", type=int, default=300)
    ap.add_argument("--switch", default="0:0", help="step:shape pairs, e.g. 0:4,300:5")
    ap.add_argument("--all-shapes", action="store_true", help="env e takes shape e %% S at step 0 (instead of --switch)")
    ap.add_argument("--model", default=None, help="MADDPG checkpoint (model.pt)")
    ap.add_argument("--random-actor", action="store_true", help="a randomly initialised actor instead of --model")
    ap.add_argument("--models", nargs="+", default=None, metavar="CKPT",
                    help="several checkpoints of one shape, evaluated in one call: env group m runs checkpoint m")
    ap.add_argument("--random-actors", type=int, default=None, metavar="M", help="M randomly initialised actors instead of --models")
    ap.add_argument("--precision", default="bf16x3", choices=("bf16", "bf16x3"),
                    help="bf16x3 follows the reference's fp32 actor to ~1e-4")
    ap.add_argument("--results_file", default=None, help="shape set in the reference's results.pkl layout (default: synthetic)")
    ap.add_argument("--seed", type=int, default=226)
    ap.add_argument("--env", type=int, default=0, help="the env metrics.pkl / state_data.npz are written for")
    ap.add_argument("--out", default="eval_results")
    args = ap.parse_args()
    if args.models is None and args.random_actors is None:
        if (args.model is None) == (not args.random_actor):
            ap.error("give exactly one of --model and --random-actor")
    elif check_actor_args(args):
        ap.error(check_actor_args(args))
    if not torch.cuda.is_available():
        raise SystemExit("eval_device: no HIP device (the evaluation loop has no CPU path)")
    shapes = load_results(args.results_file) if args.results_file else synthetic_shape_set()
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    sb = SwarmBatch(n_env=args.envs, n_agents=args.n_a, n_cells_max=ng_max, r_avoid=r_avoid_for(args.n_a, shapes))
    sb.set_shapes(shapes)
    names = None
    if args.models is not None or args.random_actors is not None:
        if args.models is not None:
            modules, names = [load_actor(f) for f in args.models], list(args.models)
        else:
            torch.manual_seed(args.seed)
            modules = [PolicyMLP(sb.obs_dim, 2, 180) for _ in range(args.random_actors)]
            names = ["random %d" % k for k in range(args.random_actors)]
        policy = FusedPolicyBank([m.to(sb.device) for m in modules], device=sb.device, precision=args.precision)
    else:
        if args.random_actor:
            torch.manual_seed(args.seed)
            module = PolicyMLP(sb.obs_dim, 2, 180)
        else:
            module = load_actor(args.model)
        policy = FusedPolicy(module.to(sb.device), device=sb.device, precision=args.precision)
    S = len(shapes["l_cell"])
    switch = all_shapes_switch(args.envs, S) if args.all_shapes else parse_switch(args.switch)
    _, trace = rollout_eval(sb, policy, args.episode_length, reset=(args.seed, 0, 0), switch=switch, trace_state=True)
    paths = save_eval_results(trace, args.out, env=args.env)
    if args.all_shapes:
        paths += (save_eval_by_shape(trace, args.out, S),)
        with np.load(paths[-1]) as z:
            print(by_shape_table(z["mean"][-1], z["count"][-1]))
    if names is not None:
        paths += (save_eval_by_member(trace, policy.member_of_env(args.envs), args.out),)
        with np.load(paths[-1]) as z:
            print(by_member_table(z["mean"][-1], z["count"][-1], names))
    m = trace.metrics[-1].cpu().numpy()
    with np.errstate(all="ignore"):
        print("last step over %d envs: coverage %.4f, distribution uniformity %.4f, voronoi uniformity %.4f | mean reward %.4f"
              % (args.envs, np.nanmean(m[:, 0]), np.nanmean(m[:, 1]), np.nanmean(m[:, 2]), float(trace.reward_stats[:, 0].mean())))
    for p in paths:
        print(p)
    sb.close()
    policy.close()


if __name__ == "__main__":
    main()
