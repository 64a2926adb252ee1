#!/usr/bin/env python3
"""Cost of the rule-based expert above 256 agents, in milliseconds of GPU timeline between two HIP events (f32 rows).

Per large_swarm config (agents x envs: 300 x 256, 512 x 128, 1024 x 64, 1024 x 256), after a device reset and a warm-up of
`--steps` expert steps (the expert calms its own states down), `--reps` alternating repetitions of
  rule      `--calls` rule_action() calls on the state as it stands: the cap_even export pass + k_rule_large, per call
  expert    one rollout_expert(source="rule") call of `--steps` steps: export pass + k_rule_large + the large step, per step

and at 256 x 1024 on two default handles from the same reset and warm-up -- the same states: the two kernels write the same
bits -- alternating, rule_action() with debug_flags 0 (k_rule) and 32 (k_rule_large, the in-binary stand-in).  Both calls
hold the same export pass, so the difference of the two rows is the difference of the kernels; the kernels' own durations
come from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/rule_large_bench.py --only pair, or
--only large --config 1024x64 for one large size).

Output: a table (median [min, max] ms) and one JSON line per row; --out FILE also writes them there
(profiles/r19/rule_large_bench.txt is such a file)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from marl_llm_amd.batched import SwarmBatch
from marl_llm_amd.rollout import ChainedReplay, rollout_expert
from marl_llm_amd.shapes import r_avoid_for, synthetic_shape_set

LARGE = ((300, 256), (512, 128), (1024, 64), (1024, 256))
PAIR = (256, 1024)


def handle(shapes, n_a, E, **kw):
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    sb = SwarmBatch(n_env=E, n_agents=n_a, n_cells_max=ng_max, r_avoid=r_avoid_for(n_a, shapes), **kw)
    sb.set_shapes(shapes)
    ring = ChainedReplay(1, E * n_a, sb.obs_dim, 2, sb.device, obs_dtype=torch.float32)
    rollout_expert(sb, 0, replay=ring, reset=(226, 0), track_reward=False)
    return sb, ring


def timed(fn, per):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / per


def row(what, n_a, E, ms, **kw):
    med = statistics.median(ms)
    return dict(what=what, agents=n_a, envs=E, reps=len(ms), ms=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                agent_steps_per_s=round(n_a * E / (med * 1e-3)), **kw)


def measure_large(shapes, n_a, E, steps, calls, reps):
    sb, ring = handle(shapes, n_a, E, large_swarm=True)

    def rule():
        for _ in range(calls):
            sb.rule_action()

    expert = lambda: rollout_expert(sb, steps, replay=ring, track_reward=False)
    timed(expert, steps); timed(rule, calls)                  # warm-up: code objects, lazy allocations; the swarm assembles
    ms = {"rule": [], "expert": []}
    for _ in range(reps):
        ms["rule"].append(timed(rule, calls))
        ms["expert"].append(timed(expert, steps))
    sb.close()
    return [row("rule_action", n_a, E, ms["rule"], kernel="k_rule_large", per="call", n=calls),
            row("rollout_expert step", n_a, E, ms["expert"], kernel="k_rule_large", per="step", n=steps)]


def measure_pair(shapes, steps, calls, reps):
    n_a, E = PAIR
    runs = {}
    for flags in (0, 32):
        sb, ring = handle(shapes, n_a, E, debug_flags=flags)
        timed(lambda: rollout_expert(sb, steps, replay=ring, track_reward=False), steps)
        runs[flags] = dict(sb=sb, ms=[])

    def rule(sb):
        for _ in range(calls):
            sb.rule_action()

    for r in runs.values():
        timed(lambda: rule(r["sb"]), calls)
    for _ in range(reps):                                     # alternate the handles
        for r in runs.values():
            r["ms"].append(timed(lambda: rule(r["sb"]), calls))
    assert torch.equal(runs[0]["sb"].rule_action(), runs[32]["sb"].rule_action())
    out = [row("rule_action", n_a, E, r["ms"], kernel="k_rule_large" if flags else "k_rule", per="call", n=calls, debug_flags=flags)
           for flags, r in runs.items()]
    for r in runs.values():
        r["sb"].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="expert steps per timed rollout_expert call (and of the warm-up)")
    ap.add_argument("--calls", type=int, default=20, help="rule_action() calls per timed repetition")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("large", "pair"), default=None)
    ap.add_argument("--config", default=None, help="one large_swarm size only, AGENTSxENVS (e.g. 1024x64)")
    ap.add_argument("--out", default=None, help="also write the table and the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rule_large_bench: no HIP device (this is a GPU measurement)")
    shapes = synthetic_shape_set()
    rows = []
    if args.only != "pair":
        for n_a, E in ([tuple(int(x) for x in args.config.lower().split("x"))] if args.config else LARGE):
            rows += measure_large(shapes, n_a, E, args.steps, args.calls, args.reps)
    if args.only != "large":
        rows += measure_pair(shapes, args.steps, args.calls, args.reps)
    lines = [f"{torch.cuda.get_device_name(0)}; {args.reps} alternating repetitions of {args.calls} rule_action() calls / one {args.steps}-step "
             "rollout_expert call, f32 rows",
             f"{'config':>14} | {'what':>19} | {'kernel':>12} | {'ms: median [min, max]':>30} | agent-steps / s"]
    for r in rows:
        lines.append(f"{r['agents']:>5} x {r['envs']:<6} | {r['what']:>19} | {r['kernel']:>12} | "
                     + f"{r['ms']:>10.4f} [{r['ms_min']:.4f}, {r['ms_max']:.4f}]".ljust(30) + f" | {r['agent_steps_per_s']:>15,}")
    pair = [r for r in rows if "debug_flags" in r]
    if len(pair) == 2:
        lines.append(f"rule_action at {PAIR[0]} x {PAIR[1]}: k_rule_large / k_rule (both with the export pass) = {pair[1]['ms'] / pair[0]['ms']:.3f}")
    text = "\n".join(lines + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
