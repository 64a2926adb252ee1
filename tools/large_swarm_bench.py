#!/usr/bin/env python3
"""Cost of the env step on large_swarm handles, in milliseconds of GPU timeline between two HIP events, next to the step
kernel where it exists and to the CPU oracle.  Per config (agents x envs; f32 observation rows), after a warm-up of
`--steps` prior-policy steps from a device reset (the swarm assembles) `--reps` alternating repetitions of `--steps`
prior-policy steps (the step's own a_prior fed back as the action):

  256 x 1024            large_swarm 0 and 1, alternating: what the simple kernels cost where the step kernel exists
  300 x 256, 512 x 128, 1024 x 64, 1024 x 256      large_swarm 1 (the step kernel ends at 256 agents)

and for each config the wall time of ONE batched step of the oracle on 16 threads (tests/helpers.ThreadedOracle) from the
state the device run left: the floor of usefulness.

Output: a table (median [min, max] ms per step, agent-steps per second of the median) and one JSON line per row;
--out FILE also writes them there (profiles/r10/large_swarm_bench.txt is such a file)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from marl_llm_amd.batched import SwarmBatch
from marl_llm_amd.shapes import r_avoid_for, synthetic_shape_set

CONFIGS = ((256, 1024, (0, 1)), (300, 256, (1,)), (512, 128, (1,)), (1024, 64, (1,)), (1024, 256, (1,)))


def measure(n_a, E, modes, steps, reps, shapes, with_oracle):
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    ra = r_avoid_for(n_a, shapes)
    runs = {}
    for m in modes:
        sb = SwarmBatch(n_env=E, n_agents=n_a, n_cells_max=ng_max, r_avoid=ra, large_swarm=bool(m))
        sb.set_shapes(shapes)
        sb.reset(seed=226)
        runs[m] = dict(sb=sb, act=torch.zeros((E, n_a, 2), dtype=torch.float32, device=sb.device), ms=[])

    def timed(r):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sb, act = r["sb"], r["act"]
        torch.cuda.synchronize()
        a.record()
        for _ in range(steps):
            act = sb.step(act)[3]
        b.record()
        torch.cuda.synchronize()
        r["act"] = act.clone()
        return a.elapsed_time(b) / steps

    for r in runs.values():                       # warm-up: code objects, allocator; the swarm assembles
        timed(r)
    for _ in range(reps):                         # alternate the handles
        for r in runs.values():
            r["ms"].append(timed(r))
    oracle_s = None
    if with_oracle:
        from helpers import ThreadedOracle
        from oracle.oracle_py import Oracle
        r = runs[modes[-1]]
        sb = r["sb"]
        p, dp = [x.cpu().numpy() for x in sb.get_state()]
        nei = sb.indices(False, False)["neighbor_index"].cpu().numpy()
        cells, n_g = sb.get_cells()
        l_cell = np.asarray(shapes["l_cell"], np.float64)[sb.get_shape_index()]
        with ThreadedOracle(Oracle(), cells, n_g, l_cell, ra, workers=16) as to:
            a = np.swapaxes(r["act"].cpu().numpy(), 1, 2).astype(np.float64)
            t0 = time.perf_counter()
            to.step(p, dp, a, nei)
            oracle_s = time.perf_counter() - t0
    out = []
    for m, r in runs.items():
        med = statistics.median(r["ms"])
        out.append(dict(agents=n_a, envs=E, large_swarm=m, steps_per_call=steps, reps=reps, ms=round(med, 4), ms_min=round(min(r["ms"]), 4),
                        ms_max=round(max(r["ms"]), 4), agent_steps_per_s=round(n_a * E / (med * 1e-3)),
                        oracle_16_threads_s=None if oracle_s is None else round(oracle_s, 3)))
        r["sb"].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--config", default=None, help="one size only, AGENTSxENVS (e.g. 300x256)")
    ap.add_argument("--no-oracle", action="store_true", help="leave out the oracle's batched step")
    ap.add_argument("--out", default=None, help="also write the table and the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("large_swarm_bench: no HIP device (this is a GPU measurement)")
    shapes = synthetic_shape_set()
    configs = CONFIGS
    if args.config:
        n_a, E = (int(x) for x in args.config.lower().split("x"))
        configs = ((n_a, E, (0, 1) if n_a <= 256 else (1,)),)
    lines = [f"{torch.cuda.get_device_name(0)}; {args.steps} prior-policy steps per timed call, {args.reps} alternating repetitions, f32 rows",
             f"{'config':>14} | {'large_swarm':>11} | {'ms per step: median [min, max]':>34} | {'agent-steps / s':>15} | oracle, one batched step, 16 threads"]
    js = []
    for n_a, E, modes in configs:
        for r in measure(n_a, E, modes, args.steps, args.reps, shapes, not args.no_oracle):
            o = "-" if r["oracle_16_threads_s"] is None else "%.3f s" % r["oracle_16_threads_s"]
            lines.append(f"{n_a:>5} x {E:<6} | {r['large_swarm']:>11} | {r['ms']:>12.4f} [{r['ms_min']:.4f}, {r['ms_max']:.4f}]".ljust(68)
                         + f" | {r['agent_steps_per_s']:>15,} | {o}")
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
