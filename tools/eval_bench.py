#!/usr/bin/env python3
"""Cost of device evaluation per step, in microseconds of GPU timeline between two HIP events (so host-bound gaps of an
eager loop count, as they do for its user).  Per config (agents x envs; f32 observation rows, bf16 actor), after a warm-up
of every path and on the assembled state the warm-up leaves, alternating `--reps` times:

  a  eager      the evaluation loop from the entry points that predate swarm_rollout_eval, per step: get_state (trace),
                metrics, FusedPolicy, step -- the baseline (identical code before and after this loop existed)
  b  device     rollout_device(noise_scale=0): the loop without evaluation
  c  eval       rollout_eval with metrics
  d  eval+trace rollout_eval with metrics and the state trace
  e  switch     one shape switch: SwarmBatch.select_shape against the eager set_cells + observe (host upload + synchronise);
                switch_shapes / switch_shapes_pose: the per-env switch, SwarmBatch.select_shapes with device tensors (every env
                the next shape of the set; without a pose, and at a per-env rotation and offset)

No path records reward statistics (track_reward=False in b, c, d).  (a) is what a user of the eager entry points runs: its
get_state() copies the state and synchronises every step, so (a) includes the host-bound gaps that (c) and (d) do not have.

--config 64x4096 restricts the run to one size and --paths eager,eval to some paths: under
`rocprofv3 --kernel-trace --stats -- python tools/eval_bench.py --config 64x4096 --paths eager,eval` the kernel statistics
then hold k_metrics (launched by a) and k_metrics_step (launched by c) on the same trajectory at one size.  --fig-shapes runs
on the reference's seven fig/*.png shapes (tests/golden/fig_cells.npz) instead of the synthetic set.

Output: a table, and one JSON line per config."""
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
from marl_llm_amd.rollout import ChainedReplay, FusedPolicy, PolicyMLP, rollout_device, rollout_eval
from marl_llm_amd.shapes import r_avoid_for, synthetic_shape_set

CONFIGS = ((64, 4096), (30, 500))              # the headline size; the reference's N = 30 at a small batch


def measure(n_a, E, steps, reps, shapes, module, paths=None):
    ng_max = max(np.asarray(g).shape[0] for g in shapes["grid_coords"])
    sb = SwarmBatch(n_env=E, n_agents=n_a, n_cells_max=ng_max, r_avoid=r_avoid_for(n_a, shapes))
    sb.set_shapes(shapes)
    pol = FusedPolicy(module, device=sb.device)
    n = E * n_a
    ring = ChainedReplay(8, n, sb.obs_dim, 2, sb.device)
    grids = [np.asarray(g, np.float64).T for g in shapes["grid_coords"]]
    cells = np.zeros((len(grids), 2, ng_max))
    for k, g in enumerate(grids):
        cells[k, :, : g.shape[1]] = g
    state = {"obs": sb.reset(seed=226), "shape": 0}

    def eager(k):
        obs = state["obs"]
        for _ in range(k):
            sb.get_state()
            sb.metrics()
            act = pol(obs.reshape(n, -1), noise_scale=0)
            obs = sb.step(act.view(E, n_a, 2))[0]
        state["obs"] = obs

    def device(k):
        state["obs"], _ = rollout_device(sb, pol, k, obs=state["obs"], replay=ring, noise_scale=0.0, track_reward=False)

    def evaluate(k, trace=False):
        state["obs"], _ = rollout_eval(sb, pol, k, obs=state["obs"], replay=ring, trace_state=trace, track_reward=False)

    def switch_device(k):
        for _ in range(k):
            state["shape"] = (state["shape"] + 1) % len(grids)
            sb.select_shape(state["shape"])

    def switch_eager(k):
        for _ in range(k):
            s = state["shape"] = (state["shape"] + 1) % len(grids)
            sb.set_cells(np.repeat(cells[s][None], E, 0), np.full(E, grids[s].shape[1], np.int32), np.full(E, shapes["l_cell"][s]))
            sb.observe()

    rng = np.random.default_rng(226)
    ang = rng.uniform(-np.pi, np.pi, E)
    pose = torch.from_numpy(np.column_stack([np.cos(ang), np.sin(ang), rng.uniform(-1, 1, (E, 2))])).to(sb.device)
    index = [torch.full((E,), s, dtype=torch.int32, device=sb.device) for s in range(len(grids))]

    def switch_shapes(k, pose=None):
        for _ in range(k):
            state["shape"] = (state["shape"] + 1) % len(grids)
            sb.select_shapes(index[state["shape"]], pose=pose)

    def timed(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn(k)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k * 1e3

    k_sw = 4
    cases = [("eager", eager, steps), ("device", device, steps), ("eval", evaluate, steps),
             ("eval_trace", lambda k: evaluate(k, True), steps), ("switch_device", switch_device, k_sw), ("switch_eager", switch_eager, k_sw),
             ("switch_shapes", switch_shapes, k_sw), ("switch_shapes_pose", lambda k: switch_shapes(k, pose), k_sw)]
    if paths:
        cases = [c for c in cases if c[0] in paths]
    for _, fn, k in cases:                                       # warm-up: code objects, allocator, LDS attributes; the swarm assembles
        timed(fn, k)
    res = {name: [] for name, _, _ in cases}
    for _ in range(reps):                                        # alternate the paths
        for name, fn, k in cases:
            res[name].append(timed(fn, k))
    sb.close()
    pol.close()
    out = dict(agents=n_a, envs=E, steps_per_call=steps, reps=reps)
    for name in res:
        out[name + "_us"] = round(statistics.median(res[name]), 2)
        out[name + "_us_min"] = round(min(res[name]), 2)
        out[name + "_us_max"] = round(max(res[name]), 2)
    if "eval_us" in out and "device_us" in out:
        out["eval_cost_us"] = round(out["eval_us"] - out["device_us"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--config", default=None, help="one size only, AGENTSxENVS (e.g. 64x4096)")
    ap.add_argument("--paths", default=None, help="comma-separated subset of eager,device,eval,eval_trace,switch_device,switch_eager,"
                                                 "switch_shapes,switch_shapes_pose")
    ap.add_argument("--fig-shapes", action="store_true", help="the reference's fig/*.png shapes instead of the synthetic set")
    ap.add_argument("--out", default=None, help="also write the table and the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no HIP device (this is a GPU measurement)")
    if args.fig_shapes:
        from marl_llm_amd.shape_images import unpack_cells_npz
        shapes = unpack_cells_npz(os.path.join(ROOT, "tests", "golden", "fig_cells.npz"))
    else:
        shapes = synthetic_shape_set()
    torch.manual_seed(0)
    module = PolicyMLP(192, 2, 180).cuda()
    names = ("eager", "device", "eval", "eval_trace", "switch_device", "switch_eager", "switch_shapes", "switch_shapes_pose")
    paths = args.paths.split(",") if args.paths else None
    if paths:
        if set(paths) - set(names):
            raise SystemExit("--paths: unknown path in %r" % (paths,))
        names = tuple(x for x in names if x in paths)
    configs = CONFIGS if not args.config else (tuple(int(x) for x in args.config.lower().split("x")),)
    lines = [f"{torch.cuda.get_device_name(0)}; {args.steps} steps per timed call, {args.reps} alternating repetitions; "
             "us per step (per switch), median [min, max]",
             f"{'config':>14} | " + " | ".join(f"{x:>30}" for x in names)]
    js = []
    for n_a, E in configs:
        r = measure(n_a, E, args.steps, args.reps, shapes, module, paths)
        f = lambda k: f"{r[k + '_us']:10.1f} [{r[k + '_us_min']:.1f}, {r[k + '_us_max']:.1f}]"
        lines.append(f"{n_a:>5} x {E:<6} | " + " | ".join(f"{f(x):>30}" for x in names))
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
