#!/usr/bin/env python3
"""Step time of mixed batches: k of the E envs hold cells the lattice row walk does not serve (a jittered copy of their own
cells), spread evenly over the batch; the others keep their tiled shapes.  Microseconds of GPU timeline per step between two
HIP events, prior-policy actions (the action of a step is the a_prior of the one before), on the assembled state a warm-up
leaves.  Per k three handles are timed in alternation, `--reps` times each:

  default  one launch of each kernel, side by side (the generic launch on the handle's auxiliary stream)
  serial   debug_flags bit 4: the same two launches one after the other on the handle's stream
  demote   debug_flags bit 3: one generic launch for the whole batch -- what every mixed batch ran before the per-workgroup
           choice existed

At k = 0 (all walk) and k = E (none walks) the three are the same single launch and must time alike: the tool checks that
their medians agree within the largest [min, max] spread of the row and prints the verdict (exit status 1 if not); k = E is
the generic kernel's own step time at that size.  path_envs() of the default handle is printed beside each row.

Output: a table, and one JSON line per (config, k); --out also writes them to a file (profiles/r09/mixed_bench.txt)."""
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
from marl_llm_amd.shapes import r_avoid_for, synthetic_shape_set
from marl_llm_amd.synth import synthetic_batch

CONFIGS = ((64, 4096), (32, 8192))
VARIANTS = (("default", 0), ("serial", 16), ("demote", 8))
FRACTIONS = ("0", "1", "1%", "10%", "50%", "100%")


def n_generic(frac, E):
    return int(frac) if not frac.endswith("%") else max(1, round(E * float(frac[:-1]) / 100.0))


def measure(n_a, E, steps, reps, warm, shapes, fractions):
    sy = synthetic_batch(E, n_a, shapes, seed=226, assembled_fraction=1.0)
    ra = r_avoid_for(n_a, shapes)
    handles = {name: SwarmBatch(n_env=E, n_agents=n_a, n_cells_max=sy["cells"].shape[2], r_avoid=ra, debug_flags=flags)
               for name, flags in VARIANTS}
    rows = []
    for frac in fractions:
        k = n_generic(frac, E)
        cells = sy["cells"].copy()
        rng = np.random.default_rng(k)
        for e in np.unique(np.linspace(0, E - 1, k).round().astype(int)) if k else ():
            cells[e, :, : sy["n_g"][e]] += rng.normal(0, 0.004, (2, sy["n_g"][e]))
        act = {}
        for name, sb in handles.items():
            sb.set_cells(cells, sy["n_g"], sy["l_cell"])
            sb.set_state(sy["p"], sy["dp"])
            sb.observe()
            a = torch.zeros((E, n_a, 2), dtype=torch.float32, device=sb.device)
            for _ in range(warm):                                    # code objects, LDS attributes; the swarm settles
                a = sb.step(a)[3]
            act[name] = a

        def timed(name):
            sb, a = handles[name], act[name]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(steps):
                a = sb.step(a)[3]
            t1.record()
            torch.cuda.synchronize()
            act[name] = a
            return t0.elapsed_time(t1) / steps * 1e3

        res = {name: [] for name, _ in VARIANTS}
        for _ in range(reps):                                        # alternate the variants
            for name, _ in VARIANTS:
                res[name].append(timed(name))
        row = dict(agents=n_a, envs=E, generic=k, fraction=frac, path_envs=handles["default"].path_envs(), steps_per_call=steps, reps=reps)
        for name in res:
            row[name + "_us"] = round(statistics.median(res[name]), 2)
            row[name + "_us_min"] = round(min(res[name]), 2)
            row[name + "_us_max"] = round(max(res[name]), 2)
        rows.append(row)
    for sb in handles.values():
        sb.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--config", default=None, help="one size only, AGENTSxENVS (e.g. 64x4096)")
    ap.add_argument("--out", default=None, help="also write the table and the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mixed_bench: no HIP device (this is a GPU measurement)")
    shapes = synthetic_shape_set()
    configs = CONFIGS if not args.config else (tuple(int(x) for x in args.config.lower().split("x")),)
    names = [v[0] for v in VARIANTS]
    lines = [f"{torch.cuda.get_device_name(0)}; {args.steps} steps per timed call, {args.reps} alternating repetitions, "
             f"{args.warmup} warm-up steps; us per step, median [min, max]",
             f"{'config':>12} | {'generic envs':>14} | {'walk, scan':>12} | " + " | ".join(f"{x:>30}" for x in names)]
    js, rows_all = [], []
    for n_a, E in configs:
        for r in measure(n_a, E, args.steps, args.reps, args.warmup, shapes, FRACTIONS):
            f = lambda k: f"{r[k + '_us']:10.1f} [{r[k + '_us_min']:.1f}, {r[k + '_us_max']:.1f}]"
            lines.append(f"{n_a:>4} x {E:<5} | {r['generic']:>6} ({r['fraction']:>4}) | {str(tuple(r['path_envs'])):>12} | "
                         + " | ".join(f"{f(x):>30}" for x in names))
            js.append(json.dumps(r)); rows_all.append(r)
            print(lines[-1], flush=True)
    # k = 0 and k = E: the three variants are one and the same launch, so their medians must agree within the largest
    # [min, max] spread any of them shows on that row
    ok = True
    for r in rows_all:
        if r["generic"] not in (0, r["envs"]):
            continue
        med = [r[x + "_us"] for x in names]
        spread = max(r[x + "_us_max"] - r[x + "_us_min"] for x in names)
        same = max(med) - min(med) <= spread
        ok = ok and same
        lines.append(f"same-launch row {r['agents']} x {r['envs']}, k = {r['generic']}: medians differ by {max(med) - min(med):.2f} us, "
                     f"largest spread {spread:.2f} us: {'agree' if same else 'DISAGREE'}")
        print(lines[-1])
    lines.append("same-launch rows agree within the largest spread: " + ("yes" if ok else "NO"))
    print(lines[-1])
    text = "\n".join(lines + js) + "\n"
    print("\n".join(js))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
