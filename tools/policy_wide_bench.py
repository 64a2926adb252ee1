#!/usr/bin/env python3
"""What the wide geometry of the fused actor (csrc/policy_wide.hip) costs per call, beside the narrow kernel and beside torch.

262,144 rows (64 agents x 4096 envs), fp32 and bf16 rows, both precisions, at
  (192,180,2) narrow, (192,180,2) wide, (288,180,2), (192,256,2), (384,256,2)        (in_dim, hidden, act_dim)
and, as the yardstick, the same PolicyMLP run by torch on the same rows: in fp32 beside bf16x3, under
torch.autocast(bfloat16) beside bf16.

Every repetition is a FRESH process (`--child`) that measures all cells, one after another, in the same order, so the
cells alternate across the repetitions; a cell is `--iters` calls between two HIP events after `--warmup` calls, us per call.
The parent prints median [min, max] over the repetitions and one JSON line per cell, also written to --out
(profiles/r21/policy_wide_bench.txt is such a file).  One GPU process at a time."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = 262144
CELLS = [((192, 180, 2), False), ((192, 180, 2), True), ((288, 180, 2), True), ((192, 256, 2), True), ((384, 256, 2), True)]
# MFMAs per 32-row tile in bf16 mode: layer 1 (k-steps x feature tiles) + two hidden layers + the output layer
MFMAS = {((192, 180, 2), False): 228, ((192, 180, 2), True): 12 * 6 + 2 * 12 * 6 + 12, ((288, 180, 2), True): 20 * 6 + 2 * 12 * 6 + 12,
         ((192, 256, 2), True): 12 * 8 + 2 * 16 * 8 + 16, ((384, 256, 2), True): 24 * 8 + 2 * 16 * 8 + 16}


def child(args):
    import torch
    from marl_llm_amd.rollout import FusedPolicy, PolicyMLP
    if not torch.cuda.is_available():
        raise SystemExit("policy_wide_bench: no HIP device (this is a GPU measurement)")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.iters * 1e3

    res = []
    for shape, wide in CELLS:
        in_dim, hidden, act = shape
        torch.manual_seed(0)
        m = PolicyMLP(in_dim, act, hidden).cuda()
        x32 = torch.rand(ROWS, in_dim, device="cuda") * 2 - 1
        rows = {"f32": x32, "bf16": x32.to(torch.bfloat16)}
        out = torch.empty(ROWS, act, device="cuda")
        for precision in ("bf16", "bf16x3"):
            f = FusedPolicy(m, precision=precision, wide=wide)
            for name, x in rows.items():
                us = timed(lambda: f(x, out=out))
                res.append(dict(kind="fused", shape=list(shape), wide=wide, precision=precision, rows_dtype=name, us=us))
            f.close()
    for shape in sorted(set(s for s, _ in CELLS)):
        in_dim, hidden, act = shape
        torch.manual_seed(0)
        m = PolicyMLP(in_dim, act, hidden).cuda()
        x32 = torch.rand(ROWS, in_dim, device="cuda") * 2 - 1
        rows = {"f32": x32, "bf16": x32.to(torch.bfloat16)}
        with torch.no_grad():
            for name, x in rows.items():
                us = timed(lambda: m(x.float()))                            # fp32 module: the yardstick of bf16x3
                res.append(dict(kind="torch", shape=list(shape), precision="fp32", rows_dtype=name, us=us))

                def autocast():
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        return m(x)
                us = timed(autocast)                                         # the yardstick of bf16
                res.append(dict(kind="torch", shape=list(shape), precision="autocast-bf16", rows_dtype=name, us=us))
    print("RESULT " + json.dumps(dict(device=torch.cuda.get_device_name(0), cells=res)), flush=True)


def mmm(v, nd=1):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def fmt(d, w=7):
    return f"{d['median']:{w}.1f} [{d['min']:.1f}, {d['max']:.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="fresh processes (at least 5)")
    ap.add_argument("--iters", type=int, default=50, help="timed calls per cell and process")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", action="store_true", help="measure every cell once in this process and print one RESULT line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "policy_wide_bench.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.reps < 5:
        raise SystemExit("policy_wide_bench: --reps must be at least 5")
    runs, device = [], "?"
    for rep in range(args.reps):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--warmup", str(args.warmup)],
                           stdout=subprocess.PIPE, universal_newlines=True, timeout=600)
        if p.returncode != 0:
            raise SystemExit("policy_wide_bench: repetition %d failed (exit %d); stopping" % (rep, p.returncode))
        line = next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))
        r = json.loads(line[7:])
        device = r["device"]
        runs.append(r["cells"])
        print("repetition %d of %d done" % (rep + 1, args.reps), flush=True)
    key = lambda c: (c["kind"], tuple(c["shape"]), c.get("wide"), c["precision"], c["rows_dtype"])
    us = {}
    for cells in runs:
        for c in cells:
            us.setdefault(key(c), []).append(c["us"])
    lines = [f"{device}; {ROWS} rows, us per call between HIP events ({args.iters} calls after {args.warmup} warm-up calls); median [min, max] "
             f"over {args.reps} fresh processes",
             f"{'shape':>14} {'kernel':>7} {'mode':>7} {'rows':>5} | {'fused us':>24} | {'torch us':>24} | fused / torch | MFMAs per tile"]
    js = []
    for shape, wide in CELLS:
        for precision in ("bf16", "bf16x3"):
            for name in ("f32", "bf16"):
                fu = mmm(us[("fused", shape, wide, precision, name)])
                to = mmm(us[("torch", shape, None, "autocast-bf16" if precision == "bf16" else "fp32", name)])
                n_mfma = MFMAS[(shape, wide)] * (1 if precision == "bf16" else 3)
                ratio = round(fu["median"] / to["median"], 3)
                js.append(json.dumps(dict(shape=list(shape), kernel="wide" if wide else "narrow", precision=precision, rows_dtype=name,
                                          rows=ROWS, fused_us=fu, torch_us=to, fused_over_torch=ratio, mfmas_per_tile=n_mfma)))
                lines.append(f"{'%d-%d-%d' % shape:>14} {'wide' if wide else 'narrow':>7} {precision:>7} {name:>5} | {fmt(fu):>24} | "
                             f"{fmt(to):>24} | {ratio:13.3f} | {n_mfma}")
    print("\n".join(lines + js))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + js) + "\n")


if __name__ == "__main__":
    main()
