#!/usr/bin/env python3
"""What an actor bank (FusedPolicyBank, swarm_policy_bank_create) costs per call, beside what a caller had before it.

(192, 180, 2), 262,144 rows (64 agents x 4096 envs), fp32 and bf16 rows, both precisions, M in {1, 4, 16, 64, 256} members:
  (a) bank    -- ONE launch of the bank's kernel, member m on rows [m R, (m + 1) R), R = 262144 / M;
  (b) handles -- M launches of M plain handles over the same segments on one stream: what was possible without a bank;
  (c) plain   -- one plain handle over all rows: the M = 1 yardstick (measured beside every M, so that it alternates with them).

Every repetition is a FRESH process (`--child`) that measures all cells, one after another, in the same order, so the cells
alternate across the repetitions; a cell is `--iters` calls between two HIP events after `--warmup` calls, us per call.  The
parent prints median [min, max] over the repetitions and one JSON line per cell, also written to --out
(profiles/r23/policy_bank_bench.txt is such a file).  One GPU process at a time."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = 262144
SHAPE = (192, 180, 2)
MEMBERS = (1, 4, 16, 64, 256)


def child(args):
    import torch
    from marl_llm_amd.rollout import FusedPolicy, FusedPolicyBank, PolicyMLP
    if not torch.cuda.is_available():
        raise SystemExit("policy_bank_bench: no HIP device (this is a GPU measurement)")

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

    in_dim, hidden, act = SHAPE
    mods = []
    for k in range(max(MEMBERS)):
        torch.manual_seed(k)
        mods.append(PolicyMLP(in_dim, act, hidden).cuda())
    plain = [FusedPolicy(m) for m in mods]
    x32 = torch.rand(ROWS, in_dim, device="cuda") * 2 - 1
    rows = {"f32": x32, "bf16": x32.to(torch.bfloat16)}
    out = torch.empty(ROWS, act, device="cuda")
    res = []
    for M in MEMBERS:
        bank = FusedPolicyBank(mods[:M])
        R = ROWS // M
        for precision in ("bf16", "bf16x3"):
            for f in [bank] + plain[:M]:
                assert f.lib.swarm_policy_set_precision(f.handle, 1 if precision == "bf16x3" else 0) == 0
            for name, x in rows.items():
                segs = [(plain[m], x[m * R:(m + 1) * R], out[m * R:(m + 1) * R]) for m in range(M)]

                def handles():
                    for f, xs, os_ in segs:
                        f(xs, out=os_)
                cell = dict(members=M, precision=precision, rows_dtype=name)
                res.append(dict(cell, kind="bank", us=timed(lambda: bank(x, out=out))))
                res.append(dict(cell, kind="handles", us=timed(handles)))
                res.append(dict(cell, kind="plain", us=timed(lambda: plain[0](x, out=out))))
        bank.close()
    print("RESULT " + json.dumps(dict(device=torch.cuda.get_device_name(0), cells=res)), flush=True)


def mmm(v, nd=1):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def fmt(d, w=7):
    return f"{d['median']:{w}.1f} [{d['min']:.1f}, {d['max']:.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="fresh processes (at least 5)")
    ap.add_argument("--iters", type=int, default=20, help="timed calls per cell and process")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", action="store_true", help="measure every cell once in this process and print one RESULT line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "policy_bank_bench.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.reps < 5:
        raise SystemExit("policy_bank_bench: --reps must be at least 5")
    runs, device = [], "?"
    for rep in range(args.reps):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--warmup", str(args.warmup)],
                           stdout=subprocess.PIPE, universal_newlines=True, timeout=300)
        if p.returncode != 0:
            raise SystemExit("policy_bank_bench: repetition %d failed (exit %d); stopping" % (rep, p.returncode))
        line = next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))
        r = json.loads(line[7:])
        device = r["device"]
        runs.append(r["cells"])
        print("repetition %d of %d done" % (rep + 1, args.reps), flush=True)
    key = lambda c: (c["kind"], c["members"], c["precision"], c["rows_dtype"])
    us = {}
    for cells in runs:
        for c in cells:
            us.setdefault(key(c), []).append(c["us"])
    lines = [f"{device}; {'-'.join(map(str, SHAPE))}, {ROWS} rows, us per call between HIP events ({args.iters} calls after {args.warmup} warm-up "
             f"calls); median [min, max] over {args.reps} fresh processes",
             f"{'mode':>7} {'rows':>5} {'M':>4} | {'(a) bank, 1 launch':>24} | {'(b) M handles, M launches':>26} | {'(c) plain, all rows':>24} | (a) / (b) | (a) / (c)"]
    js = []
    for precision in ("bf16", "bf16x3"):
        for name in ("f32", "bf16"):
            for M in MEMBERS:
                a, b, c = (mmm(us[(kind, M, precision, name)]) for kind in ("bank", "handles", "plain"))
                js.append(json.dumps(dict(shape=list(SHAPE), rows=ROWS, members=M, precision=precision, rows_dtype=name, bank_us=a, handles_us=b,
                                          plain_us=c, bank_over_handles=round(a["median"] / b["median"], 3),
                                          bank_over_plain=round(a["median"] / c["median"], 3))))
                lines.append(f"{precision:>7} {name:>5} {M:4d} | {fmt(a):>24} | {fmt(b):>26} | {fmt(c):>24} | {a['median'] / b['median']:9.3f} | "
                             f"{a['median'] / c['median']:9.3f}")
    print("\n".join(lines + js))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + js) + "\n")


if __name__ == "__main__":
    main()
