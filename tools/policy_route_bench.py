#!/usr/bin/env python3
"""What routing an actor bank by env (FusedPolicyBank.assign, swarm_policy_bank_route) costs per call, beside the bank's own launch.

(192, 180, 2), 262,144 rows as 64 agents x 4096 envs, fp32 and bf16 rows, both precisions, M in {1, 4, 16, 64, 256} members:
  (a) bank    -- the existing bank launch, equal contiguous groups (no route), measured beside every routed figure;
  (b) equal   -- the routed launch with the table of those same groups, e // (E / M);
  (c) perm    -- the routed launch with a random permutation of that table: the same counts, every tile gathered;
  (d) skew    -- the routed launch with half the envs on member 0, the rest spread over all members at random;
  route       -- swarm_policy_bank_route on a device table, the C call itself, at E = 4096 and E = 32768 envs of 64 rows: time
                 per call between two HIP events, i.e. the routing kernel wherever the host enqueues faster than it runs.
At M = 1 the three tables are the same array (all zeros): (b), (c) and (d) are then ONE launch measured three times.

Every repetition is a FRESH process (`--child`) that measures all cells; a cell is `--iters` calls between two HIP events after
`--warmup` calls, us per call.  The four kinds of a (M, precision, rows) block are measured one after another, and repetition
r starts the block at kind r % 4: over a multiple of four repetitions every kind stands in every position equally often, so
that (a) is measured beside every routed figure and not always in front of them.  The parent prints median [min, max] over
the repetitions, what the POSITION in the block alone does to a figure, and one JSON line per cell, also written to --out
(profiles/r26/policy_route_bench.txt is such a file).  No ratio is asserted: the figures to read are (b)/(a) and (c)/(a).
One GPU process at a time."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_AGENTS, N_ENV = 64, 4096
ROWS = N_AGENTS * N_ENV
SHAPE = (192, 180, 2)
MEMBERS = (1, 4, 16, 64, 256)
ROUTE_ENVS = (4096, 32768)
KINDS = ("bank", "equal", "perm", "skew")


def tables(M, E, rng):
    import numpy as np
    equal = np.arange(E) // (E // M)
    skew = np.where(np.arange(E) % 2 == 0, 0, rng.integers(0, M, E))
    return dict(equal=equal, perm=rng.permutation(equal), skew=skew)


def child(args):
    import ctypes
    import numpy as np
    import torch
    from marl_llm_amd.rollout import FusedPolicyBank, PolicyMLP
    if not torch.cuda.is_available():
        raise SystemExit("policy_route_bench: no HIP device (this is a GPU measurement)")

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
    x32 = torch.rand(ROWS, in_dim, device="cuda") * 2 - 1
    rows = {"f32": x32, "bf16": x32.to(torch.bfloat16)}
    out = torch.empty(ROWS, act, device="cuda")
    rng = np.random.default_rng(26)
    res = []
    for M in MEMBERS:
        bank = FusedPolicyBank(mods[:M])
        dev = {k: torch.from_numpy(t.astype(np.int32)).cuda() for k, t in tables(M, N_ENV, rng).items()}
        for precision in ("bf16", "bf16x3"):
            assert bank.lib.swarm_policy_set_precision(bank.handle, 1 if precision == "bf16x3" else 0) == 0
            for name, x in rows.items():
                cell = dict(members=M, precision=precision, rows_dtype=name)
                for pos in range(len(KINDS)):
                    kind = KINDS[(pos + args.rotate) % len(KINDS)]
                    bank.assign(None if kind == "bank" else dev[kind], N_AGENTS)
                    res.append(dict(cell, kind=kind, pos=pos, us=timed(lambda: bank(x, out=out))))
        for E in ROUTE_ENVS:                                   # the routing kernel alone
            t = torch.from_numpy(rng.integers(0, M, E).astype(np.int32)).cuda()
            bank.assign(t, N_AGENTS)                           # the allocation for this size, outside the timed calls
            h, ptr, st = bank.handle, ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            res.append(dict(members=M, kind="route", envs=E, us=timed(lambda: bank.lib.swarm_policy_bank_route(h, ptr, E, N_AGENTS, st))))
        bank.close()
    print("RESULT " + json.dumps(dict(device=torch.cuda.get_device_name(0), cells=res)), flush=True)


def mmm(v, nd=1):
    return dict(median=round(statistics.median(v), nd), min=round(min(v), nd), max=round(max(v), nd))


def fmt(d, w=7):
    return f"{d['median']:{w}.1f} [{d['min']:.1f}, {d['max']:.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8, help="fresh processes (at least 8, a multiple of 4: one per starting kind)")
    ap.add_argument("--rotate", type=int, default=0, help="(child) the kind a block starts with")
    ap.add_argument("--iters", type=int, default=20, help="timed calls per cell and process")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", action="store_true", help="measure every cell once in this process and print one RESULT line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26", "policy_route_bench.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.reps < 8 or args.reps % len(KINDS):
        raise SystemExit("policy_route_bench: --reps must be at least 8 and a multiple of %d" % len(KINDS))
    runs, device = [], "?"
    for rep in range(args.reps):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--warmup", str(args.warmup),
                            "--rotate", str(rep % len(KINDS))],
                           stdout=subprocess.PIPE, universal_newlines=True, timeout=300)
        if p.returncode != 0:
            raise SystemExit("policy_route_bench: repetition %d failed (exit %d); stopping" % (rep, p.returncode))
        line = next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))
        r = json.loads(line[7:])
        device = r["device"]
        runs.append(r["cells"])
        print("repetition %d of %d done" % (rep + 1, args.reps), flush=True)
    key = lambda c: (c["kind"], c["members"], c.get("precision"), c.get("rows_dtype"), c.get("envs"))
    us = {}
    for cells in runs:
        for c in cells:
            us.setdefault(key(c), []).append(c["us"])
    lines = [f"{device}; {'-'.join(map(str, SHAPE))}, {ROWS} rows = {N_AGENTS} x {N_ENV} envs, us per call between HIP events ({args.iters} calls after "
             f"{args.warmup} warm-up calls); median [min, max] over {args.reps} fresh processes",
             f"{'mode':>7} {'rows':>5} {'M':>4} | {'(a) bank, equal groups':>24} | {'(b) routed, equal table':>24} | {'(c) routed, permuted':>24} | "
             f"{'(d) routed, skewed':>24} | (b) / (a) | (c) / (a) | (d) / (a)"]
    js = []
    for precision in ("bf16", "bf16x3"):
        for name in ("f32", "bf16"):
            for M in MEMBERS:
                a, b, c, d = (mmm(us[(kind, M, precision, name, None)]) for kind in KINDS)
                js.append(json.dumps(dict(shape=list(SHAPE), rows=ROWS, members=M, precision=precision, rows_dtype=name, bank_us=a, equal_us=b,
                                          perm_us=c, skew_us=d, equal_over_bank=round(b["median"] / a["median"], 3),
                                          perm_over_bank=round(c["median"] / a["median"], 3), skew_over_bank=round(d["median"] / a["median"], 3))))
                lines.append(f"{precision:>7} {name:>5} {M:4d} | {fmt(a):>24} | {fmt(b):>24} | {fmt(c):>24} | {fmt(d):>24} | "
                             f"{b['median'] / a['median']:9.3f} | {c['median'] / a['median']:9.3f} | {d['median'] / a['median']:9.3f}")
    # what the position in a block alone does: every figure over its cell's median, pooled by position
    med = {k: statistics.median(v) for k, v in us.items()}
    by_pos = {}
    for cells in runs:
        for c in cells:
            if "pos" in c:
                by_pos.setdefault(c["pos"], []).append(c["us"] / med[key(c)])
    pos_line = ", ".join("position %d: %.3f" % (p, statistics.median(v)) for p, v in sorted(by_pos.items()))
    lines.append("a figure over its cell's median, by position in the block (median over all cells and kinds): " + pos_line)
    js.append(json.dumps(dict(position_over_cell_median={str(p): round(statistics.median(v), 4) for p, v in sorted(by_pos.items())})))
    lines.append(f"us per swarm_policy_bank_route call (the routing kernel, one workgroup, behind the host's enqueue); rows_per_env {N_AGENTS}")
    lines.append(f"{'M':>4} | " + " | ".join(f"{'E = %d' % E:>24}" for E in ROUTE_ENVS))
    for M in MEMBERS:
        r = [mmm(us[("route", M, None, None, E)]) for E in ROUTE_ENVS]
        js.append(json.dumps(dict(members=M, rows_per_env=N_AGENTS, route_us={str(E): v for E, v in zip(ROUTE_ENVS, r)})))
        lines.append(f"{M:4d} | " + " | ".join(f"{fmt(v):>24}" for v in r))
    print("\n".join(lines + js))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + js) + "\n")


if __name__ == "__main__":
    main()
