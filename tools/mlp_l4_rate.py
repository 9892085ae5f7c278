#!/usr/bin/env python3
"""Developer tool: self.mlp = Linear(100, 400) -> ReLU -> Linear(400, 100) of num_layer 4 on rows that already exist -- the streamed
matrix-core kernels (fused_feature.mlp_l4 -> tpnet_mlp_l4_f32 / tpnet_mlp_l4_bwd_f32, csrc/mlp_l4.hip) against the torch layers on the
same tensors, alternated inside one process.  What sets fused_feature.MLP_L4_FROM and MLP_L4_BWD_FROM.

    tools/mlp_l4_rate.py [--n 1000 80000 800000] [--windows 5] [--limit 300] [--md OUT.md] [--json OUT.json]

Every size is measured by a child process of its own (`--one N`) under a time limit of `--limit` seconds; the first child that fails
or runs out of time ends the tool.  Two legs per size:
  forward   under no_grad: ff.mlp_l4(mlp, x) against mlp(x)
  training  forward + backward from gy: autograd through ff.mlp_l4 (the train kernel that records the ReLU's decisions, the two
            backward launches, the sum of the partials) against autograd through the torch layers
One window = device events around `calls` calls (fewer at the longer lists), then a synchronise; both variants are warmed up first,
then take turns window by window.  Per leg: median and min-max of each variant in us per call, the peak of the allocator above what
was allocated before the call (one call of each, MiB), the largest |difference| of the two results over the scale, and whether the
kernel's median is below torch's by more than the larger of the two spreads (max - min).  The rule: the threshold = the smallest n
from which that holds at every larger measured n; None if it never does."""
import argparse
import json
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[1000, 80000, 800000])
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--limit", type=int, default=300)
ap.add_argument("--one", type=int, default=None)
ap.add_argument("--md", default=None)
ap.add_argument("--json", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def first_winning(rows):
    rows = sorted(rows, key=lambda r: r["n"])
    for i, r in enumerate(rows):
        if all(q["kernel_wins"] for q in rows[i:]):
            return r["n"]
    return None


def driver():
    rows = []
    for n in args.n:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", str(n), "--windows", str(args.windows)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"n={n}: the measuring process ended with status {p.returncode}; nothing more is started")
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        print(p.stdout, end="", flush=True)
    legs = {leg: [r for r in rows if r["leg"] == leg] for leg in ("forward", "training")}
    rule = dict(MLP_L4_FROM=first_winning(legs["forward"]), MLP_L4_BWD_FROM=first_winning(legs["training"]))
    lines = []
    for leg, rs in legs.items():
        lines += [f"{leg}:", "", "| n | calls | kernel us (min-max) | torch us (min-max) | torch / kernel | kernel peak MiB | torch peak MiB | max abs diff / scale | kernel wins |",
                  "|---|---|---|---|---|---|---|---|---|"]
        lines += [f"| {r['n']} | {r['calls']} | {r['kernel_us']} ({r['kernel_min']}-{r['kernel_max']}) | {r['torch_us']} ({r['torch_min']}-{r['torch_max']}) | "
                  f"{r['torch_us'] / r['kernel_us']:.2f} | {r['kernel_peak_mib']} | {r['torch_peak_mib']} | {r['rel_diff']:.1e} | "
                  f"{'yes' if r['kernel_wins'] else 'no'} |" for r in rs]
        lines.append("")
    lines.append(f"{args.windows} windows per variant, alternating, on {rows[0]['device'] if rows else '?'}; rule: {rule}")
    print("\n".join(lines))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(rows=rows, **rule), f, indent=1)


def one(n):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from tpnet_amd import fused_feature as ff
    if not torch.cuda.is_available():
        sys.exit("mlp_l4_rate.py measures on a GPU: none found")
    dev = torch.device("cuda:0")
    calls = max(20, min(1000, 20_000_000 // n))
    ff.MLP_L4_FROM = ff.MLP_L4_BWD_FROM = 0                          # the kernels at every length
    torch.manual_seed(100)
    mlp = torch.nn.Sequential(torch.nn.Linear(100, 400), torch.nn.ReLU(), torch.nn.Linear(400, 100)).to(dev)
    params = list(mlp.parameters())
    x = torch.log1p(torch.expm1(torch.rand(n, 100, device=dev, dtype=torch.float64) * 20.0)).float()
    gy = torch.randn(n, 100, device=dev)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls * 1e3

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        del out
        return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    def measure(leg, variants, diff):
        for fn in variants.values():
            window(fn)
        ts = {k: [] for k in variants}
        for _ in range(args.windows):
            for k, fn in variants.items():
                ts[k].append(window(fn))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        spread = max(max(v) - min(v) for v in ts.values())
        row = dict(leg=leg, n=n, calls=calls, device=torch.cuda.get_device_name(0), rel_diff=diff,
                   kernel_wins=bool(med["torch"] - med["kernel"] > spread))
        for k, v in ts.items():
            row.update({f"{k}_us": round(med[k], 2), f"{k}_min": round(min(v), 2), f"{k}_max": round(max(v), 2), f"{k}_peak_mib": peak(variants[k])})
        print(json.dumps(row), flush=True)

    with torch.no_grad():
        variants = {"kernel": lambda: ff.mlp_l4(mlp, x), "torch": lambda: mlp(x)}
        seen = ff.calls["l4"]
        y = {k: fn() for k, fn in variants.items()}
        if y["kernel"] is None or ff.calls["l4"] != seen + 1:
            sys.exit("tpnet_mlp_l4_f32 declined the call")
        diff = float((y["kernel"] - y["torch"]).abs().max() / max(1.0, float(y["torch"].abs().max())))
        del y
        measure("forward", variants, diff)
    variants = {"kernel": lambda: torch.autograd.grad(ff.mlp_l4(mlp, x), params, gy), "torch": lambda: torch.autograd.grad(mlp(x), params, gy)}
    seen = ff.calls["l4_bwd"]
    g = {k: fn() for k, fn in variants.items()}
    if ff.calls["l4_bwd"] != seen + 2:
        sys.exit("tpnet_mlp_l4_bwd_f32 declined the call")
    diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(g["kernel"], g["torch"]))
    del g
    measure("training", variants, diff)


if args.one is not None:
    one(args.one)
else:
    driver()
