#!/usr/bin/env python3
"""Developer tool: self.mlp = Linear(F, 4F) -> ReLU -> Linear(4F, F) for num_layer 1 and 2 (F = 16, 36) on rows that already exist --
the matrix-core kernel (fused_feature.mlp_f32 -> tpnet_mlp_rows_f32, csrc/mlp_rows.hip) against the route these widths had before
it, the torch expression mlp(x) on the same tensor, alternated inside one process.  What sets fused_feature.MLP_ROWS_FROM.

    tools/mlp_rows_rate.py [--F 16 36] [--n 1000 8192 80000 800000] [--bwd-n 1000 80000 800000] [--calls 200] [--windows 5]
                           [--md OUT.md] [--json OUT.json]

One window = device events around `calls` calls, then a synchronise; both variants are warmed up first, then take turns window by
window.  Per (F, n): median and min-max of each variant in us per call, the largest |difference| of the two outputs over the output
scale, and whether the kernel's median is below torch's by more than the larger of the two spreads (max - min).  The rule:
MLP_ROWS_FROM[F] = the smallest n from which that holds at every larger measured n; None if it never does.

The backward leg (--bwd-n; what sets fused_feature.MLP_ROWS_BWD_FROM by the same rule): the weight gradients of the four tensors by
fused_feature.weight_grads_f32 routed to tpnet_mlp_rows_bwd_f32 (csrc/mlp_rows_bwd.hip: one launch + the sum of the workgroups'
partials) against _dense.layer_grads, the fp32 torch expressions, on the same tensors; the difference column is the largest
|difference| of a gradient over the largest entry of that gradient."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--F", type=int, nargs="+", default=[16, 36])
ap.add_argument("--n", type=int, nargs="+", default=[1000, 8192, 80000, 800000])
ap.add_argument("--bwd-n", type=int, nargs="*", default=[1000, 80000, 800000])
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--md", default=None)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tpnet_amd import _dense, fused_feature as ff                   # noqa: E402

if not torch.cuda.is_available():
    sys.exit("mlp_rows_rate.py measures on a GPU: none found")
dev = torch.device("cuda:0")


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.calls * 1e3


def measure(variants):
    """Median, min and max (us per call) of each variant: one untimed window each, then the variants take turns window by window."""
    for fn in variants.values():
        window(fn)
    ts = {k: [] for k in variants}
    for _ in range(args.windows):
        for k, fn in variants.items():
            ts[k].append(window(fn))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    spread = max(max(v) - min(v) for v in ts.values())
    row = dict(kernel_wins=bool(med["torch"] - med["kernel"] > spread))
    for k, v in ts.items():
        row.update({f"{k}_us": round(med[k], 2), f"{k}_min": round(min(v), 2), f"{k}_max": round(max(v), 2)})
    return row


def first_winning(rows):
    rows = sorted(rows, key=lambda r: r["n"])
    for i, r in enumerate(rows):
        if all(q["kernel_wins"] for q in rows[i:]):
            return r["n"]
    return None


results, bwd_results = [], []
with torch.no_grad():
    for F in args.F:
        ff.MLP_ROWS_FROM[F] = 0                                     # the kernel at every length
        torch.manual_seed(F)
        mlp = torch.nn.Sequential(torch.nn.Linear(F, 4 * F), torch.nn.ReLU(), torch.nn.Linear(4 * F, F)).to(dev)
        for n in args.n:
            x = torch.log1p(torch.expm1(torch.rand(n, F, device=dev, dtype=torch.float64) * 20.0)).float()
            variants = {"kernel": lambda: ff.mlp_f32(mlp, x), "torch": lambda: mlp(x)}
            y = {k: fn() for k, fn in variants.items()}
            if y["kernel"] is None:
                sys.exit(f"F={F}: tpnet_mlp_rows_f32 declined the call")
            diff = float((y["kernel"] - y["torch"]).abs().max() / max(1.0, float(y["torch"].abs().max())))
            results.append(dict(F=F, n=n, rel_diff=diff, **measure(variants)))
            print(json.dumps(results[-1]), flush=True)
        # the backward leg: weight_grads_f32 on the kernel at every length against the torch expressions
        ff.MLP_ROWS_BWD_FROM[F] = 0
        w1, b1, w2 = mlp[0].weight, mlp[0].bias, mlp[2].weight
        prep = ff.prepared(mlp, F)
        for n in args.bwd_n:
            x = torch.log1p(torch.expm1(torch.rand(n, F, device=dev, dtype=torch.float64) * 20.0)).float()
            gy = torch.randn(n, F, device=dev)
            variants = {"kernel": lambda: ff.weight_grads_f32(x, gy, w1, b1, w2, prep, "mfma"), "torch": lambda: _dense.layer_grads(x, gy, w1, b1, w2)}
            seen = ff.calls["rows_bwd"]
            g = {k: fn() for k, fn in variants.items()}
            if ff.calls["rows_bwd"] != seen + 1:
                sys.exit(f"F={F}: tpnet_mlp_rows_bwd_f32 declined the call")
            diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(g["kernel"], g["torch"]))
            bwd_results.append(dict(F=F, n=n, rel_diff=diff, **measure(variants)))
            print(json.dumps(dict(backward=bwd_results[-1])), flush=True)

rule = {F: first_winning(r for r in results if r["F"] == F) for F in args.F}
bwd_rule = {F: first_winning(r for r in bwd_results if r["F"] == F) for F in args.F}
print(json.dumps(dict(MLP_ROWS_FROM=rule, MLP_ROWS_BWD_FROM=bwd_rule)))
HEAD = ["| F | n | kernel us (min-max) | torch us (min-max) | torch / kernel | max abs diff / scale | kernel wins |", "|---|---|---|---|---|---|---|"]


def table(rows):
    return HEAD + [f"| {r['F']} | {r['n']} | {r['kernel_us']} ({r['kernel_min']}-{r['kernel_max']}) | {r['torch_us']} ({r['torch_min']}-{r['torch_max']}) | "
                   f"{r['torch_us'] / r['kernel_us']:.2f} | {r['rel_diff']:.1e} | {'yes' if r['kernel_wins'] else 'no'} |" for r in rows]


lines = table(results)
lines.append("")
lines.append(f"{args.windows} windows of {args.calls} calls per variant, alternating, on {torch.cuda.get_device_name(0)}; rule: MLP_ROWS_FROM = {rule}")
if bwd_results:
    lines += ["", "Backward (weight gradients: one launch + the sum of the partials against the fp32 torch expressions):", ""] + table(bwd_results)
    lines += ["", f"rule: MLP_ROWS_BWD_FROM = {bwd_rule}"]
print("\n".join(lines))
if args.md:
    with open(args.md, "w") as f:
        f.write("\n".join(lines) + "\n")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(results=results, MLP_ROWS_FROM=rule, backward=bwd_results, MLP_ROWS_BWD_FROM=bwd_rule), f, indent=1)
