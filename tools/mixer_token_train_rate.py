#!/usr/bin/env python3
"""Developer tool: forward + backward of the token-mixing half of one MLP-Mixer layer (models/TPNet.py:371-416;
x + token_feedforward(token_norm(x^T))^T, K = 20 tokens, hidden 10, C = 172 channels) in train mode at the call sizes of C1, C2
and C3 (n = 400 / 2 000 / 20 000 nodes), alternated inside one process, at dropout p = 0.1 and p = 0:

  torch   the stock torch layers under autograd
  fused   fused_mixer.token_train: one launch forward, one backward + the sum of the partials

    tools/mixer_token_train_rate.py [--shapes C1 C2 C3] [--reps 9] [--inner 5] [--json OUT]

One repeat = HIP events around `inner` x (forward, backward with respect to x and the six Parameters from a fixed gy), then a
synchronise; per (shape, p, route) the median, the range and the spread (max - min) / median over the repeats, in us per
forward + backward.  Every route is warmed up by one untimed repeat.  peak_mib: the most memory one forward + backward holds above
what was allocated before it (torch.cuda.max_memory_allocated).  grad_err: the fused gradients against torch's at p = 0,
max |difference| / max(1, max |torch|) over the seven tensors."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["C1", "C2", "C3"])
ap.add_argument("--K", type=int, default=20)
ap.add_argument("--C", type=int, default=172)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tpnet_amd                                                    # noqa: E402
from tpnet_amd import fused_mixer as fm                             # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("mixer_token_train_rate: needs a GPU")
dev = torch.device("cuda:0")
NODES = {"C1": 400, "C2": 2000, "C3": 20000}


def one_repeat(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.inner * 1e3


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


results = []
for cfg in args.shapes:
    n, K, C = NODES[cfg], args.K, args.C
    torch.manual_seed(1)
    mixer = tpnet_amd.MLPMixer(num_tokens=K, num_channels=C, dropout=0.1).to(dev).train()
    ffn = mixer.token_feedforward.ffn
    params = (mixer.token_norm.weight, mixer.token_norm.bias, ffn[0].weight, ffn[0].bias, ffn[3].weight, ffn[3].bias)
    x = torch.randn(n, K, C, device=dev).requires_grad_(True)
    gy = torch.randn(n, K, C, device=dev)

    def set_rate(p):
        ffn[2].p = ffn[4].p = p

    def torch_step():
        y = mixer.token_feedforward(mixer.token_norm(x.permute(0, 2, 1))).permute(0, 2, 1) + x
        return torch.autograd.grad(y, (x,) + params, gy)

    def fused_step():
        return torch.autograd.grad(fm.token_train(mixer, x, ffn[2].p), (x,) + params, gy)

    set_rate(0.0)
    grad_err = max(float((a - b).abs().max() / max(1.0, float(b.abs().max()))) for a, b in zip(fused_step(), torch_step()))
    routes = {"torch": torch_step, "fused": fused_step}
    variants = [(p, k) for p in (0.1, 0.0) for k in routes]
    times = {v: [] for v in variants}
    peaks = {}
    for p, k in variants:                                           # warm-up, then the peak of one step
        set_rate(p)
        one_repeat(routes[k])
        peaks[(p, k)] = peak_mib(routes[k])
    for _ in range(args.reps):                                      # the variants take turns inside the run
        for p, k in variants:
            set_rate(p)
            times[(p, k)].append(one_repeat(routes[k]))
    for (p, k), ts in times.items():
        med = float(np.median(ts))
        results.append(dict(shape=cfg, nodes=n, columns=n * C, p=p, route=k, median_us=round(med, 1), min_us=round(min(ts), 1),
                            max_us=round(max(ts), 1), spread=round((max(ts) - min(ts)) / med, 3), reps=len(ts),
                            peak_mib=round(peaks[(p, k)], 2), grad_err=grad_err))
for r in results:
    print(json.dumps(r), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(results=results), f, indent=1)
