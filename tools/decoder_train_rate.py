#!/usr/bin/env python3
"""Developer tool: LinkPredictor_v1 (172 + 172 + 64 -> 172 -> 1, the reference's default sizes) under autograd, `fused = "f32"`
(tpnet_decoder_f32 / tpnet_decoder_f32_bwd) against `fused = False` (the torch layers) in ONE process.

Per n in 200, 1 000, 10 000: forward + backward with the gradient taken with respect to the four Parameters and the three inputs, and the
no_grad forward.  The two sides alternate, window by window, after a warm-up of both; a window is --reps calls between two device
events, a figure is the median over --windows windows with the spread (min .. max).  Peak memory is torch's allocator peak above
what was allocated before the call, per side.  --profile N runs N plain forward + backward steps of ONE side at n = --n and nothing else:
the program to put behind `rocprofv3 --kernel-trace --stats --` (launches per step = calls of a kernel / N).
Without a GPU it fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tpnet_amd import fused_decoder as fd  # noqa: E402
from tpnet_amd.callers import LinkPredictor_v1  # noqa: E402

D, F, H = 172, 64, 172


class Feat(torch.nn.Module):
    pair_wise_feature_dim = F

    def __init__(self, n, dev):
        super().__init__()
        self.f = torch.nn.Parameter(torch.rand(n, F, device=dev) * 3)

    def get_pair_wise_feature(self, src_node_ids, dst_node_ids):
        return self.f[: len(src_node_ids)]


def setup(n, dev):
    torch.manual_seed(n)
    dec = LinkPredictor_v1(D, D, H, 1, Feat(n, dev), False).to(dev)
    src = torch.randn(n, D, device=dev, requires_grad=True)
    dst = torch.randn(n, D, device=dev, requires_grad=True)
    g = torch.randn(n, 1, device=dev) / n
    wrt = [dec.fc1.weight, dec.fc1.bias, dec.fc2.weight, dec.fc2.bias, src, dst, dec.random_projections.f]
    return dec, src, dst, g, wrt, np.arange(n)


def step(dec, ids, src, dst, g, wrt):
    return torch.autograd.grad(dec(ids, ids, src, dst), wrt, g)


def infer(dec, ids, src, dst):
    with torch.no_grad():
        return dec(ids, ids, src, dst)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3                                 # us per call


def peak(fn, dev):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated(dev) - base
    del out
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--side", choices=("f32", "torch"), default="f32")
    ap.add_argument("--n", type=int, default=1000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decoder_train_rate: needs a GPU")
    dev = torch.device("cuda:0")
    if a.profile:
        dec, src, dst, g, wrt, ids = setup(a.n, dev)
        dec.fused = "f32" if a.side == "f32" else False
        for _ in range(a.profile):
            step(dec, ids, src, dst, g, wrt)
        torch.cuda.synchronize()
        print(json.dumps({"profile": a.side, "n": a.n, "steps": a.profile, "calls": fd.calls}))
        return
    for n in (200, 1000, 10000):
        dec, src, dst, g, wrt, ids = setup(n, dev)
        sides = {"f32": "f32", "torch": False}

        def run(side, what):
            dec.fused = sides[side]
            return step(dec, ids, src, dst, g, wrt) if what == "train" else infer(dec, ids, src, dst)

        rec = {"n": n, "reps": a.reps, "windows": a.windows}
        for what in ("train", "no_grad"):
            for side in sides:                                              # warm-up of both sides, this shape
                for _ in range(20):
                    run(side, what)
            times = {s: [] for s in sides}
            for _ in range(a.windows):
                for side in sides:                                          # alternating
                    times[side].append(window(lambda: run(side, what), a.reps))
            for side in sides:
                t = times[side]
                rec[f"{what}_{side}_us"] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
                rec[f"{what}_{side}_peak_bytes"] = peak(lambda: run(side, what), dev)
        got, want = run("f32", "no_grad"), run("torch", "no_grad")
        rec["max_logit_diff_over_scale"] = float((got - want).abs().max() / want.abs().max())
        print(json.dumps(rec), flush=True)
    print(json.dumps({"calls": fd.calls}))


if __name__ == "__main__":
    main()
