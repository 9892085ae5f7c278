#!/usr/bin/env python3
"""Developer tool: one batch of the all-node ranking evaluation, the logit matrix against the streaming counts, timed on the GPU with
the variants alternating in one process after every shape has been warmed.

  variants  (a) forward_one_to_all + add_skip      the [B, 1 + C] logits are written, then read to be counted
            (b) rank_one_to_all + add_counts       the counts are formed in the scoring kernel, unfiltered
            (c) (b) with filter 'same_time'        + filter_lists_device and one list-mode score call for the lists
            (d) (b) with filter 'known'
  shapes    C2-shaped table (d = 128) and C3-shaped table (d = 256), B = 200 queries against all candidates: the id range [1, N)
            (profiles/score_fanout.md's shapes); the queries are the last 200 edges of the stream the sampler is built on

Before a shape is timed, (b)'s record is held to (a)'s bit for bit.

    tools/rank_streaming_rate.py [--reps 11] [--inner 20] [--json OUT]

One sample = HIP events around `inner` calls, then a synchronise; per case the median and the range over the samples, in us per call,
and the peak of torch.cuda.max_memory_allocated above what was allocated before the variant ran."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import tpnet_amd                                                    # noqa: E402
from tpnet_amd import GpuNegativeEdgeSampler, LinkRankingMeter     # noqa: E402
from tpnet_amd import score_fanout as sf                            # noqa: E402
from tpnet_amd.callers import LinkPredictor_v1                      # noqa: E402
from tpnet_amd.stream import CONFIGS, synthetic_stream             # noqa: E402

dev = torch.device("cuda:0")
D = lambda x, dt=torch.int64: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)
results = []
B = 200


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.inner * 1e3


def table(cfg):
    c = CONFIGS[cfg]
    E = 6 * c["B"] if cfg == "C2" else 2 * c["B"]
    src, dst, t, N = synthetic_stream(c["U"], c["I"], E, c["span"] * E / c["E"], 0)
    torch.manual_seed(c["d"])
    rp = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=c["E"], dim_factor=10, num_layer=3, time_decay_weight=c["lam"],
                                          device="cuda:0", use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                          enforce_dim=c["d"]).to(dev)
    rp.run_stream(D(src), D(dst), None, D(t, torch.float64), c["B"], want_neg=False, want_pos=False)
    dec = LinkPredictor_v1(172, 172, 172, 1, rp, not_encode=True).to(dev)
    sampler = GpuNegativeEdgeSampler(src, dst, t, negative_sample_strategy="random", seed=1, device=dev)
    return rp, dec, N, sampler, (D(src[-B:]), D(dst[-B:]), D(t[-B:], torch.float64))


def variants(dec, sampler, q, N):
    s, d, t = q
    lo, hi = 1, N
    meter = LinkRankingMeter(1, dev)

    def a():
        meter.reset()
        x = dec.forward_one_to_all(s, lo, hi, lead_node_ids=d)
        meter.add_skip(x, torch.where((d >= lo) & (d < hi), d - lo, torch.full_like(d, -1)))

    def streaming(mode):
        def run():
            meter.reset()
            fil = n_fil = None
            if mode is not None:
                fil, n_fil = sampler.filter_lists_device(s, d, t, mode, (lo, hi))
            counts, p, fl = dec.rank_one_to_all(s, d, lo, hi, filter_ids=fil)
            meter.add_counts(counts, p, fl, fil, n_fil)
        return run
    return meter, {"(a) logits + add_skip": a, "(b) streaming": streaming(None), "(c) streaming same_time": streaming("same_time"),
                   "(d) streaming known": streaming("known")}


work = []
with torch.no_grad():
    for cfg in ("C2", "C3"):
        rp, dec, N, sampler, q = table(cfg)
        assert sf.serves(dec)
        name = f"{cfg}-shaped N={N} d={rp.dim} B={B} all [1, N)"
        meter, vs = variants(dec, sampler, q, N)
        # ---- checked and warmed before anything is timed
        vs["(a) logits + add_skip"]()
        rec_a = meter.records()[0].copy()
        vs["(b) streaming"]()
        assert np.array_equal(meter.records()[0], rec_a), "the streaming record is not the logit matrix's"
        print(f"{name}: filter capacities same_time {sampler.filter_capacity('same_time')}, known {sampler.filter_capacity('known')}; "
              f"logit matrix {4 * B * N / 1e6:.1f} MB", flush=True)
        for fn in vs.values():
            for _ in range(3):
                fn()
        work.append((name, vs))
    torch.cuda.synchronize()
    for name, vs in work:
        times = {k: [] for k in vs}
        peak = {}
        for _ in range(args.reps):
            for k, fn in vs.items():
                times[k].append(events(fn))
        for k, fn in vs.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
        for k, v in times.items():
            r = dict(group=name, variant=k, median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), reps=len(v),
                     inner=args.inner, peak_bytes=int(peak[k]))
            results.append(r)
            print(f"{name:44s} {k:26s} {r['median_us']:10.1f} us  [{r['min_us']:.1f} .. {r['max_us']:.1f}]  peak {peak[k] / 1e6:8.2f} MB",
                  flush=True)

if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
