#!/usr/bin/env python3
"""Developer tool: top-k link recommendation against all nodes, the logit matrix + torch.topk against the lists formed in the
scoring kernel, timed on the GPU with the variants alternating in one process after every shape has been warmed.

  variants  (a) recommend_links                     today's path: forward_one_to_all writes [B, C] logits, torch.topk reads them
            (b) recommend_links(streaming=True)     tpnet_score_topk_range: the k best kept in the scoring kernel
            (c) (b) with exclude='known'            + filter_lists_device; the exclusion cursor runs inside the kernel
            (d) ONE query, streaming=True           the latency case: units of four ids, merged by the second launch
            (d') ONE query, today's path            (d)'s baseline
            (e) tpnet_score_rank_range alone        the counting epilogue on the same shape (with its launch for the positives):
                                                    what the list epilogue costs over the counting one is (b) - (e)
  shapes    C2-shaped table (d = 128) and C3-shaped table (d = 256), B = 200 queries against all candidates: the id range [1, N)
            (profiles/rank_streaming.md's shapes); the queries are the sources of the last 200 edges of the stream
  k         10 and 100

Before a shape is timed, (b)'s values are held to (a)'s and (b)'s, (c)'s and (d)'s ids to the rule (`topk_host`) on the logits.

    tools/topk_streaming_rate.py [--reps 11] [--inner 20] [--json OUT]

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
from tpnet_amd import GpuNegativeEdgeSampler                        # noqa: E402
from tpnet_amd import score_fanout as sf                            # noqa: E402
from tpnet_amd.callers import LinkPredictor_v1, recommend_links     # noqa: E402
from tpnet_amd.stream import CONFIGS, synthetic_stream             # noqa: E402

dev = torch.device("cuda:0")
D = lambda x, dt=torch.int64: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)
results = []
B = 200
KS = (10, 100)


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
    return rp, dec, N, sampler, D(src[-B:]), D(dst[-B:])


def variants(dec, sampler, s, d, N):
    lo, hi = 1, N
    vs = {}
    for k in KS:
        vs[f"(a) logits + torch.topk, k={k}"] = lambda k=k: recommend_links(dec, s, k, (lo, hi))
        vs[f"(b) streaming, k={k}"] = lambda k=k: recommend_links(dec, s, k, (lo, hi), streaming=True)
        vs[f"(c) streaming, known, k={k}"] = lambda k=k: recommend_links(dec, s, k, (lo, hi), streaming=True, exclude="known",
                                                                          negative_sampler=sampler)
        vs[f"(d) one query, streaming, k={k}"] = lambda k=k: recommend_links(dec, s[:1], k, (lo, hi), streaming=True)
        vs[f"(d') one query, logits + torch.topk, k={k}"] = lambda k=k: recommend_links(dec, s[:1], k, (lo, hi))
    vs["(e) tpnet_score_rank_range alone"] = lambda: sf.rank_range(dec, s, d, (lo, hi))
    return vs


def check(dec, sampler, s, N, vs):
    """Held to the rule before anything is timed."""
    lo, hi = 1, N
    x = dec.forward_one_to_all(s, lo, hi).cpu().numpy()
    fil, n_fil = sampler.filter_lists_device(s, torch.full_like(s, -1), torch.zeros(len(s), dtype=torch.float64, device=dev), "known", (lo, hi))
    eq = lambda a, b: bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())
    for k in KS:
        ids_a, val_a = vs[f"(a) logits + torch.topk, k={k}"]()
        ids_b, val_b = vs[f"(b) streaming, k={k}"]()
        want = sf.topk_host(x, k, lo)
        assert torch.equal(val_a, val_b) and np.array_equal(ids_b.cpu().numpy(), want[0]), "streaming is not the logit matrix's top-k"
        ids_c, val_c = vs[f"(c) streaming, known, k={k}"]()
        want = sf.topk_host(x, k, lo, exclude_ids=fil.cpu().numpy(), n_exclude=n_fil.cpu().numpy())
        assert np.array_equal(ids_c.cpu().numpy(), want[0]) and eq(val_c.cpu().numpy(), want[1]), "the filtered top-k is not the rule's"
        ids_d, val_d = vs[f"(d) one query, streaming, k={k}"]()
        want = sf.topk_host(x[:1], k, lo)
        assert np.array_equal(ids_d.cpu().numpy(), want[0]) and eq(val_d.cpu().numpy(), want[1]), "one query: not the rule's"
    return int(n_fil.max().item()), fil.shape[1]


work = []
with torch.no_grad():
    for cfg in ("C2", "C3"):
        rp, dec, N, sampler, s, d = table(cfg)
        assert sf.serves(dec)
        name = f"{cfg}-shaped N={N} d={rp.dim} B={B} all [1, N)"
        vs = variants(dec, sampler, s, d, N)
        longest, cap = check(dec, sampler, s, N, vs)
        print(f"{name}: known lists up to {longest} ids (capacity {cap}); logit matrix {4 * B * (N - 1) / 1e6:.1f} MB", flush=True)
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
            print(f"{name:44s} {k:44s} {r['median_us']:10.1f} us  [{r['min_us']:.1f} .. {r['max_us']:.1f}]  peak {peak[k] / 1e6:8.2f} MB",
                  flush=True)

if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
