#!/usr/bin/env python3
"""Developer tool: the pieces of the one-vs-many ranking evaluation, timed on the GPU with the variants alternating in one process.

  readout   pair_gram_one_to_many (the fan-out kernel) against pair_gram on the same expanded device ids (the general pair kernel),
            as the Gram alone and with _apply_mlp behind both; C2's table (d = 128, L = 3) at (B, C) = (200, 100), (1000, 20),
            (1000, 100) and C3's (d = 256) at (1000, 100) -- tables that stay in the caches -- and on a table of --big-nodes nodes
            (d = 128, 20 GB at the default 4 M: every row of a random pair comes from HBM).  The two outputs are compared before
            they are timed.
  sampler   GpuNegativeEdgeSampler.sample_many_device per call on a Wikipedia-shaped history (C2's stream), B = 200, Q = 20 / 100
  meter     LinkRankingMeter.add against the torch expression with its .item(), logits [200, 101] and [1000, 101]
  loop      one evaluate_link_ranking pass at decoder level (decoder not_encode, the default routes): 20 batches of 200 edges, Q = 100

    tools/link_ranking_rate.py [--reps 11] [--inner 10] [--json OUT]

One repeat = HIP events around `inner` calls, then a synchronise (the meter's torch expression synchronises by itself: a host clock);
per case the median and the range over the repeats, in us per call."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--big-nodes", type=int, default=4000000, help="nodes of the HBM-resident table (20 GB at 4 M); 0: skip it")
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import tpnet_amd                                                    # noqa: E402
from tpnet_amd.callers import LinkPredictor_v1, evaluate_link_ranking, evaluate_with_restore   # noqa: E402
from tpnet_amd.stream import CONFIGS, synthetic_stream             # noqa: E402

dev = torch.device("cuda:0")
D = lambda x, dt=torch.int64: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)
results = []


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.inner * 1e3


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.inner * 1e6


def alternate(group, calls, clock=events):
    """calls: name -> function; the variants take turns inside every repeat."""
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            times[k].append(clock(fn))
    for k, v in times.items():
        r = dict(group=group, variant=k, median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), reps=len(v))
        results.append(r)
        print(f"{group:44s} {k:14s} {r['median_us']:10.1f} us  [{r['min_us']:.1f} .. {r['max_us']:.1f}]", flush=True)


def table(cfg, L=3):
    c = CONFIGS[cfg]
    E = 6 * c["B"] if cfg == "C2" else 2 * c["B"]
    src, dst, t, N = synthetic_stream(c["U"], c["I"], E, c["span"] * E / c["E"], 0)
    torch.manual_seed(c["d"])
    rp = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=c["E"], dim_factor=10, num_layer=L, time_decay_weight=c["lam"],
                                          device="cuda:0", use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                          enforce_dim=c["d"]).to(dev)
    rp.run_stream(D(src), D(dst), None, D(t, torch.float64), c["B"], want_neg=False, want_pos=False)
    rp.FANOUT_PAIRS_FROM = 0                                         # pair_gram_one_to_many = the fan-out kernel at every length
    return rp, N


# ---- readout
for cfg, shapes in (("C2", ((200, 100), (1000, 20), (1000, 100))), ("C3", ((1000, 100),))):
    rp, N = table(cfg)
    for B, C in shapes:
        rng = np.random.RandomState(B + C)
        s, cand = D(rng.randint(1, N, B)), D(rng.randint(1, N, (B, C)))
        es, ec = s.repeat_interleave(C), cand.reshape(-1)
        a, b = rp.pair_gram_one_to_many(s, cand).view(B * C, -1), rp.pair_gram(es, ec)
        worst = (a - b).abs().max().item()
        print(f"{cfg} B={B} C={C}: max |fan-out - pair_gram| = {worst:.3e} (features up to {b.abs().max().item():.2f})", flush=True)
        assert worst <= 1e-4 * max(1.0, b.abs().max().item())
        with torch.no_grad():
            alternate(f"readout {cfg} d={rp.dim} B={B} C={C} gram", {"fan-out": lambda: rp.pair_gram_one_to_many(s, cand),
                                                                      "pair_gram": lambda: rp.pair_gram(es, ec)})
            alternate(f"readout {cfg} d={rp.dim} B={B} C={C} gram+mlp", {"fan-out": lambda: rp.get_pair_wise_feature_one_to_many(s, cand),
                                                                          "pair_gram": lambda: rp._apply_mlp(rp.pair_gram(es, ec))})
    del rp

# ---- readout on a table far larger than the 256 MB Infinity Cache: every row of a random pair comes from HBM
if args.big_nodes:
    Nb = args.big_nodes
    rp = tpnet_amd.RandomProjectionModule(node_num=Nb, edge_num=10 * Nb, dim_factor=10, num_layer=3, time_decay_weight=1e-7,
                                          device="cuda:0", use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                          enforce_dim=128, alloc_device="cuda:0").to(dev)
    rp.FANOUT_PAIRS_FROM = 0
    rng = np.random.RandomState(5)
    for k in range(3):                                               # three batches of 100 000 edges: layers 1..3 are filled where touched
        rp.update(rng.randint(0, Nb, 100000), rng.randint(0, Nb, 100000), np.sort(rng.uniform(k, k + 1, 100000)) * 1e5)
    for B, C in ((1000, 100), (1000, 20), (10000, 100)):
        s, cand = D(rng.randint(0, Nb, B)), D(rng.randint(0, Nb, (B, C)))
        es, ec = s.repeat_interleave(C), cand.reshape(-1)
        a, b = rp.pair_gram_one_to_many(s, cand).view(B * C, -1), rp.pair_gram(es, ec)
        assert (a - b).abs().max().item() <= 1e-4 * max(1.0, b.abs().max().item())
        with torch.no_grad():
            alternate(f"readout N={Nb} d=128 B={B} C={C} gram", {"fan-out": lambda: rp.pair_gram_one_to_many(s, cand),
                                                                  "pair_gram": lambda: rp.pair_gram(es, ec)})
            alternate(f"readout N={Nb} d=128 B={B} C={C} gram+mlp", {"fan-out": lambda: rp.get_pair_wise_feature_one_to_many(s, cand),
                                                                      "pair_gram": lambda: rp._apply_mlp(rp.pair_gram(es, ec))})
    del rp
    torch.cuda.empty_cache()

# ---- sampler, meter, loop on C2's stream
c = CONFIGS["C2"]
E = 40000
src, dst, t, N = synthetic_stream(c["U"], c["I"], E, c["span"] * E / c["E"], 0)
smp = tpnet_amd.GpuNegativeEdgeSampler(src, dst, t, negative_sample_strategy="random", seed=1, device="cuda:0")
B = 200
q = slice(E - 4000, E - 4000 + B)
bs, bd, bt = D(src[q]), D(dst[q]), D(t[q], torch.float64)
for Q in (20, 100):
    alternate(f"sample_many_device B={B} Q={Q} (E={E})", {"device": lambda: smp.sample_many_device(bs, bd, bt, Q)})

for Bm in (200, 1000):
    x = torch.randn(Bm, 101, device=dev)
    meter = tpnet_amd.LinkRankingMeter(args.inner * (args.reps + 3) * 2 + 8, dev)

    def torch_expr():
        p, qn = x[:, :1], x[:, 1:]
        m = 2 + 2 * (qn > p).sum(1) + (qn == p).sum(1)
        mrr = (2.0 / m.double()).mean().item()
        return mrr, [(m <= 2 * k).double().mean().item() for k in (1, 3, 10)]

    def device_add():
        if len(meter) >= meter.capacity:
            meter.reset()
        meter.add(x)
    alternate(f"meter logits [{Bm}, 101]", {"meter.add": device_add}, clock=events)
    alternate(f"meter logits [{Bm}, 101] (host clock)", {"meter.add+sync": device_add, "torch+.item()": torch_expr}, clock=host_clock)

n_eval = 4000
ev = slice(E - n_eval, E)
torch.manual_seed(7)
rp = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=c["E"], dim_factor=10, num_layer=3, time_decay_weight=c["lam"],
                                      device="cuda:0", use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                      enforce_dim=c["d"]).to(dev)
rp.run_stream(D(src[:E - n_eval]), D(dst[:E - n_eval]), None, D(t[:E - n_eval], torch.float64), c["B"], want_neg=False, want_pos=False)
dec = LinkPredictor_v1(172, 172, 172, 1, rp, not_encode=True).to(dev)
smp_loop = tpnet_amd.GpuNegativeEdgeSampler(src, dst, t, negative_sample_strategy="random", seed=2, device="cuda:0")


def one_pass():
    return evaluate_with_restore(rp, lambda: evaluate_link_ranking(rp, smp_loop, src[ev], dst[ev], t[ev], 200, 100, dec))


res = one_pass()
print(f"loop: {len(res)} batches, totals {res.totals}", flush=True)
args.inner = 1
alternate(f"evaluate_link_ranking {n_eval} edges, batches of 200, Q=100 (with restore)", {"pass": one_pass}, clock=host_clock)

if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
