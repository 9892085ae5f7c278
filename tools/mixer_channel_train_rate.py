#!/usr/bin/env python3
"""Developer tool: forward + backward of the channel-mixing half of one MLP-Mixer layer (models/TPNet.py:371-416;
x + channel_feedforward(channel_norm(x)), C = 172 channels, hidden 688) in train mode on the rows of C1, C2 and C3 (8 000 / 40 000 /
400 000 rows), alternated inside one process, at dropout p = 0.1 and p = 0:

  torch   the stock torch layers under autograd
  fused   fused_mixer.channel_train: one launch forward, two backward + the sum of the partials

    tools/mixer_channel_train_rate.py [--shapes C1 C2 C3] [--reps 9] [--inner 5] [--partials 32] [--no-call] [--json OUT]

One repeat = HIP events around `inner` x (forward, backward with respect to x and the six Parameters from a fixed gy), then a
synchronise; per (shape, p, route) the median, the range and the spread (max - min) / median over the repeats, in us per
forward + backward.  Every route is warmed up by one untimed repeat.  peak_mib: the most memory one forward + backward holds above
what was allocated before it (torch.cuda.max_memory_allocated; the fused route's figure includes the backward's workspace).
grad_err: the fused gradients against torch's at p = 0, max |difference| / max(1, max |torch|) over the seven tensors.
--partials: fused_mixer.CHANNEL_PARTIALS for this run (the row parts of the weight kernel).
Unless --no-call: a whole TPNet.compute_src_dst_node_temporal_embeddings forward + backward of embeddings.sum() at C2 (device sampler,
two mixer layers, dropout 0.1, train mode) with both training switches on against both off, timed the same way.
Kernel times: run this tool under a kernel trace, in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["C1", "C2", "C3"])
ap.add_argument("--C", type=int, default=172)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--partials", type=int, default=None)
ap.add_argument("--no-call", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tpnet_amd                                                    # noqa: E402
from tpnet_amd import fused_mixer as fm                             # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("mixer_channel_train_rate: needs a GPU")
if args.partials is not None:
    fm.CHANNEL_PARTIALS = args.partials
dev = torch.device("cuda:0")
ROWS = {"C1": 8000, "C2": 40000, "C3": 400000}


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


def measure(variants, routes, prepare):
    """{variant: (times, peak)}: warm-up and the peak of one step, then the variants take turns inside the run."""
    times, peaks = {v: [] for v in variants}, {}
    for v in variants:
        prepare(v)
        one_repeat(routes[v[-1]])
        peaks[v] = peak_mib(routes[v[-1]])
    for _ in range(args.reps):
        for v in variants:
            prepare(v)
            times[v].append(one_repeat(routes[v[-1]]))
    return times, peaks


def row(ts, **kw):
    med = float(np.median(ts))
    return dict(median_us=round(med, 1), min_us=round(min(ts), 1), max_us=round(max(ts), 1), spread=round((max(ts) - min(ts)) / med, 3),
                reps=len(ts), **kw)


results = []
for cfg in args.shapes:
    n, C = ROWS[cfg], args.C
    torch.manual_seed(1)
    mixer = tpnet_amd.MLPMixer(num_tokens=20, num_channels=C, dropout=0.1).to(dev).train()
    ffn = mixer.channel_feedforward.ffn
    params = (mixer.channel_norm.weight, mixer.channel_norm.bias, ffn[0].weight, ffn[0].bias, ffn[3].weight, ffn[3].bias)
    x = torch.randn(n, C, device=dev).requires_grad_(True)
    gy = torch.randn(n, C, device=dev)

    def set_rate(v):
        ffn[2].p = ffn[4].p = v[0]

    def torch_step():
        return torch.autograd.grad(mixer.channel_feedforward(mixer.channel_norm(x)) + x, (x,) + params, gy)

    def fused_step():
        return torch.autograd.grad(fm.channel_train(mixer, x, ffn[2].p), (x,) + params, gy)

    set_rate((0.0,))
    grad_err = max(float((a - b).abs().max() / max(1.0, float(b.abs().max()))) for a, b in zip(fused_step(), torch_step()))
    routes = {"torch": torch_step, "fused": fused_step}
    times, peaks = measure([(p, k) for p in (0.1, 0.0) for k in routes], routes, set_rate)
    for (p, k), ts in times.items():
        results.append(row(ts, shape=cfg, rows=n, p=p, route=k, partials=fm.CHANNEL_PARTIALS, peak_mib=round(peaks[(p, k)], 2),
                           grad_err=grad_err))

if not args.no_call:
    from tpnet_amd.sampler import GpuRecentNeighborSampler         # noqa: E402
    from tpnet_amd.stream import CONFIGS, synthetic_stream         # noqa: E402
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c = CONFIGS["C2"]
    B, K = c["B"], 20
    E = 6 * B
    src, dst, t, N = synthetic_stream(c["U"], c["I"], E, c["span"] * E / c["E"], 0)
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    rp = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=c["E"], dim_factor=10, num_layer=3, time_decay_weight=c["lam"],
                                          device="cuda:0", use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                          enforce_dim=c["d"]).to(dev)
    rp.run_stream(D(src[:-B]), D(dst[:-B]), None, D(t[:-B]), B, want_neg=False, want_pos=False)
    sampler = GpuRecentNeighborSampler(src, dst, t, np.arange(1, E + 1, dtype=np.int64), device="cuda:0", num_nodes=N)
    model = tpnet_amd.TPNet(node_raw_features=rng.normal(0, 1, (N, 172)).astype(np.float32),
                            edge_raw_features=rng.normal(0, 1, (E + 1, 172)).astype(np.float32), neighbor_sampler=sampler,
                            time_feat_dim=100, dropout=0.1, random_projections=rp, num_layers=2, num_neighbors=K, device="cuda:0").to(dev)
    model.train()
    emb = model.embedding_module
    bs, bd, bt = src[-B:], dst[-B:], t[-B:]

    def call():
        model.zero_grad(set_to_none=True)
        a, b = model.compute_src_dst_node_temporal_embeddings(bs, bd, bt)
        (a.sum() + b.sum()).backward()

    def switches(v):
        emb.fused_token_training = emb.fused_channel_training = v[0]

    times, peaks = measure([(False, "call"), (True, "call")], {"call": call}, switches)
    for (on, _), ts in times.items():
        results.append(row(ts, shape="C2 call", rows=2 * B * K, p=0.1, route="both switches on" if on else "both switches off",
                           partials=fm.CHANNEL_PARTIALS, peak_mib=round(peaks[(on, "call")], 2)))
for r in results:
    print(json.dumps(r), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(results=results), f, indent=1)
