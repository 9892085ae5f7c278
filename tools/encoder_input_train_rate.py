#!/usr/bin/env python3
"""Developer tool: forward + backward of the encoder's input stage (models/TPNet.py:297-330; gathers, time encoding, concat and
projection_layer at the reference's widths 172 / 100 / 172 / 64 -> 344 -> 172) on the rows of C1, C2 and C3 (8 000 / 40 000 /
400 000 rows, K = 20), alternated inside one process:

  torch   the stock-torch expression of tools/encoder_input_rate.py under autograd
  fused   fused_input.encoder_input_train: one launch forward, two backward + the sum of the partials

    tools/encoder_input_train_rate.py [--shapes C1 C2 C3] [--reps 9] [--inner 5] [--partials 32] [--no-call] [--json OUT]

One repeat = HIP events around `inner` x (forward, backward with respect to the six Parameters and feats from a fixed gy), then a
synchronise; per (shape, route) the median, the range and the spread (max - min) / median over the repeats, in us per
forward + backward.  Every route is warmed up by one untimed repeat.  peak_mib: the most memory one forward + backward holds above
what was allocated before it (torch.cuda.max_memory_allocated; the fused route's figure includes the backward's workspace).
grad_err: the fused gradients against torch's, max |difference| / max(1, max |torch|) over the seven tensors.
--partials: fused_input.MAX_PARTIALS for this run (the row parts of the weight kernel).
Unless --no-call: a whole TPNet.compute_src_dst_node_temporal_embeddings forward + backward of embeddings.sum() at C2 (device sampler,
two mixer layers, dropout 0.1, train mode) with all three training switches on against the token and channel switches only, timed
the same way.
Kernel times: run this tool under a kernel trace, in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["C1", "C2", "C3"])
ap.add_argument("--K", type=int, default=20)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--partials", type=int, default=None)
ap.add_argument("--no-call", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tpnet_amd                                                    # noqa: E402
from tpnet_amd import fused_input as fi                             # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("encoder_input_train_rate: needs a GPU")
if args.partials is not None:
    fi.MAX_PARTIALS = args.partials
dev = torch.device("cuda:0")
ROWS = {"C1": 8000, "C2": 40000, "C3": 400000}
Dn, Dt, De, F = 172, 100, 172, 64


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


def stock_torch_stage(node_raw, edge_raw, time_w, proj, neigh, eids, tn, tq, feats):
    """tools/encoder_input_rate.py's expression: what a user writes behind encoder_pair_features in stock PyTorch."""
    n, K = neigh.shape
    node_f = node_raw[neigh]
    delta = torch.log((tq[:, None] - tn).float() + 1.0)
    time_f = torch.cos(time_w(delta.unsqueeze(2)))
    edge_f = edge_raw[eids]
    rel = torch.cat([feats[:n * K], feats[n * K:]], dim=1).reshape(n, K, -1)
    return proj(torch.cat([node_f, time_f, edge_f, rel], dim=2))


results = []
for cfg in args.shapes:
    K = args.K
    n = ROWS[cfg] // K
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    Nn, Ne = 10000, 60000
    node_raw, edge_raw = torch.randn(Nn, Dn, device=dev), torch.randn(Ne, De, device=dev)
    te = tpnet_amd.TimeEncoder(time_dim=Dt).to(dev)
    proj = torch.nn.Sequential(torch.nn.Linear(Dn + Dt + De + 2 * F, 2 * Dn), torch.nn.ReLU(), torch.nn.Linear(2 * Dn, Dn)).to(dev)
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    neigh, eids = D(rng.randint(0, Nn, (n, K)).astype(np.int64)), D(rng.randint(0, Ne, (n, K)).astype(np.int64))
    tq_h = rng.uniform(1e5, 2e6, n)
    tq, tn = D(tq_h), D(tq_h[:, None] - rng.uniform(0, 1e5, (n, K)))
    feats = torch.randn(2 * n * K, F, device=dev).requires_grad_(True)
    gy = torch.randn(n, K, Dn, device=dev)
    wrt = tuple(proj.parameters()) + (te.w.weight, te.w.bias, feats)

    def torch_step():
        return torch.autograd.grad(stock_torch_stage(node_raw, edge_raw, te.w, proj, neigh, eids, tn, tq, feats), wrt, gy)

    def fused_step():
        return torch.autograd.grad(fi.encoder_input_train(proj, te, node_raw, edge_raw, neigh, eids, tn, tq, feats), wrt, gy)

    grad_err = max(float((a - b).abs().max() / max(1.0, float(b.abs().max()))) for a, b in zip(fused_step(), torch_step()))
    routes = {"torch": torch_step, "fused": fused_step}
    times, peaks = measure([(k,) for k in routes], routes, lambda v: None)
    for (k,), ts in times.items():
        results.append(row(ts, shape=cfg, rows=n * K, route=k, partials=fi.MAX_PARTIALS, peak_mib=round(peaks[(k,)], 2), grad_err=grad_err))
    del node_raw, edge_raw, feats, gy, neigh, eids, tn, tq

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
    emb.fused_token_training = emb.fused_channel_training = True
    bs, bd, bt = src[-B:], dst[-B:], t[-B:]

    def call():
        model.zero_grad(set_to_none=True)
        a, b = model.compute_src_dst_node_temporal_embeddings(bs, bd, bt)
        (a.sum() + b.sum()).backward()

    def switches(v):
        emb.fused_input_training = v[0]

    c0 = dict(fi.calls)
    times, peaks = measure([(False, "call"), (True, "call")], {"call": call}, switches)
    served = fi.calls["backward"] - c0["backward"]
    emb.check_device_errors()
    for (on, _), ts in times.items():
        results.append(row(ts, shape="C2 call", rows=2 * B * K, route="all three switches on" if on else "token and channel switches only",
                           partials=fi.MAX_PARTIALS, peak_mib=round(peaks[(on, "call")], 2), fused_backwards=served))
for r in results:
    print(json.dumps(r), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(results=results), f, indent=1)
