#!/usr/bin/env python3
"""Developer tool: the encoder's input stage (models/TPNet.py:297-330) at the call sizes of C2, C1 and C3 (2 B K rows, K = 20) and
the reference's real widths 172 / 100 / 172 / 64 -> 344 -> 172, alternated inside one process:

  torch_stage   what a user without the encoder module writes behind encoder_pair_features in stock PyTorch: two index gathers,
                cos(Linear), two cats and two nn.Linear (written out below -- not project code)
  fused_stage   fused_input.encoder_input: one launch, the concat never written
  torch_call    TPNet.compute_src_dst_node_temporal_embeddings under no_grad with fused_input = False (device sampler, readout,
                torch input stage, two mixers, mean)
  fused_call    the same call with fused_input = True

    tools/encoder_input_rate.py [--shapes C2 C1 C3] [--reps 9] [--inner 5] [--json OUT]

One repeat = HIP events around `inner` calls, then a synchronise; per (shape, variant) the median, the range and the spread
(max - min) / median over the repeats, in us per call.  Every variant is warmed up by one untimed repeat."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["C2", "C1", "C3"])
ap.add_argument("--K", type=int, default=20)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tpnet_amd                                                    # noqa: E402
from tpnet_amd import fused_input as fi                             # noqa: E402
from tpnet_amd.sampler import GpuRecentNeighborSampler             # noqa: E402
from tpnet_amd.stream import CONFIGS, synthetic_stream             # noqa: E402

dev = torch.device("cuda:0")
D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
Dn, Dt, De = 172, 100, 172


def one_repeat(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.inner * 1e3


def stock_torch_stage(node_raw, edge_raw, time_w, proj, neigh, eids, tn, tq, feats):
    """The user's own expression at the parent commit, given encoder_pair_features' [4BK, F] output."""
    n, K = neigh.shape
    node_f = node_raw[neigh]
    delta = torch.log((tq[:, None] - tn).float() + 1.0)
    time_f = torch.cos(time_w(delta.unsqueeze(2)))
    edge_f = edge_raw[eids]
    rel = torch.cat([feats[:n * K], feats[n * K:]], dim=1).reshape(n, K, -1)
    return proj(torch.cat([node_f, time_f, edge_f, rel], dim=2))


results = []
for cfg in args.shapes:
    c = CONFIGS[cfg]
    B, K = c["B"], args.K
    E = 6 * B
    src, dst, t, N = synthetic_stream(c["U"], c["I"], E, c["span"] * E / c["E"], 0)
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    rp = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=c["E"], dim_factor=10, num_layer=3, time_decay_weight=c["lam"],
                                          device="cuda:0", use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                          enforce_dim=c["d"]).to(dev)
    rp.run_stream(D(src[:-B]), D(dst[:-B]), None, D(t[:-B]), B, want_neg=False, want_pos=False)
    sampler = GpuRecentNeighborSampler(src, dst, t, np.arange(1, E + 1, dtype=np.int64), device="cuda:0", num_nodes=N)
    model = tpnet_amd.TPNet(node_raw_features=rng.normal(0, 1, (N, Dn)).astype(np.float32),
                            edge_raw_features=rng.normal(0, 1, (E + 1, De)).astype(np.float32), neighbor_sampler=sampler,
                            time_feat_dim=Dt, dropout=0.1, random_projections=rp, num_layers=2, num_neighbors=K, device="cuda:0").to(dev)
    model.eval()
    emb = model.embedding_module
    bs, bd, bt = src[-B:], dst[-B:], t[-B:]
    with torch.no_grad():
        tq = D(np.tile(bt, 2))
        neigh, eids, tn = sampler.sample_device(D(np.concatenate([bs, bd])), tq, K, with_edges=True)
        feats = rp.get_pair_wise_feature_anchored(neigh, np.tile(bs, 2), np.tile(bd, 2))
        prep = fi.prepared(emb.projection_layer, Dn, Dt, De, rp.pair_wise_feature_dim)
        w = model.time_encoder.w

        def whole(fused):
            emb.fused_input = fused
            return model.compute_src_dst_node_temporal_embeddings(bs, bd, bt)

        calls = {
            "torch_stage": lambda: stock_torch_stage(model.node_raw_features, model.edge_raw_features, w, emb.projection_layer, neigh,
                                                     eids, tn, tq, feats),
            "fused_stage": lambda: fi.encoder_input(prep, model.node_raw_features, model.edge_raw_features, neigh, eids, tn, tq,
                                                    w.weight, w.bias, feats),
            "torch_call": lambda: whole(False),
            "fused_call": lambda: whole(True),
        }
        a, b = calls["torch_stage"](), calls["fused_stage"]()
        stage_err = float((a - b).abs().max() / max(1.0, float(a.abs().max())))
        ea, eb = torch.cat(calls["torch_call"]()), torch.cat(calls["fused_call"]())
        call_err = float((ea - eb).abs().max() / max(1.0, float(ea.abs().max())))
        emb.check_device_errors()
        times = {k: [] for k in calls}
        for fn in calls.values():
            one_repeat(fn)
        for _ in range(args.reps):                                  # the variants take turns inside the run
            for k, fn in calls.items():
                times[k].append(one_repeat(fn))
    for k, ts in times.items():
        med = float(np.median(ts))
        results.append(dict(shape=cfg, rows=int(neigh.numel()), variant=k, median_us=round(med, 1), min_us=round(min(ts), 1),
                            max_us=round(max(ts), 1), spread=round((max(ts) - min(ts)) / med, 3), reps=len(ts),
                            stage_err=stage_err, call_err=call_err))
for r in results:
    print(json.dumps(r), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(results=results), f, indent=1)
