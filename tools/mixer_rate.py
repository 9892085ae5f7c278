#!/usr/bin/env python3
"""Developer tool: one MLP-Mixer layer (models/TPNet.py:371-416) at the call sizes of C2, C1 and C3 (2 B nodes, K = 20 tokens,
C = 172 channels -> token hidden 10, channel hidden 688), alternated inside one process:

  torch_layer    tpnet_amd.MLPMixer.forward: the stock torch layers
  fused_layer    fused_mixer.mixer_forward: two launches
  fused_token    ... its token kernel alone
  fused_channel  ... its channel kernel alone (on the token kernel's output)
  torch_call     TPNet.compute_src_dst_node_temporal_embeddings under no_grad with fused_mixer = False (device sampler, readout, the
                 one-launch input stage, two torch mixers, mean)
  fused_call     the same call with fused_mixer = True (fused_input = True in both)

    tools/mixer_rate.py [--shapes C2 C1 C3] [--reps 9] [--inner 5] [--json OUT]

One repeat = HIP events around `inner` calls, then a synchronise; per (shape, variant) the median, the range and the spread
(max - min) / median over the repeats, in us per call.  Every variant is warmed up by one untimed repeat.  layer_err / call_err:
the fused result against torch's, max |difference| / max(1, max |torch|)."""
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
from tpnet_amd import fused_mixer as fm                             # noqa: E402
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


def scaled_err(got, want):
    return float((got - want).abs().max() / max(1.0, float(want.abs().max())))


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
    emb.fused_input = True
    bs, bd, bt = src[-B:], dst[-B:], t[-B:]
    mixer = emb.mlp_mixers[0]
    with torch.no_grad():
        # the first mixer's real input: the projection's output of this call
        rec = {}
        hook = emb.projection_layer.register_forward_hook(lambda m, a, o: rec.__setitem__("x", o.detach()))
        emb.fused_input = False
        model.compute_src_dst_node_temporal_embeddings(bs, bd, bt)
        emb.fused_input = True
        hook.remove()
        x = rec["x"].contiguous()
        prep = fm.prepared(mixer)
        tok = fm.mixer_token(mixer, x)

        def whole(fused):
            emb.fused_mixer = fused
            return model.compute_src_dst_node_temporal_embeddings(bs, bd, bt)

        calls = {
            "torch_layer": lambda: mixer(x),
            "fused_layer": lambda: fm.mixer_forward(prep, mixer, x),
            "fused_token": lambda: fm.mixer_token(mixer, x),
            "fused_channel": lambda: fm.mixer_channel(prep, mixer, tok),
            "torch_call": lambda: whole(False),
            "fused_call": lambda: whole(True),
        }
        layer_err = scaled_err(calls["fused_layer"](), calls["torch_layer"]())
        call_err = scaled_err(torch.cat(calls["fused_call"]()), torch.cat(calls["torch_call"]()))
        emb.check_device_errors()
        times = {k: [] for k in calls}
        for fn in calls.values():
            one_repeat(fn)
        for _ in range(args.reps):                                  # the variants take turns inside the run
            for k, fn in calls.items():
                times[k].append(one_repeat(fn))
        emb.fused_mixer = False
    for k, ts in times.items():
        med = float(np.median(ts))
        results.append(dict(shape=cfg, nodes=int(x.shape[0]), rows=int(x.shape[0] * K), variant=k, median_us=round(med, 1),
                            min_us=round(min(ts), 1), max_us=round(max(ts), 1), spread=round((max(ts) - min(ts)) / med, 3),
                            reps=len(ts), layer_err=layer_err, call_err=call_err))
for r in results:
    print(json.dumps(r), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(results=results), f, indent=1)
