#!/usr/bin/env python3
"""Developer tool: the encoder's call (models/TPNet.py:311-324, 129) at a given row width, on C2's shape (B = 1 000, K = 20: 80 000
pairs per call) and C3's (B = 10 000), every route the build under `--tree` has for it, alternated inside one process:

  anchored   get_pair_wise_feature_anchored(neigh, a1, a2) on device ids: one launch on the matrix cores where served
  dev_uv     get_pair_wise_feature(u, v) on device id tensors: general pair kernel, then self.mlp
  host_uv    get_pair_wise_feature(u, v) on host arrays, as the reference's encoder issues it (pattern recognised where served)
  wide       tpnet_anchored_features_wide on device ids, no feature buffer: the one-launch kernel for rows of 164..512 floats
             (csrc/anchored_feature.hip) whatever the default route of `anchored` is
  rows8      `anchored` with RandomProjectionModule.rows8_readout set: rows of dim % 4 == 2 (110 / 130 / 150) on the matrix cores,
             one launch (at dim % 4 == 0 the switch changes nothing)
  fallback   what TPNetEmbedding.compute_node_temporal_embeddings does where the anchored call does not serve the width: the
             u / v index lists spelled out with torch on the device, the general pair kernel, self.mlp as the torch layers
  tpnet_off / tpnet_on   one encoder-level batch: tpnet_amd.TPNet.compute_src_dst_node_temporal_embeddings (device sampler, raw
             features of 172 / 172 floats, time encoding of 100, two mixers) with rows8_readout off / on

    tools/encoder_width_rate.py --dim 110 112 --routes rows8 fallback dev_uv anchored tpnet_off tpnet_on --shapes C2
    tools/encoder_width_rate.py --dim 120 128 140 160 [--shapes C2 C3] [--reps 11] [--inner 10] [--tree OTHER_CHECKOUT] [--json OUT]

One repeat = HIP events around `inner` calls, then a synchronise; per (shape, width, route) the median and the range over the
repeats, in us per call.  `--tree` imports tpnet_amd from another (built) checkout: the same command on the parent commit gives the
A/B.  A route the build does not have at a width is listed with its error."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--dim", type=int, nargs="+", default=[120, 128, 140, 160])
ap.add_argument("--shapes", nargs="+", default=["C2", "C3"])
ap.add_argument("--K", type=int, default=20)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--routes", nargs="+", default=["anchored", "dev_uv", "host_uv"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--json", default=None)
ap.add_argument("--once", action="store_true", help="one call per (shape, width, route) and no timing: for a kernel trace")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import tpnet_amd                                                    # noqa: E402
from tpnet_amd.stream import CONFIGS, synthetic_stream             # noqa: E402

dev = torch.device("cuda:0")
D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def one_repeat(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.inner * 1e3


results = []
for cfg in args.shapes:
    c = CONFIGS[cfg]
    B, K = c["B"], args.K
    E = 6 * B
    src, dst, t, N = synthetic_stream(c["U"], c["I"], E, c["span"] * E / c["E"], 0)
    rng = np.random.RandomState(1)
    n = 2 * B
    neigh = rng.randint(1, N, (n, K)).astype(np.int64)
    a1, a2 = np.tile(src[-B:], 2), np.tile(dst[-B:], 2)
    u = np.tile(neigh.reshape(-1), 2)
    v = np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])
    neigh_d, a1_d, a2_d, u_d, v_d = D(neigh), D(a1), D(a2), D(u), D(v)
    calls, checks = {}, {}
    for d in args.dim:
        torch.manual_seed(d)
        rp = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=c["E"], dim_factor=10, num_layer=3, time_decay_weight=c["lam"],
                                              device="cuda:0", use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                              enforce_dim=d).to(dev)
        rp.run_stream(D(src), D(dst), None, D(t), B, want_neg=False, want_pos=False)
        def wide(rp=rp):
            from tpnet_amd import _lib
            prep = rp._overlapped_mlp()
            out = torch.empty((2 * n * K, 64), dtype=torch.float32, device=dev)
            _lib.check(_lib.load().tpnet_anchored_features_wide(
                rp._st_ref(), neigh_d.data_ptr(), a1_d.data_ptr(), a2_d.data_ptr(), n, K, rp._now_host, float(rp.time_decay_weight),
                rp._readout_flags(), prep.ref, None, out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                "anchored_features_wide")
            return out

        def switched(fn, rp=rp):
            def call():
                rp.rows8_readout = True
                try:
                    return fn()
                finally:
                    rp.rows8_readout = False
            return call

        def fallback(rp=rp):
            uu = neigh_d.reshape(-1).repeat(2)
            vv = torch.cat([a1_d.repeat_interleave(K), a2_d.repeat_interleave(K)])
            return rp.mlp(rp.pair_gram(uu, vv))

        def tpnet_batch(rp=rp, model=[]):
            if not model:
                from tpnet_amd.sampler import GpuRecentNeighborSampler
                g = np.random.RandomState(d)
                model.append(tpnet_amd.TPNet(node_raw_features=g.randn(N, 172).astype(np.float32),
                                             edge_raw_features=g.randn(E + 1, 172).astype(np.float32),
                                             neighbor_sampler=GpuRecentNeighborSampler(src, dst, t, device="cuda:0", num_nodes=N),
                                             time_feat_dim=100, dropout=0.1, random_projections=rp, num_layers=2, num_neighbors=K,
                                             device="cuda:0").to(dev).eval())
            es, ed = model[0].compute_src_dst_node_temporal_embeddings(src[-B:], dst[-B:], t[-B:])
            return torch.cat([es, ed])

        routes = {"anchored": lambda rp=rp: rp.get_pair_wise_feature_anchored(neigh_d, a1_d, a2_d),
                  "dev_uv": lambda rp=rp: rp.get_pair_wise_feature(u_d, v_d),
                  "host_uv": lambda rp=rp: rp.get_pair_wise_feature(u, v), "wide": wide,
                  "rows8": switched(lambda rp=rp: rp.get_pair_wise_feature_anchored(neigh_d, a1_d, a2_d)),
                  "fallback": fallback, "tpnet_off": tpnet_batch, "tpnet_on": switched(tpnet_batch)}
        refs = {}                                                   # (pair features; the tpnet_* routes: embeddings)
        for name in args.routes:
            try:
                with torch.no_grad():
                    y = routes[name]()                              # warm-up (and: does the build have this route here?)
                    torch.cuda.synchronize()
                    ref = refs.setdefault(name.startswith("tpnet"), y)
                    checks[(d, name)] = float((y - ref).abs().max() / ref.abs().max())
                calls[(d, name)] = routes[name]
            except Exception as e:                                  # noqa: BLE001
                results.append(dict(shape=cfg, d=d, route=name, pairs=int(u.size), error=f"{type(e).__name__}: {e}"[:200]))
    if args.once:
        continue
    times = {k: [] for k in calls}
    with torch.no_grad():
        for k, fn in calls.items():                                 # warmed up: one untimed repeat each
            one_repeat(fn)
        for _ in range(args.reps):                                  # the variants take turns inside the run
            for k, fn in calls.items():
                times[k].append(one_repeat(fn))
    for (d, name), ts in times.items():
        results.append(dict(shape=cfg, d=d, route=name, pairs=int(u.size), median_us=round(float(np.median(ts)), 2),
                            min_us=round(min(ts), 2), max_us=round(max(ts), 2), reps=len(ts),
                            rel_diff_to_first_route=checks[(d, name)]))
for r in results:
    print(json.dumps(r), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tree=os.path.abspath(args.tree), results=results), f, indent=1)
