#!/usr/bin/env python3
"""Developer tool: the encoder's readout (models/TPNet.py:311-324) at num_layer 1, 2 and 4 with RandomProjectionModule.layers_readout
on and off, alternated inside one process:

  layers   the switch on: pair_gram_anchored on the matrix cores (csrc/encoder_layers.hip)
  walk     the switch off: the vector-ALU anchored walk (the route without the switch)

each as the Gram alone (pair_gram_anchored on device ids) and with self.mlp behind it (get_pair_wise_feature_anchored), on C2's
80 000-pair call (2 000 rows x K = 20 x 2 anchors) at d = 128 and d = 120, and on 800 000 pairs at d = 128.

    tools/encoder_layers_rate.py [--layers 1 2 4] [--reps 11] [--inner 10] [--json OUT]
    tools/encoder_layers_rate.py --once          # one call per case and no timing: for a kernel trace

One repeat = HIP events around `inner` calls, then a synchronise; per case the median and the range over the repeats, in us per
call."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, nargs="+", default=[1, 2, 4])
ap.add_argument("--cases", nargs="+", default=["2000x128", "2000x120", "20000x128"], help="ROWSxDIM")
ap.add_argument("--K", type=int, default=20)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--json", default=None)
ap.add_argument("--once", action="store_true", help="one call per case and no timing: for a kernel trace")
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


c = CONFIGS["C2"]
B, K = c["B"], args.K
E = 6 * B
src, dst, t, N = synthetic_stream(c["U"], c["I"], E, c["span"] * E / c["E"], 0)
results = []
for case in args.cases:
    n, d = (int(x) for x in case.split("x"))
    rng = np.random.RandomState(1)
    neigh_d = D(rng.randint(1, N, (n, K)).astype(np.int64))
    a1_d, a2_d = D(rng.randint(1, N, n).astype(np.int64)), D(rng.randint(1, N, n).astype(np.int64))
    calls, checks = {}, {}
    for L in args.layers:
        torch.manual_seed(d + L)
        rp = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=c["E"], dim_factor=10, num_layer=L, time_decay_weight=c["lam"],
                                              device="cuda:0", use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                              enforce_dim=d).to(dev)
        rp.run_stream(D(src), D(dst), None, D(t), B, want_neg=False, want_pos=False)

        def route(on, with_mlp, rp=rp):
            def call():
                rp.layers_readout = on
                if with_mlp:
                    return rp.get_pair_wise_feature_anchored(neigh_d, a1_d, a2_d)
                return rp.pair_gram_anchored(neigh_d, a1_d, a2_d)
            return call
        for with_mlp in (False, True):
            ref = None
            for name, on in (("walk", False), ("layers", True)):
                key = (L, "gram+mlp" if with_mlp else "gram", name)
                with torch.no_grad():
                    y = route(on, with_mlp)()
                    torch.cuda.synchronize()
                ref = y if ref is None else ref
                checks[key] = float((y - ref).abs().max() / ref.abs().max())
                calls[key] = route(on, with_mlp)
    if args.once:
        continue
    times = {k: [] for k in calls}
    with torch.no_grad():
        for k, fn in calls.items():                                 # warmed up: one untimed repeat each
            one_repeat(fn)
        for _ in range(args.reps):                                  # the variants take turns inside the run
            for k, fn in calls.items():
                times[k].append(one_repeat(fn))
    for (L, what, name), ts in times.items():
        results.append(dict(rows=n, d=d, L=L, what=what, route=name, pairs=2 * n * K, median_us=round(float(np.median(ts)), 2),
                            min_us=round(min(ts), 2), max_us=round(max(ts), 2), reps=len(ts), rel_diff_to_walk=checks[(L, what, name)]))
for r in results:
    print(json.dumps(r), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tree=os.path.abspath(args.tree), results=results), f, indent=1)
