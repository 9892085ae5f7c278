#!/usr/bin/env python3
"""Developer tool: the device neighbour sampler per strategy ('recent', 'uniform', 'time_interval_aware') at the C2 encoder shape
(Wikipedia-shape stream, n = 2 000 queries, K = 20) and at K = 128: `sample_device` as a caller pays for it, the C call alone on
preallocated outputs, the host loop it replaces (the reference's per-node searchsorted + RandomState.choice + argsort on
callers.RecentNeighborSampler's arrays), and `TPNet.compute_src_dst_node_temporal_embeddings` with the device sampler against the
same call fed by that host sampler.  Every figure: median [min .. max] over interleaved rounds of device-event (GPU calls) or
host-clock (host loop, encoder call with a synchronise) windows.  Writes a markdown report (--out)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tpnet_amd
from tpnet_amd import _lib
from tpnet_amd.callers import RecentNeighborSampler
from tpnet_amd.sampler import GpuNeighborSampler, GpuRecentNeighborSampler
from tpnet_amd.stream import CONFIGS, synthetic_stream

STRATEGIES = ("recent", "uniform", "time_interval_aware")
SCALE = 1e-6                                     # the reference's default time_scaling_factor (utils/load_configs.py)


class HostSampler(RecentNeighborSampler):
    """The reference's get_historical_neighbors loop (utils/utils.py:160-224) on the flat arrays of RecentNeighborSampler."""

    def __init__(self, src, dst, t, strategy, scale=0.0, seed=0):
        super().__init__(src, dst, t)
        self.sample_neighbor_strategy, self.seed, self.time_scaling_factor = strategy, seed, scale
        self.random_state = np.random.RandomState(seed)
        if strategy == "time_interval_aware":
            self._p = np.zeros(len(self._t))
            for nid in range(len(self._start) - 1):
                lo, hi = self._start[nid], self._start[nid + 1]
                if hi > lo:
                    with np.errstate(all="ignore"):
                        e = np.exp(scale * (self._t[lo:hi] - self._t[hi - 1]))
                        p = e / np.cumsum(e)
                    p[np.isnan(p)] = -1e10
                    self._p[lo:hi] = p

    def reset_random_state(self):
        self.random_state = np.random.RandomState(self.seed)

    def get_historical_neighbors(self, node_ids, node_interact_times, num_neighbors=20):
        if self.sample_neighbor_strategy == "recent":
            return super().get_historical_neighbors(node_ids, node_interact_times, num_neighbors)
        n, K = len(node_ids), num_neighbors
        ids, eids, ts = np.zeros((n, K), np.int64), np.zeros((n, K), np.int64), np.zeros((n, K))
        for i in range(n):
            nid = node_ids[i]
            if nid + 1 >= len(self._start):
                continue
            lo, hi = self._start[nid], self._start[nid + 1]
            m = np.searchsorted(self._t[lo:hi], node_interact_times[i])
            if m == 0:
                continue
            p = None
            if self.sample_neighbor_strategy == "time_interval_aware":
                p = torch.softmax(torch.from_numpy(self._p[lo:lo + m]).float(), dim=0).numpy()
            j = lo + self.random_state.choice(a=m, size=K, p=p)
            j = j[self._t[j].argsort()]
            ids[i], eids[i], ts[i] = self._nbr[j], self._e[j], self._t[j]
        return ids, eids, ts


def windows(fns, reps, rounds):
    """Device-event windows of `reps` calls, the functions interleaved round by round: {name: [us per call, ...]}."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / reps * 1e3)
    return out


def host_windows(fns, rounds, sync=False):
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            if sync:
                torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e6)
    return out


def fmt(xs):
    return f"{np.median(xs):.1f} [{min(xs):.1f} .. {max(xs):.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "sampler_strategies.md"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampler_rate.py measures on the GPU: none found")
    c = CONFIGS["C2"]
    B, E = c["B"], c["E"]
    src, dst, t, N = synthetic_stream(c["U"], c["I"], E, c["span"], 0)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = ["# Device neighbour sampler per strategy", "",
             f"{torch.cuda.get_device_name(0)}; C2 stream (Wikipedia shape: {N} nodes, {E} edges), queries = the last batch's [src; dst] "
             f"at tile(t, 2): n = {2 * B}; time_scaling_factor = {SCALE}.  Microseconds per call, median [min .. max] over {a.rounds} "
             f"interleaved rounds; device-event windows of {a.reps} calls unless said otherwise.  `tools/sampler_rate.py` wrote this file.", ""]
    build = {}
    gpu = {}
    for s in STRATEGIES:
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            gpu[s] = GpuRecentNeighborSampler(src, dst, t, device=dev, num_nodes=N) if s == "recent" else \
                GpuNeighborSampler(src, dst, t, device=dev, num_nodes=N, sample_neighbor_strategy=s, time_scaling_factor=SCALE, seed=1)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        build[s] = ts
    sl = slice(E - B, E)
    nodes, times = np.concatenate([src[sl], dst[sl]]), np.tile(t[sl], 2)
    dn, dt = torch.from_numpy(nodes).to(dev), torch.from_numpy(times).to(dev)
    n = 2 * B
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lines += ["## Sampler build (host clock, ms, three builds each: CSR, and the weights table of time_interval_aware)", "",
              "| strategy | build ms |", "|---|---|"] + [f"| {s} | {fmt(build[s])} |" for s in STRATEGIES] + [""]
    for K in (20, 128):
        ids = torch.empty((n, K), dtype=torch.int64, device=dev)
        eids, tt = torch.empty_like(ids), torch.empty((n, K), dtype=torch.float64, device=dev)

        def raw(s):
            g = gpu[s]
            if s == "recent":
                return lambda: lib.tpnet_sample_recent(g._buf.data_ptr(), g.E, g.num_nodes, dn.data_ptr(), dt.data_ptr(), n, K, ids.data_ptr(),
                                                       eids.data_ptr(), tt.data_ptr(), stream)
            w = g._weights.data_ptr() if g._weights is not None else None
            return lambda: lib.tpnet_sample_random(g._buf.data_ptr(), w, g.E, g.num_nodes, dn.data_ptr(), dt.data_ptr(), n, K, 1, 0,
                                                   ids.data_ptr(), eids.data_ptr(), tt.data_ptr(), stream)
        fns = {}
        for s in STRATEGIES:
            fns[s + " sample_device"] = (lambda g: lambda: g.sample_device(dn, dt, K))(gpu[s])
            fns[s + " C call"] = raw(s)
        w = windows(fns, a.reps, a.rounds)
        hosts = {s: HostSampler(src, dst, t, s, SCALE, 1) for s in STRATEGIES}
        h = host_windows({s: (lambda x: lambda: x.get_historical_neighbors(nodes, times, K))(hosts[s]) for s in STRATEGIES}, 3)
        lines += [f"## n = {n}, K = {K}", "", "| strategy | sample_device (3 outputs allocated per call) | C call, preallocated outputs | "
                  "host loop (host clock, 3 runs) |", "|---|---|---|---|"]
        lines += [f"| {s} | {fmt(w[s + ' sample_device'])} | {fmt(w[s + ' C call'])} | {fmt(h[s])} |" for s in STRATEGIES] + [""]
    # the encoder call: device sampler against the same model fed by the host loop (real widths 172 / 172 / 100, two mixer layers)
    rp = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=E, dim_factor=10, num_layer=3, time_decay_weight=c["lam"], device="cuda:0",
                                          use_matrix=False, beginning_time=np.float64(0.0), not_scale=False, enforce_dim=c["d"]).to(dev)
    D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    pre = (E - B) // B * B                        # the state before the last batch: whole batches of the stream
    rp.run_stream(D(src[:pre]), D(dst[:pre]), None, D(t[:pre]), B, want_neg=False, want_pos=False)
    rng = np.random.RandomState(2)
    model = tpnet_amd.TPNet(node_raw_features=rng.normal(0, 1, (N, 172)).astype(np.float32),
                            edge_raw_features=rng.normal(0, 1, (E + 1, 172)).astype(np.float32), neighbor_sampler=None, time_feat_dim=100,
                            dropout=0.1, random_projections=rp, num_layers=2, num_neighbors=20, device="cuda:0").to(dev).eval()

    def call(sampler):
        def fn():
            model.embedding_module.neighbor_sampler = sampler
            with torch.no_grad():
                model.compute_src_dst_node_temporal_embeddings(src[sl], dst[sl], t[sl])
        return fn
    lines += [f"## TPNet.compute_src_dst_node_temporal_embeddings, B = {B}, K = 20, d = {c['d']} (host clock around the call and a "
              "synchronise)", "", "| strategy | device sampler | host sampler | ratio of medians |", "|---|---|---|---|"]
    for s in STRATEGIES:
        fns = {"device": call(gpu[s]), "host": call(HostSampler(src, dst, t, s, SCALE, 1))}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        r = host_windows(fns, a.rounds, sync=True)
        lines.append(f"| {s} | {fmt(r['device'])} | {fmt(r['host'])} | {np.median(r['host']) / np.median(r['device']):.1f} |")
    lines += ["", "The device-event windows hold the host's enqueue as well as the kernel: a call whose kernel is shorter than its enqueue "
              "is bound by the enqueue.  Kernel times alone (a profiler's kernel trace) were not taken.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
