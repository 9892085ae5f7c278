#!/usr/bin/env python3
"""Developer tool: the device negative edge sampler ('historical', 'inductive') on a Wikipedia-shaped stream (C1: 157 474 edges), the
reference's evaluation batch of 200, calls spread over the last 30 % of the stream: `sample_device` as a caller pays for it and the C
call alone on preallocated outputs, each for the size <= M branch (size = min(200, M)) and for a forced fill (size = M + 200), beside
the host time of the reference's rule restated in numpy on the same calls (masks over the time column, np.unique / setdiff1d of edge
keys, RandomState.choice; the fill draws from |unique src| x |unique dst| by index instead of materialising the pairs).  Device
figures: median [min .. max] over interleaved rounds of device-event windows, one window = `--passes` runs through every call.  Writes a
markdown report."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tpnet_amd import _lib
from tpnet_amd.negative_sampler import GpuNegativeEdgeSampler
from tpnet_amd.stream import CONFIGS, synthetic_stream

BATCH = 200


class HostRule:
    """NegativeEdgeSampler.historical_sample / inductive_sample (utils/utils.py:420-498) on numpy arrays of edge keys."""

    def __init__(self, src, dst, t, strategy, last_observed_time, seed):
        self.keys, self.t, self.strategy = (src << 32) | dst, t, strategy
        self.us, self.ud = np.unique(src), np.unique(dst)
        self.observed = np.unique(self.keys[t <= last_observed_time]) if strategy == "inductive" else None
        self.rng = np.random.RandomState(seed)

    def candidates(self, t0, t1):
        c = np.setdiff1d(np.unique(self.keys[self.t <= t0]), np.unique(self.keys[(self.t >= t0) & (self.t <= t1)]), assume_unique=True)
        return np.setdiff1d(c, self.observed, assume_unique=True) if self.observed is not None else c

    def sample(self, size, bs, bd, t0, t1):
        c = self.candidates(t0, t1)
        if size <= len(c):
            k = c[self.rng.choice(len(c), size=size, replace=False)]
        else:
            F, nd = size - len(c), len(self.ud)
            x = self.rng.choice(len(self.us) * nd, size=F + len(bs), replace=False)        # F + B distinct pairs hold F outside the batch
            fill = (self.us[x // nd] << 32) | self.ud[x % nd]
            k = np.concatenate([fill[~np.isin(fill, (bs << 32) | bd)][:F], c])
        return k >> 32, k & 0xFFFFFFFF


def fmt(xs):
    return f"{np.median(xs):.1f} [{min(xs):.1f} .. {max(xs):.1f}]"


def windows(fns, rounds):
    """Device-event windows, the functions interleaved round by round; a function issues `n` calls: {name: [us per call, ...]}."""
    for fn, _ in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (fn, n) in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / n * 1e3)
    return out


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "profiles", "negative_sampler.md"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--passes", type=int, default=40, help="times a window runs through its calls")
    ap.add_argument("--host-calls", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("negative_sampler_rate.py measures on the GPU: none found")
    c = CONFIGS["C1"]
    E = c["E"]
    src, dst, t, N = synthetic_stream(c["U"], c["I"], E, c["span"], 0)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lot = float(t[int(0.7 * E)])                          # 'inductive': the training split's end
    starts = np.linspace(int(0.7 * E), E - BATCH, a.calls).astype(np.int64)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lines = ["# Device negative edge sampler", "",
             f"{torch.cuda.get_device_name(0)}; C1 stream (Wikipedia shape: {N} nodes, {E} edges), batches of {BATCH}, {a.calls} calls spread "
             f"over the last 30 % of the stream; 'inductive': last_observed_time = t[0.7 E].  Microseconds per call.  Device figures: median "
             f"[min .. max] over {a.rounds} interleaved rounds of device-event windows of {a.passes} x {a.calls} calls (host enqueue included).  "
             "`tools/negative_sampler_rate.py` wrote this file.", ""]
    rows, builds, nscr = [], [], 0
    for strategy in ("historical", "inductive"):
        t0 = time.perf_counter()
        smp = GpuNegativeEdgeSampler(src, dst, t, last_observed_time=lot if strategy == "inductive" else None,
                                     negative_sample_strategy=strategy, seed=1, device=dev)
        torch.cuda.synchronize()
        builds.append(f"| {strategy} | {(time.perf_counter() - t0) * 1e3:.1f} | {smp.num_unique_edges} | {len(smp.unique_src_node_ids)} x "
                      f"{len(smp.unique_dst_node_ids)} | {smp._buf.numel() / 2 ** 20:.1f} |")
        host = HostRule(src, dst, t, strategy, lot, 1)
        calls = []
        for b0 in starts:
            sl = slice(b0, b0 + BATCH)
            calls.append(dict(bs=torch.from_numpy(src[sl]).to(dev), bd=torch.from_numpy(dst[sl]).to(dev), hs=src[sl], hd=dst[sl],
                              t0=float(t[b0]), t1=float(t[b0 + BATCH - 1]), M=len(host.candidates(t[b0], t[b0 + BATCH - 1]))))
        Ms = [k["M"] for k in calls]
        out_s = torch.empty(max(Ms) + BATCH, dtype=torch.int64, device=dev)
        out_d = torch.empty_like(out_s)
        scratch = smp._scratch_for(max(Ms) + BATCH, BATCH)
        size_of = {"size <= M": lambda k: max(1, min(BATCH, k["M"])), "forced fill": lambda k: k["M"] + BATCH}
        fns = {}
        for branch, size in size_of.items():
            def device(size=size):
                for _ in range(a.passes):
                    for k in calls:
                        smp.sample_device(size(k), k["bs"], k["bd"], k["t0"], k["t1"])

            def raw(size=size):
                for _ in range(a.passes):
                    for i, k in enumerate(calls):
                        lib.tpnet_neg_sample(smp._buf.data_ptr(), smp.E, 1 if strategy == "historical" else 2, size(k), k["bs"].data_ptr(),
                                             k["bd"].data_ptr(), BATCH, k["t0"], k["t1"], 1, i, scratch.data_ptr(), scratch.numel(),
                                             out_s.data_ptr(), out_d.data_ptr(), stream)
            fns[branch + " sample_device"] = (device, a.passes * len(calls))
            fns[branch + " C call"] = (raw, a.passes * len(calls))
        w = windows(fns, a.rounds)
        for branch, size in size_of.items():
            hs = []
            for k in calls[::max(1, len(calls) // a.host_calls)]:
                h0 = time.perf_counter()
                host.sample(size(k), k["hs"], k["hd"], k["t0"], k["t1"])
                hs.append((time.perf_counter() - h0) * 1e6)
            sizes = [size(k) for k in calls]
            rows.append(f"| {strategy} | {branch} | {min(Ms)} .. {max(Ms)} | {min(sizes)} .. {max(sizes)} | {fmt(w[branch + ' sample_device'])} | "
                        f"{fmt(w[branch + ' C call'])} | {fmt(hs)} ({len(hs)} calls) |")
        nscr = max(nscr, lib.tpnet_neg_scratch_bytes(E, max(Ms) + BATCH, BATCH))
    lines += ["## Build (host clock around the constructor and a synchronise, one build each)", "",
              "| strategy | build ms | unique edges U | unique src x dst | sampler buffer MiB |", "|---|---|---|---|---|"] + builds + [""]
    lines += ["## Per call", "", "| strategy | branch | M over the calls | size over the calls | sample_device (two outputs allocated per call) | "
              "C call, preallocated outputs | host rule in numpy (host clock) |", "|---|---|---|---|---|---|---|"] + rows + [""]
    lines += [f"Launches per call: 4 (candidate flags + tile sums, scan of the tile sums, compaction, pick); a batch of more than 1 024 pairs adds "
              f"its key sort.  Scratch for the largest call here (size = max M + {BATCH}, B = {BATCH}): {nscr / 2 ** 20:.2f} MiB (tpnet_neg_scratch_bytes).  The device-event "
              "windows hold the host's enqueue as well as the kernels: a call whose kernels are shorter than their enqueue is bound by the "
              "enqueue.  Kernel times alone (a profiler's kernel trace) were not taken.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
