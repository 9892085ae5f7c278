#!/usr/bin/env python3
"""Developer tool: what RandomProjectionModule.padded_rows costs and buys at the default rule's widths 110 / 130 / 150
(models/TPNet.py:30-33), against the same widths with the switch off and against the native neighbours 112 / 132 / 152.

One process; the variants of a leg take turns inside every repetition (other people's work shares the host: a drift hits all of
them alike); per (leg, variant) the median and the min..max over `--reps` repetitions.  Times are host clocks around work that ends
in a device synchronise.

  a  one epoch of the C2-shaped synthetic stream (stream.synthetic_stream, 157 474 edges, B = 1 000) through run_stream from a reset
     table, planned anew (`cold`, replay=False) and with the plan of the run before replayed (`replay`); ms per epoch
  b  the decoder-level drop-in loop on host arrays: 2 x get_pair_wise_feature + update per batch of 1 000; us per batch
  c  the encoder's 80 000-pair call as the reference issues it (host arrays, src = tile(neighbours, 2)); us per call.  Off: the default
     route and `rows8_readout`; on: padded
  d  the one-off cost of switching on for a live table: the wide copy of P[0] plus the import (the two launches alone, and the whole
     assignment-to-first-call path with the export and the allocation), N = 9 228 and N = 1 000 000; ms
  e  device memory of the module's table (Parameters + engine), off and on; MiB

    tools/padded_rows_rate.py [--reps 7] [--legs a b c d e] [--json OUT] [--md OUT]

The check the design allows: with the switch on, legs a-c run the kernels of the native neighbour width on the same bytes, so each
`on` median must lie inside the neighbour's own min..max (over its repetitions and its two instances: the same module built twice
lands elsewhere in memory); `within` in the output says whether it does."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--legs", nargs="+", default=["a", "b", "c", "d", "e"])
ap.add_argument("--widths", type=int, nargs="+", default=[110, 130, 150])
ap.add_argument("--loop-batches", type=int, default=60)
ap.add_argument("--json", default=None)
ap.add_argument("--md", default=None)
args = ap.parse_args()
if args.reps < 5:
    ap.error("--reps: at least five repetitions per variant")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tpnet_amd                                                    # noqa: E402
from tpnet_amd import _lib                                          # noqa: E402
from tpnet_amd.stream import CONFIGS, synthetic_stream             # noqa: E402

if not torch.cuda.is_available():
    sys.exit("padded_rows_rate.py measures on the GPU: none here")
dev = torch.device("cuda:0")
D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
c2 = CONFIGS["C2"]
B, K = c2["B"], 20
src, dst, t, N = synthetic_stream(c2["U"], c2["I"], c2["E"], c2["span"], 0)
E = len(src)
src_d, dst_d, t_d = D(src), D(dst), D(t)


def module(d, padded=False, rows8=False, n=N):
    torch.manual_seed(d)
    rp = tpnet_amd.RandomProjectionModule(node_num=n, edge_num=c2["E"], dim_factor=10, num_layer=3, time_decay_weight=c2["lam"],
                                          device="cuda:0", use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                          enforce_dim=d, alloc_device=dev)
    rp.padded_rows = padded
    rp.rows8_readout = rows8
    return rp.to(dev)


def variants(with_rows8=False):
    """{name: (width, module)}: per width off / on (/ rows8), and the native neighbour."""
    out = {}
    for d in args.widths:
        out[f"{d} off"] = module(d)
        if with_rows8:
            out[f"{d} rows8"] = module(d, rows8=True)
        out[f"{d} on"] = module(d, padded=True)
        out[f"{(d + 3) // 4 * 4} native"] = module((d + 3) // 4 * 4)
        out[f"{(d + 3) // 4 * 4} native'"] = module((d + 3) // 4 * 4)      # a second instance: what another placement in memory costs
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def take_turns(calls, before=None):
    """calls: {name: fn}.  One warm-up each, then `reps` rounds in which every variant runs once; seconds per call."""
    times = {k: [] for k in calls}
    for rep in range(args.reps + 1):
        for k, fn in calls.items():
            if before is not None:
                before(k)
            dt = timed(fn)
            if rep:
                times[k].append(dt)
    return times


results = []


def report(leg, unit, scale, times, extra=None):
    rows = {}
    for k, ts in times.items():
        ts = [x * scale for x in ts]
        rows[k] = dict(leg=leg, variant=k, unit=unit, median=round(float(np.median(ts)), 3), min=round(min(ts), 3),
                       max=round(max(ts), 3), reps=len(ts), **(extra or {}).get(k, {}))
    for k, r in rows.items():
        if k.endswith(" on"):
            w = (int(k.split()[0]) + 3) // 4 * 4
            nat = [rows[n] for n in (f"{w} native", f"{w} native'") if n in rows]
            if nat:                                 # (the native leg's spread: its repetitions, over its two instances)
                r["within"] = bool(min(x["min"] for x in nat) <= r["median"] <= max(x["max"] for x in nat))
        results.append(r)
        print(json.dumps(r), flush=True)


with torch.no_grad():
    if "a" in args.legs:
        mods = variants()
        for kind, replay in (("cold", False), ("replay", None)):
            calls, sched = {}, {}
            for k, rp in mods.items():
                calls[k] = rp.prepare_stream(src_d, dst_d, None, t_d, B, want_neg=False, t_end=float(t[-1]), schedule="auto", replay=replay)
            times = take_turns(calls, before=lambda k: mods[k].reset_random_projections())
            extra = {k: dict(schedule=mods[k].last_stream_schedule, replayed=bool(mods[k].last_stream_replayed),
                             edges_per_s=None) for k in mods}
            for k in mods:
                extra[k]["edges_per_s"] = round(E / float(np.median(times[k])) / 1e6, 1)
            report(f"a {kind}", "ms/epoch", 1e3, times, extra)
        del mods, calls

    if "b" in args.legs:
        mods = variants()
        nbt = args.loop_batches
        rng = np.random.RandomState(1)
        neg = rng.randint(c2["U"] + 1, N, nbt * B).astype(np.int64)

        def loop(rp):
            def run():
                for b in range(nbt):
                    s = slice(b * B, (b + 1) * B)
                    rp.get_pair_wise_feature(src[s], dst[s])
                    rp.get_pair_wise_feature(src[s], neg[s])
                    rp.update(src[s], dst[s], t[s])
            return run
        times = take_turns({k: loop(rp) for k, rp in mods.items()}, before=lambda k: mods[k].reset_random_projections())
        report("b", "us/batch", 1e6 / nbt, times)
        del mods

    if "c" in args.legs:
        mods = variants(with_rows8=True)
        rng = np.random.RandomState(2)
        n = 2 * B
        neigh = rng.randint(1, N, (n, K)).astype(np.int64)
        a1, a2 = np.tile(src[-B:], 2), np.tile(dst[-B:], 2)
        u = np.tile(neigh.reshape(-1), 2)
        v = np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])
        for rp in mods.values():                                   # a table with history behind it
            rp.run_stream(src_d[:20 * B], dst_d[:20 * B], None, t_d[:20 * B], B, want_pos=False, want_neg=False)
        inner = 10

        def call(rp):
            def run():
                for _ in range(inner):
                    rp.get_pair_wise_feature(u, v)
            return run
        times = take_turns({k: call(rp) for k, rp in mods.items()})
        report("c", "us/call", 1e6 / inner, times, {k: dict(pairs=int(u.size)) for k in mods})
        del mods

    if "d" in args.legs:
        lib = _lib.load()
        for n_rows in (9228, 1000000):
            for d in args.widths:
                rp = module(d, n=n_rows)
                rp.run_stream(src_d[:4 * B] % n_rows, dst_d[:4 * B] % n_rows, None, t_d[:4 * B], B, want_pos=False, want_neg=False)
                whole, kernels = [], []
                for rep in range(args.reps + 1):
                    rp.padded_rows = False
                    rp._ensure_engine()
                    rp.update(src[:B] % n_rows, dst[:B] % n_rows, t[:B] + 1e7 * (rep + 1))     # the engine holds the truth again
                    def on():
                        rp.padded_rows = True
                        rp._ensure_engine()
                        rp._st_ref()
                    dt = timed(on)
                    st, eng = rp._state(), rp._eng
                    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    def two():
                        _lib.check(lib.tpnet_pad_rows(rp._plist()[0].data_ptr(), d, eng["p0w"].data_ptr(), eng["d"], n_rows, stream), "pad_rows")
                        _lib.check(lib.tpnet_import_layers_ld(C.byref(st), rp._layer_ptrs(), d, rp._now_host, stream), "import_layers_ld")
                    rp._materialize()
                    dk = timed(two)
                    if rep:
                        whole.append(dt)
                        kernels.append(dk)
                report(f"d N={n_rows}", "ms", 1e3, {f"{d} assignment to first call": whole, f"{d} wide copy + import": kernels})
                del rp
                torch.cuda.empty_cache()

    if "e" in args.legs:
        for d in args.widths:
            for name, padded in (("off", False), ("on", True)):
                rp = module(d, padded=padded)
                rp._ensure_engine()
                rp._st_ref()
                eng = rp._eng
                b = sum(p.numel() * p.element_size() for p in rp._plist())
                b += sum(eng[k].numel() * eng[k].element_size() for k in ("q", "meta", "err") if eng[k] is not None)
                wide = eng["p0w"].numel() * 4 if eng["p0w"] is not None else 0
                r = dict(leg="e", variant=f"{d} {name}", unit="MiB", table=round((b + wide) / 2 ** 20, 2), wide_copy_of_p0=round(wide / 2 ** 20, 2))
                results.append(r)
                print(json.dumps(r), flush=True)

if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, results=results), f, indent=1)
if args.md:
    with open(args.md, "w") as f:
        f.write("| leg | variant | unit | median | min | max | notes |\n|---|---|---|---|---|---|---|\n")
        for r in results:
            notes = ", ".join(f"{k} {r[k]}" for k in ("schedule", "replayed", "edges_per_s", "within", "table", "wide_copy_of_p0") if k in r)
            f.write(f"| {r['leg']} | {r['variant']} | {r['unit']} | {r.get('median', '')} | {r.get('min', '')} | {r.get('max', '')} | {notes} |\n")
