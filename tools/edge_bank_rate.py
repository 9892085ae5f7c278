#!/usr/bin/env python3
"""Developer tool: the device EdgeBank (tpnet_amd/edge_bank.py, csrc/edgebank.hip) per test batch of B positive and B negative pairs,
B = 200 and 1 000, in its four configurations, on a Wikipedia-shaped synthetic stream (157 474 edges, 8 227 x 1 000 nodes, a pool of
20 000 pairs, popularity by a power law, seeded): `GpuEdgeBank.predict_device` as a caller pays for it (two output tensors + the C call; nothing synchronises)
and the C call alone.  The history grows batch by batch through the last 15 % of the stream, as in the evaluation loop.  Device
figures: median [min .. max] over interleaved rounds of device-event windows, one window = `--passes` calls.  Also the table's bytes,
the launches per call and the compiler's resource usage of the kernels.  Writes a markdown report.

`--reference-dir DIR --reference-json OUT` is a mode of its own for a CPU host that has the reference checkout: it times the reference's
`edge_bank_link_prediction` (which rebuilds its memory per batch) on the same stream for `--host-batches` batches per configuration,
host clock, touches no GPU and writes OUT; the GPU run quotes OUT (`--reference-json`) in a section that names the host.  The two sets
of numbers come from different machines."""
import argparse
import ctypes as C
import json
import os
import platform
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

E, N_SRC, N_DST, N_POOL = 157474, 8227, 1000, 20000
SIZES = (200, 1000)
CONFIGS = [("unlimited_memory", "fixed_proportion"), ("time_window_memory", "fixed_proportion"), ("time_window_memory", "repeat_interval"),
           ("repeat_threshold_memory", "fixed_proportion")]
PROPORTION = 0.15
N_HISTORY = int(E * 0.85)


def stream():
    rng = np.random.RandomState(157474)
    pick = lambda n, size: np.minimum((n * rng.power(0.35, size)).astype(np.int64), n - 1)      # a few ids take most of the edges
    pool = pick(N_POOL, E)                                     # ... and a pool of pairs repeats, as the dataset's 18 257 unique edges do
    src = (1 + pick(N_SRC, N_POOL))[pool]
    dst = (1 + N_SRC + pick(N_DST, N_POOL))[pool]
    t = np.sort(rng.uniform(0.0, 2.68e6, E)).round(0)
    return src, dst, t


def negatives(rng, size):
    return 1 + rng.randint(0, N_SRC, size), 1 + N_SRC + rng.randint(0, N_DST, size)


def fmt(xs):
    return f"{np.median(xs):.1f} [{min(xs):.1f} .. {max(xs):.1f}]"


def reference_mode(a):
    sys.path.insert(0, a.reference_dir)
    from models.EdgeBank import edge_bank_link_prediction
    from utils.DataLoader import Data
    src, dst, t = stream()
    rng = np.random.RandomState(1)
    out = {"host": f"{platform.processor() or platform.machine()}, {os.cpu_count()} CPUs, Python {platform.python_version()}",
           "batches": a.host_batches, "rows": []}
    for mem, win in CONFIGS:
        for B in SIZES:
            us = []
            for b in range(a.host_batches):
                h = N_HISTORY + b * B
                hist = Data(src[:h], dst[:h], t[:h], np.arange(h), np.zeros(h))
                neg = negatives(rng, B)
                t0 = time.perf_counter()
                edge_bank_link_prediction(hist, (src[h:h + B], dst[h:h + B]), neg, mem, win, PROPORTION)
                us.append((time.perf_counter() - t0) * 1e6)
            out["rows"].append({"memory": mem, "window": win, "B": B, "us": us})
            print(mem, win, B, fmt(us))
    with open(a.reference_json, "w") as f:
        json.dump(out, f)


def kernel_resources(saved):
    if saved:
        text = open(saved).read()
    else:
        csrc = os.path.join(HERE, "tpnet_amd", "csrc")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
               "-I" + os.path.join(HERE, "include"), "-mllvm", "-amdgpu-kernarg-preload-count=16", "-Rpass-analysis=kernel-resource-usage",
               "-c", os.path.join(csrc, "edgebank.hip"), "-o", os.devnull]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    rows = []
    for block in re.split(r"remark: Function Name: ", text)[1:]:
        name = re.search(r"k_eb_[a-z]+", block.split()[0])
        val = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        if name and name.group(0) in ("k_eb_stats", "k_eb_predict"):
            rows.append((name.group(0), val("VGPRs"), val("TotalSGPRs"), val("ScratchSize [bytes/lane]"), val("VGPRs Spill"),
                         val("SGPRs Spill"), val("LDS Size [bytes/block]"), val("Occupancy [waves/SIMD]")))
    return rows


def windows(fns, rounds):
    import torch
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "edge_bank.md"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--passes", type=int, default=20, help="calls (consecutive test batches) per device-event window")
    ap.add_argument("--host-batches", type=int, default=5, help="reference mode: batches per configuration and size")
    ap.add_argument("--resources", default=None, help="saved output of hipcc -Rpass-analysis=kernel-resource-usage for edgebank.hip")
    ap.add_argument("--reference-dir", default=None, help="reference mode (CPU only): the reference checkout")
    ap.add_argument("--reference-json", default=None, help="reference mode: where to write; GPU mode: what to quote")
    a = ap.parse_args()
    if a.reference_dir:
        return reference_mode(a)
    import torch
    from tpnet_amd import _lib
    from tpnet_amd.edge_bank import GpuEdgeBank, edge_bank_host
    if not torch.cuda.is_available():
        raise SystemExit("edge_bank_rate.py measures on the GPU: none found")
    resources = kernel_resources(a.resources)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream_ptr = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    src, dst, t = stream()
    rng = np.random.RandomState(1)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(dev)
    src_d, dst_d = to(src), to(dst)
    rows, table_bytes, uniq = [], 0, 0
    for mem, win in CONFIGS:
        t0 = time.perf_counter()
        bank = GpuEdgeBank(src_d, dst_d, t, mem, win, PROPORTION, device=dev)
        build_ms = (time.perf_counter() - t0) * 1e3
        table_bytes, uniq = bank.table_bytes, bank.num_unique_edges
        for B in SIZES:
            ns, nd = (to(x) for x in negatives(rng, B * a.passes))
            out0, out1 = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
            hs = [N_HISTORY + b * B for b in range(a.passes)]

            def call():
                for b, h in enumerate(hs):
                    bank.predict_device(h, src_d[h:h + B], dst_d[h:h + B], ns[b * B:b * B + B], nd[b * B:b * B + B])

            def raw():
                for b, h in enumerate(hs):
                    lib.tpnet_edgebank_predict(bank._buf.data_ptr(), bank.E, bank._mem, bank._win, PROPORTION, h, src_d.data_ptr() + 8 * h,
                                               dst_d.data_ptr() + 8 * h, B, out0.data_ptr(), ns.data_ptr() + 8 * b * B,
                                               nd.data_ptr() + 8 * b * B, B, out1.data_ptr(), bank._scratch.data_ptr(),
                                               bank._scratch.numel(), bank._window.data_ptr(), stream_ptr)
            w = windows({"call": (call, a.passes), "raw": (raw, a.passes)}, a.rounds)
            h = hs[-1]                                         # the last batch against the host rule
            p, n = bank.predict_device(h, src_d[h:h + B], dst_d[h:h + B], ns[-B:], nd[-B:])
            want, _ = edge_bank_host(src, dst, t, h, np.concatenate([src[h:h + B], ns[-B:].cpu().numpy()]),
                                     np.concatenate([dst[h:h + B], nd[-B:].cpu().numpy()]), mem, win, PROPORTION)
            got = torch.cat([p, n]).cpu().numpy()
            launches = 2 if (mem, win) == ("time_window_memory", "repeat_interval") else 1
            rows.append(f"| {mem} / {win if mem == 'time_window_memory' else '-'} | {B} + {B} | {fmt(w['call'])} | {fmt(w['raw'])} | {launches} | "
                        f"{int((got != want).sum())} of {2 * B} (mean prediction {got[:B].mean():.2f} / {got[B:].mean():.2f}) | {build_ms:.1f} |")
    lines = ["# Device EdgeBank", "",
             f"{torch.cuda.get_device_name(0)}; a Wikipedia-shaped synthetic stream: {E} edges, {N_SRC} x {N_DST} nodes, {uniq} unique edges, "
             f"ids resident on the device; the history grows from {N_HISTORY} edges batch by batch.  One batch = B positive + B negative pairs "
             f"in ONE call.  Microseconds per batch.  Median [min .. max] over {a.rounds} interleaved rounds of device-event windows of "
             f"{a.passes} consecutive batches (host enqueue included; nothing synchronises inside a window).  `tools/edge_bank_rate.py` wrote "
             f"this file.", "",
             "## Per batch", "",
             "| memory / window mode | P + N | `predict_device` (2 output tensors + the call) | C call alone | launches per call | "
             "predictions that differ from `edge_bank_host` (last batch) | table build, ms (host clock, one sync; the first one loads the code) |",
             "|---|---|---|---|---|---|---|"] + rows + [""]
    lines += [f"The table: {table_bytes} bytes for {E} edges ({table_bytes / E:.0f} per edge, the build's sort buffers included); the scratch "
              f"buffer of a call: {lib.tpnet_edgebank_scratch_bytes(E)} bytes.  Launches: `k_eb_predict` always; `k_eb_stats` in front of it "
              "for 'repeat_interval' only.  The windows hold the host's enqueue as well as the kernels: a call whose kernels are shorter "
              "than their enqueue is bound by the enqueue.", "",
              "## Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", "",
              "| kernel | VGPRs | SGPRs | scratch bytes / lane | VGPR spills | SGPR spills | LDS bytes / workgroup | waves / SIMD |",
              "|---|---|---|---|---|---|---|---|"] + ["| " + " | ".join(str(v) for v in r) + " |" for r in resources] + [""]
    if a.reference_json and os.path.exists(a.reference_json):
        ref = json.load(open(a.reference_json))
        lines += ["## The reference's `edge_bank_link_prediction` per batch, on ANOTHER machine", "",
                  f"Host: {ref['host']} -- a CPU host with the reference checkout, not the GPU machine above; the same synthetic stream and "
                  f"history lengths, {ref['batches']} batches per row, host clock around the call (it rebuilds its memory from the whole "
                  "history per batch).  The two tables come from different machines: no ratio between them is a measured speed-up.", "",
                  "| memory / window mode | P + N | microseconds per batch |", "|---|---|---|"]
        lines += [f"| {r['memory']} / {r['window'] if r['memory'] == 'time_window_memory' else '-'} | {r['B']} + {r['B']} | {fmt(r['us'])} |"
                  for r in ref["rows"]] + [""]
    else:
        lines += ["The reference's cost per batch: not measured (no `--reference-json`).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
