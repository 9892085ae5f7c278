#!/usr/bin/env python3
"""Developer tool: the device link-prediction metrics (tpnet_amd/metrics.py, csrc/metrics.hip) per batch of B positive and B negative
logits, B = 200, 1 000, 10 000: `LinkPredictionMeter.add` as a caller pays for it (torch's sigmoid + tpnet_lp_metrics, nothing
synchronises) and the C call alone on scores formed beforehand, beside the reference's route on the same logits
(evaluate_models_utils.py:186-193: BCEWithLogitsLoss + `loss.item()`, `predicts.sigmoid().cpu()`, sklearn's average_precision_score
and roc_auc_score) on the host clock -- that route synchronises per batch, so a host clock around it is its time.  Without sklearn
on the machine only its copies (`loss.item()`, `.sigmoid().cpu()`) are timed, and the report says so.  Device figures: median
[min .. max] over interleaved rounds of device-event windows, one window = `--passes` calls.  Also the compiler's resource usage
of the two kernels (hipcc -Rpass-analysis=kernel-resource-usage on csrc/metrics.hip, or a saved copy of its output).  Writes a
markdown report."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tpnet_amd import _lib
from tpnet_amd.metrics import LinkPredictionMeter

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (200, 1000, 10000)


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


def kernel_resources(saved):
    """[(kernel, VGPRs, SGPRs, scratch bytes per lane, VGPR spills, SGPR spills, LDS bytes, waves per SIMD)] from the compiler's remarks."""
    if saved:
        text = open(saved).read()
    else:
        csrc = os.path.join(HERE, "tpnet_amd", "csrc")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
               "-I" + os.path.join(HERE, "include"), "-mllvm", "-amdgpu-kernarg-preload-count=16", "-Rpass-analysis=kernel-resource-usage",
               "-c", os.path.join(csrc, "metrics.hip"), "-o", os.devnull]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    rows = []
    for block in re.split(r"remark: Function Name: ", text)[1:]:
        name = re.search(r"k_lpm_[a-z]+", block.split()[0])
        val = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        if name:
            rows.append((name.group(0), val("VGPRs"), val("TotalSGPRs"), val("ScratchSize [bytes/lane]"), val("VGPRs Spill"),
                         val("SGPRs Spill"), val("LDS Size [bytes/block]"), val("Occupancy [waves/SIMD]")))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "metrics.md"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--passes", type=int, default=200, help="calls per device-event window")
    ap.add_argument("--host-batches", type=int, default=20, help="batches of the reference's route per size")
    ap.add_argument("--resources", default=None, help="saved output of hipcc -Rpass-analysis=kernel-resource-usage for metrics.hip")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_rate.py measures on the GPU: none found")
    resources = kernel_resources(a.resources)
    try:
        from sklearn.metrics import average_precision_score, roc_auc_score
    except ImportError:
        average_precision_score = roc_auc_score = None
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(1)
    loss_func = torch.nn.BCEWithLogitsLoss()
    rows = []
    for B in SIZES:
        pl = torch.randn(B, 1, device=dev, generator=gen) + 0.5
        nl = torch.randn(B, 1, device=dev, generator=gen) - 0.5
        ps, ns = torch.sigmoid(pl).reshape(-1), torch.sigmoid(nl).reshape(-1)
        meter = LinkPredictionMeter(a.passes, dev)
        nscr = lib.tpnet_lp_metrics_scratch_bytes(B, B)
        scratch = torch.empty(nscr, dtype=torch.uint8, device=dev)
        record = torch.zeros(8, dtype=torch.int64, device=dev)

        def add():
            meter.reset()
            for _ in range(a.passes):
                meter.add(pl, nl)

        def raw():
            for _ in range(a.passes):
                lib.tpnet_lp_metrics(ps.data_ptr(), B, ns.data_ptr(), B, pl.data_ptr(), nl.data_ptr(), scratch.data_ptr(), nscr,
                                     record.data_ptr(), stream)
        w = windows({"add": (add, a.passes), "raw": (raw, a.passes)}, a.rounds)
        losses, metrics = meter.results()

        def reference():
            predicts = torch.cat([pl.squeeze(-1), nl.squeeze(-1)], dim=0)
            labels = torch.cat([torch.ones_like(pl.squeeze(-1)), torch.zeros_like(nl.squeeze(-1))], dim=0)
            loss = loss_func(input=predicts, target=labels).item()
            s, y = predicts.sigmoid().cpu().numpy(), labels.cpu().numpy()
            if average_precision_score is None:
                return loss, None, None
            return loss, average_precision_score(y_true=y, y_score=s), roc_auc_score(y_true=y, y_score=s)
        reference()
        torch.cuda.synchronize()
        hs = []
        for _ in range(a.host_batches):
            h0 = time.perf_counter()
            ref = reference()
            hs.append((time.perf_counter() - h0) * 1e6)
        agree = "not compared (no sklearn)"
        if ref[1] is not None:
            agree = (f"dloss {abs(losses[0] - ref[0]):.1e} (the reference's loss is fp32), dAP {abs(metrics[0]['average_precision'] - ref[1]):.1e}, "
                     f"dAUC {abs(metrics[0]['roc_auc'] - ref[2]):.1e}")
        rows.append(f"| {B} + {B} | {fmt(w['add'])} | {fmt(w['raw'])} | {fmt(hs)} | {nscr} | {agree} |")
    ref_what = ("`BCEWithLogitsLoss(...).item()`, `predicts.sigmoid().cpu()`, `average_precision_score`, `roc_auc_score`" if average_precision_score
                else "sklearn does not import on this machine: ONLY the route's copies, `BCEWithLogitsLoss(...).item()` and `predicts.sigmoid().cpu()`")
    lines = ["# Device link-prediction metrics", "",
             f"{torch.cuda.get_device_name(0)}; one batch = B positive + B negative fp32 logits ~ N(+-0.5, 1) resident on the device.  Microseconds "
             f"per batch.  Device figures: median [min .. max] over {a.rounds} interleaved rounds of device-event windows of {a.passes} calls (host "
             f"enqueue included; nothing synchronises inside a window).  The reference's route synchronises per batch: host clock around "
             f"{a.host_batches} batches of {ref_what}.  `tools/metrics_rate.py` wrote this file.", "",
             "## Per batch", "",
             "| P + N | `meter.add` (sigmoid x 2 + 3 launches) | C call alone, scores given | the reference's route (host clock) | scratch bytes | "
             "the last record against the reference's route |", "|---|---|---|---|---|---|"] + rows + [""]
    lines += ["Launches per `tpnet_lp_metrics`: the counters' fill, the counting kernel on ceil(P / 256) x ceil((P + N) / 256) workgroups (its first "
              "row also sums the loss terms), one finish workgroup of 1024 threads.  The device-event windows hold the host's enqueue as well as the kernels: a call whose kernels "
              "are shorter than their enqueue is bound by the enqueue.  Kernel times alone are not this tool's to take: a profiler's kernel trace, in a run of its own.", "",
              "## Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", "",
              "| kernel | VGPRs | SGPRs | scratch bytes / lane | VGPR spills | SGPR spills | LDS bytes / workgroup | waves / SIMD |",
              "|---|---|---|---|---|---|---|---|"] + ["| " + " | ".join(str(v) for v in r) + " |" for r in resources] + [""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
