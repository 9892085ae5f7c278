#!/usr/bin/env python3
"""Developer tool: `optimizer.step()` of tpnet_amd.DeviceAdam / DeviceSGD / DeviceRMSprop (one launch of k_optim_step per step)
against torch.optim's own step, in ONE process.

Part 1, the step alone.  The trainable tensors of a TPNet at the reference's default widths (node / edge features 172, time encoding
100, 20 neighbours, two mixers) plus LinkPredictor_v1(172, 172, 172, 1), with resident gradients.  Per rule the variants
  device         the class of tpnet_amd/optimizer.py
  torch          torch.optim.X as utils.create_optimizer constructs it (on a GPU: the foreach implementation)
  torch_single   foreach=False
  torch_fused    Adam only: fused=True
each on its own copy of the tensors.  After a warm-up of all, the variants alternate window by window; a window is --reps steps
between two device events.  Two figures per variant, median (min .. max) over --windows windows, in us per step: `host` = the host
clock around each step() call (until it returns), `gpu` = the events' time over the window (the larger of what the host can issue and
what the GPU needs).
Part 2, a whole training step with torch's Adam and with DeviceAdam over the same Parameters, alternating windows of --batches steps
closed by a synchronise, wall clock per step:
  decoder level  C2's batch: two get_pair_wise_feature calls with a gradient, update, BCE loss, zero_grad, backward, step (rp.mlp)
  encoder level  the same batch through TPNet.compute_src_dst_node_temporal_embeddings and LinkPredictor_v1 (all 38 tensors)
Prints one JSON line per measurement.  Without a GPU it fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tpnet_amd  # noqa: E402
from tpnet_amd.callers import LinkPredictor_v1  # noqa: E402
from tpnet_amd.stream import CONFIGS, synthetic_stream  # noqa: E402

DEVICE = {"Adam": tpnet_amd.DeviceAdam, "SGD": tpnet_amd.DeviceSGD, "RMSprop": tpnet_amd.DeviceRMSprop}
TORCH = {"Adam": torch.optim.Adam, "SGD": torch.optim.SGD, "RMSprop": torch.optim.RMSprop}
LR = {"Adam": 1e-4, "SGD": 1e-4, "RMSprop": 1e-4}


def build_model(dev, K=20, d=128, batches=8):
    """-> (rp, model, decoder, src, dst, t, N, B): C2's stream, a TPNet at the default widths and its LinkPredictor_v1."""
    c = CONFIGS["C2"]
    B = c["B"]
    E = batches * B
    src, dst, t, N = synthetic_stream(c["U"], c["I"], E, c["span"] * E / c["E"], 0)
    torch.manual_seed(0)
    rp = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=c["E"], dim_factor=10, num_layer=3, time_decay_weight=c["lam"],
                                          device=str(dev), use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                          enforce_dim=d).to(dev)
    g = np.random.RandomState(0)
    sampler = tpnet_amd.GpuRecentNeighborSampler(src, dst, t, device=str(dev), num_nodes=N) if dev.type == "cuda" else None
    model = tpnet_amd.TPNet(node_raw_features=g.randn(N, 172).astype(np.float32), edge_raw_features=g.randn(E + 1, 172).astype(np.float32),
                            neighbor_sampler=sampler, time_feat_dim=100, dropout=0.1, random_projections=rp, num_layers=2,
                            num_neighbors=K, device=str(dev)).to(dev)
    dec = LinkPredictor_v1(172, 172, 172, 1, rp, False).to(dev)
    return rp, model, dec, src, dst, t, N, B


def trainable(model, dec):
    seen, out = set(), []
    for p in list(model.parameters()) + list(dec.parameters()):
        if p.requires_grad and id(p) not in seen:
            seen.add(id(p))
            out.append(p)
    return out


def stats(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def step_alone(params, a):
    shapes = [tuple(p.shape) for p in params]
    print(json.dumps({"tensors": len(params), "floats": int(sum(p.numel() for p in params)),
                      "adam_bytes_per_step": int(sum(p.numel() for p in params)) * 4 * 7}), flush=True)
    for rule in ("Adam", "SGD", "RMSprop"):
        variants = {"device": lambda ps: DEVICE[rule](ps, lr=LR[rule], weight_decay=0.0),
                    "torch": lambda ps: TORCH[rule](ps, lr=LR[rule], weight_decay=0.0),
                    "torch_single": lambda ps: TORCH[rule](ps, lr=LR[rule], weight_decay=0.0, foreach=False)}
        if rule == "Adam":
            variants["torch_fused"] = lambda ps: TORCH[rule](ps, lr=LR[rule], weight_decay=0.0, fused=True)
        opts = {}
        for name, make in variants.items():
            ps = [torch.nn.Parameter(p.detach().clone()) for p in params]
            for p in ps:
                p.grad = torch.randn_like(p) * 1e-3
            opts[name] = make(ps)
        for opt in opts.values():                                           # warm-up of every variant
            for _ in range(30):
                opt.step()
        torch.cuda.synchronize()
        host = {n: [] for n in opts}
        gpu = {n: [] for n in opts}
        for _ in range(a.windows):
            for name, opt in opts.items():                                  # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                h = 0.0
                e0.record()
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    opt.step()
                    h += time.perf_counter() - t0
                e1.record()
                torch.cuda.synchronize()
                host[name].append(h / a.reps * 1e6)
                gpu[name].append(e0.elapsed_time(e1) / a.reps * 1e3)
        print(json.dumps({"part": "step_alone", "rule": rule, "reps": a.reps, "windows": a.windows, "shapes": len(shapes),
                          "host_us": {n: stats(v) for n, v in host.items()}, "gpu_us": {n: stats(v) for n, v in gpu.items()}}), flush=True)


def whole_step(level, batch_step, params, a, reset):
    opts = {"torch": torch.optim.Adam(params, lr=1e-4), "device": tpnet_amd.DeviceAdam(params, lr=1e-4)}
    for opt in opts.values():
        reset()                                                             # (every window streams the same batches from a reset state)
        for b in range(6):
            batch_step(b, opt)
    torch.cuda.synchronize()
    times = {n: [] for n in opts}
    for _ in range(a.windows):
        for name, opt in opts.items():
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(a.batches):
                batch_step(b, opt)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.batches * 1e6)
    print(json.dumps({"part": "whole_step", "level": level, "batches": a.batches, "windows": a.windows, "tensors": len(params),
                      "us_per_step": {n: stats(v) for n, v in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--dry", action="store_true", help="build the model on the CPU, print the tensor count and stop (no timing)")
    a = ap.parse_args()
    if a.dry:
        rp, model, dec, *_ = build_model(torch.device("cpu"), batches=2)
        ps = trainable(model, dec)
        print(json.dumps({"tensors": len(ps), "floats": int(sum(p.numel() for p in ps))}))
        return
    if not torch.cuda.is_available():
        sys.exit("optimizer_rate: needs a GPU")
    dev = torch.device("cuda:0")
    rp, model, dec, src, dst, t, N, B = build_model(dev, batches=max(a.batches, 6))
    params = trainable(model, dec)
    step_alone(params, a)

    rng = np.random.RandomState(1)
    neg = rng.randint(1, N, len(src)).astype(np.int64)
    labels = torch.cat([torch.ones(B, device=dev), torch.zeros(B, device=dev)])
    lossf = torch.nn.BCEWithLogitsLoss()

    def decoder_level(b, opt):
        s = slice(b * B, (b + 1) * B)
        f1, f2 = rp.get_pair_wise_feature(src[s], dst[s]), rp.get_pair_wise_feature(src[s], neg[s])
        rp.update(src[s], dst[s], t[s])
        loss = lossf(torch.cat([f1.sum(1), f2.sum(1)]), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def encoder_level(b, opt):
        s = slice(b * B, (b + 1) * B)
        es, ed = model.compute_src_dst_node_temporal_embeddings(src[s], dst[s], t[s])
        ns, nd = model.compute_src_dst_node_temporal_embeddings(src[s], neg[s], t[s])
        pos, ng = dec(src[s], dst[s], es, ed), dec(src[s], neg[s], ns, nd)
        rp.update(src[s], dst[s], t[s])
        loss = lossf(torch.cat([pos, ng]).squeeze(1), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()

    for level, fn, ps in (("decoder", decoder_level, list(rp.mlp.parameters())), ("encoder", encoder_level, params)):
        try:
            whole_step(level, fn, ps, a, rp.reset_random_projections)
        except Exception as e:                                              # (the other measurements stand on their own)
            print(json.dumps({"part": "whole_step", "level": level, "error": f"{type(e).__name__}: {e}"}), flush=True)


if __name__ == "__main__":
    main()
