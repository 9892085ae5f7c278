#!/usr/bin/env python3
"""Developer tool: the tail of a training batch (train_link_prediction.py:375-386) per batch of B positive and B negative logits
that require a gradient, B = 200, 1 000, 10 000, three ways in one process:

  (a) the reference's expression: cat, BCEWithLogitsLoss, `loss.item()`, `get_link_prediction_metrics(predicts.sigmoid(), labels)`
      (`.cpu()` + the two host metrics), `loss.backward()` down to the logits.  The host metrics are sklearn's
      average_precision_score / roc_auc_score where sklearn imports, else `link_prediction_metrics_host`; the report says which.
  (b) the same without the `.item()` and metrics lines: no synchronisation, and no loss or metrics for the caller either.
  (c) `LinkPredictionMeter.add_training` + `loss.backward()`: loss, AP and AUC logged on the device, no synchronisation.

Median [min .. max] over interleaved rounds of device-event windows, one window = `--passes` batches (`tools/metrics_rate.py` times
the evaluation meter the same way); a window holds the host's work as well as the kernels, which is what a training loop pays.
Writes a markdown report with the ratios (c) / (a) and (c) / (b) of the medians."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tpnet_amd.metrics import LinkPredictionMeter, link_prediction_metrics_host

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (200, 1000, 10000)


def fmt(xs):
    return f"{np.median(xs):.1f} [{min(xs):.1f} .. {max(xs):.1f}]"


def windows(fns, rounds, n):
    """Device-event windows, the functions interleaved round by round; a function issues `n` batches: {name: [us per batch, ...]}."""
    for _ in range(2):                                           # untimed: code objects, allocator, clocks
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / n * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "train_loss.md"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--passes", type=int, default=100, help="batches per device-event window")
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("at least five rounds")
    if not torch.cuda.is_available():
        raise SystemExit("train_loss_rate.py measures on the GPU: none found")
    try:
        from sklearn.metrics import average_precision_score, roc_auc_score
        host_what = "sklearn's `average_precision_score` / `roc_auc_score`"

        def host_metrics(predicts, labels):                      # utils/metrics.py:8-22
            s, y = predicts.cpu().detach().numpy(), labels.cpu().numpy()
            return {"average_precision": average_precision_score(y_true=y, y_score=s), "roc_auc": roc_auc_score(y_true=y, y_score=s)}
    except ImportError:
        host_what = "`link_prediction_metrics_host` (sklearn does not import on this machine)"

        def host_metrics(predicts, labels):
            s, y = predicts.cpu().detach().numpy(), labels.cpu().numpy()
            r = link_prediction_metrics_host(s[y == 1], s[y != 1])
            return {"average_precision": r["ap"], "roc_auc": r["auc"]}
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    loss_func = torch.nn.BCEWithLogitsLoss()
    rows, ratios = [], []
    for B in SIZES:
        pl = (torch.randn(B, 1, device=dev, generator=gen) + 0.5).requires_grad_()
        nl = (torch.randn(B, 1, device=dev, generator=gen) - 0.5).requires_grad_()
        meter = LinkPredictionMeter(a.passes, dev)
        last = {}

        def reference(with_host):
            for _ in range(a.passes):
                pl.grad = nl.grad = None
                p, n = pl.squeeze(dim=-1), nl.squeeze(dim=-1)
                predicts = torch.cat([p, n], dim=0)
                labels = torch.cat([torch.ones_like(p), torch.zeros_like(n)], dim=0)
                loss = loss_func(input=predicts, target=labels)
                if with_host:
                    last["loss"] = loss.item()
                    last["metrics"] = host_metrics(predicts.sigmoid(), labels)
                loss.backward()
            last["grad" if with_host else "grad_b"] = pl.grad

        def device():
            meter.reset()
            for _ in range(a.passes):
                pl.grad = nl.grad = None
                meter.add_training(pl, nl).backward()
            last["grad_c"] = pl.grad

        w = windows({"a": lambda: reference(True), "b": lambda: reference(False), "c": device}, a.rounds, a.passes)
        losses, metrics = meter.results()
        dgrad = (last["grad_c"] - last["grad"]).abs().max().item() * 2 * B
        agree = (f"dloss {abs(losses[-1] - last['loss']):.1e} (the reference's loss is fp32), dAP "
                 f"{abs(metrics[-1]['average_precision'] - last['metrics']['average_precision']):.1e}, dAUC "
                 f"{abs(metrics[-1]['roc_auc'] - last['metrics']['roc_auc']):.1e}, max |dgrad| (P + N) {dgrad:.1e}")
        ma, mb, mc = (float(np.median(w[k])) for k in "abc")
        rows.append(f"| {B} + {B} | {fmt(w['a'])} | {fmt(w['b'])} | {fmt(w['c'])} | {mc / ma:.3f} | {mc / mb:.2f} | {agree} |")
        ratios.append((B, mc / ma, mc / mb))
    lines = ["# The training batch's loss on the device", "",
             f"{torch.cuda.get_device_name(0)}; one batch = B positive + B negative fp32 logits ~ N(+-0.5, 1), `[B, 1]` leaves that require a "
             f"gradient, resident on the device.  Microseconds per batch: median [min .. max] over {a.rounds} interleaved rounds of device-event "
             f"windows of {a.passes} batches, all three in one process; a window holds the host's work (enqueue, autograd, and for (a) its "
             f"synchronisations and host metrics) as well as the kernels.  `tools/train_loss_rate.py` wrote this file.", "",
             "* (a) the reference's expression (train_link_prediction.py:375-386): `cat`, `BCEWithLogitsLoss`, `loss.item()`, "
             f"`get_link_prediction_metrics(predicts.sigmoid(), labels)` with {host_what}, `loss.backward()` down to the logits.",
             "* (b) the same without the `.item()` and metrics lines: it does not synchronise, and gives the caller no loss and no metrics "
             "-- the floor of the stock route, not an alternative to (c).",
             "* (c) `LinkPredictionMeter.add_training(pos, neg)` + `loss.backward()`: two sigmoids, the fill, the counting kernel (its first "
             "row writes the gradients), the finish workgroup, and two multiplications in the backward; loss, AP and AUC are in the log.", "",
             "| P + N | (a) reference | (b) reference, no `.item()` / metrics | (c) `add_training` + `backward` | (c) / (a) | (c) / (b) | "
             "the last batch of (c) against (a) |", "|---|---|---|---|---|---|---|"] + rows + [""]
    lines += ["Ratios of the medians: " + "; ".join(f"B = {B}: (c) / (a) = {ra:.3f}, (c) / (b) = {rb:.2f}" for B, ra, rb in ratios) + ".", "",
              "Not measured here: kernel times alone (a profiler's kernel trace, in a run of its own), a whole training step around these "
              "lines, and the effect of the removed synchronisations on how far the host queues ahead in such a step.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
