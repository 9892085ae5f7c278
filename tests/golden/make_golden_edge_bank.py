"""Generates tests/golden/g15_edge_bank.npz (fixture G15): the reference's own `edge_bank_link_prediction` (models/EdgeBank.py) on a
toy stream, CPU.

Runs only where the read-only reference checkout is present (TPNET_REFERENCE, default /root/reference); the fixture holds DATA only.
The window start (the threshold, for 'repeat_threshold_memory') is the reference's own local variable, read from the frame of its
function when it returns -- nothing of the rule is restated here.

Graph: RandomState(15), E = 400 edges drawn from a pool of 90 distinct pairs of 15 source nodes (1..15) x 25 destination nodes
(16..40); integer stamps sort(randint(0, 80, 400)) as float64 -- five edges per stamp on average, so prefixes end inside runs of tied
stamps.

Block 1, per configuration c (CONFIGS) and recorded prefix h (h = 1..39, then every 7th, then E): a 60-pair query list --
the 20 stream edges from position h - 1 on (the first is the last history edge, the rest are future edges, some never seen before,
some stamped t[h - 1]; clipped at the stream's end), then 40 uniform pairs over sources 0..17 x destinations 14..43 (ids that occur
nowhere among them) --, the reference's predictions for it and its window start.  A 'repeat_interval' prefix is recorded only if it
holds no repeated edge (S = 0 in any order) or no stamp within 1e-6 of the reference's window start (a prediction cannot hang on the
order of a float64 sum); the generator prints how many it dropped and refuses to drop more than 5 %.

Block 2, the evaluation loop (evaluate_models_utils.py:269-318): history = the first 250 edges, test = the last 150, batches of 25;
explicit negatives, half of them pairs of the stream; per configuration the reference's per-batch predictions, `nn.BCELoss` on float64
tensors (the formula, not fp32 rounding) and `get_link_prediction_metrics`."""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("TPNET_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.modules.setdefault("wandb", types.ModuleType("wandb"))      # utils/metrics.py imports it for its logger class only

import models.EdgeBank as EB  # noqa: E402
from utils.DataLoader import Data  # noqa: E402
from utils.metrics import get_link_prediction_metrics  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
E, NQ_STREAM, NQ_UNIFORM = 400, 20, 40
N_HISTORY, BATCH = 250, 25
CONFIGS = [("unlimited_memory", "fixed_proportion", 0.15), ("time_window_memory", "fixed_proportion", 0.15),
           ("time_window_memory", "repeat_interval", 0.15), ("repeat_threshold_memory", "fixed_proportion", 0.15)]
PREFIXES = list(range(1, 40)) + list(range(46, E, 7)) + [E]


def graph():
    rng = np.random.RandomState(15)
    pool = rng.permutation(15 * 25)[:90]
    pick = pool[rng.randint(0, 90, E)]
    src = (pick // 25 + 1).astype(np.int64)
    dst = (pick % 25 + 16).astype(np.int64)
    t = np.sort(rng.randint(0, 80, E)).astype(np.float64)
    return src, dst, t


def reference(src, dst, t, h, pos, neg, config):
    """-> (positive predictions, negative predictions, the reference's window start / threshold or nan)."""
    seen = {}

    def tracer(frame, event, arg):
        if frame.f_code.co_name not in ("edge_bank_time_window_memory", "edge_bank_repeat_threshold_memory"):
            return None

        def local(frame, event, arg):
            if event == "return":
                loc = frame.f_locals
                seen["bound"] = float(loc["time_window_start_time"] if "time_window_start_time" in loc else loc["threshold"])
            return local
        return local

    data = Data(src_node_ids=src[:h], dst_node_ids=dst[:h], node_interact_times=t[:h], edge_ids=np.arange(1, h + 1),
                labels=np.zeros(h))
    sys.settrace(tracer)
    try:
        p, n = EB.edge_bank_link_prediction(history_data=data, positive_edges=pos, negative_edges=neg, edge_bank_memory_mode=config[0],
                                            time_window_mode=config[1], time_window_proportion=config[2])
    finally:
        sys.settrace(None)
    return np.asarray(p, dtype=np.float64), np.asarray(n, dtype=np.float64), seen.get("bound", float("nan"))


def main():
    src, dst, t = graph()
    rng = np.random.RandomState(1515)
    out = dict(src=src, dst=dst, t=t, config_memory=np.array([c[0] for c in CONFIGS]), config_window=np.array([c[1] for c in CONFIGS]),
               config_proportion=np.array([c[2] for c in CONFIGS]), n_stream_queries=NQ_STREAM)

    # ---- block 1: prefixes
    queries = {}
    for h in PREFIXES:
        at = np.minimum(h - 1 + np.arange(NQ_STREAM), E - 1)
        queries[h] = (np.concatenate([src[at], rng.randint(0, 18, NQ_UNIFORM)]).astype(np.int64),
                      np.concatenate([dst[at], rng.randint(14, 44, NQ_UNIFORM)]).astype(np.int64))
    for c, config in enumerate(CONFIGS):
        hs, qs, qd, pred, bound = [], [], [], [], []
        dropped = 0
        for h in PREFIXES:
            q = queries[h]
            p, _, b = reference(src, dst, t, h, q, (q[0][:0], q[1][:0]), config)
            if config[1] == "repeat_interval":
                repeated = len(set(zip(src[:h], dst[:h]))) < h
                if repeated and np.min(np.abs(t[:h] - b)) <= 1e-6:
                    dropped += 1
                    continue
                assert repeated or b == t[h - 1]
            hs.append(h), qs.append(q[0]), qd.append(q[1]), pred.append(p), bound.append(b)
        pred = np.stack(pred)
        if config[1] == "repeat_interval":
            print(f"repeat_interval: dropped {dropped} of {len(PREFIXES)} prefixes (a stamp within 1e-6 of the window start)")
            assert dropped <= 0.05 * len(PREFIXES)
        for part in (pred[:, :NQ_STREAM], pred[:, NQ_STREAM:]):           # both outcomes among the stream's pairs and the uniform ones
            assert part.min() == 0.0 and part.max() == 1.0, config
        out.update({f"h_{c}": np.array(hs, dtype=np.int64), f"query_src_{c}": np.stack(qs), f"query_dst_{c}": np.stack(qd),
                    f"pred_{c}": pred, f"bound_{c}": np.array(bound)})
        print(config, len(hs), "prefixes, mean prediction", pred.mean())

    # ---- block 2: the evaluation loop
    ts, td = src[N_HISTORY:], dst[N_HISTORY:]
    n_test = E - N_HISTORY
    neg_src, neg_dst = rng.randint(1, 16, n_test).astype(np.int64), rng.randint(16, 41, n_test).astype(np.int64)
    own = rng.permutation(n_test)[:n_test // 2]                           # half of the negatives: pairs of the stream itself
    at = rng.randint(0, E, len(own))
    neg_src[own], neg_dst[own] = src[at], dst[at]
    out.update(n_history=N_HISTORY, batch=BATCH, neg_src=neg_src, neg_dst=neg_dst)
    loss_func = torch.nn.BCELoss()
    for c, config in enumerate(CONFIGS):
        pp, nn, losses, aps, aucs = [], [], [], [], []
        for b0 in range(0, n_test, BATCH):
            s = slice(b0, b0 + BATCH)
            p, n, _ = reference(src, dst, t, N_HISTORY + b0, (ts[s], td[s]), (neg_src[s], neg_dst[s]), config)
            predicts = torch.from_numpy(np.concatenate([p, n]))           # float64: the formula, not fp32 rounding
            labels = torch.cat([torch.ones(len(p), dtype=torch.float64), torch.zeros(len(n), dtype=torch.float64)])
            losses.append(float(loss_func(input=predicts, target=labels)))
            m = get_link_prediction_metrics(predicts=predicts, labels=labels)
            pp.append(p), nn.append(n), aps.append(m["average_precision"]), aucs.append(m["roc_auc"])
        pp, nn = np.stack(pp), np.stack(nn)
        for part in (pp, nn):
            assert part.min() == 0.0 and part.max() == 1.0, config
        out.update({f"loop_pos_{c}": pp, f"loop_neg_{c}": nn, f"loop_loss_{c}": np.array(losses), f"loop_ap_{c}": np.array(aps),
                    f"loop_auc_{c}": np.array(aucs)})
        print(config, "loop: loss", np.round(losses, 3), "ap", np.round(aps, 3))
    path = os.path.join(HERE, "g15_edge_bank.npz")
    np.savez_compressed(path, **out)
    print("g15_edge_bank.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
