"""Generates tests/golden/g14_metrics.npz (fixture G14): per case, what the reference's evaluation loop computes from a batch's logits
(evaluate_models_utils.py:186-193, utils/metrics.py:19-20) -- sklearn's `average_precision_score` and `roc_auc_score` on
`predicts.sigmoid()`, and `binary_cross_entropy_with_logits` -- on the CPU.  The loss is taken in float64 (the reference's own is
fp32; the fixture pins the formula, not fp32 rounding).

Needs scikit-learn and torch; it is run by hand, never by the tests.  The fixture holds DATA only: per case k the fp32 logits
(`pos_logit_k`, `neg_logit_k`), the fp32 scores `torch.sigmoid(logits)` (`pos_score_k`, `neg_score_k`) and, in `ap`, `auc`, `loss`,
the three float64 results; `P`, `N`, `names`.

Cases (P, N), RandomState(14).  Random logits are N(0.5, 2) for the positives and N(-0.5, 2) for the negatives, rounded to
multiples of 1 / 128 (exact in fp32: the file compresses to under 100 KB, and the larger cases hold many tied scores beside the
distinct ones):
  (1, 1), (3, 2), (200, 200), (257, 4099), (1000, 1000), (5000, 5003)   random
  (300, 300)   logits drawn from four values: heavy ties
  (64, 64)     every logit +-0.0: all scores equal
  (200, 200)   logits N(+-20, 10): the fp32 sigmoid saturates -- most positives score exactly 1 and tie, the negatives' scores go
               down to 1e-20 (an fp32 sigmoid reaches exactly 0 only below about -103)
  (150, 400)   positives N(-1.5, 1), negatives N(1.5, 1): worse than chance
In every case positive 0 has the logit +0.0 and negative 0 the logit -0.0: both score 0.5, a tie across the classes whose signed
zeros the loss has to take alike.

The sigmoid is evaluated once per DISTINCT logit: torch's CPU kernel rounds its vector body and its scalar tail differently in the
last bit, so equal logits at different positions of one tensor would get different scores and a tie would break by position.
AP and AUC depend on the scores through their order and ties alone.  In every case but the saturated one, two distinct scores lie
at least MIN_GAP_ULPS fp32 spacings apart (asserted here), so another sigmoid that is good to a few ulps -- the GPU's -- ranks
these logits the same way; where the sigmoid saturates, neighbouring logits round to equal or adjacent scores as the
implementation's last bit decides, and the ties are a property of that implementation."""
import os

import numpy as np
import torch
from sklearn.metrics import average_precision_score, roc_auc_score

HERE = os.path.dirname(os.path.abspath(__file__))
GRID = 128.0
MIN_GAP_ULPS = 8.0


def min_gap_ulps(scores):
    """Smallest gap between two distinct scores, in units of the larger one's fp32 spacing."""
    s = np.unique(scores)
    return float(np.min((s[1:] - s[:-1]) / np.spacing(s[1:]))) if len(s) > 1 else np.inf


def cases():
    rng = np.random.RandomState(14)
    grid = lambda x: np.round(x * GRID) / GRID
    out = []
    for P, N in ((1, 1), (3, 2), (200, 200), (257, 4099), (1000, 1000), (5000, 5003)):
        out.append((f"random_{P}_{N}", grid(rng.normal(0.5, 2.0, P)), grid(rng.normal(-0.5, 2.0, N))))
    levels = np.array([-1.25, 0.0, 0.75, 2.0])                                # (0.0: the +-0.0 pair below adds no fifth score)
    out.append(("four_values_300_300", levels[rng.randint(0, 4, 300)], levels[rng.randint(0, 4, 300)]))
    out.append(("all_equal_64_64", np.zeros(64), -np.zeros(64)))
    out.append(("saturated_200_200", grid(rng.normal(20.0, 10.0, 200)), grid(rng.normal(-20.0, 10.0, 200))))
    out.append(("worse_than_chance_150_400", grid(rng.normal(-1.5, 1.0, 150)), grid(rng.normal(1.5, 1.0, 400))))
    res = []
    for name, pos, neg in out:
        pos, neg = pos.astype(np.float32), neg.astype(np.float32)
        pos[0], neg[0] = np.float32(0.0), np.float32(-0.0)
        res.append((name, pos, neg))
    return res


def main():
    out = dict(names=[], P=[], N=[], ap=[], auc=[], loss=[])
    for k, (name, pos, neg) in enumerate(cases()):
        logits = torch.from_numpy(np.concatenate([pos, neg]))
        labels = torch.cat([torch.ones(len(pos)), torch.zeros(len(neg))])
        u, inv = np.unique(logits.numpy(), return_inverse=True)
        s = torch.sigmoid(torch.from_numpy(u)).numpy()[inv]                    # fp32, as the reference ranks them
        y = labels.numpy()
        if not name.startswith("saturated"):
            assert min_gap_ulps(s) >= MIN_GAP_ULPS, (name, min_gap_ulps(s))
        out["names"].append(name), out["P"].append(len(pos)), out["N"].append(len(neg))
        out["ap"].append(float(average_precision_score(y_true=y, y_score=s)))
        out["auc"].append(float(roc_auc_score(y_true=y, y_score=s)))
        out["loss"].append(float(torch.nn.functional.binary_cross_entropy_with_logits(logits.double(), labels.double())))
        out[f"pos_logit_{k}"], out[f"neg_logit_{k}"] = pos, neg
        out[f"pos_score_{k}"], out[f"neg_score_{k}"] = s[:len(pos)].copy(), s[len(pos):].copy()
        print(f"{name}: ap {out['ap'][-1]:.6f} auc {out['auc'][-1]:.6f} loss {out['loss'][-1]:.6f} "
              f"distinct scores {len(np.unique(s))} of {len(s)}")
    for key, dt in (("names", None), ("P", np.int64), ("N", np.int64), ("ap", np.float64), ("auc", np.float64), ("loss", np.float64)):
        out[key] = np.array(out[key], dtype=dt)
    path = os.path.join(HERE, "g14_metrics.npz")
    np.savez_compressed(path, **out)
    print("g14_metrics.npz:", len(out["names"]), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
