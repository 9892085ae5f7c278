"""Link-prediction metrics (tpnet_amd/metrics.py, csrc/metrics.hip: tpnet_lp_metrics) against fixture G14
(tests/golden/make_golden_metrics.py: sklearn's average_precision_score / roc_auc_score and float64 binary_cross_entropy_with_logits
per case) and against the numpy restatement of the rule, `link_prediction_metrics_host`.

The rule (include/tpnet_hip.h): per positive i, a_i = #{p_j >= p_i}, b_i = #{q_k >= p_i}, c_i = #{q_k == p_i};
AP = mean a_i / (a_i + b_i), U2 = sum (2 (N - b_i) + c_i), AUC = U2 / (2 P N).

Bounds: |dAP|, |dAUC| <= 1e-10 and |dloss| <= 1e-12 max(1, loss).  Both sides sum at most 2^18 terms of [0, 1] in float64: the worst
rounding is 2 * 2^18 * 2^-53 ~ 6e-11.  The integers (U2, sizes, flags) are compared for equality, and the device's AUC bit for bit
with U2 / (2 P N)."""
import ctypes as C
import math
import os
import warnings

import numpy as np
import pytest
import torch

from tpnet_amd.metrics import (FLAG_NAN_SCORE, FLAG_ONE_CLASS, LinkPredictionMeter, get_link_prediction_metrics,
                               link_prediction_metrics_host)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AP_TOL = 1e-10
CASES = [(1, 1), (3, 2), (200, 200), (257, 4099), (1000, 1000), (5000, 5003), (300, 300), (64, 64), (200, 200), (150, 400)]
SATURATED = 8                 # the case whose fp32 sigmoid saturates: its ties belong to the sigmoid that made them (see the generator)

_cache = {}


def g14():
    """Fixture G14 and, per case, the host function's fields: loaded and computed once, never written."""
    if "g" not in _cache:
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g14_metrics.npz")))
        _cache["g"] = g
        _cache["host"] = [link_prediction_metrics_host(g[f"pos_score_{k}"], g[f"neg_score_{k}"], g[f"pos_logit_{k}"], g[f"neg_logit_{k}"])
                          for k in range(len(g["names"]))]
    return _cache["g"], _cache["host"]


def loss_tol(loss):
    return 1e-12 * max(1.0, abs(loss))


def same(x, y):
    """Equal floats, NaN equal to NaN."""
    return x == y or (math.isnan(x) and math.isnan(y))


# ------------------------------------------------------------------------------------------------------------------- CPU

def test_fixture_holds_the_cases():
    g, _ = g14()
    assert [(int(p), int(n)) for p, n in zip(g["P"], g["N"])] == CASES
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g14_metrics.npz")) < 100_000
    for k, (P, N) in enumerate(CASES):
        pl, nl, ps, ns = (g[f"{a}_{k}"] for a in ("pos_logit", "neg_logit", "pos_score", "neg_score"))
        assert pl.dtype == ps.dtype == np.float32 and pl.shape == ps.shape == (P,) and nl.shape == ns.shape == (N,)
        assert pl[0] == 0 and not np.signbit(pl[0]) and nl[0] == 0 and np.signbit(nl[0])           # the +-0.0 pair
        assert ps[0] == ns[0] == np.float32(0.5)
        x, s = np.concatenate([pl, nl]), np.unique(np.concatenate([ps, ns]))
        assert len(s) == len(np.unique(x)) or k == SATURATED                   # equal logits have equal scores, distinct ones distinct
        if k != SATURATED and len(s) > 1:                                      # ... and no two scores are within rounding of each other
            assert np.min((s[1:] - s[:-1]) / np.spacing(s[1:])) >= 8.0
    assert len(np.unique(np.concatenate([g["pos_score_6"], g["neg_score_6"]]))) == 4              # heavy ties
    assert len(np.unique(np.concatenate([g["pos_score_7"], g["neg_score_7"]]))) == 1              # all equal
    assert (g["pos_score_8"] == 1).sum() > 50 and g["neg_score_8"].min() < 1e-12                  # the fp32 sigmoid saturated
    assert g["auc"][9] < 0.1                                                                      # worse than chance


@pytest.mark.parametrize("k", range(len(CASES)))
def test_host_rule_against_g14(k):
    g, host = g14()
    r = host[k]
    print(g["names"][k], "dAP", abs(r["ap"] - g["ap"][k]), "dAUC", abs(r["auc"] - g["auc"][k]), "dloss", abs(r["loss"] - g["loss"][k]))
    assert abs(r["ap"] - g["ap"][k]) <= AP_TOL and abs(r["auc"] - g["auc"][k]) <= AP_TOL
    assert abs(r["loss"] - g["loss"][k]) <= loss_tol(g["loss"][k])
    assert (r["n_pos"], r["n_neg"], r["flags"]) == (CASES[k][0], CASES[k][1], 0)
    assert r["auc"] == r["u2"] / (2 * r["n_pos"] * r["n_neg"])


def test_host_rule_against_sklearn():
    """Random batches straight against the two sklearn calls of utils/metrics.py: distinct scores, heavy ties, saturated fp32
    sigmoids, worse-than-chance scores, signed zeros."""
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.RandomState(5)
    worst = 0.0
    for trial in range(60):
        P, N = int(rng.randint(1, 300)), int(rng.randint(1, 300))
        kind = trial % 4
        if kind == 0:
            s = rng.uniform(0, 1, P + N)
        elif kind == 1:
            s = rng.randint(0, 1 + trial % 7, P + N) / 8.0 * rng.choice([1.0, -1.0], P + N)       # few values, -0.0 among them
        elif kind == 2:
            s = torch.sigmoid(torch.from_numpy(rng.normal(0, 25, P + N).astype(np.float32))).numpy()
        else:
            s = np.concatenate([rng.normal(-1, 1, P), rng.normal(1, 1, N)])
        s = s.astype(np.float32)
        y = np.concatenate([np.ones(P), np.zeros(N)])
        r = link_prediction_metrics_host(s[:P], s[P:])
        d_ap = abs(r["ap"] - sk.average_precision_score(y_true=y, y_score=s))
        d_auc = abs(r["auc"] - sk.roc_auc_score(y_true=y, y_score=s))
        worst = max(worst, d_ap, d_auc)
        assert d_ap <= AP_TOL and d_auc <= AP_TOL, (trial, P, N)
        assert math.isnan(r["loss"])
    print("largest difference to sklearn:", worst)


def test_host_rule_on_degenerate_batches():
    p = np.array([0.25, 0.75, 0.5], dtype=np.float32)
    x = np.array([-1.0, 1.0, 0.0], dtype=np.float32)
    want_loss = float(np.mean(np.log1p(np.exp(-x.astype(np.float64)))))                           # all labels 1: softplus(-x)
    r = link_prediction_metrics_host(p, [], x, None)                                               # N = 0
    assert r["flags"] == FLAG_ONE_CLASS and math.isnan(r["ap"]) and math.isnan(r["auc"]) and r["u2"] == 0
    assert (r["n_pos"], r["n_neg"]) == (3, 0) and abs(r["loss"] - want_loss) <= loss_tol(want_loss)
    r = link_prediction_metrics_host([], p, None, x)                                               # P = 0
    assert r["flags"] == FLAG_ONE_CLASS and math.isnan(r["ap"]) and math.isnan(r["auc"]) and r["u2"] == 0
    assert abs(r["loss"] - float(np.mean(np.log1p(np.exp(x.astype(np.float64)))))) <= 1e-12
    r = link_prediction_metrics_host([], [])
    assert r["flags"] == FLAG_ONE_CLASS and math.isnan(r["loss"])
    r = link_prediction_metrics_host([0.5, np.nan], [0.25, 0.5, 0.75])                             # a NaN positive: counted nowhere
    assert r["flags"] == FLAG_NAN_SCORE and math.isnan(r["ap"]) and math.isnan(r["auc"])
    assert r["u2"] == (2 * 1 + 1) + 2 * 3                                    # 0.5: one negative below, one tied; NaN: b = c = 0
    r = link_prediction_metrics_host([0.5], [np.nan, 0.25])
    assert r["flags"] == FLAG_NAN_SCORE and r["u2"] == 2 * 2                 # the NaN negative is never at or above anything
    r = link_prediction_metrics_host([np.nan], [])
    assert r["flags"] == FLAG_ONE_CLASS | FLAG_NAN_SCORE
    r = link_prediction_metrics_host([0.0, -0.0], [-0.0, 0.0, 1.0])                                # signed zeros tie
    assert r["flags"] == 0 and r["u2"] == 2 * 2 and r["auc"] == 4 / 12 and abs(r["ap"] - 2 / 5) <= 1e-15


def test_get_link_prediction_metrics_on_cpu_tensors():
    """The reference's signature and dict, labels interleaved (not positives first)."""
    g, _ = g14()
    for k in (1, 2, 6, 8):
        P, N = CASES[k]
        rng = np.random.RandomState(k)
        order = rng.permutation(P + N)
        s = np.concatenate([g[f"pos_score_{k}"], g[f"neg_score_{k}"]])[order]
        y = np.concatenate([np.ones(P, dtype=np.float32), np.zeros(N, dtype=np.float32)])[order]
        for predicts, labels in ((torch.from_numpy(s), torch.from_numpy(y)), (s, y)):
            m = get_link_prediction_metrics(predicts=predicts, labels=labels)
            assert sorted(m) == ["average_precision", "roc_auc"] and all(type(v) is float for v in m.values())
            assert abs(m["average_precision"] - g["ap"][k]) <= AP_TOL and abs(m["roc_auc"] - g["auc"][k]) <= AP_TOL


def test_too_many_scores_are_refused_without_a_launch(hip_lib):
    """P + N = 2^18 + 1: TPNET_ERR_BAD_ARG before anything touches a device -- so this holds on a machine without one."""
    big = (1 << 18) + 1
    assert hip_lib.tpnet_lp_metrics_scratch_bytes(big - 1, 1) == 0 and hip_lib.tpnet_lp_metrics_scratch_bytes(-1, 4) == 0
    assert hip_lib.tpnet_lp_metrics_scratch_bytes(1 << 17, 1 << 17) >= 3 * 4 * (1 << 17)
    assert hip_lib.tpnet_lp_metrics(8, big - 1, 8, 1, None, None, 8, 1 << 30, 8, None) == -1
    assert hip_lib.tpnet_lp_metrics(8, 1, 8, big - 1, None, None, 8, 1 << 30, 8, None) == -1
    assert hip_lib.tpnet_lp_metrics(8, -1, 8, 4, None, None, 8, 1 << 30, 8, None) == -1
    assert hip_lib.tpnet_lp_metrics(None, 4, 8, 4, None, None, 8, 1 << 30, 8, None) == -1         # a missing score array
    assert hip_lib.tpnet_lp_metrics(8, 4, 8, 4, None, None, 8, 1 << 30, None, None) == -1         # no record
    assert hip_lib.tpnet_lp_metrics(8, 4, 8, 4, None, None, 8, 16, 8, None) == -2                 # scratch too small


# ------------------------------------------------------------------------------------------------------------------- GPU

def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to("cuda:0")


def _abi_record(pos, neg, pos_logit=None, neg_logit=None, runs=1):
    """tpnet_lp_metrics through ctypes -> (status, [record bytes per run]); every run on a scratch buffer filled with ones (the call
    must zero what it counts in)."""
    from tpnet_amd import _lib
    lib = _lib.load()
    ps, ns = _dev(pos), _dev(neg)
    pl = _dev(pos_logit) if pos_logit is not None else None
    nl = _dev(neg_logit) if neg_logit is not None else None
    ptr = lambda v: v.data_ptr() if v is not None and v.numel() else None
    nbytes = lib.tpnet_lp_metrics_scratch_bytes(ps.numel(), ns.numel())
    assert nbytes >= 12 * ps.numel()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []
    for _ in range(runs):
        scratch = torch.full((nbytes,), 1, dtype=torch.uint8, device="cuda:0")
        record = torch.full((8,), -1, dtype=torch.int64, device="cuda:0")
        rc = lib.tpnet_lp_metrics(ptr(ps), ps.numel(), ptr(ns), ns.numel(), ptr(pl), ptr(nl), scratch.data_ptr(), nbytes,
                                  record.data_ptr(), stream)
        if rc != 0:
            return rc, out
        out.append(record.cpu().numpy().tobytes())
    return 0, out


def _fields(raw):
    f, i = np.frombuffer(raw, dtype=np.float64), np.frombuffer(raw, dtype=np.int64)
    return {"loss": float(f[0]), "ap": float(f[1]), "auc": float(f[2]), "u2": int(i[3]), "n_pos": int(i[4]), "n_neg": int(i[5]),
            "flags": int(i[6]), "reserved": int(i[7])}


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)))
def test_device_record_against_host_rule_and_g14(k):
    """Through the C ABI: the integers equal the host rule's, AUC is U2 / (2 P N) bit for bit, AP and loss are within the bounds of
    the fixture; a second run of the same call gives the same 64 bytes."""
    _need_gpu()
    g, host = g14()
    rc, raws = _abi_record(g[f"pos_score_{k}"], g[f"neg_score_{k}"], g[f"pos_logit_{k}"], g[f"neg_logit_{k}"], runs=2)
    assert rc == 0
    r, h = _fields(raws[0]), host[k]
    print(g["names"][k], "dAP", abs(r["ap"] - g["ap"][k]), "dAUC", abs(r["auc"] - g["auc"][k]), "dloss", abs(r["loss"] - g["loss"][k]))
    assert (r["u2"], r["n_pos"], r["n_neg"], r["flags"], r["reserved"]) == (h["u2"], h["n_pos"], h["n_neg"], h["flags"], 0)
    assert r["auc"] == r["u2"] / (2 * r["n_pos"] * r["n_neg"])
    assert abs(r["ap"] - g["ap"][k]) <= AP_TOL and abs(r["auc"] - g["auc"][k]) <= AP_TOL
    assert abs(r["loss"] - g["loss"][k]) <= loss_tol(g["loss"][k])
    assert raws[1] == raws[0]


@pytest.mark.gpu
def test_device_record_without_logits_and_on_degenerate_batches():
    _need_gpu()
    g, host = g14()
    rc, raws = _abi_record(g["pos_score_3"], g["neg_score_3"])                                     # NULL logits: no loss
    r = _fields(raws[0])
    assert rc == 0 and math.isnan(r["loss"]) and r["u2"] == host[3]["u2"] and abs(r["ap"] - g["ap"][3]) <= AP_TOL
    rc, raws = _abi_record(g["pos_score_3"], g["neg_score_3"], g["pos_logit_3"], None)             # one side's logits only: no loss
    assert rc == 0 and math.isnan(_fields(raws[0])["loss"])
    p = np.array([0.25, 0.75, 0.5], dtype=np.float32)
    x = np.array([-1.0, 1.0, 0.0], dtype=np.float32)
    nan = np.float32("nan")
    for pos, neg, pl, nl in ((p, [], x, None), ([], p, None, x), ([], [], None, None), ([0.5, nan], [0.25, 0.5, 0.75], None, None),
                             ([0.5], [nan, 0.25], [0.5], [0.25, -2.0]), ([nan], [], None, None),
                             ([0.0, -0.0], [-0.0, 0.0, 1.0], None, None)):
        rc, raws = _abi_record(pos, neg, pl, nl, runs=2)
        assert rc == 0                                                                             # reported, not refused
        r, h = _fields(raws[0]), link_prediction_metrics_host(pos, neg, pl, nl)
        assert (r["u2"], r["n_pos"], r["n_neg"], r["flags"]) == (h["u2"], h["n_pos"], h["n_neg"], h["flags"]), (pos, neg)
        assert same(r["auc"], h["auc"]) and (same(r["ap"], h["ap"]) or abs(r["ap"] - h["ap"]) <= AP_TOL)
        assert same(r["loss"], h["loss"]) or abs(r["loss"] - h["loss"]) <= loss_tol(h["loss"])
        if h["flags"]:
            assert math.isnan(r["ap"]) and math.isnan(r["auc"])
        assert raws[1] == raws[0]


@pytest.mark.gpu
def test_device_refuses_too_many_scores():
    _need_gpu()
    from tpnet_amd import _lib
    lib = _lib.load()
    big = (1 << 18) + 1
    s = torch.zeros(big, dtype=torch.float32, device="cuda:0")
    record = torch.full((8,), -1, dtype=torch.int64, device="cuda:0")
    scratch = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.tpnet_lp_metrics(s.data_ptr(), big - 1, s.data_ptr(), 1, None, None, scratch.data_ptr(), scratch.numel(), record.data_ptr(),
                              stream)
    assert rc == -1
    assert (record.cpu() == -1).all()                                                              # nothing was launched
    meter = LinkPredictionMeter(1, "cuda:0")
    with pytest.raises(_lib.TPNetHipError):
        meter.add(s[:big - 1], s[:1])
    assert len(meter) == 0


@pytest.mark.gpu
def test_meter_logs_every_case_and_reads_once():
    """G14's cases into one meter, one results() call.  The meter ranks the device's own sigmoid of the logits, so each record is
    held to the host rule on exactly those scores (integers and AUC equal, AP and loss to the bounds), and to the fixture's values:
    the loss always, AP and AUC wherever the ranking cannot hang on a sigmoid's last bit -- every case but the saturated one, whose
    ties differ between two correct sigmoids (CPU and GPU) by construction."""
    _need_gpu()
    g, _ = g14()
    meter = LinkPredictionMeter(len(CASES), "cuda:0")
    logits = [(_dev(g[f"pos_logit_{k}"]), _dev(g[f"neg_logit_{k}"])) for k in range(len(CASES))]
    shapes = [(-1,), (-1, 1), (1, -1)]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")              # a synchronising torch call inside add() would raise
    try:
        for k, (pl, nl) in enumerate(logits):
            assert meter.add(pl.reshape(shapes[k % 3]), nl.reshape(shapes[(k + 1) % 3])) == k
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert len(meter) == len(CASES)
    with pytest.raises(IndexError):
        meter.add(*logits[0])
    res = meter.results()
    losses, metrics = res
    assert len(res) == 2 and len(losses) == len(metrics) == len(CASES) and res.flags == [0] * len(CASES)
    rec = meter.records()
    for k, (pl, nl) in enumerate(logits):
        ps, ns = torch.sigmoid(pl).cpu().numpy(), torch.sigmoid(nl).cpu().numpy()
        moved = int((ps != g[f"pos_score_{k}"]).sum() + (ns != g[f"neg_score_{k}"]).sum())
        h = link_prediction_metrics_host(ps, ns, g[f"pos_logit_{k}"], g[f"neg_logit_{k}"])
        ap, auc = metrics[k]["average_precision"], metrics[k]["roc_auc"]
        print(g["names"][k], "device sigmoid differs from the fixture's in", moved, "scores; dAP", abs(ap - g["ap"][k]), "dAUC",
              abs(auc - g["auc"][k]), "dloss", abs(losses[k] - g["loss"][k]))
        assert (int(rec[k, 3]), int(rec[k, 4]), int(rec[k, 5])) == (h["u2"], h["n_pos"], h["n_neg"])
        assert auc == h["auc"] and abs(ap - h["ap"]) <= AP_TOL and abs(losses[k] - h["loss"]) <= loss_tol(h["loss"])
        assert abs(losses[k] - g["loss"][k]) <= loss_tol(g["loss"][k])
        if k != SATURATED:                               # distinct scores are >= 8 fp32 spacings apart: any sigmoid ranks them alike
            assert abs(ap - g["ap"][k]) <= AP_TOL and abs(auc - g["auc"][k]) <= AP_TOL
    meter.reset()
    assert len(meter) == 0 and meter.results() == ([], [])
    assert meter.add(*logits[2]) == 0 and meter.add(logits[2][0], logits[2][1][:0]) == 1           # the second one: no negatives
    with pytest.warns(RuntimeWarning, match="no AP / AUC"):
        losses2, metrics2 = res2 = meter.results()
    assert res2.flags == [0, FLAG_ONE_CLASS] and metrics2[0] == metrics[2] and losses2[0] == losses[2]
    assert math.isnan(metrics2[1]["average_precision"]) and math.isnan(metrics2[1]["roc_auc"]) and not math.isnan(losses2[1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                                             # warned once per meter
        meter.results()
    with pytest.raises(TypeError):
        meter.add(logits[0][0].double(), logits[0][1])
    with pytest.raises(TypeError):
        meter.add(logits[0][0].cpu(), logits[0][1])


@pytest.mark.gpu
def test_get_link_prediction_metrics_on_cuda_tensors():
    """Interleaved labels: the CUDA route gives the dict of the CPU route on the same tensors."""
    _need_gpu()
    g, _ = g14()
    for k in (1, 3, 6, 8, 9):
        P, N = CASES[k]
        order = np.random.RandomState(k).permutation(P + N)
        s = torch.from_numpy(np.concatenate([g[f"pos_score_{k}"], g[f"neg_score_{k}"]])[order])
        y = torch.from_numpy(np.concatenate([np.ones(P, dtype=np.float32), np.zeros(N, dtype=np.float32)])[order])
        cpu = get_link_prediction_metrics(predicts=s, labels=y)
        gpu = get_link_prediction_metrics(predicts=s.to("cuda:0"), labels=y.to("cuda:0"))
        assert sorted(gpu) == ["average_precision", "roc_auc"] and all(type(v) is float for v in gpu.values())
        assert abs(gpu["average_precision"] - cpu["average_precision"]) <= AP_TOL and gpu["roc_auc"] == cpu["roc_auc"]
        assert abs(gpu["average_precision"] - g["ap"][k]) <= AP_TOL and abs(gpu["roc_auc"] - g["auc"][k]) <= AP_TOL


class _Encoder(torch.nn.Module):
    def __init__(self, width, dim):
        super().__init__()
        self.lin = torch.nn.Linear(width, dim)

    def forward(self, features, node_ids, times):                          # [2B, K, 2F] -> [2B, D]
        return self.lin(features.mean(dim=1))


class _Decoder(torch.nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.lin = torch.nn.Linear(2 * dim, 1)

    def forward(self, src_node_ids, dst_node_ids, src_node_embeddings, dst_node_embeddings):
        return self.lin(torch.cat([src_node_embeddings, dst_node_embeddings], dim=1))


@pytest.mark.gpu
def test_evaluate_link_prediction_on_the_toy_graph(golden_dir):
    """The toy graph and helpers of test_negative_sampler's run_evaluation test, a small torch encoder / decoder: the losses and
    metrics returned equal the host rule on the logits that an on_batch spy sees in an identical second evaluation."""
    _need_gpu()
    import tpnet_amd
    from tpnet_amd.callers import evaluate_link_prediction, run_evaluation
    from test_negative_sampler import _module, _sampler, g13
    g = g13(golden_dir)
    src, dst, t = g["src"], g["dst"], g["t"]
    rp, twin = _module(41), _module(41)
    twin.mlp.load_state_dict(rp.mlp.state_dict())
    assert torch.equal(rp.random_projections[0], twin.random_projections[0])
    nbr = tpnet_amd.GpuRecentNeighborSampler(src, dst, t, device="cuda:0", num_nodes=41)
    neg = _sampler(src, dst, t, seed=3)
    torch.manual_seed(3)
    enc, dec = _Encoder(2 * rp.pair_wise_feature_dim, 16).to("cuda:0"), _Decoder(16).to("cuda:0")
    seen = []
    with torch.no_grad():
        run_evaluation(twin, nbr, neg, src, dst, t, 25, 4, enc, dec,
                       on_batch=lambda i, ns, nd, res: seen.append((res[1][0].clone(), res[1][1].clone())))
    neg.reset_random_state()
    res = evaluate_link_prediction(rp, nbr, neg, src, dst, t, 25, 4, enc, dec)
    losses, metrics = res
    assert len(seen) == len(losses) == len(metrics) == 12 and res.flags == [0] * 12
    for k, (pl, nl) in enumerate(seen):
        assert pl.shape == (25, 1) and nl.shape == (25, 1)
        h = link_prediction_metrics_host(torch.sigmoid(pl).cpu().numpy(), torch.sigmoid(nl).cpu().numpy(), pl.cpu().numpy(),
                                         nl.cpu().numpy())
        assert metrics[k]["roc_auc"] == h["auc"] and abs(metrics[k]["average_precision"] - h["ap"]) <= AP_TOL
        assert abs(losses[k] - h["loss"]) <= loss_tol(h["loss"])
    assert len({m["roc_auc"] for m in metrics}) > 1                        # (the batches do differ)
    for i in range(4):                                                     # both evaluations streamed the same updates
        assert torch.equal(rp.random_projections[i].detach(), twin.random_projections[i].detach())
    meter = LinkPredictionMeter(30, "cuda:0")                              # a caller's meter is appended to
    meter.add(*seen[0])
    neg.reset_random_state()
    losses3, metrics3 = evaluate_link_prediction(twin, nbr, neg, src[:50], dst[:50], t[:50] + 100.0, 25, 4, enc, dec, meter=meter)
    assert len(losses3) == 3 and metrics3[0] == metrics[0] and losses3[0] == losses[0]
