"""The training batch's loss on the device: `LinkPredictionMeter.add_training` (tpnet_amd/metrics.py, csrc/metrics.hip:
tpnet_lp_train_loss) and `callers.train_link_prediction_epoch`, the tail of train_link_prediction.py:375-386.

Every expectation is formed here from stock torch / numpy in float64 and from `link_prediction_metrics_host`:
  loss   the float64 rule of the record, bound 1e-12 max(1, loss) (tests/test_metrics.py); the returned scalar is that word rounded once.
  g64    d(mean BCE) / dx = (sigmoid(x) - y) / (P + N), times the factor c of `loss.mul(c).backward()`, in float64 from the fp32 logit.
         For a positive sigmoid(x) - 1 is evaluated as -1 / (1 + exp(x)), which is the same number without the cancellation (in
         float64 sigmoid(88) - 1 is 0, the derivative is -6e-39).
  bound  |g - g64| <= 2^-22 |g64| + 2^-126: two fp32 roundings of 2^-24 each (the store of the gradient, the scale by c in the
         backward) and room to spare, plus the flush of a subnormal.
  torch  against BCEWithLogitsLoss's own fp32 autograd: |g - g_torch| <= 2^-22 c / (P + N), twice a 2-ulp error of an fp32 sigmoid near
         1, the cancellation of torch's sigmoid(x) - y.
Shapes: a chunk of the counting kernel holds 256 scores of the positives-then-negatives axis and a workgroup row 256 positives, so
(255, 1) and (3, 5) put both lists into one chunk, (256, 256) is whole chunks, (257, 255), (300, 513) and (1000, 1000) have several
workgroup rows (only the first may write gradients) and chunks, and (5, 0) / (0, 5) have an empty side."""
import copy
import math
import os

import numpy as np
import pytest
import torch

from tpnet_amd.metrics import FLAG_NAN_SCORE, LinkPredictionMeter, link_prediction_metrics_host

SHAPES = [(1, 1), (3, 5), (5, 0), (0, 5), (255, 1), (256, 256), (257, 255), (300, 513), (1000, 1000)]
AP_TOL = 1e-10
NAN = float("nan")
# what the second set of logits writes over the head of each side (as far as the side is long): +-0.0, +-20, +-88, +-100, a
# repeated value; the positives lead with +88 and the negatives with -88, where an fp32 sigmoid - label is 0
SPECIAL_POS = [88.0, 0.0, -0.0, 20.0, -20.0, -88.0, 100.0, -100.0, 1.5, 1.5, 1.5]
SPECIAL_NEG = [-88.0, 0.0, -0.0, 20.0, -20.0, 88.0, 100.0, -100.0, 1.5, 1.5, -2.25, -2.25]

_cache = {}


def loss_tol(loss):
    return 1e-12 * max(1.0, abs(loss))


def same(x, y):
    return x == y or (math.isnan(x) and math.isnan(y))


def logits_of(P, N, special):
    """-> (pos, neg) fp32 arrays, the same for every test that asks: normal logits scaled by 3; special: the values above over the
    head of each side and ONE NaN, the last element of the longer side (when that side has at least two elements)."""
    key = (P, N, special)
    if key not in _cache:
        rng = np.random.RandomState(1000 * P + N)
        pos, neg = (3.0 * rng.standard_normal(P)).astype(np.float32), (3.0 * rng.standard_normal(N)).astype(np.float32)
        if special:
            pos[:len(SPECIAL_POS)] = SPECIAL_POS[:P]
            neg[:len(SPECIAL_NEG)] = SPECIAL_NEG[:N]
            longer = pos if P >= N else neg
            if len(longer) >= 2:
                longer[-1] = np.nan
        pos.setflags(write=False)
        neg.setflags(write=False)
        _cache[key] = (pos, neg)
    return _cache[key]


def grad64(pos, neg):
    """(sigmoid(x) - y) / (P + N) in float64 from the fp32 logits, each side in the form that does not cancel."""
    n = float(len(pos) + len(neg))
    with np.errstate(over="ignore"):
        return -1.0 / (1.0 + np.exp(pos.astype(np.float64))) / n, 1.0 / (1.0 + np.exp(-neg.astype(np.float64))) / n


# ------------------------------------------------------------------------------------------------------------------- CPU

def test_train_loss_refuses_bad_arguments_without_a_launch(hip_lib):
    """Every refusal of tpnet_lp_train_loss is TPNET_ERR_BAD_ARG before anything touches a device -- so this holds on a machine
    without one.  Arguments: scores, sizes, logits, scratch, record, the two gradient arrays, loss_out, stream."""
    f = hip_lib.tpnet_lp_train_loss
    big = (1 << 18) + 1
    assert f(8, 4, 8, 4, None, 8, 8, 1 << 30, 8, 8, 8, 8, None) == -1            # no logits of the positives
    assert f(8, 4, 8, 4, 8, None, 8, 1 << 30, 8, 8, 8, 8, None) == -1            # ... of the negatives
    assert f(8, 4, 8, 0, None, None, 8, 1 << 30, 8, 8, None, 8, None) == -1      # ... of the only side there is
    assert f(8, 4, 8, 4, 8, 8, 8, 1 << 30, 8, None, 8, 8, None) == -1            # no gradient array of the positives
    assert f(8, 4, 8, 4, 8, 8, 8, 1 << 30, 8, 8, None, 8, None) == -1            # ... of the negatives
    assert f(None, 0, 8, 4, None, 8, 8, 1 << 30, 8, None, None, 8, None) == -1   # ... of the only side there is
    assert f(8, 4, 8, 4, 8, 8, 8, 1 << 30, 8, 8, 8, None, None) == -1            # no loss_out
    assert f(8, 4, 8, 4, 8, 8, 8, 1 << 30, 8, 8, 8, 6, None) == -1               # a misaligned one
    assert f(8, 0, 8, 0, 8, 8, 8, 1 << 30, 8, 8, 8, 8, None) == -1               # an empty batch has no mean
    assert f(None, 0, None, 0, None, None, None, 0, 8, None, None, 8, None) == -1
    assert f(8, big - 1, 8, 1, 8, 8, 8, 1 << 30, 8, 8, 8, 8, None) == -1         # beyond one call's scores
    assert f(8, 1, 8, big - 1, 8, 8, 8, 1 << 30, 8, 8, 8, 8, None) == -1
    assert f(8, -1, 8, 4, 8, 8, 8, 1 << 30, 8, 8, 8, 8, None) == -1
    assert f(None, 4, 8, 4, 8, 8, 8, 1 << 30, 8, 8, 8, 8, None) == -1            # what tpnet_lp_metrics refuses: a missing score array,
    assert f(8, 4, 8, 4, 8, 8, 8, 1 << 30, None, 8, 8, 8, None) == -1            # no record,
    assert f(8, 4, 8, 4, 8, 8, None, 1 << 30, 8, 8, 8, 8, None) == -1            # no scratch
    assert f(8, 4, 8, 4, 8, 8, 8, 16, 8, 8, 8, 8, None) == -2                    # (a short scratch: TPNET_ERR_WORKSPACE, as there)
    assert hip_lib.tpnet_abi_version() == 7                                      # additive


class _Log:
    """Stubs that record their calls in one list."""

    def __init__(self):
        self.events = []

    # rp
    def reset_random_projections(self):
        self.events.append("reset")

    def get_pair_wise_feature(self, src_node_ids, dst_node_ids):
        self.events.append(("readout", len(src_node_ids)))
        return torch.zeros(len(src_node_ids), 4)

    def update(self, src_node_ids, dst_node_ids, node_interact_times):
        self.events.append(("update", list(src_node_ids), list(dst_node_ids), list(node_interact_times)))

    # neighbour sampler
    def get_historical_neighbors(self, node_ids, node_interact_times, num_neighbors):
        z = np.zeros((len(node_ids), num_neighbors), dtype=np.int64)
        return z, z, z.astype(np.float64)

    # negative sampler
    def sample(self, size):
        self.events.append(("sample", size))
        return np.zeros(size, dtype=np.int64), np.full(size, 9, dtype=np.int64)

    # encoder / decoder
    def encoder(self, features, node_ids, times):
        self.events.append(("encoder", tuple(features.shape), list(node_ids)))
        return torch.zeros(features.shape[0], 3)

    def decoder(self, src_node_ids, dst_node_ids, src_node_embeddings, dst_node_embeddings):
        self.events.append(("decoder", list(dst_node_ids)))
        return torch.full((len(src_node_ids), 1), float(len(self.events)))

    # optimizer
    def zero_grad(self):
        self.events.append("zero_grad")

    def step(self):
        self.events.append("step")

    # meter and the loss it returns
    def add_training(self, pos_logits, neg_logits):
        self.events.append(("add_training", tuple(pos_logits.shape), tuple(neg_logits.shape), float(pos_logits[0]), float(neg_logits[0])))
        return self

    def backward(self):
        self.events.append("backward")

    def results(self):
        self.events.append("results")
        return "the meter's results"


def test_training_epoch_follows_the_reference_order():
    """train_link_prediction.py:246-386 with stubs that record their calls: reset once; per chronological batch the negatives, the
    two encoder readouts (positives first), the two decoder calls, the update, the loss from the meter, zero_grad, backward, step;
    the ragged last batch is there; the meter is read once, at the end, and what it returns is returned."""
    from tpnet_amd.callers import train_link_prediction_epoch
    log = _Log()
    src, dst, t = np.arange(1, 8), np.arange(11, 18), np.arange(7, dtype=np.float64)
    seen = []
    out = train_link_prediction_epoch(log, log, log, src, dst, t, 3, 2, log.encoder, log.decoder, log, meter=log,
                                      on_batch=lambda i, neg, res, loss: seen.append((i, len(neg), loss is log, len(log.events))))
    assert out == "the meter's results"
    want = ["reset"]
    for b0, size in ((0, 3), (3, 3), (6, 1)):
        s, d = list(src[b0:b0 + size]), list(dst[b0:b0 + size])
        at = len(want)                                                        # (the stub decoder returns the event count as its logit)
        want += [("sample", size),
                 ("readout", 4 * size * 2), ("encoder", (2 * size, 2, 8), s + d),
                 ("readout", 4 * size * 2), ("encoder", (2 * size, 2, 8), s + [9] * size),
                 ("decoder", d), ("decoder", [9] * size),
                 ("update", s, d, list(t[b0:b0 + size])),
                 ("add_training", (size, 1), (size, 1), float(at + 6), float(at + 7)),
                 "zero_grad", "backward", "step"]
    want.append("results")
    assert log.events == want
    assert seen == [(0, 3, True, 13), (1, 3, True, 25), (2, 1, True, 37)]    # on_batch: after the step of its batch


# ------------------------------------------------------------------------------------------------------------------- GPU

def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")


def _leaf(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).to("cuda:0").requires_grad_()      # (a copy: the cached arrays are read-only)


@pytest.mark.gpu
@pytest.mark.parametrize("special", [False, True], ids=["normal", "special"])
@pytest.mark.parametrize("P,N", SHAPES)
def test_loss_record_and_gradient(P, N, special):
    """One batch through add_training and through add: the same 64 bytes; the scalar is the record's loss rounded once; the loss is
    the float64 rule's; the gradient of c * loss, c = 1 and 3, is within the bound of g64 and of stock torch's; +88 on a positive
    keeps a negative gradient; the NaN stays in its element."""
    _need_gpu()
    pos, neg = logits_of(P, N, special)
    meter = LinkPredictionMeter(3, "cuda:0")
    g_pos64, g_neg64 = grad64(pos, neg)
    labels = torch.cat([torch.ones(P), torch.zeros(N)]).to("cuda:0")
    n_nan = int(np.isnan(pos).sum() + np.isnan(neg).sum())
    assert n_nan == (1 if special and max(P, N) >= 2 else 0)
    losses = []
    for c in (1.0, 3.0):
        pl, nl = _leaf(pos), _leaf(neg)
        loss = meter.add_training(pl, nl)
        assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
        loss.mul(c).backward()
        losses.append(loss.item())
        pt, nt = _leaf(pos), _leaf(neg)
        torch.nn.BCEWithLogitsLoss()(torch.cat([pt, nt]), labels).mul(c).backward()
        for x, g, g64, gt in ((pos, pl.grad, g_pos64, pt.grad), (neg, nl.grad, g_neg64, nt.grad)):
            assert g.shape == x.shape and g.dtype == torch.float32
            g, gt, g64 = g.cpu().numpy().astype(np.float64), gt.cpu().numpy().astype(np.float64), c * g64
            ok = ~np.isnan(x)
            assert np.isnan(g[~ok]).all() and np.isfinite(g[ok]).all()          # the NaN logit's gradient, and only that one
            if ok.any():
                err = np.abs(g[ok] - g64[ok])
                bound = 2.0 ** -22 * np.abs(g64[ok]) + 2.0 ** -126
                vs_torch = np.abs(g[ok] - gt[ok]).max() / (2.0 ** -22 * c / (P + N))
                print(f"P {P} N {N} special {special} c {c}: |g - g64| / bound <= {(err / bound).max():.3f}, |g - g_torch| / bound <= {vs_torch:.3f}")
                assert (err <= bound).all()
                assert vs_torch <= 1.0
        if special and P:
            assert pos[0] == 88.0 and pl.grad[0].item() < 0.0                   # (an fp32 sigmoid(88) - 1 is 0)
    k = meter.add(_leaf(pos), _leaf(neg))
    rec = meter.records()
    assert k == 2 and len(meter) == 3
    assert np.array_equal(rec[0], rec[2]) and np.array_equal(rec[1], rec[2])      # bit for bit add's record
    word = float(rec[0].view(np.float64)[0])
    h = link_prediction_metrics_host(torch.sigmoid(_leaf(pos)).detach().cpu().numpy(), torch.sigmoid(_leaf(neg)).detach().cpu().numpy(), pos, neg)
    assert same(word, h["loss"]) or abs(word - h["loss"]) <= loss_tol(h["loss"])
    assert math.isnan(word) == (n_nan > 0) and (int(rec[0, 6]) & FLAG_NAN_SCORE != 0) == (n_nan > 0)
    for v in losses:
        assert same(np.float32(v), np.float32(word))


@pytest.mark.gpu
def test_shapes_needs_and_graphs():
    """[B, 1] and non-contiguous inputs get gradients in their own shapes; a side that needs no gradient gets none; without a graph
    the record is written all the same; a second-order backward raises; the errors are add's."""
    _need_gpu()
    pos, neg = logits_of(300, 513, False)
    g_pos64, g_neg64 = grad64(pos, neg)
    meter = LinkPredictionMeter(8, "cuda:0")
    flat = meter.add_training(_leaf(pos), _leaf(neg)).item()
    pl = _leaf(pos.reshape(-1, 1))                                               # what a decoder gives
    wide = _leaf(np.stack([neg, -neg], axis=1))                                  # [N, 2]: column 0 is not contiguous
    nl = wide[:, 0]
    assert not nl.is_contiguous()
    loss = meter.add_training(pl, nl)
    loss.backward()
    assert pl.grad.shape == (300, 1) and wide.grad.shape == (513, 2) and loss.item() == flat
    assert np.abs(pl.grad.cpu().numpy().reshape(-1) - g_pos64).max() <= 2.0 ** -22 * np.abs(g_pos64).max()
    assert np.abs(wide.grad[:, 0].cpu().numpy() - g_neg64).max() <= 2.0 ** -22 * np.abs(g_neg64).max()
    assert (wide.grad[:, 1] == 0).all()
    pl, nl = _leaf(pos), _leaf(neg).detach()                                     # only the positives need a gradient
    meter.add_training(pl, nl).backward()
    assert nl.grad is None and pl.grad is not None and pl.grad.shape == (300,)
    pl, nl = _leaf(pos).detach(), _leaf(neg)
    meter.add_training(pl, nl).backward()
    assert pl.grad is None and nl.grad.shape == (513,)
    with torch.no_grad():
        quiet = meter.add_training(_leaf(pos), _leaf(neg))
    assert quiet.grad_fn is None and not quiet.requires_grad and quiet.item() == flat
    plain = meter.add_training(_leaf(pos).detach(), _leaf(neg).detach())         # neither side requires a gradient
    assert plain.grad_fn is None and not plain.requires_grad and plain.item() == flat
    rec = meter.records()
    assert len(meter) == 6 and all(np.array_equal(rec[0], r) for r in rec[1:])
    pl, nl = _leaf(pos), _leaf(neg)
    g, = torch.autograd.grad(meter.add_training(pl, nl), pl, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()                                                       # once_differentiable: there is no second order
    with pytest.raises(ValueError):
        meter.add_training(_leaf(pos[:0]), _leaf(neg[:0]))
    with pytest.raises(TypeError):
        meter.add_training(_leaf(pos).double(), _leaf(neg))
    with pytest.raises(TypeError):
        meter.add_training(_leaf(pos), _leaf(neg).cpu())
    assert len(meter) == 7
    meter.add_training(_leaf(pos), _leaf(neg))
    with pytest.raises(IndexError):
        meter.add_training(_leaf(pos), _leaf(neg))                               # the log is full
    assert len(meter) == 8


@pytest.mark.gpu
def test_training_steps_do_not_synchronise():
    """Five add_training + backward steps and two adds in between, under torch's synchronisation check: nothing raises; the log then
    holds the seven batches in order."""
    _need_gpu()
    shapes = [(3, 5), (256, 256), (257, 255), (5, 0), (300, 513), (1000, 1000), (255, 1)]
    training = [True, True, False, True, True, False, True]
    batches = [logits_of(P, N, False) for P, N in shapes]
    leaves = [(_leaf(p), _leaf(n)) for p, n in batches]
    meter = LinkPredictionMeter(7, "cuda:0")
    meter.add_training(*leaves[0]).backward()                                    # (first use: loads the code objects)
    meter.reset()
    for p, n in leaves:
        p.grad = n.grad = None
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for (p, n), train in zip(leaves, training):
            if train:
                meter.add_training(p, n).backward()
            else:
                meter.add(p, n)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    with pytest.warns(RuntimeWarning, match="no AP / AUC"):                      # (5, 0) has one class
        losses, metrics = meter.results()
    assert len(losses) == len(metrics) == 7
    for k, ((pos, neg), (p, n)) in enumerate(zip(batches, leaves)):
        h = link_prediction_metrics_host(torch.sigmoid(p).detach().cpu().numpy(), torch.sigmoid(n).detach().cpu().numpy(), pos, neg)
        assert abs(losses[k] - h["loss"]) <= loss_tol(h["loss"])
        assert same(metrics[k]["roc_auc"], h["auc"]) and (same(metrics[k]["average_precision"], h["ap"])
                                                           or abs(metrics[k]["average_precision"] - h["ap"]) <= AP_TOL)
        assert (p.grad is not None) == training[k]
        if training[k]:
            assert np.abs(p.grad.cpu().numpy() - grad64(pos, neg)[0]).max() <= 2.0 ** -22 / (len(pos) + len(neg))


@pytest.mark.gpu
def test_chain_rule_through_a_model():
    """logits = z @ w, 3 positives and 4 negatives: w.grad through add_training against sum_i z_i g64_i in float64 on the device's own
    fp32 logits.  Bound 2^-21 sum_i |z_ij g64_i| per component: the gradient's rounding, the product's and six additions are 8
    roundings of 2^-24 at the most."""
    _need_gpu()
    rng = np.random.RandomState(8)
    z = torch.from_numpy(rng.standard_normal((7, 8)).astype(np.float32)).to("cuda:0")
    w = torch.nn.Parameter(torch.from_numpy(rng.standard_normal(8).astype(np.float32)).to("cuda:0"))
    logits = z @ w
    meter = LinkPredictionMeter(1, "cuda:0")
    meter.add_training(logits[:3], logits[3:]).backward()
    x = logits.detach().cpu().numpy()
    g64 = np.concatenate(grad64(x[:3], x[3:]))
    terms = z.cpu().numpy().astype(np.float64) * g64[:, None]
    err, bound = np.abs(w.grad.cpu().numpy() - terms.sum(axis=0)), 2.0 ** -21 * np.abs(terms).sum(axis=0)
    print("chain rule: error / bound <=", (err / bound).max())
    assert (err <= bound).all()


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


def _toy(golden_dir):
    """The toy graph of test_metrics' evaluation test, two modules that hold the same mlp, a device neighbour sampler, a seeded host
    negative sampler and a small torch encoder / decoder."""
    import tpnet_amd
    from tpnet_amd.callers import RandomNegativeSampler
    from test_negative_sampler import _module, g13
    g = g13(golden_dir)
    src, dst, t = g["src"], g["dst"], g["t"]
    rp, twin = _module(41), _module(41)
    twin.mlp.load_state_dict(rp.mlp.state_dict())
    nbr = tpnet_amd.GpuRecentNeighborSampler(src, dst, t, device="cuda:0", num_nodes=41)
    neg = RandomNegativeSampler(src, dst, seed=3)
    torch.manual_seed(3)
    enc, dec = _Encoder(2 * rp.pair_wise_feature_dim, 16).to("cuda:0"), _Decoder(16).to("cuda:0")
    return src, dst, t, rp, twin, nbr, neg, enc, dec


@pytest.mark.gpu
def test_training_epoch_with_fixed_parameters(golden_dir):
    """SGD(lr = 0) leaves the parameters alone, so a plain-torch restatement of the epoch (run_epoch, float64 BCE, the host rule on
    torch's fp32 sigmoid) sees the logits of train_link_prediction_epoch: every batch's loss, AP and AUC agree to the bounds of
    tests/test_metrics.py.  300 edges in batches of 26: the last one has 14."""
    _need_gpu()
    from tpnet_amd.callers import run_epoch, train_link_prediction_epoch
    src, dst, t, rp, twin, nbr, neg, enc, dec = _toy(golden_dir)
    params = list(enc.parameters()) + list(dec.parameters())
    opt = torch.optim.SGD(params, lr=0.0)
    torch.manual_seed(77)                                                  # (the reset draws P[0] from torch's generator)
    sizes = []
    res = train_link_prediction_epoch(rp, nbr, neg, src, dst, t, 26, 4, enc, dec, opt,
                                      on_batch=lambda i, nd, r, loss: sizes.append((i, len(nd), tuple(r[1][0].shape), loss.shape)))
    losses, metrics = res
    assert len(losses) == len(metrics) == 12 and res.flags == [0] * 12
    assert sizes == [(i, 26 if i < 11 else 14, (26 if i < 11 else 14, 1), ()) for i in range(12)]
    assert all(p.grad is not None for p in params)

    want = []

    def restated(i, nd, r):
        pl, nl = r[1]
        x = torch.cat([pl, nl]).squeeze(-1)
        y = torch.cat([torch.ones_like(pl), torch.zeros_like(nl)]).squeeze(-1)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(x.double(), y.double())
        h = link_prediction_metrics_host(torch.sigmoid(pl).detach().cpu().numpy(), torch.sigmoid(nl).detach().cpu().numpy())
        opt.zero_grad()
        loss.backward()
        opt.step()
        want.append((loss.item(), h["ap"], h["auc"]))

    neg.reset_random_state()
    torch.manual_seed(77)
    run_epoch(twin, nbr, neg, src, dst, t, 26, 4, enc, dec, on_batch=restated)
    assert torch.equal(rp.random_projections[0].detach(), twin.random_projections[0].detach())
    for k, (loss, ap, auc) in enumerate(want):
        print("batch", k, "dloss", abs(losses[k] - loss), "dAP", abs(metrics[k]["average_precision"] - ap), "dAUC", abs(metrics[k]["roc_auc"] - auc))
        assert abs(losses[k] - loss) <= loss_tol(loss)
        assert abs(metrics[k]["average_precision"] - ap) <= AP_TOL and abs(metrics[k]["roc_auc"] - auc) <= AP_TOL
    assert len({m["roc_auc"] for m in metrics}) > 1                        # (the batches do differ)
    meter = LinkPredictionMeter(30, "cuda:0")                              # a caller's meter is appended to
    meter.add(torch.zeros(2, device="cuda:0"), torch.ones(3, device="cuda:0"))
    neg.reset_random_state()
    torch.manual_seed(77)
    losses2, metrics2 = train_link_prediction_epoch(rp, nbr, neg, src[:52], dst[:52], t[:52], 26, 4, enc, dec, opt, meter=meter)
    assert len(losses2) == 3 and losses2[1] == losses[0] and metrics2[1] == metrics[0]


@pytest.mark.gpu
def test_training_epoch_takes_the_stock_sgd_step(golden_dir):
    """One batch of 25 edges, SGD(lr = 0.1), two copies of the model from one initial state: one steps through
    train_link_prediction_epoch, the other through BCEWithLogitsLoss.  Per parameter element theta, with S = sum over the 50
    logits of |d logit_i / d theta| / 50 (50 backward passes on the stock side): the two gradients differ by at most 2^-22 S through
    the logits' gradients (the bound against torch above) and the fp32 sums of the backward, which see different inputs, round
    differently -- another 2^-22 S is allowed for that, S being an upper bound of sum |terms| because |sigmoid - y| <= 1.  So
    |d theta| <= 0.1 * 2^-21 S, plus one ulp of theta for the two roundings of theta - 0.1 g."""
    _need_gpu()
    from tpnet_amd.callers import run_epoch, train_link_prediction_epoch
    src, dst, t, rp, twin, nbr, neg, enc, dec = _toy(golden_dir)
    src, dst, t = src[:25], dst[:25], t[:25]
    enc2, dec2 = copy.deepcopy(enc), copy.deepcopy(dec)
    mine, stock = list(enc.parameters()) + list(dec.parameters()), list(enc2.parameters()) + list(dec2.parameters())
    before = [p.detach().clone() for p in mine]
    torch.manual_seed(78)
    losses, _ = train_link_prediction_epoch(rp, nbr, neg, src, dst, t, 25, 4, enc, dec, torch.optim.SGD(mine, lr=0.1))
    assert len(losses) == 1
    opt = torch.optim.SGD(stock, lr=0.1)
    S = [torch.zeros_like(p) for p in stock]
    stock_loss = []

    def step(i, nd, r):
        pl, nl = r[1]
        x = torch.cat([pl, nl]).squeeze(-1)
        assert x.shape == (50,)
        for k in range(50):
            for s, g in zip(S, torch.autograd.grad(x[k], stock, retain_graph=True)):
                s += g.abs() / 50.0
        loss = torch.nn.BCEWithLogitsLoss()(x, torch.cat([torch.ones_like(pl), torch.zeros_like(nl)]).squeeze(-1))
        opt.zero_grad()
        loss.backward()
        opt.step()
        stock_loss.append(loss.item())

    neg.reset_random_state()
    torch.manual_seed(78)
    run_epoch(twin, nbr, neg, src, dst, t, 25, 4, enc2, dec2, on_batch=step)
    assert abs(losses[0] - stock_loss[0]) <= 1e-5 * max(1.0, stock_loss[0])                # (both saw the same batch; torch's loss is fp32)
    for a, b, s, p0 in zip(mine, stock, S, before):
        a, b, s = a.detach().double(), b.detach().double(), s.double()
        bound = 0.1 * 2.0 ** -21 * s + 2.0 ** -23 * b.abs()
        print(tuple(a.shape), "moved by", (b - p0.double()).abs().max().item(), "difference / bound <=", ((a - b).abs() / bound).max().item())
        assert ((a - b).abs() <= bound).all()
        assert (b - p0.double()).abs().max() > 100 * (a - b).abs().max()                   # (a step was taken, and the same one)
