"""Link-prediction metrics of a batch: BCE loss, average precision and ROC-AUC (C ABI: tpnet_lp_metrics, csrc/metrics.hip).

The reference scores every evaluation batch on the host (evaluate_models_utils.py:186-193, utils/metrics.py:8-22): `loss.item()`,
`predicts.sigmoid().cpu()` and sklearn's `average_precision_score` / `roc_auc_score` -- two synchronisations and two CPU sorts per
batch.  Here a batch's three numbers are one 64-byte record that a kernel appends to a device-resident log; nothing synchronises
until the log is read, once, when the split is over (`LinkPredictionMeter`).  The one-vs-many ranking protocol (MRR, Hits@k:
tpnet_lp_ranking, `LinkRankingMeter`, `link_ranking_metrics_host`) is at the end of this file.

The rule (include/tpnet_hip.h spells it out): with the scores p[0..P) of the positives and q[0..N) of the negatives, per positive i
  a_i = #{j : p_j >= p_i},  b_i = #{k : q_k >= p_i},  c_i = #{k : q_k == p_i}
  AP = (1 / P) sum_i a_i / (a_i + b_i),   U2 = sum_i (2 (N - b_i) + c_i),   AUC = U2 / (2 P N)
which is sklearn's definition with ties; the loss is the mean of max(x, 0) - x y + log1p(exp(-|x|)) over the P + N logits, in float64."""
import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib

MAX_SCORES = 1 << 18          # P + N of one device call
FLAG_ONE_CLASS = 1            # P == 0 or N == 0: AP = AUC = NaN
FLAG_NAN_SCORE = 2            # a NaN among the scores: AP = AUC = NaN
_RECORD_WORDS = 8             # {f64 loss, f64 ap, f64 auc, i64 u2, i64 n_pos, i64 n_neg, i64 flags, i64 reserved}


def _has_loss(P, N, pos_logit, neg_logit):
    """The loss needs the logits of every side that is not empty (tpnet_lp_metrics: the pointer of an empty side is not looked at)."""
    return (pos_logit is not None or neg_logit is not None) and (P == 0 or pos_logit is not None) and (N == 0 or neg_logit is not None)


def link_prediction_metrics_host(pos, neg, pos_logit=None, neg_logit=None):
    """The rule in numpy: -> {'loss', 'ap', 'auc', 'u2', 'n_pos', 'n_neg', 'flags'}, the fields of the device record.  pos / neg: the
    scores (taken as fp32); pos_logit / neg_logit (optional, fp32): without them the loss is NaN.  The counts come from binary
    searches in the sorted scores, which is the same three integers per positive; a NaN score compares false and is counted nowhere.
    This is the CPU path of `get_link_prediction_metrics` and what the device record is held to."""
    p = np.asarray(pos, dtype=np.float32).reshape(-1)
    q = np.asarray(neg, dtype=np.float32).reshape(-1)
    P, N = len(p), len(q)
    nan_p, nan_q = np.isnan(p), np.isnan(q)
    ps, qs = np.sort(p[~nan_p]), np.sort(q[~nan_q])
    lo = np.searchsorted(qs, p, side="left")
    a = np.where(nan_p, 0, len(ps) - np.searchsorted(ps, p, side="left")).astype(np.int64)
    b = np.where(nan_p, 0, len(qs) - lo).astype(np.int64)
    c = np.where(nan_p, 0, np.searchsorted(qs, p, side="right") - lo).astype(np.int64)
    u2 = int(np.sum(2 * (N - b) + c))
    flags = (FLAG_ONE_CLASS if P == 0 or N == 0 else 0) | (FLAG_NAN_SCORE if nan_p.any() or nan_q.any() else 0)
    if flags:
        ap = auc = float("nan")
    else:
        ap = float(np.sum(a.astype(np.float64) / (a + b).astype(np.float64)) / P)
        auc = u2 / (2 * P * N)
    loss = float("nan")
    if _has_loss(P, N, pos_logit, neg_logit) and P + N > 0:
        xs = [np.asarray(v, dtype=np.float32).reshape(-1).astype(np.float64) for v in (pos_logit, neg_logit) if v is not None]
        x = np.concatenate(xs)
        assert len(x) == P + N, "one logit per score"
        y = np.concatenate([np.ones(P), np.zeros(N)])
        loss = float(np.sum(np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))) / (P + N))
    return {"loss": loss, "ap": ap, "auc": auc, "u2": u2, "n_pos": P, "n_neg": N, "flags": flags}


def _check_f32(x, device, what):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != device:
        raise TypeError(f"{what}: an fp32 tensor on {device} is expected")


def _flat_f32(x, device, what):
    _check_f32(x, device, what)
    return x.detach().reshape(-1).contiguous()


def _enqueue(pos, neg, pos_logit, neg_logit, scratch, record_ptr, device):
    """tpnet_lp_metrics on the current stream of `device`: flat fp32 device tensors -> the record at record_ptr."""
    ptr = lambda v: v.data_ptr() if v is not None and v.numel() else None
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _lib.check(_lib.load().tpnet_lp_metrics(ptr(pos), pos.numel(), ptr(neg), neg.numel(), ptr(pos_logit), ptr(neg_logit),
                                            ptr(scratch), scratch.numel() if scratch is not None else 0, record_ptr, stream),
               "lp_metrics")


class _TrainingLoss(torch.autograd.Function):
    """tpnet_lp_train_loss as an autograd node: (pos_logits, neg_logits) -> the batch's mean BCE-with-logits loss, a 0-dim fp32 tensor.
    The forward's launches append the record and write d(loss) / d(logit) of both sides into buffers of this call's own (a later
    call may run before this one's backward); the backward scales them by grad_output on the device."""

    @staticmethod
    def forward(ctx, pos_logits, neg_logits, scratch, record_ptr, device):
        pl, nl = pos_logits.detach().reshape(-1).contiguous(), neg_logits.detach().reshape(-1).contiguous()
        ps, ns = torch.sigmoid(pl), torch.sigmoid(nl)
        gp, gn = torch.empty_like(pl), torch.empty_like(nl)
        loss = torch.empty((), dtype=torch.float32, device=device)
        ptr = lambda v: v.data_ptr() if v.numel() else None
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _lib.check(_lib.load().tpnet_lp_train_loss(ptr(ps), ps.numel(), ptr(ns), ns.numel(), ptr(pl), ptr(nl), ptr(scratch),
                                                   scratch.numel(), record_ptr, ptr(gp), ptr(gn), loss.data_ptr(), stream),
                   "lp_train_loss")
        ctx.save_for_backward(gp, gn)
        ctx.shapes = (pos_logits.shape, neg_logits.shape)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        gp, gn = ctx.saved_tensors
        return ((grad_output * gp).reshape(ctx.shapes[0]) if ctx.needs_input_grad[0] else None,
                (grad_output * gn).reshape(ctx.shapes[1]) if ctx.needs_input_grad[1] else None, None, None, None)


def _scratch_for(P, N, old, device):
    need = _lib.load().tpnet_lp_metrics_scratch_bytes(P, N)
    if need == 0:
        raise _lib.TPNetHipError(f"tpnet_hip lp_metrics: {P} + {N} scores are more than one call counts ({MAX_SCORES})")
    if old is None or old.numel() < need:
        return torch.empty(need, dtype=torch.uint8, device=device)
    return old


def get_link_prediction_metrics(predicts, labels):
    """The reference's `get_link_prediction_metrics` (utils/metrics.py:8-22): predicts = the scores, labels = 1 for a positive, anything
    else for a negative -> {'average_precision': float, 'roc_auc': float}.  CUDA tensors are split by `labels` with torch and counted by
    the kernel; this call SYNCHRONISES, because it returns Python floats (`LinkPredictionMeter` is the path that does not).  CPU
    tensors and arrays take `link_prediction_metrics_host`.  A batch of one class, or one with a NaN score, gives NaN for both where
    sklearn raises."""
    if isinstance(predicts, torch.Tensor) and predicts.is_cuda:
        device = predicts.device
        s = predicts.detach().reshape(-1).to(torch.float32)
        m = torch.as_tensor(labels, device=device).reshape(-1) == 1
        pos, neg = s[m].contiguous(), s[~m].contiguous()
        record = torch.zeros(_RECORD_WORDS, dtype=torch.int64, device=device)
        scratch = _scratch_for(pos.numel(), neg.numel(), None, device)
        _enqueue(pos, neg, None, None, scratch, record.data_ptr(), device)
        r = record.cpu().numpy().view(np.float64)
        return {"average_precision": float(r[1]), "roc_auc": float(r[2])}
    to_np = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    s, m = to_np(predicts).reshape(-1), to_np(labels).reshape(-1) == 1
    r = link_prediction_metrics_host(s[m], s[~m])
    return {"average_precision": r["ap"], "roc_auc": r["auc"]}


class LinkPredictionResults(tuple):
    """`(losses, metrics)`, the return value of the reference's `evaluate_model_link_prediction` (evaluate_models_utils.py:198): a list
    of floats and a list of {'average_precision', 'roc_auc'} dicts, one entry per batch.  `.flags` holds the records' flag words
    (FLAG_ONE_CLASS, FLAG_NAN_SCORE) in the same order."""

    def __new__(cls, losses, metrics, flags):
        self = super().__new__(cls, (losses, metrics))
        self.flags = flags
        return self


class LinkPredictionMeter:
    """A device-resident log of up to `capacity` batches' loss, average precision and ROC-AUC.

    `add` enqueues torch's sigmoid and the three launches of tpnet_lp_metrics on the current stream and returns; it copies nothing to
    the host and never synchronises.  `add_training` is `add` for a training batch: the same record, and the loss as a differentiable
    device scalar whose gradient the same launches write.  `results` reads the log with ONE copy; training and evaluation records
    share it.  The scratch buffer is the meter's own: calls belong on one stream."""

    def __init__(self, capacity: int, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.TPNetHipError("LinkPredictionMeter needs a cuda device (link_prediction_metrics_host is the CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        _lib.load()
        self.capacity = int(capacity)
        assert self.capacity > 0
        self._log = torch.zeros((self.capacity, _RECORD_WORDS), dtype=torch.int64, device=self.device)
        self._n = 0
        self._scratch = None
        self._warned = False

    def __len__(self):
        return self._n

    def add(self, pos_logits: torch.Tensor, neg_logits: torch.Tensor) -> int:
        """The decoder's logits of a batch's positive and negative pairs (fp32 tensors on the meter's device, any shape: flattened) ->
        the index of the record written.  The scores that are ranked are torch's own `sigmoid` of the logits, as in the reference
        (`predicts.sigmoid()`): where the fp32 sigmoid saturates it creates ties that the logits do not have."""
        if self._n >= self.capacity:
            raise IndexError(f"LinkPredictionMeter: the log of {self.capacity} records is full (results(), then reset())")
        pl = _flat_f32(pos_logits, self.device, "pos_logits")
        nl = _flat_f32(neg_logits, self.device, "neg_logits")
        self._scratch = _scratch_for(pl.numel(), nl.numel(), self._scratch, self.device)
        ps, ns = torch.sigmoid(pl), torch.sigmoid(nl)
        k = self._n
        _enqueue(ps, ns, pl, nl, self._scratch, self._log.data_ptr() + k * _RECORD_WORDS * 8, self.device)
        self._n = k + 1
        return k

    def add_training(self, pos_logits: torch.Tensor, neg_logits: torch.Tensor) -> torch.Tensor:
        """A TRAINING batch (train_link_prediction.py:375-386): the logits as `add` takes them -> the batch's `BCEWithLogitsLoss`
        (mean over the P + N logits, labels 1 / 0) as a differentiable 0-dim fp32 tensor on the device.  The same three launches
        append the record `add` would write for these logits (same scores: torch's `sigmoid`), write the loss and write its gradient
        by every logit, (sigmoid(x) - y) / (P + N), formed from the logit in float64 (include/tpnet_hip.h: tpnet_lp_train_loss) --
        `loss.backward()` multiplies it by the incoming gradient and hands it on in the inputs' shapes.  Nothing synchronises, here or
        in the backward.  Under `no_grad`, or when neither input requires a gradient, the record and the loss are the same and there
        is no graph.  An empty batch has no mean: ValueError."""
        if self._n >= self.capacity:
            raise IndexError(f"LinkPredictionMeter: the log of {self.capacity} records is full (results(), then reset())")
        _check_f32(pos_logits, self.device, "pos_logits")
        _check_f32(neg_logits, self.device, "neg_logits")
        P, N = pos_logits.numel(), neg_logits.numel()
        if P + N == 0:
            raise ValueError("LinkPredictionMeter.add_training: an empty batch has no mean loss")
        self._scratch = _scratch_for(P, N, self._scratch, self.device)
        k = self._n
        loss = _TrainingLoss.apply(pos_logits, neg_logits, self._scratch, self._log.data_ptr() + k * _RECORD_WORDS * 8, self.device)
        self._n = k + 1
        return loss

    def add_probabilities(self, pos_prob: torch.Tensor, neg_prob: torch.Tensor) -> int:
        """Probabilities of a batch's positive and negative pairs (fp32 tensors on the meter's device, any shape: flattened), as a
        model that has no logits gives them -- EdgeBank's 0 / 1 -> the index of the record written.  They are ranked as they are (no
        sigmoid).  The loss word is the reference's `nn.BCELoss` (evaluate_models_utils.py:257, 314): the mean over the P + N
        probabilities p with label y of -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)), formed in float64 from the fp32
        probabilities by torch on the same stream and copied into the record on the device; nothing synchronises."""
        if self._n >= self.capacity:
            raise IndexError(f"LinkPredictionMeter: the log of {self.capacity} records is full (results(), then reset())")
        pp = _flat_f32(pos_prob, self.device, "pos_prob")
        nq = _flat_f32(neg_prob, self.device, "neg_prob")
        self._scratch = _scratch_for(pp.numel(), nq.numel(), self._scratch, self.device)
        k = self._n
        _enqueue(pp, nq, None, None, self._scratch, self._log.data_ptr() + k * _RECORD_WORDS * 8, self.device)   # loss word: NaN
        terms = torch.cat([torch.log(pp.double()), torch.log(1.0 - nq.double())]).clamp_min(-100.0)
        loss = -terms.sum() / terms.numel()
        self._log[k, 0:1].copy_(loss.reshape(1).view(torch.int64))       # after the record's kernel, on its stream
        self._n = k + 1
        return k

    def records(self) -> np.ndarray:
        """The log's records so far as an int64 array [n][8] on the host (one copy; synchronises); words 0..2 are float64 bits."""
        return self._log[:self._n].cpu().numpy()

    def results(self) -> LinkPredictionResults:
        """One device-to-host copy (synchronises) -> `(losses, metrics)` with `.flags`.  Warns, once per meter, if any record is
        flagged: its AP and AUC are NaN."""
        rec = self.records()
        f = rec.view(np.float64)
        losses = [float(v) for v in f[:, 0]]
        metrics = [{"average_precision": float(r[1]), "roc_auc": float(r[2])} for r in f]
        flags = [int(v) for v in rec[:, 6]]
        if any(flags) and not self._warned:
            self._warned = True
            bad = [k for k, v in enumerate(flags) if v]
            warnings.warn(f"LinkPredictionMeter: {len(bad)} of {len(flags)} batches have no AP / AUC (first: batch {bad[0]}, flags "
                          f"{flags[bad[0]]}: 1 = only one class, 2 = a NaN score)", RuntimeWarning, stacklevel=2)
        return LinkPredictionResults(losses, metrics, flags)

    def reset(self):
        """Empties the log: the next `add` writes record 0.  (Records are overwritten, the buffer is kept.)"""
        self._n = 0


# ------------------------------------------------------------------------------------------------ one-vs-many ranking: MRR, Hits@k
# The rule (include/tpnet_hip.h: tpnet_lp_ranking): logits [B, 1 + C], column 0 the positive's logit p, column 1 + c a candidate's;
# per query over its valid candidates  g_i = #{q > p},  e_i = #{q == p},  m_i = 2 + 2 g_i + e_i  (twice the rank, ties at the mean of
# the optimistic and the pessimistic rank); a query with a NaN among p and its valid candidates, or with no valid candidate, is not
# counted; n = the counted queries:  mrr = (1 / n) sum 2 / m_i,  hits@k = #{m_i <= 2 k} / n.  Ranks are formed on the fp32 logits as
# given -- no sigmoid, so a saturating sigmoid adds no ties.
RANK_FLAG_NO_QUERY = 1        # n == 0: the four floats are NaN
RANK_FLAG_EMPTY_QUERY = 4     # a query without a valid candidate (not counted); FLAG_NAN_SCORE = 2: a query with a NaN (not counted)
RANK_FLAG_FILTER_OVERFLOW = 8  # a query whose filter list did not fit its row (not counted); only the records from counts set it
MAX_RANK_COLUMNS = 1 << 20    # 1 + C of one device call


def link_ranking_metrics_host(logits, valid=None, hits_at=(1, 3, 10)):
    """The rule in numpy: logits [B, 1 + C] (taken as fp32), valid [B, C] bool (None: every candidate) -> {'mrr', 'hits' (a tuple, one
    per k of hits_at), 'm_sum', 'n', 'n_valid_candidates', 'flags'}, the fields of the device record.  This is the CPU path and what
    the device record is held to."""
    x = np.asarray(logits, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("logits must be [B, 1 + C]")
    B, C = x.shape[0], x.shape[1] - 1
    v = np.ones((B, C), dtype=bool) if valid is None else np.asarray(valid, dtype=bool).reshape(B, C)
    p, q = x[:, :1], x[:, 1:]
    with np.errstate(invalid="ignore"):
        g = ((q > p) & v).sum(axis=1).astype(np.int64)
        e = ((q == p) & v).sum(axis=1).astype(np.int64)
    nv = v.sum(axis=1).astype(np.int64)
    nan = np.isnan(p[:, 0]) | (np.isnan(q) & v).any(axis=1)
    empty = nv == 0
    m = (2 + 2 * g + e)[~(nan | empty)]
    n = int(len(m))
    flags = (FLAG_NAN_SCORE if nan.any() else 0) | (RANK_FLAG_EMPTY_QUERY if empty.any() else 0) | (0 if n else RANK_FLAG_NO_QUERY)
    if n:
        mrr = float(np.sum(2.0 / m.astype(np.float64)) / n)
        hits = tuple(float(np.float64(int((m <= 2 * int(k)).sum())) / np.float64(n)) for k in hits_at)
    else:
        mrr, hits = float("nan"), tuple(float("nan") for _ in hits_at)
    return {"mrr": mrr, "hits": hits, "m_sum": int(m.sum()), "n": n, "n_valid_candidates": int(nv.sum()), "flags": flags}


def link_ranking_counts_host(counts, pos_logit, filter_logits=None, filter_ids=None, n_filter=None, hits_at=(1, 3, 10)):
    """tpnet_lp_ranking_counts' rule in numpy: counts [B, 4] = (g, e, nv, flags) per query as `score_fanout.rank_range` returns them,
    pos_logit [B] (fp32); optionally a filter: filter_logits [B, F] (fp32), filter_ids [B, F] (-1: no entry), n_filter [B] (the true
    list lengths).  Over a query's slots j < min(n_filter, F) with an id >= 0:  g_f = #{filter_logit > p}, e_f = #{== p},
    m = 2 + 2 (g - g_f) + (e - e_f), valid candidates = nv - n_filter.  Not counted: a NaN flag in counts, a NaN p or looked-at filter
    logit (FLAG_NAN_SCORE), n_filter > F (RANK_FLAG_FILTER_OVERFLOW), no valid candidate left (RANK_FLAG_EMPTY_QUERY).
    -> link_ranking_metrics_host's dict."""
    c = np.asarray(counts).astype(np.int64).reshape(-1, 4)
    p = np.asarray(pos_logit, dtype=np.float32).reshape(-1)
    B = len(p)
    g, e, nv = c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy()
    nan = ((c[:, 3] & FLAG_NAN_SCORE) != 0) | np.isnan(p)
    over = np.zeros(B, dtype=bool)
    if filter_logits is not None:
        fl = np.asarray(filter_logits, dtype=np.float32).reshape(B, -1)
        ids = np.asarray(filter_ids).reshape(B, -1)
        nf = np.maximum(np.asarray(n_filter).astype(np.int64).reshape(B), 0)
        F = fl.shape[1]
        look = (np.arange(F)[None, :] < np.minimum(nf, F)[:, None]) & (ids >= 0)
        with np.errstate(invalid="ignore"):
            g -= ((fl > p[:, None]) & look).sum(axis=1)
            e -= ((fl == p[:, None]) & look).sum(axis=1)
        nan |= (np.isnan(fl) & look).any(axis=1)
        over = nf > F
        nv = nv - nf
    empty = nv <= 0
    nv = np.maximum(nv, 0)
    m = (2 + 2 * g + e)[~(nan | empty | over)]
    n = int(len(m))
    flags = (FLAG_NAN_SCORE if nan.any() else 0) | (RANK_FLAG_EMPTY_QUERY if empty.any() else 0) | \
        (RANK_FLAG_FILTER_OVERFLOW if over.any() else 0) | (0 if n else RANK_FLAG_NO_QUERY)
    if n:
        mrr = float(np.sum(2.0 / m.astype(np.float64)) / n)
        hits = tuple(float(np.float64(int((m <= 2 * int(k)).sum())) / np.float64(n)) for k in hits_at)
    else:
        mrr, hits = float("nan"), tuple(float("nan") for _ in hits_at)
    return {"mrr": mrr, "hits": hits, "m_sum": int(m.sum()), "n": n, "n_valid_candidates": int(nv.sum()), "flags": flags}


class LinkRankingResults(list):
    """A list of per-batch dicts {'mrr', 'hits@k1', 'hits@k2', 'hits@k3'}; `.flags`: the records' flag words in the same order
    (RANK_FLAG_NO_QUERY, FLAG_NAN_SCORE, RANK_FLAG_EMPTY_QUERY); `.totals`: the same keys over all batches, each record weighted by
    its counted queries n (total MRR = sum n_b mrr_b / sum n_b), plus 'n'."""

    def __init__(self, rows, flags, totals):
        super().__init__(rows)
        self.flags = flags
        self.totals = totals


class LinkRankingMeter:
    """A device-resident log of up to `capacity` batches' ranking records (tpnet_lp_ranking): MRR and Hits@k for three k.

    `add` enqueues two launches on the current stream and returns; it copies nothing to the host and never synchronises.  `results`
    reads the log with ONE copy and forms the totals on the host from it.  The scratch buffer is the meter's own: calls belong on
    one stream."""

    def __init__(self, capacity: int, device="cuda:0", hits_at=(1, 3, 10)):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.TPNetHipError("LinkRankingMeter needs a cuda device (link_ranking_metrics_host is the CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.hits_at = tuple(int(k) for k in hits_at)
        if len(self.hits_at) != 3 or min(self.hits_at) < 1:
            raise ValueError("hits_at: three cut-offs k >= 1")
        _lib.load()
        self.capacity = int(capacity)
        assert self.capacity > 0
        self._log = torch.zeros((self.capacity, _RECORD_WORDS), dtype=torch.int64, device=self.device)
        self._n = 0
        self._scratch = None

    def __len__(self):
        return self._n

    def add(self, logits: torch.Tensor, candidates: torch.Tensor = None) -> int:
        """logits [B, 1 + C] (fp32 on the meter's device; column 0 the positive), candidates (optional) the int64 device ids [B, C]
        whose negative entries mark absent slots (`sample_many_device`'s -1) -> the index of the record written."""
        if self._n >= self.capacity:
            raise IndexError(f"LinkRankingMeter: the log of {self.capacity} records is full (results(), then reset())")
        _check_f32(logits, self.device, "logits")
        if logits.dim() != 2 or logits.shape[1] < 1 or logits.shape[1] > MAX_RANK_COLUMNS:
            raise ValueError(f"logits must be [B, 1 + C] with 1 + C <= {MAX_RANK_COLUMNS}")
        x = logits.detach().contiguous()
        B, C1 = x.shape
        cand = None
        if candidates is not None:
            if not isinstance(candidates, torch.Tensor) or candidates.dtype != torch.int64 or candidates.device != self.device \
                    or tuple(candidates.shape) != (B, C1 - 1):
                raise TypeError(f"candidates: an int64 tensor [{B}, {C1 - 1}] on {self.device} is expected")
            cand = candidates.contiguous()
        lib = _lib.load()
        need = lib.tpnet_lp_ranking_scratch_bytes(B, C1)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=self.device)
        k = self._n
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(lib.tpnet_lp_ranking(x.data_ptr() if B else None, B, C1, cand.data_ptr() if cand is not None and cand.numel() else None,
                                        self.hits_at[0], self.hits_at[1], self.hits_at[2], self._scratch.data_ptr(),
                                        self._scratch.numel(), self._log.data_ptr() + k * _RECORD_WORDS * 8, stream), "lp_ranking")
        self._n = k + 1
        return k

    def add_skip(self, logits: torch.Tensor, skip_col: torch.Tensor) -> int:
        """Ranking against all nodes (tpnet_lp_ranking_skip): logits [B, 1 + C] as for `add`, skip_col [B] int64 on the meter's
        device -- candidate column skip_col[i] (0-based among the C candidates; -1: none) of query i is absent: the query's own
        destination among all candidates.  The host rule: link_ranking_metrics_host(logits, valid) with valid[i, skip_col[i]] =
        False.  -> the index of the record written.  Two launches, nothing copied, no synchronisation."""
        if self._n >= self.capacity:
            raise IndexError(f"LinkRankingMeter: the log of {self.capacity} records is full (results(), then reset())")
        _check_f32(logits, self.device, "logits")
        if logits.dim() != 2 or logits.shape[1] < 1 or logits.shape[1] > MAX_RANK_COLUMNS:
            raise ValueError(f"logits must be [B, 1 + C] with 1 + C <= {MAX_RANK_COLUMNS}")
        x = logits.detach().contiguous()
        B, C1 = x.shape
        if not isinstance(skip_col, torch.Tensor) or skip_col.dtype != torch.int64 or skip_col.device != self.device \
                or tuple(skip_col.shape) != (B,):
            raise TypeError(f"skip_col: an int64 tensor [{B}] on {self.device} is expected")
        sk = skip_col.contiguous()
        lib = _lib.load()
        need = lib.tpnet_lp_ranking_scratch_bytes(B, C1)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=self.device)
        k = self._n
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(lib.tpnet_lp_ranking_skip(x.data_ptr() if B else None, B, C1, sk.data_ptr() if B else None, self.hits_at[0],
                                             self.hits_at[1], self.hits_at[2], self._scratch.data_ptr(), self._scratch.numel(),
                                             self._log.data_ptr() + k * _RECORD_WORDS * 8, stream), "lp_ranking_skip")
        self._n = k + 1
        return k

    def add_counts(self, counts: torch.Tensor, pos_logit: torch.Tensor, filter_logits: torch.Tensor = None,
                   filter_ids: torch.Tensor = None, n_filter: torch.Tensor = None) -> int:
        """Ranking against all nodes from COUNTS (tpnet_lp_ranking_counts; the host rule: link_ranking_counts_host): counts [B, 4]
        int32 and pos_logit [B] fp32 as `LinkPredictor_v1.rank_one_to_all` returns them; a filter is all three of filter_logits
        [B, F] fp32, filter_ids [B, F] int64 and n_filter [B] int32 (`filter_lists_device`'s layout), or none of them.  No [B, 1 + C]
        logits exist, so MAX_RANK_COLUMNS does not apply.  -> the index of the record written.  Two launches, nothing copied, no
        synchronisation."""
        if self._n >= self.capacity:
            raise IndexError(f"LinkRankingMeter: the log of {self.capacity} records is full (results(), then reset())")
        _check_f32(pos_logit, self.device, "pos_logit")
        B = int(pos_logit.numel())
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.device != self.device \
                or tuple(counts.shape) != (B, 4) or pos_logit.dim() != 1:
            raise TypeError(f"counts: an int32 tensor [{B}, 4] on {self.device} beside pos_logit [{B}] is expected")
        given = [x is not None for x in (filter_logits, filter_ids, n_filter)]
        if any(given) != all(given):
            raise ValueError("add_counts: filter_logits, filter_ids and n_filter come together")
        F, fl, fi, nf = 0, None, None, None
        if all(given):
            _check_f32(filter_logits, self.device, "filter_logits")
            F = int(filter_logits.shape[1]) if filter_logits.dim() == 2 else 0
            if filter_logits.dim() != 2 or filter_logits.shape[0] != B or not 1 <= F < 1 << 16:
                raise ValueError(f"filter_logits must be [{B}, F] with 1 <= F < 65536")
            if not isinstance(filter_ids, torch.Tensor) or filter_ids.dtype != torch.int64 or filter_ids.device != self.device \
                    or tuple(filter_ids.shape) != (B, F):
                raise TypeError(f"filter_ids: an int64 tensor [{B}, {F}] on {self.device} is expected")
            if not isinstance(n_filter, torch.Tensor) or n_filter.dtype != torch.int32 or n_filter.device != self.device \
                    or tuple(n_filter.shape) != (B,):
                raise TypeError(f"n_filter: an int32 tensor [{B}] on {self.device} is expected")
            fl, fi, nf = filter_logits.detach().contiguous(), filter_ids.contiguous(), n_filter.contiguous()
        c, p = counts.contiguous(), pos_logit.detach().contiguous()
        lib = _lib.load()
        need = lib.tpnet_lp_ranking_scratch_bytes(B, 1)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=self.device)
        k = self._n
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        ptr = lambda x: x.data_ptr() if (x is not None and B) else None
        _lib.check(lib.tpnet_lp_ranking_counts(ptr(c), ptr(p), B, ptr(fl), ptr(fi), ptr(nf), F, self.hits_at[0], self.hits_at[1],
                                               self.hits_at[2], self._scratch.data_ptr(), self._scratch.numel(),
                                               self._log.data_ptr() + k * _RECORD_WORDS * 8, stream), "lp_ranking_counts")
        self._n = k + 1
        return k

    def records(self) -> np.ndarray:
        """The log's records so far as an int64 array [n][8] on the host (one copy; synchronises); words 0..3 are float64 bits."""
        return self._log[:self._n].cpu().numpy()

    def results(self) -> LinkRankingResults:
        """One device-to-host copy (synchronises) -> the per-batch dicts with `.flags` and `.totals`."""
        rec = self.records()
        f = rec.view(np.float64)
        keys = ["mrr"] + [f"hits@{k}" for k in self.hits_at]
        rows = [{key: float(r[j]) for j, key in enumerate(keys)} for r in f]
        n = rec[:, 5].astype(np.float64)
        tot = float(n.sum())
        totals = {key: (float(np.sum(n[n > 0] * f[n > 0, j]) / tot) if tot else float("nan")) for j, key in enumerate(keys)}
        totals["n"] = int(rec[:, 5].sum())
        return LinkRankingResults(rows, [int(v) for v in rec[:, 7]], totals)

    def reset(self):
        """Empties the log: the next `add` writes record 0."""
        self._n = 0
