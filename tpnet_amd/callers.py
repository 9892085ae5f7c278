"""Callers either side of the hot path: what the reference's training / evaluation
loop does around `RandomProjectionModule`, restated so that the drop-in can be driven -- and pinned by fixtures G7 /
G8 -- without the reference's files (they never travel to the GPU box).

* `LinkPredictor_v1`        -- the decoder that consumes the pairwise feature (models/modules.py:73-117).
* `RecentNeighborSampler`   -- the 'recent' strategy of NeighborSampler (utils/utils.py:82-224), host side.
* `RandomNegativeSampler`   -- NegativeEdgeSampler.random_sample (utils/utils.py:388-400): draw order matters.
* `encoder_pair_indices`    -- the 4*B*K index pattern of the encoder's readout (models/TPNet.py:206-217,311-316).
* `run_evaluation`          -- the evaluation loop's order with any of the three negative strategies (evaluate_models_utils.py:56-72).
* `evaluate_link_prediction` -- the same loop scored on the device: per-batch loss, AP and ROC-AUC (evaluate_models_utils.py:186-198).
* `evaluate_edge_bank_link_prediction` -- the EdgeBank baseline's evaluation loop on the device (evaluate_models_utils.py:269-318).
* `evaluate_link_ranking`   -- one-vs-many ranking evaluation (MRR, Hits@k): per-query candidates, one-to-many decoder, device meter.
* `evaluate_link_ranking_all` / `recommend_links` -- ranking against ALL nodes of an id range (exact rank; unfiltered, or filtered and
  streaming on `LinkPredictor_v1.rank_one_to_all`) and top-k recommendation, on `LinkPredictor_v1.forward_one_to_all` (or
  streaming, with known destinations left out, on `LinkPredictor_v1.topk_one_to_all`).
* `link_prediction_batch` / `run_epoch` -- the per-batch order of train_link_prediction.py:253-373 (negatives, two
  encoder readouts, two decoder readouts, THEN update) and the epoch-level reset (:246-248).
* `train_link_prediction_epoch` -- the same epoch with the loss, the backward and the optimizer step (:375-386), the loss and the
  per-batch loss / AP / ROC-AUC from the device meter.
* `create_optimizer`        -- utils.create_optimizer (utils/utils.py:61-79), by default with the step on the device.
The encoder itself is tpnet_amd/encoder.py (`TPNet`); `encoder` / `decoder` stay plug-in callables here.
"""
from typing import Callable, Optional

import numpy as np
import torch
import torch.nn as nn


class LinkPredictor_v1(nn.Module):
    """concat[src_emb, dst_emb, pair feature] -> fc1 -> ReLU -> fc2 (models/modules.py:75-117); same constructor and
    forward keywords as the reference, same state-dict keys (fc1.*, fc2.*, random_projections.*)."""

    def __init__(self, input_dim1: int, input_dim2: int, hidden_dim: int, output_dim: int, random_projections,
                 not_encode: bool):
        super().__init__()
        self.random_projections = random_projections
        self.not_encode = not_encode
        self.random_feature_dim = 0 if random_projections is None else random_projections.pair_wise_feature_dim
        self.fc1 = nn.Linear(input_dim1 + input_dim2 + self.random_feature_dim, hidden_dim)
        self.fc2 = nn.Linear(hidden_dim, output_dim)
        self.act = nn.ReLU()
        # opt-in (tpnet_amd/fused_decoder.py): True = both layers in one bf16 matrix-core kernel (~1e-2 relative); "f32" = the fp32
        # class, forward and backward in HIP, where the kernels serve the call -- else the torch layers below, as with False
        self.fused = False
        # opt-in (tpnet_amd/score_fanout.py): with not_encode, no embeddings given and no gradient recorded, forward_one_to_many and
        # forward_one_to_all score a whole call in ONE launch (readout, rp.mlp and both layers: only the logits are written), in the
        # fp32 class, where the kernel serves the module -- else today's path, whatever `fused` says
        self.fused_scores = False

    # forward_one_to_all's default route where `fused_scores` is False: the one-launch kernel, because it was MEASURED faster than the
    # composition at both all-candidates shapes of tools/score_fanout_rate.py on the MI355X (profiles/score_fanout.md; medians of 11
    # samples of 50 calls, B = 200 sources against every node, us per call, kernel against fused = False / "f32"):
    #   C2-shaped table (9 228 nodes, d = 128):   1 891 [1 887 .. 1 896]  against  6 956 [6 948 .. 6 974]  /  2 189 [2 185 .. 2 191]
    #   C3-shaped table (10 985 nodes, d = 256):  2 618 [2 612 .. 2 624]  against  8 915 [8 911 .. 8 919]  /  3 236 [3 231 .. 3 239]
    # False: the composition unless `fused_scores` is set.  forward_one_to_many is routed by `fused_scores` alone
    SCORE_ALL_FUSED = True

    def _scores_fused(self, with_embeddings: bool, forced: bool) -> bool:
        """Whether a one-to-many call takes tpnet_score_one_to_many (score_fanout.serves: host arithmetic and attribute reads)."""
        if not forced or with_embeddings or not self.not_encode or self.random_projections is None:
            return False
        ps = list(self.fc1.parameters()) + list(self.fc2.parameters()) + list(self.random_projections.mlp.parameters())
        if torch.is_grad_enabled() and any(p.requires_grad for p in ps):
            return False
        if self.fc1.weight.device.type != "cuda":
            return False
        from . import score_fanout as sf
        return sf.serves(self)

    def forward(self, src_node_ids: np.ndarray, dst_node_ids: np.ndarray, src_node_embeddings: torch.Tensor,
                dst_node_embeddings: torch.Tensor):
        rp = self.random_projections
        return self._decode(lambda: rp.get_pair_wise_feature(src_node_ids=src_node_ids, dst_node_ids=dst_node_ids),
                            src_node_embeddings, dst_node_embeddings)

    def forward_one_to_many(self, src_node_ids, cand_node_ids, src_node_embeddings: Optional[torch.Tensor] = None,
                            cand_node_embeddings: Optional[torch.Tensor] = None):
        """Extension, the ranking protocol: src_node_ids [B], cand_node_ids [B, C] -> logits [B, C].  `forward` on the expanded
        pairs (repeat(src, C), cand.reshape(-1)) with the pairwise feature taken through the module's one-to-many readout
        (`get_pair_wise_feature_one_to_many`: each source's rows fetched once for its C candidates).  Embeddings, when given, are
        per pair: [B*C, D].  With `not_encode` they may be None (`forward` would zero them: modules.py:106-108); otherwise
        ValueError.  `fused` keeps its meaning."""
        cand = cand_node_ids if isinstance(cand_node_ids, torch.Tensor) else np.asarray(cand_node_ids)
        if cand.ndim != 2 or len(src_node_ids) != cand.shape[0]:
            raise ValueError("forward_one_to_many: src_node_ids [B] and cand_node_ids [B, C] are expected")
        B, C = cand.shape
        if src_node_embeddings is None or cand_node_embeddings is None:
            if not self.not_encode:
                raise ValueError("forward_one_to_many: without not_encode the per-pair embeddings [B*C, D] are required")
            if B > 0 and C > 0 and self._scores_fused(False, bool(self.fused_scores)):
                from . import score_fanout as sf
                return sf.score(self, src_node_ids, cand_ids=cand)
            w = self.fc1.weight
            D = (self.fc1.in_features - self.random_feature_dim) // 2
            src_node_embeddings = cand_node_embeddings = torch.zeros((B * C, D), dtype=w.dtype, device=w.device)
        rp = self.random_projections
        out = self._decode(lambda: rp.get_pair_wise_feature_one_to_many(src_node_ids, cand), src_node_embeddings, cand_node_embeddings)
        return out.view(B, C, -1).squeeze(-1)

    def forward_one_to_all(self, src_node_ids, first_id: int, end_id: int, lead_node_ids=None, pairs_per_call: int = 1 << 18):
        """Extension, ranking against all nodes: src_node_ids [B] scored against EVERY id of the contiguous range [first_id, end_id)
        -> logits [B, (1 if lead_node_ids is given else 0) + end_id - first_id]; lead_node_ids [B]: one more id per row (the true
        destination of a ranking query), scored into column 0 -- the layout `LinkRankingMeter` reads.  Requires `not_encode`
        (ValueError otherwise: an embedding per (source, node) pair is out of reach).  Route: tpnet_score_one_to_many in range mode
        (no id array, only the logits written) where `fused_scores` is set -- or SCORE_ALL_FUSED, the measured default -- and the
        kernel serves the call; else the composition: `forward_one_to_many` on arange ids in slices of at most pairs_per_call pairs
        (whole rows; a row longer than that is cut along the candidates), so the method works on every state the module supports."""
        if not self.not_encode:
            raise ValueError("forward_one_to_all: the decoder must be not_encode")
        lo, hi = int(first_id), int(end_id)
        if hi <= lo:
            raise ValueError("forward_one_to_all: an id range [first_id, end_id) with at least one id")
        B = len(src_node_ids)
        if lead_node_ids is not None and len(lead_node_ids) != B:
            raise ValueError("forward_one_to_all: one lead id per source")
        if B > 0 and self._scores_fused(False, bool(self.fused_scores) or bool(self.SCORE_ALL_FUSED)):
            from . import score_fanout as sf
            return sf.score(self, src_node_ids, cand_range=(lo, hi), lead_ids=lead_node_ids)
        dev = self.fc1.weight.device
        as_dev = lambda a: a.to(dev, torch.int64) if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)
        src = as_dev(src_node_ids)
        ids = torch.arange(lo, hi, dtype=torch.int64, device=dev)
        if lead_node_ids is not None:
            cols = torch.cat([as_dev(lead_node_ids).reshape(B, 1), ids.unsqueeze(0).expand(B, -1)], dim=1)
        else:
            cols = ids.unsqueeze(0).expand(B, -1)
        C1 = cols.shape[1]
        per = max(1, int(pairs_per_call))
        rows = max(1, per // C1)                                   # whole rows per slice; one row at a time if it is longer
        parts = []
        for r0 in range(0, B, rows):
            sub = cols[r0:r0 + rows]
            if C1 <= per:
                parts.append(self.forward_one_to_many(src[r0:r0 + rows], sub.contiguous()))
            else:
                parts.append(torch.cat([self.forward_one_to_many(src[r0:r0 + rows], sub[:, c0:c0 + per].contiguous())
                                        for c0 in range(0, C1, per)], dim=1))
        if not parts:
            return torch.empty((0, C1), dtype=self.fc1.weight.dtype, device=dev)
        return torch.cat(parts, dim=0)

    def rank_one_to_all(self, src_node_ids, pos_node_ids, first_id: int, end_id: int, filter_ids: Optional[torch.Tensor] = None,
                        pairs_per_call: int = 1 << 18):
        """Extension, streaming ranking against all nodes: for row i the positive's logit p = logit(src[i], pos[i]) and, over every
        id c of [first_id, end_id) other than pos[i], the counts of the logits of (src[i], c) against it -> (counts [B, 4] int32 =
        (#{q > p}, #{q == p}, the ids counted, 2 where a NaN took part), pos_logit [B] fp32, filter_logits): the [B, 1 + C] logits
        of `forward_one_to_all` never exist.  filter_ids (optional, [B, F] int64 on the device, -1 = no entry; the layout of
        `GpuNegativeEdgeSampler.filter_lists_device`): filter_logits [B, F] = the logits of (src[i], filter_ids[i, j]) -- what
        `LinkRankingMeter.add_counts` subtracts; under a -1 slot the value is not meaningful --, else None.
        Route: where the one-launch kernel serves the module (score_fanout.serves), tpnet_score_rank_range -- the counts are formed
        in the scoring kernel -- and one list-mode `score` call for the filter lists.  Every other state: `forward_one_to_all` in
        row and column slices of at most pairs_per_call pairs, the counts formed with torch integer ops and the filter logits
        gathered from the same slices -- never more than one slice is held.  Requires `not_encode`; runs under no_grad."""
        if not self.not_encode:
            raise ValueError("rank_one_to_all: the decoder must be not_encode")
        lo, hi = int(first_id), int(end_id)
        if hi <= lo:
            raise ValueError("rank_one_to_all: an id range [first_id, end_id) with at least one id")
        B = len(src_node_ids)
        if len(pos_node_ids) != B:
            raise ValueError("rank_one_to_all: one positive id per source")
        dev = self.fc1.weight.device
        if filter_ids is not None and (not isinstance(filter_ids, torch.Tensor) or filter_ids.dtype != torch.int64 or filter_ids.dim() != 2
                                       or filter_ids.shape[0] != B or filter_ids.device != dev):
            raise TypeError(f"rank_one_to_all: filter_ids must be an int64 tensor [{B}, F] on {dev}")
        as_dev = lambda a: a.to(dev, torch.int64) if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)
        with torch.no_grad():
            if B > 0 and self._scores_fused(False, True):
                from . import score_fanout as sf
                counts, p = sf.rank_range(self, src_node_ids, pos_node_ids, (lo, hi))
                fl = None
                if filter_ids is not None:
                    pos = as_dev(pos_node_ids)
                    if filter_ids.shape[1] == 0:
                        fl = torch.empty((B, 0), dtype=torch.float32, device=dev)
                    else:
                        fl = sf.score(self, src_node_ids, cand_ids=torch.where(filter_ids < 0, pos.unsqueeze(1), filter_ids).contiguous())
                return counts, p, fl
            src, pos = as_dev(src_node_ids), as_dev(pos_node_ids)
            C = hi - lo
            per = max(2, int(pairs_per_call))
            rows = max(1, per // (C + 1))                          # whole rows per slice; one row at a time if it is longer
            width = C if C + 1 <= per else per - 1                 # columns per slice (the first one carries the positive beside them)
            counts = torch.zeros((B, 4), dtype=torch.int32, device=dev)
            p_all = torch.empty(B, dtype=torch.float32, device=dev)
            fl = torch.zeros(filter_ids.shape, dtype=torch.float32, device=dev) if filter_ids is not None else None
            for r0 in range(0, B, rows):
                r = slice(r0, min(r0 + rows, B))
                p = None
                nan = None
                for c0 in range(lo, hi, width):
                    c1 = min(c0 + width, hi)
                    x = self.forward_one_to_all(src[r], c0, c1, lead_node_ids=pos[r] if p is None else None,
                                                pairs_per_call=pairs_per_call).float()
                    if p is None:
                        p, x = x[:, :1].contiguous(), x[:, 1:]
                        nan = torch.isnan(p[:, 0])
                    on = torch.arange(c0, c1, device=dev).unsqueeze(0) != pos[r].unsqueeze(1)
                    counts[r, 0] += ((x > p) & on).sum(dim=1, dtype=torch.int32)
                    counts[r, 1] += ((x == p) & on).sum(dim=1, dtype=torch.int32)
                    counts[r, 2] += on.sum(dim=1, dtype=torch.int32)
                    nan = nan | (torch.isnan(x) & on).any(dim=1)
                    if fl is not None and fl.shape[1] > 0:
                        f = filter_ids[r]
                        inside = (f >= c0) & (f < c1)
                        fl[r] = torch.where(inside, x.gather(1, (f - c0).clamp(0, c1 - c0 - 1)), fl[r])
                p_all[r] = p[:, 0]
                counts[r, 3] = nan.to(torch.int32) * 2
            return counts, p_all, fl

    def topk_one_to_all(self, src_node_ids, k: int, first_id: int, end_id: int, skip_node_ids=None,
                        exclude_ids: Optional[torch.Tensor] = None, n_exclude: Optional[torch.Tensor] = None,
                        pairs_per_call: int = 1 << 18):
        """Extension, streaming top-k against all nodes: per row the k best ids of [first_id, end_id) by the logit of (src[i], id)
        -> (ids [B, k] int64, logits [B, k] fp32, info [B, 2] int32), best first by ONE rule (`score_fanout.topk_host`): logit
        descending with NaN first and -0.0 = +0.0, id ascending at equal logits; empty slots (fewer than k admitted ids) hold id -1
        and logit -inf; info[:, 0] = the real entries, info[:, 1] = 2 where an admitted logit is NaN | 8 where the row's exclusion
        list overflowed.  The [B, end_id - first_id] logits of `forward_one_to_all` never exist.  skip_node_ids [B] (optional): one
        id per row left out (a recommender passes the source itself); exclude_ids [B, F] int64 with n_exclude [B] int32 on the
        device (optional; ascending, distinct, -1 padded: the layout of `GpuNegativeEdgeSampler.filter_lists_device`): the ids of a
        row's first min(n_exclude, F) slots are left out.
        Route: where the one-launch kernel serves the module (score_fanout.serves) and k <= 128, tpnet_score_topk_range -- the lists
        are formed in the scoring kernel.  Every other state (and a larger k): `forward_one_to_all` in row and column slices of at
        most pairs_per_call pairs, a running best-k per row merged by the same key with torch integer ops -- never more than one
        slice is held.  Requires `not_encode`; runs under no_grad."""
        if not self.not_encode:
            raise ValueError("topk_one_to_all: the decoder must be not_encode")
        lo, hi = int(first_id), int(end_id)
        k = int(k)
        if hi <= lo or hi - lo >= 1 << 31:
            raise ValueError("topk_one_to_all: an id range [first_id, end_id) of 1 .. 2^31 - 1 ids")
        if k < 1:
            raise ValueError("topk_one_to_all: k >= 1")
        B = len(src_node_ids)
        if skip_node_ids is not None and len(skip_node_ids) != B:
            raise ValueError("topk_one_to_all: one skip id per source")
        dev = self.fc1.weight.device
        if (exclude_ids is None) != (n_exclude is None):
            raise ValueError("topk_one_to_all: exclude_ids and n_exclude come together")
        if exclude_ids is not None:
            if (not isinstance(exclude_ids, torch.Tensor) or exclude_ids.dtype != torch.int64 or exclude_ids.dim() != 2
                    or exclude_ids.shape[0] != B or exclude_ids.device != dev):
                raise TypeError(f"topk_one_to_all: exclude_ids must be an int64 tensor [{B}, F] on {dev}")
            if (not isinstance(n_exclude, torch.Tensor) or n_exclude.dtype != torch.int32 or tuple(n_exclude.shape) != (B,)
                    or n_exclude.device != dev):
                raise TypeError(f"topk_one_to_all: n_exclude must be an int32 tensor [{B}] on {dev}")
        from . import score_fanout as sf
        as_dev = lambda a: a.to(dev, torch.int64) if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)
        with torch.no_grad():
            if B > 0 and k <= sf.TOPK_MAX and self._scores_fused(False, True):
                return sf.topk_range(self, src_node_ids, k, (lo, hi), skip_ids=skip_node_ids, exclude_ids=exclude_ids,
                                     n_exclude=n_exclude)
            src = as_dev(src_node_ids)
            skip = as_dev(skip_node_ids) if skip_node_ids is not None else None
            C = hi - lo
            per = max(1, int(pairs_per_call))
            rows = max(1, per // C)                                # whole rows per slice; one row at a time if it is longer
            width = min(C, per)                                    # columns per slice
            best = torch.full((B, k), sf._EMPTY_KEY, dtype=torch.int64, device=dev)
            info = torch.zeros((B, 2), dtype=torch.int32, device=dev)
            keep = None
            if exclude_ids is not None:
                F = exclude_ids.shape[1]
                keep = (torch.arange(F, device=dev).unsqueeze(0) < n_exclude.clamp(0, F).unsqueeze(1)) & (exclude_ids >= 0)
                info[:, 1] = (n_exclude > F).to(torch.int32) * sf.FLAG_OVERFLOW
            for r0 in range(0, B, rows):
                r = slice(r0, min(r0 + rows, B))
                n_adm = torch.zeros(r.stop - r0, dtype=torch.int64, device=dev)
                nan = torch.zeros(r.stop - r0, dtype=torch.bool, device=dev)
                for c0 in range(lo, hi, width):
                    c1 = min(c0 + width, hi)
                    x = self.forward_one_to_all(src[r], c0, c1, pairs_per_call=pairs_per_call).float()
                    ids = torch.arange(c0, c1, device=dev).unsqueeze(0)
                    adm = torch.ones(x.shape, dtype=torch.bool, device=dev)
                    if skip is not None:
                        adm &= ids != skip[r].unsqueeze(1)
                    if keep is not None:
                        e = exclude_ids[r]
                        rr_, cc_ = torch.nonzero(keep[r] & (e >= c0) & (e < c1), as_tuple=True)
                        adm[rr_, e[rr_, cc_] - c0] = False
                    keys = torch.where(adm, sf.topk_keys_torch(x, ids - lo), torch.full_like(ids, sf._EMPTY_KEY))
                    best[r] = torch.sort(torch.cat([best[r], keys], dim=1), dim=1, descending=True).values[:, :k]
                    n_adm += adm.sum(dim=1)
                    nan |= (torch.isnan(x) & adm).any(dim=1)
                info[r, 0] = n_adm.clamp(max=k).to(torch.int32)
                info[r, 1] |= nan.to(torch.int32) * sf.FLAG_NAN
            out_ids, out_logits = sf.topk_decode_torch(best, lo)
            return out_ids, out_logits, info

    def _decode(self, pair_feature: Callable, src_node_embeddings: torch.Tensor, dst_node_embeddings: torch.Tensor):
        """What `forward` does with its pairs' embeddings; pair_feature() = their pairwise features (called only with a module)."""
        if isinstance(self.fused, str):
            if self.fused != "f32":
                raise ValueError(f"LinkPredictor_v1.fused: {self.fused!r} is none of False, True, 'f32'")
            return self._decode_f32(pair_feature, src_node_embeddings, dst_node_embeddings)
        if self.not_encode:                                        # modules.py:106-108
            src_node_embeddings = torch.zeros_like(src_node_embeddings)
            dst_node_embeddings = torch.zeros_like(dst_node_embeddings)
        feat = None
        if self.random_projections is not None:                    # modules.py:112-114
            feat = pair_feature()
        if self.fused and src_node_embeddings.is_cuda:
            from . import fused_decoder as fd
            D, F = src_node_embeddings.shape[1], (0 if feat is None else feat.shape[1])
            if dst_node_embeddings.shape[1] == D and fd.supported(self.fc1, self.fc2, D, F):
                return fd.fused_decoder(self, self.fc1, self.fc2, src_node_embeddings, dst_node_embeddings, feat,
                                        self.not_encode)
        parts = [src_node_embeddings, dst_node_embeddings] + ([feat] if feat is not None else [])
        return self.fc2(self.act(self.fc1(torch.cat(parts, dim=1))))

    def _decode_f32(self, pair_feature, src_emb, dst_emb):
        """fused == "f32": the fp32-class kernels on the embeddings as they are (with not_encode they are not read: no zeros are
        made) where they serve the call; anything else -- a CPU module, another dtype, an unserved shape -- is fused = False's path."""
        feat = None
        if self.random_projections is not None:                    # modules.py:112-114
            feat = pair_feature()
        if src_emb.is_cuda:
            from . import fused_decoder as fd
            if fd.serves_f32(self.fc1, self.fc2, src_emb, dst_emb, feat, self.not_encode):
                return fd.fused_decoder_f32(self.fc1, self.fc2, src_emb, dst_emb, feat, self.not_encode, checked=True)
        if self.not_encode:                                        # modules.py:106-108
            src_emb, dst_emb = torch.zeros_like(src_emb), torch.zeros_like(dst_emb)
        parts = [src_emb, dst_emb] + ([feat] if feat is not None else [])
        return self.fc2(self.act(self.fc1(torch.cat(parts, dim=1))))


class RecentNeighborSampler:
    """Most-recent-K historical neighbours, strictly before the query time, left-padded with id 0
    (utils/utils.py:140-152 searchsorted side='left'; :205-213 'recent'; adjacency built as get_neighbor_sampler
    does, :293-312: undirected, per node sorted by time, stable)."""

    def __init__(self, src_node_ids: np.ndarray, dst_node_ids: np.ndarray, node_interact_times: np.ndarray,
                 edge_ids: Optional[np.ndarray] = None):
        src = np.asarray(src_node_ids, dtype=np.int64)
        dst = np.asarray(dst_node_ids, dtype=np.int64)
        t = np.asarray(node_interact_times, dtype=np.float64)
        eid = np.arange(1, len(src) + 1, dtype=np.int64) if edge_ids is None else np.asarray(edge_ids, dtype=np.int64)
        n = int(max(src.max(), dst.max())) + 1 if len(src) else 1
        # interleave (src->dst, dst->src) per edge to keep the reference's append order, then a stable sort by
        # (node, time) gives every node's list sorted by time with ties in append order
        node = np.stack([src, dst], axis=1).reshape(-1)
        nbr = np.stack([dst, src], axis=1).reshape(-1)
        tt = np.repeat(t, 2)
        ee = np.repeat(eid, 2)
        order = np.lexsort((np.arange(len(node)), tt, node))
        self._nbr, self._t, self._e = nbr[order], tt[order], ee[order]
        self._start = np.searchsorted(node[order], np.arange(n + 1))

    def get_historical_neighbors(self, node_ids: np.ndarray, node_interact_times: np.ndarray, num_neighbors: int = 20):
        assert num_neighbors > 0
        node_ids = np.asarray(node_ids, dtype=np.int64)
        times = np.asarray(node_interact_times, dtype=np.float64)
        n = len(node_ids)
        out_ids = np.zeros((n, num_neighbors), dtype=np.int64)
        out_eid = np.zeros((n, num_neighbors), dtype=np.int64)
        out_t = np.zeros((n, num_neighbors), dtype=np.float64)
        for i in range(n):
            nid = node_ids[i]
            if nid + 1 >= len(self._start):
                continue
            lo, hi = self._start[nid], self._start[nid + 1]
            cut = lo + np.searchsorted(self._t[lo:hi], times[i])       # interactions with time < query time
            first = max(lo, cut - num_neighbors)
            k = cut - first
            if k > 0:
                out_ids[i, num_neighbors - k:] = self._nbr[first:cut]
                out_eid[i, num_neighbors - k:] = self._e[first:cut]
                out_t[i, num_neighbors - k:] = self._t[first:cut]
        return out_ids, out_eid, out_t


class RandomNegativeSampler:
    """'random' strategy of NegativeEdgeSampler (utils/utils.py:388-400): src indices are drawn first, then dst
    indices, from the sorted unique id arrays; unseeded samplers use the GLOBAL numpy RNG like the reference."""

    def __init__(self, src_node_ids: np.ndarray, dst_node_ids: np.ndarray, seed: Optional[int] = None):
        self.unique_src_node_ids = np.unique(src_node_ids)
        self.unique_dst_node_ids = np.unique(dst_node_ids)
        self.seed = seed
        self.reset_random_state()

    def reset_random_state(self):
        self.random_state = np.random.RandomState(self.seed) if self.seed is not None else None

    def sample(self, size: int):
        rng = np.random if self.random_state is None else self.random_state
        si = rng.randint(0, len(self.unique_src_node_ids), size)
        di = rng.randint(0, len(self.unique_dst_node_ids), size)
        return self.unique_src_node_ids[si], self.unique_dst_node_ids[di]


def encoder_pair_indices(neighbor_node_ids: np.ndarray, src_node_ids: np.ndarray, dst_node_ids: np.ndarray):
    """Index arrays of the encoder's readout for one (src, dst) batch of B edges (models/TPNet.py:206-217, 311-316):
    nodes = [src; dst] (2B), their K neighbours each; every neighbour w is paired with the edge's src AND dst:
    u = tile(neigh.reshape(-1), 2), v = [repeat(tile(src,2), K); repeat(tile(dst,2), K)]  -> 4*B*K pairs."""
    K = neighbor_node_ids.shape[1]
    u = np.tile(neighbor_node_ids.reshape(-1), 2)
    v = np.concatenate([np.repeat(np.tile(src_node_ids, 2), K), np.repeat(np.tile(dst_node_ids, 2), K)])
    return u, v


def link_prediction_batch(rp, neighbor_sampler, src: np.ndarray, dst: np.ndarray, neg_dst: np.ndarray, t: np.ndarray,
                          num_neighbors: int, encoder: Optional[Callable] = None, decoder: Optional[Callable] = None,
                          neg_src: Optional[np.ndarray] = None):
    """One batch in the reference's order (train_link_prediction.py:325-373, evaluate_models_utils.py:132-184):
    encoder readout for (src,dst), encoder readout for (src,neg), decoder readout (src,dst), decoder readout
    (src,neg), THEN update(src,dst,t).  `encoder(pair_features[2B,K,2*F], node_ids, times) -> [2B, D]` and
    `decoder(src_ids, dst_ids, src_emb, dst_emb) -> logits` are optional plug-ins; without them the four pairwise
    feature tensors are returned.  `neg_src` (evaluation under the 'historical' / 'inductive' negatives, whose source is
    not the batch's own: evaluate_models_utils.py:72-91): the negative readouts pair (neg_src, neg_dst); None: (src, neg_dst)."""
    B = len(src)
    pairs = ((src, dst), (src if neg_src is None else neg_src, neg_dst))
    feats = []
    embs = []
    on_device = hasattr(neighbor_sampler, "sample_device") and hasattr(rp, "get_pair_wise_feature_shared")
    if on_device:      # ids stay on the GPU from the sampler to the readout (same pairs, same order as the host path)
        dev = neighbor_sampler.device
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
        src_t = to_dev(src)
        t2_t = torch.from_numpy(np.tile(np.asarray(t, dtype=np.float64), 2)).to(dev)
    for first, other in pairs:
        node_ids = np.concatenate([first, other])
        if on_device:
            first_t = src_t if first is src else to_dev(first)
            other_t = to_dev(other)
            neigh, _, _ = neighbor_sampler.sample_device(torch.cat([first_t, other_t]), t2_t, num_neighbors, with_edges=False)
            f = rp.get_pair_wise_feature_shared(neigh.reshape(-1), first_t.repeat(2).repeat_interleave(num_neighbors),
                                                other_t.repeat(2).repeat_interleave(num_neighbors))
        else:
            neigh, _, _ = neighbor_sampler.get_historical_neighbors(node_ids=node_ids,
                                                                    node_interact_times=np.tile(t, 2),
                                                                    num_neighbors=num_neighbors)
            u, v = encoder_pair_indices(neigh, first, other)
            f = rp.get_pair_wise_feature(src_node_ids=u, dst_node_ids=v)             # [4BK, F]
        half = 2 * B * num_neighbors
        f = torch.cat([f[:half], f[half:]], dim=1).reshape(2 * B, num_neighbors, -1)  # TPNet.py:318-321
        feats.append(f)
        embs.append(encoder(f, node_ids, np.tile(t, 2)) if encoder is not None else None)
    outs = []
    for (first, other), e in zip(pairs, embs):
        if decoder is not None and e is not None:
            outs.append(decoder(src_node_ids=first, dst_node_ids=other, src_node_embeddings=e[:B], dst_node_embeddings=e[B:]))
        else:
            outs.append(rp.get_pair_wise_feature(src_node_ids=first, dst_node_ids=other))
    rp.update(src_node_ids=src, dst_node_ids=dst, node_interact_times=t)             # after both readouts (:372)
    return feats, outs


def run_evaluation(rp, neighbor_sampler, negative_sampler, src: np.ndarray, dst: np.ndarray, t: np.ndarray, batch_size: int,
                   num_neighbors: int, encoder=None, decoder=None, on_batch: Optional[Callable] = None):
    """The reference's evaluation call sequence (evaluate_models_utils.py:56-72, 182-184): chronological batches, NO reset of the
    projections; a 'historical' / 'inductive' negative sampler is given the batch's arrays and its first and last stamp and returns
    the negative source as well, a 'random' one is asked for `size` destinations and the negative source is the batch's own.
    `on_batch(index, neg_src, neg_dst, result)`."""
    results = []
    for b0 in range(0, len(src), batch_size):
        s = slice(b0, min(b0 + batch_size, len(src)))
        if negative_sampler.negative_sample_strategy != "random":
            neg_src, neg_dst = negative_sampler.sample(size=s.stop - s.start, batch_src_node_ids=src[s], batch_dst_node_ids=dst[s],
                                                       current_batch_start_time=t[s][0], current_batch_end_time=t[s][-1])
        else:
            _, neg_dst = negative_sampler.sample(size=s.stop - s.start)
            neg_src = None                                         # the batch's own source (:72)
        res = link_prediction_batch(rp, neighbor_sampler, src[s], dst[s], neg_dst, t[s], num_neighbors, encoder, decoder,
                                    neg_src=neg_src)
        if on_batch is not None:
            on_batch(b0 // batch_size, src[s] if neg_src is None else neg_src, neg_dst, res)
        results.append(res)
    return results


def evaluate_link_prediction(rp, neighbor_sampler, negative_sampler, src: np.ndarray, dst: np.ndarray, t: np.ndarray, batch_size: int,
                             num_neighbors: int, encoder: Callable, decoder: Callable, meter=None):
    """`evaluate_model_link_prediction` (evaluate_models_utils.py:52-198) on `run_evaluation`: every batch's positive and negative
    logits from `decoder` go to a `LinkPredictionMeter` (tpnet_amd/metrics.py) -- loss, average precision and ROC-AUC are computed on
    the device and no batch synchronises for them; the log is read once at the end.  -> `meter.results()`: the reference's
    `(evaluate_losses, evaluate_metrics)`, with the records' flags as `.flags`.  meter: None = a new one of one record per batch; a
    given one is appended to, and everything it holds is returned."""
    from .metrics import LinkPredictionMeter
    if meter is None:
        meter = LinkPredictionMeter(max(1, -(-len(src) // batch_size)), rp.random_projections[0].device)

    def on_batch(index, neg_src, neg_dst, result):
        pos_logits, neg_logits = result[1]
        meter.add(pos_logits, neg_logits)

    with torch.no_grad():                                          # (:52)
        run_evaluation(rp, neighbor_sampler, negative_sampler, src, dst, t, batch_size, num_neighbors, encoder, decoder,
                       on_batch=on_batch)
    return meter.results()


def evaluate_edge_bank_link_prediction(edge_bank, negative_sampler, num_history_edges: int, src: np.ndarray, dst: np.ndarray,
                                       t: np.ndarray, batch_size: int, meter=None):
    """The test loop of the reference's `evaluate_edge_bank_link_prediction` (evaluate_models_utils.py:269-318) for one run.
    `edge_bank`: a `GpuEdgeBank` over history ‖ test (train ‖ val ‖ test, `num_history_edges` = the edges before the test split);
    src / dst / t: the test split's arrays.  Chronological batches; a 'random' sampler is asked for `size` destinations and paired
    with the batch's own sources, the others are given the batch and its first and last stamp; the memory of the batch at b0 is the
    first num_history_edges + b0 edges; the 0 / 1 probabilities go to `meter.add_probabilities`.  With a sampler that has
    `sample_device` (`GpuNegativeEdgeSampler`) the ids never leave the device and no batch synchronises.  -> `meter.results()`: the
    reference's per-batch `(test_losses, test_metrics)`.  meter: None = a new one of one record per batch."""
    from .metrics import LinkPredictionMeter
    dev = edge_bank.device
    if meter is None:
        meter = LinkPredictionMeter(max(1, -(-len(src) // batch_size)), dev)
    to_dev = lambda a: a.to(dev, torch.int64).contiguous() if isinstance(a, torch.Tensor) \
        else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
    src_d, dst_d = to_dev(src), to_dev(dst)
    on_device = hasattr(negative_sampler, "sample_device")
    for b0 in range(0, len(src), batch_size):
        s = slice(b0, min(b0 + batch_size, len(src)))
        size = s.stop - s.start
        if negative_sampler.negative_sample_strategy != "random":                    # (:275-281)
            if on_device:
                neg_src, neg_dst = negative_sampler.sample_device(size, src_d[s], dst_d[s], float(t[s][0]), float(t[s][-1]))
            else:
                neg_src, neg_dst = negative_sampler.sample(size=size, batch_src_node_ids=src[s], batch_dst_node_ids=dst[s],
                                                           current_batch_start_time=t[s][0], current_batch_end_time=t[s][-1])
        else:                                                                        # (:283-284)
            _, neg_dst = negative_sampler.sample_device(size) if on_device else negative_sampler.sample(size=size)
            neg_src = src_d[s]
        pos_prob, neg_prob = edge_bank.predict_device(num_history_edges + b0, src_d[s], dst_d[s], to_dev(neg_src), to_dev(neg_dst))
        meter.add_probabilities(pos_prob, neg_prob)
    return meter.results()


def evaluate_link_ranking(rp, negative_sampler, src, dst, t, batch_size: int, num_negatives: int, decoder, encoder: Optional[Callable] = None,
                          num_historical: Optional[int] = None, candidates=None, meter=None, pairs_per_call: int = 1 << 18):
    """One-vs-many ranking evaluation (extension: the protocol temporal link prediction is reported with today; the reference scores
    one negative per positive): every positive edge (s, d, t) is ranked against Q = num_negatives negative destinations of the same
    source at the same time; MRR and Hits@k per batch from a `LinkRankingMeter` (tpnet_amd/metrics.py).  Under no_grad, chronological
    batches with a ragged tail, no reset of the projections.  Per batch:
      1. the candidates [b, Q]: rows of `candidates` (host or device [E, Q], -1 = absent) if given, else
         `negative_sampler.sample_many_device(src, dst, t, Q, num_historical)`;
      2. the logits [b, 1 + Q] over [dst | candidates], an absent slot scored as the row's true destination (and not ranked):
         encoder None: `decoder.forward_one_to_many(src, ids)` (the decoder must be `not_encode`); else `encoder(src_ids, dst_ids,
         times) -> (src_emb, dst_emb)` on the expanded pairs (TPNet.compute_src_dst_node_temporal_embeddings' signature), in slices of
         at most pairs_per_call pairs, and the embeddings go to `forward_one_to_many`;
      3. `rp.update(src, dst, t)` AFTER scoring (evaluate_models_utils.py:182-184);
      4. `meter.add(logits, candidates)`.
    Candidates and logits never leave the device and no batch synchronises for the metric (`update` plans from host arrays: a
    stream given as device tensors is copied to the host once, before the loop).  -> `meter.results()`.  meter: None = a new one of one
    record per batch; a given one is appended to.  Composes with `evaluate_with_restore`."""
    from .metrics import LinkRankingMeter
    dev = rp.random_projections[0].device
    E, Q = len(src), int(num_negatives)
    if meter is None:
        meter = LinkRankingMeter(max(1, -(-E // batch_size)), dev)
    to_dev = lambda a, dt: a.to(dev, dt).contiguous() if isinstance(a, torch.Tensor) \
        else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64 if dt == torch.int64 else np.float64)).to(dev)
    src_d, dst_d, t_d = to_dev(src, torch.int64), to_dev(dst, torch.int64), to_dev(t, torch.float64)
    # `update` plans a batch from host arrays and reads its last stamp on the host: one copy of the stream, before the loop
    to_host = lambda a, dt: a.cpu().numpy().astype(dt, copy=False) if isinstance(a, torch.Tensor) else np.ascontiguousarray(a, dtype=dt)
    src_h, dst_h, t_h = to_host(src, np.int64), to_host(dst, np.int64), to_host(t, np.float64)
    cand_all = to_dev(candidates, torch.int64) if candidates is not None else None
    if cand_all is not None and tuple(cand_all.shape) != (E, Q):
        raise ValueError(f"candidates must be [{E}, {Q}]")
    with torch.no_grad():
        for b0 in range(0, E, batch_size):
            s = slice(b0, min(b0 + batch_size, E))
            b = s.stop - s.start
            if cand_all is not None:
                cand = cand_all[s]
            else:
                cand, _ = negative_sampler.sample_many_device(src_d[s], dst_d[s], t_d[s], Q, num_historical)
            # ---- from here on given and sampled candidates take the same code
            ids = torch.cat([dst_d[s].unsqueeze(1), torch.where(cand < 0, dst_d[s].unsqueeze(1), cand)], dim=1).contiguous()
            if encoder is None:
                logits = decoder.forward_one_to_many(src_d[s], ids)
            else:
                n = b * (Q + 1)
                es, ed = src_d[s].repeat_interleave(Q + 1), ids.reshape(-1)
                et = t_d[s].repeat_interleave(Q + 1)
                parts = [encoder(es[p0:p0 + pairs_per_call], ed[p0:p0 + pairs_per_call], et[p0:p0 + pairs_per_call])
                         for p0 in range(0, n, pairs_per_call)]
                logits = decoder.forward_one_to_many(src_d[s], ids, torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
            rp.update(src_h[s], dst_h[s], t_h[s])                   # after scoring (:182-184)
            meter.add(logits.reshape(b, Q + 1).float(), cand)
    return meter.results()


def recommend_links(decoder, src_node_ids, k: int, candidate_range, streaming: bool = False, exclude: Optional[str] = None,
                    negative_sampler=None, exclude_self: bool = False):
    """"Which k nodes is u most likely to link to now?": `decoder.forward_one_to_all(src_node_ids, lo, hi)` over candidate_range =
    (lo, hi), then `torch.topk` -> (ids [B, k] int64, logits [B, k]), best first, on the decoder's device.  Plain torch behind the
    scores; under no_grad.
    STREAMING (streaming = True, exclude = 'known' or exclude_self = True; the defaults are the lines above, bit for bit):
    `decoder.topk_one_to_all` -- the k best are kept where the scores are formed (tpnet_score_topk_range where the kernel serves the
    module) and no [B, hi - lo] tensor is built, so neither the logits' memory nor n_rows (1 + C) < 2^31 bound the range.  Same
    values as the default; at EQUAL logits the smaller id comes first (torch.topk promises no order there), NaN first, -0.0 = +0.0.
    exclude = 'known': the destinations the source already has in negative_sampler's table (a `GpuNegativeEdgeSampler`; ValueError
    without one) are left out -- `negative_sampler.filter_lists_device(src, -1, 0, 'known', (lo, hi))`: a destination of -1 drops no
    id from a list.  exclude_self: the source itself is left out.  A row with fewer than k admitted ids ends in empty slots: id -1,
    logit -inf."""
    lo, hi = int(candidate_range[0]), int(candidate_range[1])
    if not 1 <= int(k) <= hi - lo:
        raise ValueError("recommend_links: 1 <= k <= the number of candidates")
    if exclude is not None and exclude != "known":
        raise ValueError(f"recommend_links: exclude {exclude!r} is none of None, 'known'")
    if exclude == "known" and negative_sampler is None:
        raise ValueError("recommend_links: exclude = 'known' needs negative_sampler (a GpuNegativeEdgeSampler)")
    if streaming or exclude is not None or exclude_self:
        dev = decoder.fc1.weight.device
        src = (src_node_ids.to(dev, torch.int64) if isinstance(src_node_ids, torch.Tensor)
               else torch.from_numpy(np.asarray(src_node_ids, dtype=np.int64)).to(dev))
        fil = n_fil = None
        if exclude == "known":
            fil, n_fil = negative_sampler.filter_lists_device(src, torch.full_like(src, -1), torch.zeros(len(src), dtype=torch.float64, device=dev),
                                                              "known", (lo, hi))
        ids, logits, _ = decoder.topk_one_to_all(src, int(k), lo, hi, skip_node_ids=src if exclude_self else None, exclude_ids=fil,
                                                 n_exclude=n_fil)
        return ids, logits
    with torch.no_grad():
        logits = decoder.forward_one_to_all(src_node_ids, lo, hi)
        top = torch.topk(logits, int(k), dim=1)
    return top.indices + lo, top.values


def evaluate_link_ranking_all(rp, src, dst, t, batch_size: int, decoder, candidate_range=None, meter=None, filter: Optional[str] = None,
                              negative_sampler=None, streaming: bool = False):
    """Ranking evaluation against ALL candidates (extension): every positive edge (s, d, t) is ranked among every node of
    candidate_range = (lo, hi) -- default (1, rp.node_num): id 0 is the reference's padding row; a bipartite data set passes its item
    range -- instead of among sampled negatives.  UNFILTERED protocol: only the query's own destination is dropped from the
    candidates; other true destinations of the same source stay in as candidates.  The decoder must be `not_encode`.  Under no_grad,
    chronological batches with a ragged tail, no reset of the projections.  Per batch:
      1. `logits = decoder.forward_one_to_all(src, lo, hi, lead_node_ids=dst)`: [b, 1 + (hi - lo)], column 0 the true destination;
      2. `skip = dst - lo` where lo <= dst < hi, else -1: the destination's own column among the candidates;
      3. `rp.update(src, dst, t)` AFTER scoring (evaluate_models_utils.py:182-184), the order of `evaluate_link_ranking`;
      4. `meter.add_skip(logits, skip)` (tpnet_lp_ranking_skip: no [b, hi - lo] mask is built).
    Nothing leaves the device and no batch synchronises for the metric.  -> `meter.results()`.  meter: None = a new
    `LinkRankingMeter` of one record per batch; a given one is appended to.  Composes with `evaluate_with_restore`.
    STREAMING (streaming = True, or a filter): the counts are formed where the scores are and no [b, hi - lo] tensor is built, so
    neither the logits' memory nor the MAX_RANK_COLUMNS of one record bound the range.  Per batch:
      1. with a filter, `fil, n_fil = negative_sampler.filter_lists_device(src, dst, t, filter, (lo, hi))`: per query the
         destinations the FILTERED protocol drops from its candidates -- filter = 'same_time': other positives of the same source at
         the same instant, `evaluate_link_ranking`'s (tpnet_neg_sample_many's) notion of a negative; 'known': every destination the
         source has an edge to anywhere in the stream the sampler was built on, the filtered setting papers report.  A filter needs
         the sampler (`GpuNegativeEdgeSampler`, built on the whole stream): ValueError without one;
      2. `counts, pos_logit, fil_logits = decoder.rank_one_to_all(src, dst, lo, hi, filter_ids=fil)`;
      3. `rp.update(src, dst, t)` AFTER scoring;
      4. `meter.add_counts(counts, pos_logit, fil_logits, fil, n_fil)` (tpnet_lp_ranking_counts).
    With the defaults (filter None, streaming False) the function is what it was."""
    from .metrics import LinkRankingMeter, MAX_RANK_COLUMNS
    dev = rp.random_projections[0].device
    lo, hi = (1, int(rp.node_num)) if candidate_range is None else (int(candidate_range[0]), int(candidate_range[1]))
    if hi <= lo:
        raise ValueError("candidate_range: (lo, hi) with lo < hi")
    if filter not in (None, "same_time", "known"):
        raise ValueError(f"filter: {filter!r} is none of None, 'same_time', 'known'")
    if filter is not None and negative_sampler is None:
        raise ValueError("evaluate_link_ranking_all: a filter needs negative_sampler (its table holds the stream's edges)")
    streaming = bool(streaming) or filter is not None
    if not streaming and 1 + (hi - lo) > MAX_RANK_COLUMNS:
        raise ValueError(f"evaluate_link_ranking_all: 1 + {hi - lo} candidates exceed the {MAX_RANK_COLUMNS} columns of one ranking record")
    E = len(src)
    if meter is None:
        meter = LinkRankingMeter(max(1, -(-E // batch_size)), dev)
    to_dev = lambda a: a.to(dev, torch.int64).contiguous() if isinstance(a, torch.Tensor) \
        else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
    src_d, dst_d = to_dev(src), to_dev(dst)
    # `update` plans a batch from host arrays and reads its last stamp on the host: one copy of the stream, before the loop
    to_host = lambda a, dt: a.cpu().numpy().astype(dt, copy=False) if isinstance(a, torch.Tensor) else np.ascontiguousarray(a, dtype=dt)
    src_h, dst_h, t_h = to_host(src, np.int64), to_host(dst, np.int64), to_host(t, np.float64)
    if streaming:
        t_d = t.to(dev, torch.float64).contiguous() if isinstance(t, torch.Tensor) else torch.from_numpy(t_h).to(dev)
        for b0 in range(0, E, batch_size):
            s = slice(b0, min(b0 + batch_size, E))
            fil = n_fil = None
            if filter is not None:
                fil, n_fil = negative_sampler.filter_lists_device(src_d[s], dst_d[s], t_d[s], filter, (lo, hi))
            counts, pos_logit, fil_logits = decoder.rank_one_to_all(src_d[s], dst_d[s], lo, hi, filter_ids=fil)
            rp.update(src_h[s], dst_h[s], t_h[s])                   # after scoring (:182-184)
            meter.add_counts(counts, pos_logit, fil_logits, fil, n_fil)
        return meter.results()
    with torch.no_grad():
        for b0 in range(0, E, batch_size):
            s = slice(b0, min(b0 + batch_size, E))
            logits = decoder.forward_one_to_all(src_d[s], lo, hi, lead_node_ids=dst_d[s])
            d = dst_d[s]
            skip = torch.where((d >= lo) & (d < hi), d - lo, torch.full_like(d, -1))
            rp.update(src_h[s], dst_h[s], t_h[s])                   # after scoring (:182-184)
            meter.add_skip(logits.float(), skip)
    return meter.results()


def run_epoch(rp, neighbor_sampler, negative_sampler, src: np.ndarray, dst: np.ndarray, t: np.ndarray,
              batch_size: int, num_neighbors: int, encoder=None, decoder=None, on_batch: Optional[Callable] = None,
              after_reset: Optional[Callable] = None):
    """reset at epoch start (:246-248), chronological `range(0, E, B)` batches with a ragged tail
    (utils/DataLoader.py:31-45, shuffle=False), negatives drawn per batch (:259)."""
    rp.reset_random_projections()
    if after_reset is not None:
        after_reset(rp)           # e.g. inject a fixed P[0] (reset redraws it from the device RNG, TPNet.py:138-139)
    results = []
    for b0 in range(0, len(src), batch_size):
        s = slice(b0, min(b0 + batch_size, len(src)))
        _, neg = negative_sampler.sample(size=s.stop - s.start)
        res = link_prediction_batch(rp, neighbor_sampler, src[s], dst[s], neg, t[s], num_neighbors, encoder, decoder)
        if on_batch is not None:
            on_batch(b0 // batch_size, neg, res)
        results.append(res)
    return results


def train_link_prediction_epoch(rp, neighbor_sampler, negative_sampler, src: np.ndarray, dst: np.ndarray, t: np.ndarray,
                                batch_size: int, num_neighbors: int, encoder: Callable, decoder: Callable, optimizer, meter=None,
                                on_batch: Optional[Callable] = None):
    """One training epoch of train_link_prediction.py:246-386 on `link_prediction_batch`: reset of the projections, then per
    chronological batch (ragged tail included) the negatives, the two encoder readouts, the two decoder calls, the update, the loss,
    `optimizer.zero_grad()`, `loss.backward()`, `optimizer.step()`.  The loss is `meter.add_training(pos_logits, neg_logits)`
    (tpnet_amd/metrics.py): a device scalar whose launches also log the batch's loss, average precision and ROC-AUC, so nothing in
    the loop synchronises for `train_losses` / `train_metrics` -- what `encoder`, `decoder`, the samplers and `optimizer` do is
    theirs.  `on_batch(index, neg_dst, result, loss)` runs after the step.  -> `meter.results()`, read once after the last batch: the
    reference's `(train_losses, train_metrics)`, with the records' flags as `.flags`.  meter: None = a new one of one record per
    batch; a given one is appended to, and everything it holds is returned."""
    from .metrics import LinkPredictionMeter
    if meter is None:
        meter = LinkPredictionMeter(max(1, -(-len(src) // batch_size)), rp.random_projections[0].device)
    rp.reset_random_projections()                                                     # (:246-248)
    for b0 in range(0, len(src), batch_size):
        s = slice(b0, min(b0 + batch_size, len(src)))
        _, neg = negative_sampler.sample(size=s.stop - s.start)                      # (:259)
        res = link_prediction_batch(rp, neighbor_sampler, src[s], dst[s], neg, t[s], num_neighbors, encoder, decoder)
        pos_logits, neg_logits = res[1]
        loss = meter.add_training(pos_logits, neg_logits)                            # (:375-382)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        if on_batch is not None:
            on_batch(b0 // batch_size, neg, res, loss)
    return meter.results()


def create_optimizer(model: nn.Module, optimizer_name: str, learning_rate: float, weight_decay: float = 0.0, device_step: bool = True):
    """utils.create_optimizer (utils/utils.py:61-79): 'Adam', 'SGD' or 'RMSprop' over `model.parameters()`.  device_step: the step of
    every fp32 tensor on a GPU is one launch (tpnet_amd/optimizer.py; same state_dict as torch's classes, and a model that is moved to
    the GPU after this call, as train_link_prediction.py:220-223 does, is served from its first step); False: exactly the reference's
    torch.optim objects."""
    from . import optimizer as O
    classes = {"Adam": (O.DeviceAdam, torch.optim.Adam), "SGD": (O.DeviceSGD, torch.optim.SGD),
               "RMSprop": (O.DeviceRMSprop, torch.optim.RMSprop)}
    if optimizer_name not in classes:
        raise ValueError(f"Wrong value for optimizer {optimizer_name}!")
    cls = classes[optimizer_name][0 if device_step else 1]
    return cls(params=model.parameters(), lr=learning_rate, weight_decay=weight_decay)


def evaluate_with_restore(rp, evaluate: Callable):
    """The backup / evaluate / reload pattern of train_link_prediction.py:403-494: run `evaluate()` (which updates the
    state while it streams the split) and put the pre-evaluation state back."""
    saved = rp.backup_random_projections()
    try:
        return evaluate()
    finally:
        rp.reload_random_projections(saved)
