"""One source against many candidates scored in ONE launch (C ABI: tpnet_score_one_to_many; csrc/score_fanout.hip): the fan-out
readout, `rp.mlp` and LinkPredictor_v1's two layers (not_encode: the embedding columns of fc1 meet zeros) with nothing but the
logits written.  `serves` is the route question `LinkPredictor_v1.forward_one_to_many` / `forward_one_to_all` ask with
`fused_scores` set; `score` is the call; `score_one_to_many_host` is the four lines in float64 numpy, what the kernel is held to.
`rank_range` (C ABI: tpnet_score_rank_range) ranks each row's positive against a whole id range with the counts formed in the same
kernel: no logit matrix exists."""
import numpy as np
import torch

from . import _lib
from . import fused_feature as _ff

# launches made through this module (tests assert the dispatch through it)
calls = {"score": 0, "rank": 0}


def score_one_to_many_host(features, mlp, fc1, fc2, off):
    """features [n, 64] -> logits [n] in float64 numpy:
         y = W2m relu(W1m f + b1m) + b2m;  a = Wd[:, off:off+64] y + bd;  logit = wd2 relu(a) + bd2
    mlp = (W1m [256, 64], b1m, W2m [64, 256], b2m), fc1 = (Wd [H, ldw], bd), fc2 = (wd2 [1, H] or [H], bd2), arrays or tensors.
    Also returns the magnitudes an error bound needs, all float64:
      'y' [n, 64], 'mag_y' = |W2m| relu(|W1m||f| + |b1m|) + |b2m|, 'mag_a' = |Wd_f||y| + |bd|  [n, H],
      'abs_wdf' = |Wd_f| [H, 64], 'abs_wd2' [H], 'abs_bd2' (a float)."""
    f64 = lambda a: (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)
    f = f64(features)
    w1, b1, w2, b2 = (f64(a) for a in mlp)
    wd, bd = f64(fc1[0]), f64(fc1[1])
    wd2, bd2 = f64(fc2[0]).reshape(-1), float(f64(fc2[1]).reshape(-1)[0])
    wdf = wd[:, off:off + f.shape[1]]
    hid = np.maximum(f @ w1.T + b1, 0.0)
    y = hid @ w2.T + b2
    a = y @ wdf.T + bd
    logit = np.maximum(a, 0.0) @ wd2 + bd2
    mag_y = np.maximum(np.abs(f) @ np.abs(w1).T + np.abs(b1), 0.0) @ np.abs(w2).T + np.abs(b2)
    mag_a = np.abs(y) @ np.abs(wdf).T + np.abs(bd)
    return logit, {"y": y, "mag_y": mag_y, "mag_a": mag_a, "abs_wdf": np.abs(wdf), "abs_wd2": np.abs(wd2), "abs_bd2": abs(bd2)}


def _mlp_prepared(rp):
    """rp.mlp's prepared fp32 layouts where it is the reference's Linear-ReLU-Linear on the GPU (not the opt-in bf16 layers)."""
    if rp.fused_mlp or rp.num_layer != 3:
        return None
    prep = _ff.prepared(rp.mlp, rp.pair_wise_feature_dim)
    return prep if (prep is not None and prep.st.w1 and prep.st.w2f) else None


def _decoder_ok(decoder):
    fc1, fc2 = decoder.fc1, decoder.fc2
    if not (isinstance(fc1, torch.nn.Linear) and isinstance(fc2, torch.nn.Linear) and fc2.out_features == 1
            and fc1.bias is not None and fc2.bias is not None and fc2.in_features == fc1.out_features):
        return False
    return all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in (fc1.weight, fc1.bias, fc2.weight, fc2.bias))


def serves(decoder) -> bool:
    """Whether tpnet_score_one_to_many takes `decoder`'s one-to-many calls: `not_encode`, a module on the GPU with rows the kernel
    serves (no `use_matrix`, no `padded_rows`, num_layer 3, dim % 4 == 0 in 36..512) and the reference `mlp`, one fp32 output."""
    rp = decoder.random_projections
    if rp is None or not decoder.not_encode or decoder.random_feature_dim != 64 or not _decoder_ok(decoder):
        return False
    if rp.use_matrix or rp.num_layer != 3 or rp._plist()[0].device.type != "cuda" or rp._plist()[0].device != decoder.fc1.weight.device:
        return False
    prep = _mlp_prepared(rp)
    if prep is None:
        return False
    rp._ensure_engine()
    if rp.engine_dim != rp.dim:
        return False
    fc1 = decoder.fc1
    off = fc1.in_features - 64
    return bool(_lib.load().tpnet_score_one_to_many_supported(rp._st_ref(), prep.ref, fc1.out_features, off, fc1.in_features))


def score(decoder, src_ids, cand_ids=None, cand_range=None, lead_ids=None, want_gram: bool = False):
    """The C call on `decoder` (serves() holds): src_ids [B]; cand_ids [B, C] (list mode) or cand_range = (lo, hi) (range mode: the
    ids lo .. hi - 1 for every row); lead_ids [B] (optional: one more id per row, scored into column 0).  -> logits [B, C_1] fp32 on
    the GPU, C_1 = C or 1 + C; with want_gram (logits, features [B, C_1, 64]).  No gradient, no synchronisation."""
    rp = decoder.random_projections
    rp._ensure_engine()
    prep = _mlp_prepared(rp)
    if prep is None:
        raise _lib.TPNetHipError("score_one_to_many: rp.mlp is not the reference's Linear-ReLU-Linear on the GPU")
    dev = rp._dev()
    if (cand_ids is None) == (cand_range is None):
        raise ValueError("score: exactly one of cand_ids and cand_range")
    B = len(src_ids)
    arrays = [rp._ids(src_ids, "src_ids")]
    if cand_ids is not None:
        cd = cand_ids if isinstance(cand_ids, torch.Tensor) else np.asarray(cand_ids)
        if cd.ndim != 2 or cd.shape[0] != B:
            raise ValueError("cand_ids must be [B, C] with one row per source")
        Cn, lo = int(cd.shape[1]), 0
        arrays.append(rp._ids(cd.reshape(-1), "cand_ids"))
    else:
        lo, hi = int(cand_range[0]), int(cand_range[1])
        Cn = hi - lo
    if lead_ids is not None:
        if len(lead_ids) != B:
            raise ValueError("one lead id per source")
        arrays.append(rp._ids(lead_ids, "lead_ids"))
    C1 = Cn + (1 if lead_ids is not None else 0)
    out = torch.empty((B, C1), dtype=torch.float32, device=dev)
    gram = torch.empty((B, C1, 64), dtype=torch.float32, device=dev) if want_gram else None
    if Cn < 1:
        raise ValueError("score: at least one candidate per row")
    if B == 0:
        return (out, gram) if want_gram else out
    devs = list(rp._to_device(*arrays))
    s = devs.pop(0)
    c = devs.pop(0) if cand_ids is not None else None
    ld = devs.pop(0) if lead_ids is not None else None
    fc1, fc2 = decoder.fc1, decoder.fc2
    _lib.check(_lib.load().tpnet_score_one_to_many(
        rp._st_ref(), s.data_ptr(), None if c is None else c.data_ptr(), lo, None if ld is None else ld.data_ptr(), B, Cn,
        rp._now_host, float(rp.time_decay_weight), _lib.FLAG_NOT_SCALE if rp.not_scale else 0, prep.ref, fc1.weight.data_ptr(),
        fc1.in_features, fc1.in_features - 64, fc1.bias.data_ptr(), fc2.weight.data_ptr(), fc2.bias.data_ptr(), fc1.out_features,
        None if gram is None else gram.data_ptr(), out.data_ptr(), rp._stream()), "score_one_to_many")
    calls["score"] += 1
    return (out, gram) if want_gram else out


def rank_range(decoder, src_ids, pos_ids, cand_range):
    """tpnet_score_rank_range on `decoder` (serves() holds): src_ids [B], pos_ids [B], cand_range = (lo, hi) -> (counts [B, 4] int32,
    pos_logit [B] fp32) on the GPU.  counts[i] = (g, e, nv, flags): over the ids c of [lo, hi) other than pos_ids[i], how many logits
    of (src_ids[i], c) are above / equal to pos_logit[i] = the logit of (src_ids[i], pos_ids[i]), how many were counted, and 2 where a
    NaN took part -- exactly what `score(cand_range=, lead_ids=pos_ids)` and the integer rule give, without the [B, 1 + hi - lo]
    logits.  No gradient, no synchronisation; the scratch is the call's own."""
    rp = decoder.random_projections
    rp._ensure_engine()
    prep = _mlp_prepared(rp)
    if prep is None:
        raise _lib.TPNetHipError("score_rank_range: rp.mlp is not the reference's Linear-ReLU-Linear on the GPU")
    dev = rp._dev()
    lo, hi = int(cand_range[0]), int(cand_range[1])
    Cn, B = hi - lo, len(src_ids)
    if Cn < 1 or Cn >= 1 << 31:
        raise ValueError("rank_range: 1 <= hi - lo < 2^31 candidates")
    if len(pos_ids) != B:
        raise ValueError("one positive id per source")
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    pos_logit = torch.empty(B, dtype=torch.float32, device=dev)
    if B == 0:
        return counts, pos_logit
    s, p = rp._to_device(rp._ids(src_ids, "src_ids"), rp._ids(pos_ids, "pos_ids"))
    lib = _lib.load()
    need = lib.tpnet_score_rank_scratch_bytes(B, Cn)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    fc1, fc2 = decoder.fc1, decoder.fc2
    _lib.check(lib.tpnet_score_rank_range(
        rp._st_ref(), s.data_ptr(), p.data_ptr(), lo, B, Cn, rp._now_host, float(rp.time_decay_weight),
        _lib.FLAG_NOT_SCALE if rp.not_scale else 0, prep.ref, fc1.weight.data_ptr(), fc1.in_features, fc1.in_features - 64,
        fc1.bias.data_ptr(), fc2.weight.data_ptr(), fc2.bias.data_ptr(), fc1.out_features, scratch.data_ptr(), scratch.numel(),
        pos_logit.data_ptr(), counts.data_ptr(), rp._stream()), "score_rank_range")
    calls["rank"] += 1
    return counts, pos_logit
