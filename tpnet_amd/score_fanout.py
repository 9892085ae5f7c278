"""One source against many candidates scored in ONE launch (C ABI: tpnet_score_one_to_many; csrc/score_fanout.hip): the fan-out
readout, `rp.mlp` and LinkPredictor_v1's two layers (not_encode: the embedding columns of fc1 meet zeros) with nothing but the
logits written.  `serves` is the route question `LinkPredictor_v1.forward_one_to_many` / `forward_one_to_all` ask with
`fused_scores` set; `score` is the call; `score_one_to_many_host` is the four lines in float64 numpy, what the kernel is held to.
`rank_range` (C ABI: tpnet_score_rank_range) ranks each row's positive against a whole id range with the counts formed in the same
kernel: no logit matrix exists.  `topk_range` (C ABI: tpnet_score_topk_range) keeps each row's k best ids of a whole id range in the
same kernel; `topk_host` is its rule in numpy -- the specification every route of `LinkPredictor_v1.topk_one_to_all` is held to."""
import numpy as np
import torch

from . import _lib
from . import fused_feature as _ff

# launches made through this module (tests assert the dispatch through it)
calls = {"score": 0, "rank": 0, "topk": 0}

TOPK_MAX = 128                    # tpnet_score_topk_range's largest k (the units' lists live in LDS)
FLAG_NAN, FLAG_OVERFLOW = 2, 8    # info[:, 1] of a top-k call: the ranking records' flag values


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


# ---- top-k: ONE order, on 64-bit keys (include/tpnet_hip.h at tpnet_score_topk_range).  key = hi32 << 32 | lo32, larger = better:
# hi32 = 0xFFFFFFFF for NaN (first, as in torch.topk), else the monotone map of the fp32 bits of q + 0.0 (-0.0 ties with +0.0);
# lo32 = 0xFFFFFFFF - (id - lo) (the smaller id wins a tie); key 0 = an empty slot.

def _keys_host(q, col):
    """logits q (fp32 array) and their columns (id - lo, broadcastable) -> uint64 keys."""
    q = np.asarray(q, dtype=np.float32) + np.float32(0.0)
    b = q.view(np.uint32)
    hi = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    hi = np.where(np.isnan(q), np.uint32(0xFFFFFFFF), hi)
    lo32 = (np.uint64(0xFFFFFFFF) - np.asarray(col).astype(np.uint64)).astype(np.uint64)
    return (hi.astype(np.uint64) << np.uint64(32)) | lo32


def _decode_host(keys, lo):
    """uint64 keys -> (ids int64, logits fp32); key 0: id -1, logit -inf."""
    keys = np.asarray(keys, dtype=np.uint64)
    hi = (keys >> np.uint64(32)).astype(np.uint32)
    b = np.where(hi & np.uint32(0x80000000), hi ^ np.uint32(0x80000000), ~hi).astype(np.uint32)
    logit = b.view(np.float32).copy()
    logit[hi == np.uint32(0xFFFFFFFF)] = np.nan
    ids = int(lo) + (np.int64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF)).astype(np.int64))
    empty = keys == 0
    logit[empty] = -np.inf
    ids[empty] = -1
    return ids, logit


def topk_host(logits, k, lo, skip_ids=None, exclude_ids=None, n_exclude=None):
    """The rule of tpnet_score_topk_range in numpy.  logits [B, C]: column c is id lo + c.  skip_ids [B] (optional): the one id a row
    leaves out; exclude_ids [B, F] int64 (optional; ascending, distinct, -1 padded) with n_exclude [B] (the lists' true lengths;
    default: the entries >= 0): the ids of the first min(n_exclude, F) slots are left out.  -> (ids [B, k] int64, logits [B, k] fp32,
    info [B, 2] int32): best first by the key -- logit descending (NaN first, -0.0 = +0.0), id ascending at equal logits; empty slots
    id -1 / logit -inf; info[:, 0] = n_valid = min(k, admitted ids); info[:, 1] = 2 where an admitted logit is NaN | 8 where
    n_exclude > F."""
    x = np.asarray(logits, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("topk_host: logits [B, C]")
    B, C = x.shape
    k = int(k)
    if k < 1:
        raise ValueError("topk_host: k >= 1")
    col = np.arange(C, dtype=np.int64)
    adm = np.ones((B, C), dtype=bool)
    if skip_ids is not None:
        adm &= (int(lo) + col)[None, :] != np.asarray(skip_ids, dtype=np.int64).reshape(B, 1)
    over = np.zeros(B, dtype=bool)
    if exclude_ids is not None:
        ex = np.asarray(exclude_ids, dtype=np.int64).reshape(B, -1)
        F = ex.shape[1]
        n_ex = (ex >= 0).sum(axis=1) if n_exclude is None else np.asarray(n_exclude, dtype=np.int64).reshape(B)
        over = n_ex > F
        for i in range(B):
            e = ex[i, :max(0, min(int(n_ex[i]), F))] - int(lo)
            e = e[(e >= 0) & (e < C)]
            adm[i, e] = False
    keys = np.where(adm, _keys_host(x, col[None, :]), np.uint64(0))
    keys = np.sort(keys.astype(np.uint64), axis=1)[:, ::-1]
    if k > C:
        keys = np.concatenate([keys, np.zeros((B, k - C), dtype=np.uint64)], axis=1)
    keys = np.ascontiguousarray(keys[:, :k])
    ids, out = _decode_host(keys, lo)
    with np.errstate(invalid="ignore"):
        nan = (np.isnan(x) & adm).any(axis=1)
    info = np.stack([np.minimum(k, adm.sum(axis=1)), FLAG_NAN * nan + FLAG_OVERFLOW * over], axis=1).astype(np.int32)
    return ids, out, info


_EMPTY_KEY = -2 ** 63             # key 0 of the rule in the signed form below


def topk_keys_torch(q, col):
    """The keys of logits q (fp32 tensor) at columns col (int64, id - lo, broadcastable) as SIGNED int64: key - 2^63, so that torch's
    integer compare is the unsigned compare of the rule; an empty slot is _EMPTY_KEY."""
    q = q.float() + 0.0
    b = q.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    hi = torch.where((b & 0x80000000) != 0, ~b & 0xFFFFFFFF, b | 0x80000000)
    hi = torch.where(torch.isnan(q), torch.full_like(hi, 0xFFFFFFFF), hi)
    return (hi - 0x80000000) * (1 << 32) + (0xFFFFFFFF - col)


def topk_decode_torch(keys, lo):
    """topk_keys_torch's keys -> (ids int64, logits fp32); _EMPTY_KEY: id -1, logit -inf."""
    hi = (keys >> 32) + 0x80000000
    b = torch.where((hi & 0x80000000) != 0, hi ^ 0x80000000, ~hi & 0xFFFFFFFF)
    logit = (((b ^ 0x80000000) - 0x80000000).to(torch.int32)).view(torch.float32).clone()
    logit[hi == 0xFFFFFFFF] = float("nan")
    ids = int(lo) + (0xFFFFFFFF - (keys & 0xFFFFFFFF))
    empty = keys == _EMPTY_KEY
    logit[empty] = float("-inf")
    ids[empty] = -1
    return ids, logit


def topk_range(decoder, src_ids, k, cand_range, skip_ids=None, exclude_ids=None, n_exclude=None):
    """tpnet_score_topk_range on `decoder` (serves() holds): src_ids [B], 1 <= k <= TOPK_MAX, cand_range = (lo, hi) -> (ids [B, k]
    int64, logits [B, k] fp32, info [B, 2] int32) on the GPU: per row the k best ids of [lo, hi) by `topk_host`'s rule on the logits
    `score(cand_range=)` would write, without the [B, hi - lo] logits.  skip_ids [B] (optional): one id per row left out;
    exclude_ids [B, F] int64 with n_exclude [B] int32, both on the device (optional; `filter_lists_device`'s layout): the listed ids
    are left out.  No gradient, no synchronisation; the scratch is the call's own."""
    rp = decoder.random_projections
    rp._ensure_engine()
    prep = _mlp_prepared(rp)
    if prep is None:
        raise _lib.TPNetHipError("score_topk_range: rp.mlp is not the reference's Linear-ReLU-Linear on the GPU")
    dev = rp._dev()
    lo, hi = int(cand_range[0]), int(cand_range[1])
    Cn, B, k = hi - lo, len(src_ids), int(k)
    if Cn < 1 or Cn >= 1 << 31:
        raise ValueError("topk_range: 1 <= hi - lo < 2^31 candidates")
    if not 1 <= k <= TOPK_MAX:
        raise ValueError(f"topk_range: 1 <= k <= {TOPK_MAX}")
    if skip_ids is not None and len(skip_ids) != B:
        raise ValueError("one skip id per source")
    F = 0
    if exclude_ids is not None:
        if (not isinstance(exclude_ids, torch.Tensor) or exclude_ids.dtype != torch.int64 or exclude_ids.dim() != 2
                or exclude_ids.shape[0] != B or exclude_ids.device != dev):
            raise TypeError(f"topk_range: exclude_ids must be an int64 tensor [{B}, F] on {dev}")
        if (not isinstance(n_exclude, torch.Tensor) or n_exclude.dtype != torch.int32 or tuple(n_exclude.shape) != (B,)
                or n_exclude.device != dev):
            raise TypeError(f"topk_range: n_exclude must be an int32 tensor [{B}] on {dev}")
        F = int(exclude_ids.shape[1])
        if F == 0:
            exclude_ids = None
        else:
            exclude_ids, n_exclude = exclude_ids.contiguous(), n_exclude.contiguous()
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    logits = torch.empty((B, k), dtype=torch.float32, device=dev)
    info = torch.empty((B, 2), dtype=torch.int32, device=dev)
    if B == 0:
        return ids, logits, info
    arrays = [rp._ids(src_ids, "src_ids")] + ([rp._ids(skip_ids, "skip_ids")] if skip_ids is not None else [])
    devs = list(rp._to_device(*arrays))
    s = devs.pop(0)
    sk = devs.pop(0) if skip_ids is not None else None
    lib = _lib.load()
    need = lib.tpnet_score_topk_scratch_bytes(B, Cn, k)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    fc1, fc2 = decoder.fc1, decoder.fc2
    _lib.check(lib.tpnet_score_topk_range(
        rp._st_ref(), s.data_ptr(), None if sk is None else sk.data_ptr(), None if exclude_ids is None else exclude_ids.data_ptr(),
        None if exclude_ids is None else n_exclude.data_ptr(), F, lo, B, Cn, k, rp._now_host, float(rp.time_decay_weight),
        _lib.FLAG_NOT_SCALE if rp.not_scale else 0, prep.ref, fc1.weight.data_ptr(), fc1.in_features, fc1.in_features - 64,
        fc1.bias.data_ptr(), fc2.weight.data_ptr(), fc2.bias.data_ptr(), fc1.out_features, scratch.data_ptr(), scratch.numel(),
        ids.data_ptr(), logits.data_ptr(), info.data_ptr(), rp._stream()), "score_topk_range")
    calls["topk"] += 1
    return ids, logits, info
