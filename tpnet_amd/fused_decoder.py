"""LinkPredictor_v1's two layers (models/modules.py:73-117: concat[src_emb, dst_emb, feature] -> fc1 -> ReLU -> fc2 -> one
logit) as one bf16 matrix-core kernel (C ABI: tpnet_decoder_bf16).

Opt-in (`LinkPredictor_v1.fused = True`): bf16 operands with fp32 accumulation are NOT within the 1e-4 parity budget of
the fp32 path (expect ~1e-2 relative on a logit), so the default stays the torch fp32 layers.  Forward runs the fused
kernel (no concatenated input, no hidden layer in memory); backward recomputes the hidden layer with torch in fp32 and
returns exact fp32 gradients for fc1 / fc2 AND for the three inputs (the embeddings come from the trainable encoder, the
feature from the trainable `rp.mlp`).

`LinkPredictor_v1.fused = "f32"` is the second half of this file: the same two layers in the project's fp32 class, forward AND
backward in HIP (C ABI: tpnet_decoder_f32, tpnet_decoder_f32_bwd; csrc/decoder_train.hip), within the parity budget."""
import weakref
from typing import NamedTuple

import torch

from . import _dense, _lib

# launches made through this module, by route (tests assert the dispatch through it)
calls = {"bf16_forward": 0, "f32_forward": 0, "f32_train_forward": 0, "f32_backward": 0}


def pack_weights(fc1: torch.nn.Linear, fc2: torch.nn.Linear, D: int, F: int):
    """fc1.weight [H][2D+F] -> bf16 [32*HT][2*DP+F] with the input axis laid out [src | 0-pad | dst | 0-pad | feature]
    (DP = 16*ceil(D/16)) and zero rows beyond H; fc1.bias, fc2.weight[0] zero-padded to 32*HT; HT = ceil(H/32)."""
    H = fc1.out_features
    HT = (H + 31) // 32
    DP = (D + 15) // 16 * 16
    dev = fc1.weight.device
    w1 = fc1.weight.detach().float()
    w1p = torch.zeros((32 * HT, 2 * DP + F), dtype=torch.float32, device=dev)
    w1p[:H, :D] = w1[:, :D]
    w1p[:H, DP:DP + D] = w1[:, D:2 * D]
    if F:
        w1p[:H, 2 * DP:] = w1[:, 2 * D:]
    b1p = torch.zeros(32 * HT, dtype=torch.float32, device=dev)
    b1p[:H] = fc1.bias.detach().float()
    w2p = torch.zeros(32 * HT, dtype=torch.float32, device=dev)
    w2p[:H] = fc2.weight.detach().float()[0]
    return w1p.to(torch.bfloat16).contiguous(), b1p, w2p, float(fc2.bias.detach().float()[0]), HT


def supported(fc1, fc2, D: int, F: int) -> bool:
    return (isinstance(fc1, torch.nn.Linear) and isinstance(fc2, torch.nn.Linear) and fc2.out_features == 1
            and fc1.bias is not None and fc2.bias is not None and fc1.in_features == 2 * D + F
            and fc2.in_features == fc1.out_features and fc1.out_features <= 256 and D % 4 == 0 and F % 16 == 0
            and (D > 0 or F > 0))


class _Record(NamedTuple):
    key: tuple
    storage: tuple
    packed: tuple


_PREPARED = weakref.WeakKeyDictionary()     # the decoder module -> _Record


def _prepared(owner, fc1, fc2, D, F):
    """Packed copies of the weights, rebuilt only when a parameter changed (optimizer step, load_state_dict, .to())."""
    def build(_previous):
        with torch.no_grad():
            return _Record(key, (), pack_weights(fc1, fc2, D, F))

    key = _dense.param_key(fc1.weight, fc1.bias, fc2.weight, fc2.bias) + (fc1.weight.device, D, F)
    return _dense.cached(_PREPARED, owner, key, (), build).packed


class _FusedDecoder(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, dst, feat, w1, b1, w2, b2, prep, not_encode):
        ref = feat if feat is not None else src
        if ref.device.type != "cuda" or ref.dtype != torch.float32:
            raise _lib.TPNetHipError("fused decoder needs float32 inputs on the GPU")
        src = src.contiguous(); dst = dst.contiguous()
        n, D = src.shape
        F = 0 if feat is None else feat.shape[1]
        if feat is not None:
            feat = feat.contiguous()
        out = torch.empty((n, 1), dtype=torch.float32, device=ref.device)
        w1p, b1p, w2p, b2f, HT = prep
        _lib.check(_lib.load().tpnet_decoder_bf16(
            None if not_encode else src.data_ptr(), None if not_encode else dst.data_ptr(), D,
            None if feat is None else feat.data_ptr(), F, n, w1p.data_ptr(), b1p.data_ptr(), w2p.data_ptr(), b2f, HT,
            out.data_ptr(), _dense.stream_ptr(ref.device)), "decoder_bf16")
        ctx.not_encode = not_encode
        ctx.has_feat = feat is not None
        ctx.save_for_backward(src, dst, feat if feat is not None else src.new_empty(0), w1, b1, w2)
        return out

    @staticmethod
    def backward(ctx, gout):
        src, dst, feat, w1, b1, w2 = ctx.saved_tensors
        D = src.shape[1]
        if ctx.not_encode:                                   # modules.py:106-108: the embeddings are replaced by zeros
            src = torch.zeros_like(src); dst = torch.zeros_like(dst)
        x = torch.cat([src, dst, feat], dim=1) if ctx.has_feat else torch.cat([src, dst], dim=1)
        gw1, gb1, gw2, gb2, gx = _dense.layer_grads(x, gout, w1, b1, w2, input_grad=True)
        gsrc = None if ctx.not_encode else gx[:, :D]
        gdst = None if ctx.not_encode else gx[:, D:2 * D]
        gfeat = gx[:, 2 * D:] if ctx.has_feat else None
        return gsrc, gdst, gfeat, gw1, gb1, gw2, gb2, None, None


def fused_decoder(owner, fc1, fc2, src_emb, dst_emb, feat, not_encode: bool):
    D = src_emb.shape[1]
    F = 0 if feat is None else feat.shape[1]
    calls["bf16_forward"] += 1
    return _FusedDecoder.apply(src_emb, dst_emb, feat, fc1.weight, fc1.bias, fc2.weight, fc2.bias,
                               _prepared(owner, fc1, fc2, D, F), bool(not_encode))


# ---- the fp32 class (`LinkPredictor_v1.fused = "f32"`; C ABI: tpnet_decoder_f32*, csrc/decoder_train.hip) ----------------------------
# One launch forward; under autograd two launches backward + the fixed-order sum of the row parts' partials where there are several.
# The kernels read fc1 / fc2's Parameters as they are (no packed copy, no cache), within the project's 1e-4 parity budget (~2e-5 of a
# logit's scale), so unlike the bf16 kernel this route can stand where the torch layers stand.

# row tiles (of 32 rows) per part of the backward's weight kernel, and the most parts: up to 4 tiles (n <= 128) one part and no sum;
# n = 200 is 2 parts, n = 1 000 is 8, n = 10 000 is 64 parts of 5 tiles (64 partials of 70 521 floats at 172 x 408: 18 MB)
TILES_PER_PART = 4
MAX_PARTIALS = 64


def supported_f32(fc1, fc2, D: int, F: int) -> bool:
    """The shapes the fp32-class kernels serve (tpnet_decoder_f32_supported), on float32 contiguous Parameters on the GPU."""
    if not (isinstance(fc1, torch.nn.Linear) and isinstance(fc2, torch.nn.Linear) and fc2.out_features == 1
            and fc1.bias is not None and fc2.bias is not None and fc1.in_features == 2 * D + F
            and fc2.in_features == fc1.out_features):
        return False
    ps = (fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    return bool(all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in ps)
                and _lib.load().tpnet_decoder_f32_supported(D, F, fc1.out_features))


def serves_f32(fc1, fc2, src_emb, dst_emb, feat, not_encode: bool) -> bool:
    """Whether fused_decoder_f32 takes this call: a served shape, float32 contiguous inputs on the Parameters' GPU, and at least one
    source that is read."""
    xs = [src_emb, dst_emb] + ([] if feat is None else [feat])
    dev = fc1.weight.device
    if not all(x.dim() == 2 and x.device == dev and x.dtype == torch.float32 and x.is_contiguous() for x in xs):
        return False
    n, D = src_emb.shape
    F = 0 if feat is None else feat.shape[1]
    if tuple(dst_emb.shape) != (n, D) or (feat is not None and feat.shape[0] != n) or n >= 2 ** 31 or (not_encode and F == 0):
        return False
    return supported_f32(fc1, fc2, D, F)


class _DecoderF32(torch.autograd.Function):
    """Forward: tpnet_decoder_f32.  Saved (only where a gradient is recorded): the sources that are read and fc1.weight, fc1.bias,
    fc2.weight by reference -- no hidden layer, no decisions: the backward recomputes the forward's bits.  Backward:
    tpnet_decoder_f32_bwd in a workspace of its own; input gradients only where asked for."""

    @staticmethod
    def forward(ctx, src, dst, feat, w1, b1, w2, b2, not_encode, parts, train):
        n, D = src.shape
        F = 0 if feat is None else feat.shape[1]
        H = w1.shape[0]
        dev = w1.device
        out = torch.empty((n, 1), dtype=torch.float32, device=dev)
        if n > 0:                                               # (an empty tensor has no pointer to give)
            _lib.check(_lib.load().tpnet_decoder_f32(
                None if not_encode else src.data_ptr(), None if not_encode else dst.data_ptr(), D,
                None if feat is None else feat.data_ptr(), F, n, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), H,
                out.data_ptr(), None, _dense.stream_ptr(dev)), "decoder_f32")
            calls["f32_train_forward" if train else "f32_forward"] += 1
        if train:
            ctx.save_for_backward(None if not_encode else src, None if not_encode else dst, feat, w1, b1, w2)
            ctx.dims = (n, D, F, H, not_encode, parts)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        src, dst, feat, w1, b1, w2 = ctx.saved_tensors
        n, D, F, H, not_encode, parts = ctx.dims
        dev = w1.device
        need = ctx.needs_input_grad
        gsrc = torch.empty((n, D), dtype=torch.float32, device=dev) if need[0] and not not_encode else None
        gdst = torch.empty((n, D), dtype=torch.float32, device=dev) if need[1] and not not_encode else None
        gfeat = torch.empty((n, F), dtype=torch.float32, device=dev) if need[2] and feat is not None else None
        tot = None
        if n > 0:
            lib = _lib.load()
            gout = gout.contiguous()
            pf = int(lib.tpnet_decoder_f32_partial_floats(D, F, H))
            if parts is None:
                parts = min(MAX_PARTIALS, ((n + 31) // 32 + TILES_PER_PART - 1) // TILES_PER_PART)
            # one part: its partial IS the gradient, so the buffer is this call's own; several: the reused buffer, summed
            part = torch.empty((1, pf), dtype=torch.float32, device=dev) if parts == 1 else _dense.partial_buffer(dev, parts, pf)
            ws = torch.empty(int(lib.tpnet_decoder_f32_bwd_workspace_bytes(n, D, F, H)), dtype=torch.uint8, device=dev)
            ptr = lambda t: None if t is None else t.data_ptr()
            rc = lib.tpnet_decoder_f32_bwd(ptr(src), ptr(dst), D, ptr(feat), F, n, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), H,
                                           gout.data_ptr(), ws.data_ptr(), ptr(gsrc), ptr(gdst), ptr(gfeat), part.data_ptr(),
                                           part.shape[0], _dense.stream_ptr(dev))
            if rc <= 0:
                _lib.check(rc if rc < 0 else -1, "decoder_f32_bwd")
            tot = part[0] if parts == 1 else _dense.sum_partials(rc, part, "decoder_f32_bwd")
            calls["f32_backward"] += 1
            del ws                                              # (the caching allocator keeps it alive for the stream's launches)
        gw1, gb1, gw2 = _dense.split_grads(tot, (w1, b1, w2), need[3:6])
        gb2 = None
        if need[6]:
            gb2 = torch.zeros(1, dtype=torch.float32, device=dev) if tot is None else tot[-1:]
        return gsrc, gdst, gfeat, gw1, gb1, gw2, gb2, None, None, None


def fused_decoder_f32(fc1, fc2, src_emb, dst_emb, feat, not_encode: bool, parts=None, checked=False):
    """LinkPredictor_v1's logits [n, 1] in the fp32 class, differentiable (once) with respect to fc1 / fc2's four Parameters and the
    three inputs (those that require a gradient; with `not_encode` the embeddings count as zeros and take none): one launch, and
    under autograd two more backward (+ the sum of at most `parts` partials; None: a part per TILES_PER_PART row tiles, at most
    MAX_PARTIALS).  No synchronisation.  Raises ValueError where serves_f32() says the kernels do not take the call (`checked`: the
    caller has asked serves_f32 itself)."""
    if not checked and not serves_f32(fc1, fc2, src_emb, dst_emb, feat, not_encode):
        raise ValueError("fused_decoder_f32: the kernels do not serve this call")
    if parts is not None and int(parts) < 1:
        raise ValueError("fused_decoder_f32: parts >= 1")
    tensors = (src_emb, dst_emb, feat, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    train = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)     # (else nothing is saved)
    return _DecoderF32.apply(*tensors, bool(not_encode), None if parts is None else int(parts), train)
