"""The encoder's input stage in one launch (C ABI: tpnet_encoder_input*, csrc/encoder_input.hip): gather node / edge features,
time encoding and projection_layer = Linear(Din, H) -> ReLU -> Linear(H, Dout) (models/TPNet.py:297-330) without the [n, K, Din]
concat.  The caller (tpnet_amd/encoder.py) takes `encoder_input` when no gradient is recorded.  The split weights are kept
per projection_layer like fused_feature.prepared() keeps self.mlp's: rewritten by one launch when a Parameter's (data_ptr,
_version) changed.

The stage also runs in a TRAINING step (csrc/encoder_input_train.hip; opt-in, TPNetEmbedding.fused_input_training):
`encoder_input_train` is the same launch, which also stores one bit per (row, hidden unit) -- the ReLU's decision -- and TWO
launches backward under autograd, on the matrix cores in the fp32 class.  Between forward and backward only the index and time
tensors, `feats` and the bits live (44 bytes per row at 344 hidden units, where autograd keeps the 2 288-byte concat and the
1 376-byte hidden layer); the backward rebuilds the concat from the sources in a workspace it allocates and frees.  Its second
image (W1, W2^T and the time and relative-encoding columns of W1^T) sits in the same record and is written with the first once a
training call has asked for it.  Gradients reach projection_layer, the time encoder and `feats`; the raw tables take none."""
import ctypes as C
import weakref
from typing import NamedTuple

import torch

from . import _dense, _lib

_PREPARED = weakref.WeakKeyDictionary()     # projection_layer -> Prepared
# launches made through this binding (tests assert the dispatch through it)
calls = {"forward": 0, "prepare": 0, "train_forward": 0, "backward": 0}
# row parts of the backward's weight kernel = partial sums it writes, at most (fused_mixer.CHANNEL_PARTIALS' reasoning: at
# 572 -> 344 -> 172 a part is 44 waves, so 32 parts are 1 408 waves for the 1 024 SIMDs, and 32 partials of 256 652 floats are 33 MB)
MAX_PARTIALS = 32


class Prepared(NamedTuple):
    key: tuple          # dims + (data_ptr, _version) of w1, b1, w2, b2 when the image was last written
    dims: object        # ctypes int32[6]: Dn, Dt, De, F, H, Dout
    img: torch.Tensor   # the weight image (uint8)
    err: torch.Tensor   # the error word of this layer's calls (int32 [1])
    storage: tuple      # device + the Parameters' data_ptr()s + dims: the same storage keeps the image buffer
    bimg: torch.Tensor = None   # the backward's image, once a training call asked for it (then kept current)


def dims_of(proj, Dn: int, Dt: int, De: int, F: int):
    """(Dn, Dt, De, F, H, Dout) if `proj` is Linear -> ReLU -> Linear with biases on Dn + Dt + De + 2 F inputs, else None."""
    ls = _dense.linear_relu_linear(proj)
    if ls is None or ls[0].in_features != Dn + Dt + De + 2 * F:
        return None
    return (int(Dn), int(Dt), int(De), int(F), int(ls[0].out_features), int(ls[1].out_features))


def supported(proj, Dn: int, Dt: int, De: int, F: int) -> bool:
    d = dims_of(proj, Dn, Dt, De, F)
    if d is None or F <= 0:
        return False
    w = proj[0].weight
    return bool(w.is_cuda and w.dtype == torch.float32 and _lib.load().tpnet_encoder_input_supported(*d))


def invalidate(proj=None):
    """Forget the prepared image of `proj` (all layers' if None): for whoever writes a Parameter through `.data` or a raw pointer,
    which bumps no version counter (same contract as fused_feature.invalidate)."""
    if proj is None:
        _PREPARED.clear()
    else:
        _PREPARED.pop(proj, None)


def cached(proj):
    """The Prepared record `proj` has now (None: no launch has served it yet, or invalidate() dropped it).  No GPU call."""
    return _PREPARED.get(proj)


def prepared(proj, Dn: int, Dt: int, De: int, F: int, backward=False):
    """The Prepared record of `proj`, or None where the kernel does not serve it.  The image is rewritten in place, on the current
    stream, when a Parameter changed through a versioned op (optimizer step, load_state_dict, copy_()).  `backward`: the record
    also holds the backward's image (None where the backward does not serve the shape); from then on both are rewritten together."""
    ls = _dense.linear_relu_linear(proj)
    if ls is None:
        return None
    w1, b1, w2, b2 = ls[0].weight, ls[0].bias, ls[1].weight, ls[1].bias
    d = (int(Dn), int(Dt), int(De), int(F), int(ls[0].out_features), int(ls[1].out_features))

    def build(previous, both):
        if not supported(proj, Dn, Dt, De, F) or not all(p.is_contiguous() and p.dtype == torch.float32 for p in (w1, b1, w2, b2)):
            return None
        lib = _lib.load()
        if both and int(lib.tpnet_encoder_input_bwd_image_bytes(*d)) == 0:          # (the backward serves fewer shapes: no launch)
            return None
        bimg = None
        if previous is not None:
            dims, img, err, bimg = previous.dims, previous.img, previous.err, previous.bimg
        else:
            dims = (C.c_int32 * 6)(*d)
            img = torch.empty(int(lib.tpnet_encoder_input_image_bytes(*d)), dtype=torch.uint8, device=w1.device)
            err = torch.zeros(1, dtype=torch.int32, device=w1.device)
        _lib.check(lib.tpnet_encoder_input_prepare(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), dims, img.data_ptr(),
                                                   _dense.stream_ptr(w1.device)), "encoder_input_prepare")
        if both:
            if bimg is None:
                bimg = torch.empty(int(lib.tpnet_encoder_input_bwd_image_bytes(*d)), dtype=torch.uint8, device=w1.device)
            _lib.check(lib.tpnet_encoder_input_bwd_prepare(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), dims, bimg.data_ptr(),
                                                           _dense.stream_ptr(w1.device)), "encoder_input_bwd_prepare")
        calls["prepare"] += 1
        return Prepared(key, dims, img, err, storage, bimg)

    key = (Dn, Dt, De, F) + _dense.param_key(w1, b1, w2, b2)
    storage = (w1.device, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()) + d
    return _dense.cached_images(_PREPARED, proj, key, storage, build, backward)


def _sources(prep, node_raw, edge_raw, neigh, eids, tn, tq, tw, tb, feats, what):
    """The nine arrays as the C calls take them (contiguous, float32 / int64 / float64, on the image's device), checked against
    the prepared layer."""
    n, K = neigh.shape
    Dn, Dt, De, F, H, Dout = prep.dims
    dev = prep.img.device
    f32 = lambda x: x.contiguous() if x.dtype == torch.float32 else x.float().contiguous()
    node_raw, edge_raw, tw, tb, feats = f32(node_raw), f32(edge_raw), f32(tw), f32(tb), f32(feats)
    neigh, eids, tn, tq = neigh.contiguous(), eids.contiguous(), tn.contiguous(), tq.contiguous()
    if (node_raw.shape[1] != Dn or edge_raw.shape[1] != De or tw.numel() != Dt or tb.numel() != Dt or tuple(feats.shape) != (2 * n * K, F)
            or eids.shape != neigh.shape or tn.shape != neigh.shape or tq.numel() != n or neigh.dtype != torch.int64
            or eids.dtype != torch.int64 or tn.dtype != torch.float64 or tq.dtype != torch.float64):
        raise ValueError(f"{what}: shapes / dtypes do not match the prepared layer")
    for x in (node_raw, edge_raw, neigh, eids, tn, tq, tw, tb, feats):
        if x.device != dev:
            raise ValueError(f"{what}: every array must be on {dev}")
    return node_raw, edge_raw, neigh, eids, tn, tq, tw, tb, feats


def encoder_input(prep: Prepared, node_raw, edge_raw, neigh, eids, tn, tq, tw, tb, feats):
    """out [n, K, Dout] of projection_layer on the rows the reference concatenates (module docstring).  node_raw [Nn, Dn], edge_raw
    [Ne, De], tw [Dt, 1], tb [Dt] and feats [2 n K, F] float32; neigh, eids int64 [n, K]; tn float64 [n, K]; tq float64 [n]; all
    on the image's device.  One launch on the current stream, no synchronisation."""
    node_raw, edge_raw, neigh, eids, tn, tq, tw, tb, feats = _sources(prep, node_raw, edge_raw, neigh, eids, tn, tq, tw, tb, feats,
                                                                      "encoder_input")
    n, K = neigh.shape
    dev, Dout = prep.img.device, prep.dims[5]
    out = torch.empty((n, K, Dout), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().tpnet_encoder_input(
        node_raw.data_ptr(), node_raw.shape[0], edge_raw.data_ptr(), edge_raw.shape[0], neigh.data_ptr(), eids.data_ptr(), tn.data_ptr(),
        tq.data_ptr(), tw.data_ptr(), tb.data_ptr(), feats.data_ptr(), n, K, prep.dims, prep.img.data_ptr(), out.data_ptr(),
        prep.err.data_ptr(), _dense.stream_ptr(dev)), "encoder_input")
    calls["forward"] += 1
    return out


def check_errors(prep: Prepared):
    """Raise IndexError if a launch met a node / edge id outside the raw feature tables since the last check (synchronises)."""
    _lib.check(_lib.load().tpnet_encoder_input_check(prep.err.data_ptr(), _dense.stream_ptr(prep.err.device)), "encoder_input")


class _InputTrain(torch.autograd.Function):
    """Forward: tpnet_encoder_input_train.  Saved: the index and time tensors, the time encoder's two Parameters, feats (by
    reference) and relu_bits; the four Parameters of projection_layer only stand for their images, which are looked up again in
    the backward (an in-place change in between raises as torch does).  Backward: tpnet_encoder_input_bwd in a workspace of its
    own + the fixed-order sum of its partials."""

    @staticmethod
    def forward(ctx, w1, b1, w2, b2, tw, tb, feats, proj, node_raw, edge_raw, neigh, eids, tn, tq, parts):
        Dn, De, Dt = node_raw.shape[1], edge_raw.shape[1], tw.numel()
        F = feats.shape[1]
        prep = prepared(proj, Dn, Dt, De, F, backward=True)
        n, K = neigh.shape
        H, Dout = prep.dims[4], prep.dims[5]
        dev = prep.img.device
        out = torch.empty((n, K, Dout), dtype=torch.float32, device=dev)
        bits = torch.empty((n * K, (H + 31) // 32), dtype=torch.int32, device=dev)
        if n * K > 0:                                           # (an empty tensor has no pointer to give)
            _lib.check(_lib.load().tpnet_encoder_input_train(
                node_raw.data_ptr(), node_raw.shape[0], edge_raw.data_ptr(), edge_raw.shape[0], neigh.data_ptr(), eids.data_ptr(),
                tn.data_ptr(), tq.data_ptr(), tw.data_ptr(), tb.data_ptr(), feats.data_ptr(), n, K, prep.dims, prep.img.data_ptr(),
                out.data_ptr(), bits.data_ptr(), prep.err.data_ptr(), _dense.stream_ptr(dev)), "encoder_input_train")
            calls["train_forward"] += 1
        ctx.save_for_backward(w1, b1, w2, b2, tw, tb, feats, neigh, eids, tn, tq, bits)
        ctx.tables = (proj, node_raw, edge_raw, parts)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        w1, b1, w2, b2, tw, tb, feats, neigh, eids, tn, tq, bits = ctx.saved_tensors
        proj, node_raw, edge_raw, parts = ctx.tables
        n, K = neigh.shape
        dev = feats.device
        time_grads = ctx.needs_input_grad[4] or ctx.needs_input_grad[5]
        gfeat = torch.empty_like(feats) if ctx.needs_input_grad[6] else None
        tot = None
        if n * K > 0:
            lib = _lib.load()
            prep = prepared(proj, node_raw.shape[1], tw.numel(), edge_raw.shape[1], feats.shape[1], backward=True)
            d = tuple(prep.dims)
            gy = gy.contiguous()
            part = _dense.partial_buffer(dev, parts, lib.tpnet_encoder_input_bwd_partial_floats(*d))
            ws = torch.empty(int(lib.tpnet_encoder_input_bwd_workspace_bytes(n * K, *d)), dtype=torch.uint8, device=dev)
            rc = lib.tpnet_encoder_input_bwd(
                node_raw.data_ptr(), node_raw.shape[0], edge_raw.data_ptr(), edge_raw.shape[0], neigh.data_ptr(), eids.data_ptr(),
                tn.data_ptr(), tq.data_ptr(), tw.data_ptr(), tb.data_ptr(), feats.data_ptr(), bits.data_ptr(), gy.data_ptr(), n, K,
                prep.dims, prep.bimg.data_ptr(), ws.data_ptr(), None if gfeat is None else gfeat.data_ptr(), int(time_grads),
                part.data_ptr(), part.shape[0], prep.err.data_ptr(), _dense.stream_ptr(dev))
            tot = _dense.sum_partials(rc, part, "encoder_input_bwd")
            calls["backward"] += 1
            del ws                                              # (the caching allocator keeps it alive for the stream's launches)
        elif gfeat is not None:
            gfeat.zero_()
        grads = _dense.split_grads(tot, (w1, b1, w2, b2, tw, tb), ctx.needs_input_grad[:6])
        return (*grads, gfeat, None, None, None, None, None, None, None, None)


def encoder_input_train(proj, time_encoder, node_raw, edge_raw, neigh, eids, tn, tq, feats, parts=None):
    """encoder_input's result [n, K, Dout], differentiable (once) with respect to projection_layer's four Parameters, the two of
    `time_encoder.w` (those that require a gradient) and `feats`: one launch forward, two backward (+ the sum of at most `parts`
    partial results; None: MAX_PARTIALS), no synchronisation, on the matrix cores in the project's fp32 class.  The arrays are
    encoder_input's; the raw tables take no gradient.  Raises ValueError where the kernels do not serve `proj` (see prepared())."""
    w = time_encoder.w
    tw, tb = w.weight, w.bias
    prep = prepared(proj, node_raw.shape[1], tw.numel(), edge_raw.shape[1], feats.shape[1], backward=True)
    if prep is None:
        raise ValueError("encoder_input_train: the kernels do not serve this projection_layer")
    if node_raw.requires_grad or edge_raw.requires_grad:
        raise ValueError("encoder_input_train: the raw feature tables take no gradient")
    if not all(p.is_contiguous() and p.dtype == torch.float32 for p in (tw, tb)) or feats.dtype != torch.float32 \
            or not feats.is_contiguous():
        raise ValueError("encoder_input_train: the time encoder's Parameters and feats must be contiguous float32")
    node_raw, edge_raw, neigh, eids, tn, tq, _, _, _ = _sources(prep, node_raw, edge_raw, neigh, eids, tn, tq, tw, tb, feats,
                                                                "encoder_input_train")
    ls = _dense.linear_relu_linear(proj)
    parts = MAX_PARTIALS if parts is None else int(parts)
    if parts < 1:
        raise ValueError("encoder_input_train: parts >= 1")
    return _InputTrain.apply(ls[0].weight, ls[0].bias, ls[1].weight, ls[1].bias, tw, tb, feats, proj, node_raw, edge_raw, neigh, eids,
                             tn, tq, parts)
