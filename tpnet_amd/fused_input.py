"""The encoder's input stage in one launch (C ABI: tpnet_encoder_input*, csrc/encoder_input.hip): gather node / edge features,
time encoding and projection_layer = Linear(Din, H) -> ReLU -> Linear(H, Dout) (models/TPNet.py:297-330) without the [n, K, Din]
concat.  Forward only: the caller (tpnet_amd/encoder.py) takes it when no gradient is recorded.  The split weights are kept
per projection_layer like fused_feature.prepared() keeps self.mlp's: rewritten by one launch when a Parameter's (data_ptr,
_version) changed."""
import ctypes as C
import weakref
from typing import NamedTuple

import torch

from . import _dense, _lib

_PREPARED = weakref.WeakKeyDictionary()     # projection_layer -> Prepared
calls = {"forward": 0, "prepare": 0}        # launches made through this binding (tests assert the dispatch through it)


class Prepared(NamedTuple):
    key: tuple          # dims + (data_ptr, _version) of w1, b1, w2, b2 when the image was last written
    dims: object        # ctypes int32[6]: Dn, Dt, De, F, H, Dout
    img: torch.Tensor   # the weight image (uint8)
    err: torch.Tensor   # the error word of this layer's calls (int32 [1])
    storage: tuple      # device + the Parameters' data_ptr()s + dims: the same storage keeps the image buffer


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


def prepared(proj, Dn: int, Dt: int, De: int, F: int):
    """The Prepared record of `proj`, or None where the kernel does not serve it.  The image is rewritten in place, on the current
    stream, when a Parameter changed through a versioned op (optimizer step, load_state_dict, copy_())."""
    ls = _dense.linear_relu_linear(proj)
    if ls is None:
        return None
    w1, b1, w2, b2 = ls[0].weight, ls[0].bias, ls[1].weight, ls[1].bias
    d = (int(Dn), int(Dt), int(De), int(F), int(ls[0].out_features), int(ls[1].out_features))

    def build(previous):
        if not supported(proj, Dn, Dt, De, F) or not all(p.is_contiguous() and p.dtype == torch.float32 for p in (w1, b1, w2, b2)):
            return None
        lib = _lib.load()
        if previous is not None:
            dims, img, err = previous.dims, previous.img, previous.err
        else:
            dims = (C.c_int32 * 6)(*d)
            img = torch.empty(int(lib.tpnet_encoder_input_image_bytes(*d)), dtype=torch.uint8, device=w1.device)
            err = torch.zeros(1, dtype=torch.int32, device=w1.device)
        _lib.check(lib.tpnet_encoder_input_prepare(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), dims, img.data_ptr(),
                                                   _dense.stream_ptr(w1.device)), "encoder_input_prepare")
        calls["prepare"] += 1
        return Prepared(key, dims, img, err, storage)

    key = (Dn, Dt, De, F) + _dense.param_key(w1, b1, w2, b2)
    storage = (w1.device, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()) + d
    return _dense.cached(_PREPARED, proj, key, storage, build)


def encoder_input(prep: Prepared, node_raw, edge_raw, neigh, eids, tn, tq, tw, tb, feats):
    """out [n, K, Dout] of projection_layer on the rows the reference concatenates (module docstring).  node_raw [Nn, Dn], edge_raw
    [Ne, De], tw [Dt, 1], tb [Dt] and feats [2 n K, F] float32; neigh, eids int64 [n, K]; tn float64 [n, K]; tq float64 [n]; all
    on the image's device.  One launch on the current stream, no synchronisation."""
    n, K = neigh.shape
    Dn, Dt, De, F, H, Dout = prep.dims
    dev = prep.img.device
    f32 = lambda x: x.contiguous() if x.dtype == torch.float32 else x.float().contiguous()
    node_raw, edge_raw, tw, tb, feats = f32(node_raw), f32(edge_raw), f32(tw), f32(tb), f32(feats)
    neigh, eids, tn, tq = neigh.contiguous(), eids.contiguous(), tn.contiguous(), tq.contiguous()
    if (node_raw.shape[1] != Dn or edge_raw.shape[1] != De or tw.numel() != Dt or tb.numel() != Dt or tuple(feats.shape) != (2 * n * K, F)
            or eids.shape != neigh.shape or tn.shape != neigh.shape or tq.numel() != n or neigh.dtype != torch.int64
            or eids.dtype != torch.int64 or tn.dtype != torch.float64 or tq.dtype != torch.float64):
        raise ValueError("encoder_input: shapes / dtypes do not match the prepared layer")
    for x in (node_raw, edge_raw, neigh, eids, tn, tq, tw, tb, feats):
        if x.device != dev:
            raise ValueError(f"encoder_input: every array must be on {dev}")
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
