"""What the fused_* modules share: the structural tests of a Linear -> ReLU -> Linear block and of an MLP-Mixer layer, the current
stream as the C calls take it, the fp32 torch expressions of the two layers' gradients, the launch of the matrix-core weight-gradient kernels, the
Python side of a backward that writes partial sums (their buffer, their sum, the cut into per-Parameter gradients), and the cache of
derived weight buffers."""
import ctypes as C
from typing import NamedTuple

import torch

from . import _lib


def linear_relu_linear(m):
    """(first, second) Linear of `m` if it is Sequential(Linear, ReLU, Linear) with both biases and matching widths, else None."""
    if not (isinstance(m, torch.nn.Sequential) and len(m) == 3 and isinstance(m[0], torch.nn.Linear)
            and isinstance(m[1], torch.nn.ReLU) and isinstance(m[2], torch.nn.Linear)):
        return None
    l1, l2 = m[0], m[2]
    if l1.bias is None or l2.bias is None or l2.in_features != l1.out_features:
        return None
    return l1, l2


class MixerLayers(NamedTuple):
    token_norm: torch.nn.LayerNorm
    token: tuple            # (first, second) Linear of token_feedforward.ffn
    channel_norm: torch.nn.LayerNorm
    channel: tuple          # ... of channel_feedforward.ffn
    dropout: float          # the largest p of the four Dropouts


def _gelu_ffn(ff):
    """(first Linear, second Linear, largest dropout p) of `ff.ffn` if it is Sequential(Linear, GELU(approximate='none'), Dropout,
    Linear, Dropout) with both biases, mapping n -> hidden -> n, else None."""
    m = getattr(ff, "ffn", None)
    nn = torch.nn
    if not (isinstance(m, nn.Sequential) and len(m) == 5 and isinstance(m[0], nn.Linear) and isinstance(m[1], nn.GELU)
            and getattr(m[1], "approximate", "none") == "none" and isinstance(m[2], nn.Dropout) and isinstance(m[3], nn.Linear)
            and isinstance(m[4], nn.Dropout)):
        return None
    l1, l2 = m[0], m[3]
    if l1.bias is None or l2.bias is None or l2.in_features != l1.out_features or l2.out_features != l1.in_features:
        return None
    return l1, l2, max(float(m[2].p), float(m[4].p))


def mixer_layers(m):
    """MixerLayers of `m` if it has the structure of the reference's MLPMixer (models/TPNet.py:371-416; by attributes, not by class:
    the reference's own module passes): token_norm / channel_norm LayerNorms over one axis with affine parameters, token_feedforward /
    channel_feedforward what _gelu_ffn accepts, the norms' widths the FFNs'.  Else None."""
    tn, cn = getattr(m, "token_norm", None), getattr(m, "channel_norm", None)
    for ln in (tn, cn):
        if not (isinstance(ln, torch.nn.LayerNorm) and ln.elementwise_affine and ln.weight is not None and ln.bias is not None
                and len(ln.normalized_shape) == 1):
            return None
    tf, cf = _gelu_ffn(getattr(m, "token_feedforward", None)), _gelu_ffn(getattr(m, "channel_feedforward", None))
    if tf is None or cf is None or tn.normalized_shape[0] != tf[0].in_features or cn.normalized_shape[0] != cf[0].in_features:
        return None
    return MixerLayers(tn, tf[:2], cn, cf[:2], max(tf[2], cf[2]))


def stream_ptr(device):
    """The current stream of `device`, as the C calls take it."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def layer_grads(x, gy, w1, b1, w2, input_grad=False):
    """fp32 torch expressions of the gradients of (w1, b1, w2, b2) of y = relu(x w1^T + b1) w2^T + b2 given gy = dL/dy, the hidden
    layer recomputed; with `input_grad` dL/dx comes fifth."""
    pre = torch.addmm(b1, x, w1.t())                 # fp32 recompute of the hidden layer
    hid = torch.relu(pre)
    gh = (gy @ w2) * (pre > 0)
    grads = (gh.t() @ x, gh.sum(0), gy.t() @ hid, gy.sum(0))
    return grads + (gh @ w1,) if input_grad else grads


_PARTIALS = {}      # (device, parts, floats per partial) -> the reused [parts, floats] buffer


def partial_buffer(device, parts, floats):
    """The float32 [parts, floats] buffer a backward launch writes its partial sums into: one per (device, parts, floats), reused by
    every later call (the launches of a stream run in order)."""
    key = (device, int(parts), int(floats))
    part = _PARTIALS.get(key)
    if part is None:
        part = _PARTIALS[key] = torch.empty(key[1:], dtype=torch.float32, device=device)
    return part


def sum_partials(rc, part, what):
    """The sum of the first `rc` partials in a fixed order: run-to-run identical bits.  rc = the C call's return value: the number of
    partials written; <= 0 raises as _lib.check does (0: no partial of a call with rows is an error too)."""
    if rc <= 0:
        _lib.check(rc if rc < 0 else -1, what)
    return part[:rc].sum(0)


def split_grads(tot, tensors, needs):
    """`tot` (one summed partial: the gradients of `tensors`, flat, in order) cut into one gradient per tensor, in its shape; None
    where `needs` says it is not needed, zeros where tot is None (a call without rows)."""
    grads, off = [], 0
    for t, need in zip(tensors, needs):
        g = None
        if need:
            g = torch.zeros_like(t) if tot is None else tot[off:off + t.numel()].view(t.shape)
        grads.append(g)
        off += t.numel()
    return grads


def mlp64_bwd(call, x, gy, H=256, F=64, pf=None):
    """One launch of a weight-gradient kernel (tpnet_mlp64_bwd_*; tpnet_mlp_rows_bwd_f32 with its (H, F) and partial size `pf`) +
    the fixed-order sum of its workgroups' partial results (deterministic).  A partial is gW1 [H][F] | gW2 [F][H] | gb1 [H].
    call(x_ptr, gy_ptr, n, partial_ptr, n_partial, stream) -> the C call's return value rc: the number of partials written, or
    <= 0 where it declined.  Returns (rc, (gw1, gb1, gw2, gb2) or None)."""
    n = int(x.shape[0])
    x = x.contiguous()
    gy = gy.contiguous().float()
    if pf is None:
        pf = int(_lib.load().tpnet_mlp64_bwd_partial_floats())
    nblk = min(256, (n + 31) // 32)
    part = torch.empty((nblk, pf), dtype=torch.float32, device=x.device)
    rc = call(x.data_ptr(), gy.data_ptr(), n, part.data_ptr(), nblk, stream_ptr(x.device))
    if rc <= 0:
        return rc, None
    tot = sum_partials(rc, part, "mlp64_bwd")
    return rc, (tot[:H * F].view(H, F), tot[2 * H * F:2 * H * F + H], tot[H * F:2 * H * F].view(F, H), gy.sum(0))


def param_key(*params):
    """(data_ptr, _version) of every Parameter: changes with an optimizer step, load_state_dict, .to() and any versioned in-place op."""
    key = ()
    for p in params:
        key += (p.data_ptr(), p._version)
    return key


def cached(cache, owner, key, storage, build):
    """The record of `owner` in `cache` (a WeakKeyDictionary: kept off the module -- ctypes objects and device buffers neither
    deepcopy nor belong in a state_dict -- and dropped with it), rebuilt by `build` when `key` changed.  A record is any object with the
    fields `key` and `storage`; build(previous) gets the previous record while `storage` is unchanged (its buffers can be
    rewritten in place), else None, and returns the new record or None (not served: nothing is cached)."""
    rec = cache.get(owner)
    if rec is not None and rec.key == key:
        return rec
    rec = build(rec if rec is not None and rec.storage == storage else None)
    if rec is not None:
        cache[owner] = rec
    return rec


def cached_images(cache, owner, key, storage, build, backward):
    """cached() for a record with a second image `bimg` that only a training call needs: build(previous, both) writes the second one
    too where `both`.  It is built once a call asks with `backward`, and from then on both are rewritten together; a record an
    inference call made (bimg None) is rebuilt once, from nothing, and kept where that build declines."""
    rec = cached(cache, owner, key, storage, lambda prev: build(prev, backward or (prev is not None and prev.bimg is not None)))
    if backward and rec is not None and rec.bimg is None:
        rec = build(None, True)
        if rec is not None:
            cache[owner] = rec
    return rec
