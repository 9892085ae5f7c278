"""What the four fused_* modules share: the structural test of a Linear -> ReLU -> Linear block, the current stream as the C calls
take it, the fp32 torch expressions of the two layers' gradients, the launch of the matrix-core weight-gradient kernels, and the
cache of derived weight buffers."""
import ctypes as C

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


def mlp64_bwd(call, x, gy, H=256, F=64):
    """One launch of a tpnet_mlp64_bwd_* kernel + the fixed-order sum of its workgroups' partial results (deterministic).
    call(x_ptr, gy_ptr, n, partial_ptr, n_partial, stream) -> the C call's return value rc: the number of partials written, or
    <= 0 where it declined.  Returns (rc, (gw1, gb1, gw2, gb2) or None)."""
    n = int(x.shape[0])
    x = x.contiguous()
    gy = gy.contiguous().float()
    pf = int(_lib.load().tpnet_mlp64_bwd_partial_floats())
    nblk = min(256, (n + 31) // 32)
    part = torch.empty((nblk, pf), dtype=torch.float32, device=x.device)
    rc = call(x.data_ptr(), gy.data_ptr(), n, part.data_ptr(), nblk, stream_ptr(x.device))
    if rc <= 0:
        return rc, None
    tot = part[:rc].sum(0)
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
