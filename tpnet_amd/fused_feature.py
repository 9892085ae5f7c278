"""get_pair_wise_feature in one launch (C ABI: tpnet_pair_feature / tpnet_host_pair_feature): the pairwise readout and
self.mlp = Linear(F, 4F) -> ReLU -> Linear(4F, F) (models/TPNet.py:63-65, 112-129) fused in fp32.

Forward = the fused kernel (the features stay in LDS between the readout and the dense layers).  When gradients are
being recorded, the kernel also writes the pre-mlp features and the backward pass is the fp32 torch expression of the two
layers' gradients (the projections carry no gradient: requires_grad=False in the reference, models/TPNet.py:49-62).
Differs from the torch layers in f32 summation order only, so it is the DEFAULT for the decoder's short pair lists."""
import ctypes as C
import os
import warnings
import weakref
from typing import NamedTuple

import torch

from . import _dense, _lib

_PREPARED = weakref.WeakKeyDictionary()     # mlp module -> Prepared (kept off the module: ctypes objects do not deepcopy)


class Prepared(NamedTuple):
    """What prepared() returns: self.mlp's weights in the layouts the kernels read."""
    key: tuple          # (data_ptr, _version) of w1, b1, w2, b2 when the derived buffers were last written
    st: object          # the tpnet_mlp struct (_lib.Mlp)
    ref: object         # its byref: what the C calls take
    derived: tuple      # (w1t, w2t, w2f or None, weight image or None): the buffers the struct points into
    params: tuple       # the Parameters (w1, b1, w2, b2)
    storage: tuple      # their data_ptr()s: the same storage keeps the derived buffers and the struct


# longer lists: the readout kernels + the dense layers as GEMMs (torch, or the bf16 kernel if opted in)
MAX_PAIRS = int(os.environ.get("TPNET_DEV_FUSED_MAX_PAIRS", "8192"))


def supported(mlp: torch.nn.Module, F: int) -> bool:
    ls = _dense.linear_relu_linear(mlp)
    return (ls is not None and ls[0].in_features == F and ls[0].out_features == 4 * F and ls[1].out_features == F
            and ls[0].weight.dtype == torch.float32 and ls[0].weight.is_cuda)


# rows from which the matrix-core backward serves a call: one launch + a sum of partials against ten small torch launches -- at the
# decoder's 1 000 rows per call a training step went 704 -> 520-570 us (bench.py, dropin.train); below, the torch expressions
MFMA_BWD_FROM = 512
# "mfma" (default): weight gradients of self.mlp on the matrix cores from MFMA_BWD_FROM rows on -- two-piece bf16 operands, three
# products per term, fp32 accumulation: ~2^-16 per PRODUCT (3-5e-6 of the terms' magnitude observed, 4e-5 allowed by the tests)
# where the reference's fp32 GEMMs carry 2^-24; "torch": always the fp32 torch expressions (five GEMMs + three elementwise passes).
# A module overrides the process-wide value with an attribute of the same name on its self.mlp (rp.mlp.mlp_backward = "torch").
mlp_backward = "mfma"
_declined_once = set()
# rows from which tpnet_mlp_rows_bwd_f32 (csrc/mlp_rows_bwd.hip: num_layer 1 and 2) takes the weight gradients from the torch
# expressions, per width; None = reachable through the C call, never routed.  MLP_ROWS_FROM's rule (below), measured by the backward
# leg of tools/mlp_rows_rate.py (profiles/mlp_rows.md): one launch + the sum of the partials against _dense.layer_grads on the same
# tensors in one process.  At 1 000 rows, the smallest size of the protocol, 28.7 / 28.6 us against 115 / 142 us; 80 000 rows
# 53.5 / 80.8 against 311 / 516 us; 800 000 rows 236 / 456 against 2 380 / 4 029 us.  Shorter lists were not measured and stay
# with torch.
MLP_ROWS_BWD_FROM = {16: 1000, 36: 1000}
# launches made from here (tests assert the dispatch through them): of tpnet_mlp_rows_bwd_f32; of tpnet_mlp_l4_f32 (one per call) and
# tpnet_mlp_l4_bwd_f32 (two per call); "l4_prepare": rebuilds of num_layer 4's weight images
calls = {"rows_bwd": 0, "l4": 0, "l4_bwd": 0, "l4_prepare": 0}


def _bwd_kernel(x, prep, n):
    """(name, call, partial floats) of the matrix-core weight-gradient kernel that serves x [n, F] under `prep`, or None."""
    lib, st = _lib.load(), prep.st
    if st.w1 and st.w2t:                                 # 64 columns
        if n < MFMA_BWD_FROM:
            return None
        return ("tpnet_mlp64_bwd_f32", lambda xp, gp, n_, part, nblk, stream: lib.tpnet_mlp64_bwd_f32(xp, gp, n_, prep.ref, part, nblk, stream),
                None)
    F = int(x.shape[1])
    rows_from = MLP_ROWS_BWD_FROM.get(F)
    if rows_from is None or n < rows_from or st.F != F:
        return None
    pf = int(lib.tpnet_mlp_rows_bwd_partial_floats(st.F, st.H))
    if not pf:
        return None

    def call(xp, gp, n_, part, nblk, stream):
        rc = lib.tpnet_mlp_rows_bwd_f32(xp, gp, n_, prep.ref, part, nblk, stream)
        calls["rows_bwd"] += rc > 0
        return rc

    return "tpnet_mlp_rows_bwd_f32", call, pf


def weight_grads_f32(x, gy, w1, b1, w2, prep, mode=None):
    """Gradients of (mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias) given the pre-mlp features x [n, F] and the gradient
    gy [n, F] of self.mlp's output, fp32 class.  Long lists (the encoder's calls: 80 000 rows each at C2) take ONE launch on the
    matrix cores (tpnet_mlp64_bwd_f32 at 64 columns from MFMA_BWD_FROM rows, tpnet_mlp_rows_bwd_f32 at 16 and 36 columns from
    MLP_ROWS_BWD_FROM[F] rows: hidden layer recomputed, both weight-gradient products contracted over the rows with
    two-piece bf16 operands and fp32 accumulation, one partial result per workgroup, summed in a fixed order) instead of five
    fp32 GEMMs and three elementwise passes over n x 4F floats; `prep` = the prepared() entry the forward used -- if a Parameter
    changed since (never in a normal training step), or for short lists and CPU tensors, the torch expressions serve.
    mode: "mfma" | "torch" (None: the module-level `mlp_backward`)."""
    mode = mode or mlp_backward
    n = int(x.shape[0])
    if (mode == "mfma" and prep is not None and x.is_cuda and x.dtype == torch.float32
            and prep.key[:6] == (w1.data_ptr(), w1._version, b1.data_ptr(), b1._version, w2.data_ptr(), w2._version)):
        kernel = _bwd_kernel(x, prep, n)
        if kernel is not None:
            name, call, pf = kernel
            rc, grads = _dense.mlp64_bwd(call, x, gy, *w1.shape, pf)
            if grads is not None:
                return grads
            if (name, rc) not in _declined_once:            # (said once per code: the torch expressions below serve the call)
                _declined_once.add((name, rc))
                warnings.warn(f"{name} declined a call of {n} rows (rc {rc}): weight gradients by the fp32 torch expressions")
    return _dense.layer_grads(x, gy, w1, b1, w2)


class _MlpF32(torch.autograd.Function):
    """self.mlp alone on the fp32 matrix cores (tpnet_mlp64_f32 at 64 columns, tpnet_mlp_rows_f32 at 16 and 36); backward =
    weight_grads_f32 (matrix-core kernels for all three widths: tpnet_mlp64_bwd_f32, tpnet_mlp_rows_bwd_f32), except when x itself
    needs a gradient: the torch expressions give all five."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, mlp_ref, prep=None, mode=None):
        x = x.contiguous()
        y = torch.empty_like(x)
        if x.shape[0]:
            if x.shape[1] == 64:
                rc = _lib.load().tpnet_mlp64_f32(x.data_ptr(), x.shape[0], mlp_ref, y.data_ptr(), _dense.stream_ptr(x.device))
                if rc:
                    _lib.check(rc, "mlp64_f32")
            elif _lib.load().tpnet_mlp_rows_f32(x.data_ptr(), x.shape[0], mlp_ref, y.data_ptr(), _dense.stream_ptr(x.device)):
                raise _RowsDeclined()                          # (nothing was launched: mlp_f32 hands the call back to torch)
        ctx.save_for_backward(x, w1, b1, w2)
        ctx.prep = prep
        ctx.mode = mode
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w1, b1, w2 = ctx.saved_tensors
        if ctx.needs_input_grad[0]:                            # (the readout's features carry no gradient; a caller's own x may)
            gw1, gb1, gw2, gb2, gx = _dense.layer_grads(x, gy, w1, b1, w2, input_grad=True)
            return gx, gw1, gb1, gw2, gb2, None, None, None
        gw1, gb1, gw2, gb2 = weight_grads_f32(x, gy, w1, b1, w2, ctx.prep, ctx.mode)
        return None, gw1, gb1, gw2, gb2, None, None, None


# rows from which tpnet_mlp_rows_f32 (csrc/mlp_rows.hip: num_layer 1 and 2) takes self.mlp from the torch layers, per width; None =
# reachable through the C call, never routed.  The rule (tools/mlp_rows_rate.py): the smallest measured n from which the kernel's
# median is below torch's by more than the larger of the two spreads.  Measured (profiles/mlp_rows.md): at 1 000 rows, the smallest
# size of the protocol, one launch takes 10.7 / 11.7 us against 47.6 / 49.6 us of the torch layers' launches; 800 000 rows
# 24.7 / 85.1 against 279 / 684 us.  Shorter lists were not measured and stay with torch.
MLP_ROWS_FROM = {16: 1000, 36: 1000}


class _RowsDeclined(Exception):
    """tpnet_mlp_rows_f32 returned an error before launching anything (a runtime that refuses the kernel's LDS or the launch)."""


def mlp_f32(mlp, x):
    """mlp(x) on the fp32 matrix cores where a kernel serves it on this GPU (else None): tpnet_mlp64_f32 if `mlp` is the reference's
    64-256-64, tpnet_mlp_rows_f32 if it is the 16-64-16 or 36-144-36 of num_layer 1 / 2 and x has MLP_ROWS_FROM[width] rows or more."""
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2:
        return None
    F = x.shape[1]
    if F == 64:
        prep = prepared(mlp, 64)
        if prep is None or not prep.st.w1:
            return None
    else:
        rows_from = MLP_ROWS_FROM.get(F)
        if rows_from is None or x.shape[0] < rows_from:
            return None
        prep = prepared(mlp, F)
        if prep is None or prep.st.F != F or not _lib.load().tpnet_mlp_rows_supported(prep.st.F, prep.st.H):
            return None
    try:
        # (a caller's own x that requires grad gets its gradient at 16 / 36 columns as it does from the torch layers)
        if needs_grad(prep.params) or (F != 64 and x.requires_grad and torch.is_grad_enabled()):
            return _MlpF32.apply(x, mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, prep.ref, prep, getattr(mlp, "mlp_backward", None))
        return _MlpF32.forward(_NoCtx(), x, None, None, None, None, prep.ref)
    except _RowsDeclined:
        return None


class _NoCtx:
    def save_for_backward(self, *a):
        pass


# ---- num_layer 4 (csrc/mlp_l4.hip): Linear(100, 400) -> ReLU -> Linear(400, 100) with the split weights streamed from an image
# rows from which tpnet_mlp_l4_f32 takes self.mlp from the torch layers under RandomProjectionModule.mlp_l4, and from which
# tpnet_mlp_l4_bwd_f32 takes the weight gradients from _dense.layer_grads; None = reachable through the C call, never routed.
# MLP_ROWS_FROM's rule, measured by tools/mlp_l4_rate.py (profiles/mlp_l4.md): under no_grad one launch takes 27.7 us at 1 000 rows, the
# smallest size of the protocol, against 48.4 us of the torch layers, 94.4 against 274 us at 80 000 rows and 834 against 2 629 us at
# 800 000; forward + backward 117 against 158 us, 569 against 1 072 us and 5 007 against 8 452 us.  Shorter lists were not measured
# and stay with torch.
MLP_L4_FROM = 1000
MLP_L4_BWD_FROM = 1000
L4_PARTIALS = 32                            # row parts of the backward's weight kernel = partial sums it writes, at most
_L4 = weakref.WeakKeyDictionary()           # mlp module -> L4Images


class L4Images(NamedTuple):
    key: tuple          # (data_ptr, _version) of w1, b1, w2, b2 when the images were last written
    img: torch.Tensor   # the forward's weight image (uint8)
    storage: tuple      # device + the Parameters' data_ptr()s: the same storage keeps the image buffers
    bimg: torch.Tensor = None   # the backward's image, once a training call asked for it (then kept current)


def l4_images(mlp, backward=False):
    """The L4Images record of `mlp`, or None if it is not Linear(100, 400) -> ReLU -> Linear(400, 100) with contiguous float32
    Parameters on a GPU.  Rewritten in place, on the current stream, when a Parameter changed through a versioned op (prepared()'s
    contract); `backward`: the record also holds the backward's image, and from then on both are rewritten together."""
    ls = _dense.linear_relu_linear(mlp)
    if ls is None or not _lib.load().tpnet_mlp_l4_supported(ls[0].in_features, ls[0].out_features) \
            or ls[1].out_features != ls[0].in_features:
        return None
    w1, b1, w2, b2 = ls[0].weight, ls[0].bias, ls[1].weight, ls[1].bias

    def build(previous, both):
        if not all(p.is_cuda and p.is_contiguous() and p.dtype == torch.float32 for p in (w1, b1, w2, b2)):
            return None
        lib, stream = _lib.load(), _dense.stream_ptr(w1.device)
        img, bimg = (previous.img, previous.bimg) if previous is not None else (None, None)
        if img is None:
            img = torch.empty(int(lib.tpnet_mlp_l4_image_bytes()), dtype=torch.uint8, device=w1.device)
        _lib.check(lib.tpnet_mlp_l4_prepare(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), img.data_ptr(), stream),
                   "mlp_l4_prepare")
        if both:
            if bimg is None:
                bimg = torch.empty(int(lib.tpnet_mlp_l4_bwd_image_bytes()), dtype=torch.uint8, device=w1.device)
            _lib.check(lib.tpnet_mlp_l4_bwd_prepare(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), bimg.data_ptr(), stream),
                       "mlp_l4_bwd_prepare")
        calls["l4_prepare"] += 1
        return L4Images(key, img, storage, bimg)

    key = _dense.param_key(w1, b1, w2, b2)
    storage = (w1.device, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr())
    return _dense.cached_images(_L4, mlp, key, storage, build, backward)


class _MlpL4(torch.autograd.Function):
    """Forward: tpnet_mlp_l4_f32; where the backward's kernels will serve (`bits`), it also records the ReLU's decisions.  Saved: x
    (the features, by reference) and relu_bits, 52 bytes per row; the Parameters stand for their images, which are looked up again
    in the backward (an in-place change in between raises as torch does).  Backward: tpnet_mlp_l4_bwd_f32 in a workspace of its
    own + the fixed-order sum of its partials; without bits, or where the C call declines, _dense.layer_grads."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, mlp, rec, bits):
        n = x.shape[0]
        y = torch.empty_like(x)
        relu_bits = torch.empty((n, 13), dtype=torch.int32, device=x.device) if bits else None
        if _lib.load().tpnet_mlp_l4_f32(x.data_ptr(), n, rec.img.data_ptr(), y.data_ptr(), relu_bits.data_ptr() if bits else None,
                                        _dense.stream_ptr(x.device)):
            raise _RowsDeclined()                              # (nothing was launched: mlp_l4 hands the call back to torch)
        calls["l4"] += 1
        ctx.save_for_backward(x, w1, b1, w2, b2, relu_bits)
        ctx.mlp = mlp
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, w1, b1, w2, b2, relu_bits = ctx.saved_tensors
        rec = l4_images(ctx.mlp, backward=True) if relu_bits is not None else None
        if rec is not None and rec.bimg is not None:
            lib, n, dev = _lib.load(), x.shape[0], x.device
            gy = gy.contiguous()
            part = _dense.partial_buffer(dev, L4_PARTIALS, lib.tpnet_mlp_l4_bwd_partial_floats())
            ws = torch.empty(int(lib.tpnet_mlp_l4_bwd_workspace_bytes(n)), dtype=torch.uint8, device=dev)
            rc = lib.tpnet_mlp_l4_bwd_f32(x.data_ptr(), relu_bits.data_ptr(), gy.data_ptr(), n, rec.bimg.data_ptr(), ws.data_ptr(),
                                          part.data_ptr(), part.shape[0], _dense.stream_ptr(dev))
            del ws                                              # (the caching allocator keeps it alive for the stream's launches)
            if rc > 0:
                calls["l4_bwd"] += 2
                grads = _dense.split_grads(_dense.sum_partials(rc, part, "mlp_l4_bwd"), (w1, b1, w2, b2), ctx.needs_input_grad[1:5])
                return (None, *grads, None, None, None)
            if ("tpnet_mlp_l4_bwd_f32", rc) not in _declined_once:
                _declined_once.add(("tpnet_mlp_l4_bwd_f32", rc))
                warnings.warn(f"tpnet_mlp_l4_bwd_f32 declined a call of {n} rows (rc {rc}): weight gradients by the fp32 torch expressions")
        return (None, *_dense.layer_grads(x, gy, w1, b1, w2), None, None, None)


def mlp_l4(mlp, x):
    """mlp(x) by tpnet_mlp_l4_f32 (one launch, fp32 class), or None where it does not serve the call: `mlp` is not num_layer 4's
    Linear(100, 400) -> ReLU -> Linear(400, 100) with contiguous float32 Parameters on the GPU of x, fewer rows than MLP_L4_FROM,
    mlp.mlp_backward = "torch" or an x that requires a gradient while one is recorded (the torch layers serve), a negative return code.
    Differentiable with respect to the four Parameters: from MLP_L4_BWD_FROM rows the forward records the ReLU's decisions and the
    backward is two launches (tpnet_mlp_l4_bwd_f32) + the sum of at most L4_PARTIALS partials."""
    if (MLP_L4_FROM is None or x.dim() != 2 or x.shape[0] < MLP_L4_FROM or x.shape[1] != 100 or x.dtype != torch.float32
            or not x.is_cuda):
        return None
    train = torch.is_grad_enabled()
    if train and (x.requires_grad or (getattr(mlp, "mlp_backward", None) or mlp_backward) == "torch"):
        return None
    ls = _dense.linear_relu_linear(mlp)
    if ls is None:
        return None
    params = (ls[0].weight, ls[0].bias, ls[1].weight, ls[1].bias)
    grads = train and any(p.requires_grad for p in params)
    bits = grads and MLP_L4_BWD_FROM is not None and x.shape[0] >= MLP_L4_BWD_FROM
    rec = l4_images(mlp, backward=bits)
    if rec is None or rec.img.device != x.device:
        return None
    x = x.contiguous()
    try:
        if grads:
            return _MlpL4.apply(x, *params, mlp, rec, bits)
        return _MlpL4.forward(_NoCtx(), x, None, None, None, None, None, rec, False)
    except _RowsDeclined:
        return None


def invalidate(mlp=None):
    """Forget the prepared copies of `mlp`'s weights (all modules' if None).  The cache is keyed on (data_ptr, _version) of the
    four tensors; an in-place write THROUGH `.data` (p.data.copy_(), p.data.mul_(): some EMA / weight-averaging helpers) bumps
    neither, so whoever writes that way calls this afterwards.  Optimizer steps, load_state_dict, .to() and plain in-place ops
    on the Parameters are seen without it."""
    if mlp is None:
        _PREPARED.clear()
        _L4.clear()
    else:
        _PREPARED.pop(mlp, None)
        _L4.pop(mlp, None)


def prepared(mlp, F):
    """A Prepared record, or None if `mlp` is not the reference's Linear-ReLU-Linear on
    a GPU: transposed f32 copies of the weights, rebuilt only when a parameter changed (optimizer step, load_state_dict,
    .to()): keyed on (data_ptr, _version) of the four tensors.
    CONTRACT: the Parameters are updated through versioned ops (optimizer steps, copy_(), load_state_dict, .to()).  b1, b2 and
    tpnet_mlp::w1 are the Parameters' OWN storage while w1t / w2t / w2f / wimg are derived copies, so a write that bumps no version
    counter (p.data.clamp_(), a raw pointer) leaves a MIX of live and stale values until invalidate(mlp) is called; and the derived
    buffers are rewritten in place on the CURRENT stream -- update the Parameters on the stream that runs the module's kernels (the
    reference's loop has one stream)."""
    try:
        l1, l2 = mlp._modules["0"], mlp._modules["2"]
        p1, p2 = l1._parameters, l2._parameters      # (the dicts behind l1.weight ...: nn.Module.__getattr__ is ~0.4 us per read,
        w1, b1, w2, b2 = p1["weight"], p1["bias"], p2["weight"], p2["bias"]   #  and this runs on every call)
        if w1 is None or b1 is None or w2 is None or b2 is None:
            return None
    except (KeyError, AttributeError):
        return None
    # (this runs on every per-batch call: the key and its check stay inline -- _dense.param_key / _dense.cached would add two
    # Python frames to the hit path; the rebuild below goes through the shared cache function)
    key = (w1.data_ptr(), w1._version, b1.data_ptr(), b1._version, w2.data_ptr(), w2._version, b2.data_ptr(), b2._version)
    cache = _PREPARED.get(mlp)
    if cache is not None and cache.key == key:
        return cache
    storage = (w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr())

    def build(previous):
        if not supported(mlp, F) or not (w1.is_contiguous() and w2.is_contiguous() and b1.is_contiguous() and b2.is_contiguous()):
            return None
        # the derived layouts (w1t, w2t and, for F = 64, the gathered w2f) live in buffers that stay with the module and are
        # rewritten by ONE launch (tpnet_mlp_prepare) when a parameter changed; b1, b2 and tpnet_mlp::w1 are the Parameters' own
        # storage.  (As torch expressions -- two transposes, a copy, an index gather -- this was ~100 us of every training step.)
        if previous is not None:
            keep, st = previous.derived, previous.st
        else:
            H = w1.shape[0]
            x64 = F == 64 and H == 256
            keep = (torch.empty((F, H), dtype=torch.float32, device=w1.device), torch.empty((H, F), dtype=torch.float32, device=w1.device),
                    torch.empty(F * H, dtype=torch.float32, device=w1.device) if x64 else None,
                    # the weight image of the encoder's one-launch readout + dense layers (csrc/encoder_mfma.hip)
                    torch.empty(int(_lib.load().tpnet_mlp_image_bytes()), dtype=torch.uint8, device=w1.device) if x64 else None)
            st = _lib.Mlp(w1t=keep[0].data_ptr(), b1=b1.data_ptr(), w2t=keep[1].data_ptr(), b2=b2.data_ptr(), F=F, H=H,
                          w1=w1.data_ptr() if keep[2] is not None else None,
                          w2f=keep[2].data_ptr() if keep[2] is not None else None,
                          wimg=keep[3].data_ptr() if keep[3] is not None else None)
        _lib.check(_lib.load().tpnet_mlp_prepare(w1.data_ptr(), w2.data_ptr(), F, w1.shape[0], keep[0].data_ptr(), keep[1].data_ptr(),
                                                 keep[2].data_ptr() if keep[2] is not None else None, _dense.stream_ptr(w1.device)), "mlp_prepare")
        if keep[3] is not None:
            _lib.check(_lib.load().tpnet_mlp_prepare_image(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), keep[3].data_ptr(),
                                                           _dense.stream_ptr(w1.device)), "mlp_prepare_image")
        return Prepared(key, st, C.byref(st), keep, (w1, b1, w2, b2), storage)

    return _dense.cached(_PREPARED, mlp, key, storage, build)


class _FusedFeature(torch.autograd.Function):
    """forward(w1, b1, w2, b2, launch): `launch(out_gram)` enqueues the fused kernel and returns the features."""

    @staticmethod
    def forward(ctx, w1, b1, w2, b2, launch, n, F, prep=None, mode=None):
        gram = torch.empty((n, F), dtype=torch.float32, device=w1.device)
        out = launch(gram)
        ctx.save_for_backward(gram, w1, b1, w2)
        ctx.prep = prep
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, gy):
        x, w1, b1, w2 = ctx.saved_tensors
        gw1, gb1, gw2, gb2 = weight_grads_f32(x, gy, w1, b1, w2, ctx.prep, ctx.mode)
        return gw1, gb1, gw2, gb2, None, None, None, None, None


def needs_grad(keep_params) -> bool:
    return torch.is_grad_enabled() and any(p.requires_grad for p in keep_params)


def apply_with_grad(mlp, launch, n, F):
    return _FusedFeature.apply(mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, launch, n, F, _PREPARED.get(mlp),
                               getattr(mlp, "mlp_backward", None))
