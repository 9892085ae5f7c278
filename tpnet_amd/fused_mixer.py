"""One MLP-Mixer layer in two launches (C ABI: tpnet_mixer_*, csrc/mixer.hip): token mixing as an exact-fp32 kernel, channel mixing
(LayerNorm -> Linear(C, Ch) -> GELU -> Linear(Ch, C) -> + residual, models/TPNet.py:371-416) on the matrix cores in the project's
fp32 class, dropout as identity.  Forward only and opt-in: the caller (tpnet_amd/encoder.py, TPNetEmbedding.fused_mixer) takes it
when no gradient is recorded and no dropout is active.  The split weights of the channel FFN are kept per mixer like
fused_input.prepared() keeps projection_layer's: rewritten by one launch when a Parameter's (data_ptr, _version) changed.  The
LayerNorms' and the token FFN's Parameters are read in place at every call and need no image.

The token-mixing half also runs in a TRAINING step (csrc/mixer_token_train.hip; opt-in, TPNetEmbedding.fused_token_training):
`token_train` is x + token_feedforward(token_norm(x^T))^T with both dropouts as ONE launch forward and ONE launch backward under
autograd.  The backward recomputes the forward from x, so x is the only activation saved.  The dropout masks come from a
counter-based generator on the device, keyed per call (include/tpnet_hip.h): they follow nn.Dropout's probabilities but are NOT
torch's dropout stream.

So does the channel-mixing half (csrc/mixer_channel_train.hip; opt-in, TPNetEmbedding.fused_channel_training): `channel_train` is
x + channel_feedforward(channel_norm(x)) with both dropouts as ONE launch forward and TWO backward on the matrix cores, in the
fp32 class.  Again x is the only activation saved; the backward's transposed operands live in a workspace that is allocated and
freed inside the backward.  Its second image (W1, W2^T, W1^T) sits in the same per-mixer record and is written with the first once
a training call has asked for it.  Its masks are again nn.Dropout's probabilities from the device's counter-based generator, NOT
torch's dropout stream."""
import weakref
from typing import NamedTuple

import torch

from . import _dense, _lib

_PREPARED = weakref.WeakKeyDictionary()                 # mixer -> Prepared
# launches made through this binding (tests assert the dispatch through it)
calls = {"token": 0, "channel": 0, "prepare": 0, "token_train": 0, "token_bwd": 0, "channel_train": 0, "channel_bwd": 0}
MAX_PARTIALS = 256                                      # workgroups of a backward launch = partial sums it writes, at most
# row parts of the channel backward's weight kernel = partial sums it writes, at most: 2 ceil(Ch / 32) waves per part, so 32 parts of
# the reference's 172 -> 688 -> 172 are 1 408 waves for the 1 024 SIMDs, and 32 partials of 237 876 floats are 30 MB
# (profiles/mixer_channel_training.md)
CHANNEL_PARTIALS = 32

layers_of = _dense.mixer_layers                         # the structural test: MixerLayers, or None for another module


class Prepared(NamedTuple):
    key: tuple          # dims + (data_ptr, _version) of the channel FFN's w1, b1, w2, b2 when the image was last written
    dims: tuple         # K, Kh, C, Ch
    img: torch.Tensor   # the channel FFN's weight image (uint8)
    storage: tuple      # device + the Parameters' data_ptr()s + dims: the same storage keeps the image buffer
    bimg: torch.Tensor = None   # the channel backward's image of (W1, W2^T, W1^T), once a training call asked for it (then kept current)


def _dims(ls):
    return (int(ls.token[0].in_features), int(ls.token[0].out_features), int(ls.channel[0].in_features), int(ls.channel[0].out_features))


def _params(ls):
    """The twelve Parameters: token norm, token FFN, channel norm, channel FFN."""
    return (ls.token_norm.weight, ls.token_norm.bias, ls.token[0].weight, ls.token[0].bias, ls.token[1].weight, ls.token[1].bias,
            ls.channel_norm.weight, ls.channel_norm.bias, ls.channel[0].weight, ls.channel[0].bias, ls.channel[1].weight,
            ls.channel[1].bias)


def supported(mixer) -> bool:
    ls = layers_of(mixer)
    if ls is None:
        return False
    ps = _params(ls)
    dev = ps[0].device
    if not all(p.is_cuda and p.device == dev and p.dtype == torch.float32 and p.is_contiguous() and p.data_ptr() % 16 == 0 for p in ps):
        return False
    return bool(_lib.load().tpnet_mixer_supported(*_dims(ls)))


def invalidate(mixer=None):
    """Forget the prepared image of `mixer` (all mixers' if None): for whoever writes a Parameter through `.data` or a raw pointer,
    which bumps no version counter (same contract as fused_input.invalidate)."""
    if mixer is None:
        _PREPARED.clear()
    else:
        _PREPARED.pop(mixer, None)


def cached(mixer):
    """The Prepared record `mixer` has now (None: no launch has served it yet, or invalidate() dropped it).  No GPU call."""
    return _PREPARED.get(mixer)


def prepared(mixer, backward=False):
    """The Prepared record of `mixer`, or None where the kernels do not serve it.  The image is rewritten in place, on the current
    stream, when a Parameter of the channel FFN changed through a versioned op (optimizer step, load_state_dict, copy_()).
    `backward`: the record also holds the channel backward's image; from then on both are rewritten together."""
    ls = layers_of(mixer)
    if ls is None:
        return None
    w1, b1, w2, b2 = ls.channel[0].weight, ls.channel[0].bias, ls.channel[1].weight, ls.channel[1].bias
    d = _dims(ls)

    def build(previous, both):
        if not supported(mixer):
            return None
        lib = _lib.load()
        img = bimg = None
        if previous is not None:
            img, bimg = previous.img, previous.bimg
        else:
            img = torch.empty(int(lib.tpnet_mixer_channel_image_bytes(d[2], d[3])), dtype=torch.uint8, device=w1.device)
        _lib.check(lib.tpnet_mixer_channel_prepare(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), d[2], d[3], img.data_ptr(),
                                                   _dense.stream_ptr(w1.device)), "mixer_channel_prepare")
        if both:
            if bimg is None:
                bimg = torch.empty(int(lib.tpnet_mixer_channel_bwd_image_bytes(d[2], d[3])), dtype=torch.uint8, device=w1.device)
            _lib.check(lib.tpnet_mixer_channel_bwd_prepare(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), d[2], d[3], bimg.data_ptr(),
                                                           _dense.stream_ptr(w1.device)), "mixer_channel_bwd_prepare")
        calls["prepare"] += 1
        return Prepared(key, d, img, storage, bimg)

    key = d + _dense.param_key(w1, b1, w2, b2)
    storage = (w1.device, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()) + d
    return _dense.cached_images(_PREPARED, mixer, key, storage, build, backward)


def mixer_token(mixer, x):
    """x + token_feedforward(token_norm(x^T))^T of x [n, K, C] float32 (contiguous, on the Parameters' device) as a new tensor: one
    launch on the current stream, no synchronisation."""
    ls = layers_of(mixer)
    K, Kh, C, _ = _dims(ls)
    _check_token_input(ls, x, "mixer_token")
    out = torch.empty_like(x)
    g, b, w1, b1, w2, b2 = _params(ls)[:6]
    _lib.check(_lib.load().tpnet_mixer_token(x.data_ptr(), x.shape[0], K, C, g.data_ptr(), b.data_ptr(), float(ls.token_norm.eps),
                                             w1.data_ptr(), b1.data_ptr(), Kh, w2.data_ptr(), b2.data_ptr(), out.data_ptr(),
                                             _dense.stream_ptr(x.device)), "mixer_token")
    calls["token"] += 1
    return out


def mixer_channel(prep: Prepared, mixer, x):
    """x + channel_feedforward(channel_norm(x)) of x [..., C] float32 (contiguous, on the image's device) as a new tensor: one launch
    on the current stream, no synchronisation."""
    ls = layers_of(mixer)
    C, Ch = prep.dims[2:]
    if x.dtype != torch.float32 or x.dim() < 1 or x.shape[-1] != C or not x.is_contiguous() or x.device != prep.img.device:
        raise ValueError("mixer_channel: x must be a contiguous float32 [..., C] on the prepared mixer's device")
    out = torch.empty_like(x)
    g, b = ls.channel_norm.weight, ls.channel_norm.bias
    _lib.check(_lib.load().tpnet_mixer_channel(x.data_ptr(), x.numel() // C, C, Ch, g.data_ptr(), b.data_ptr(), float(ls.channel_norm.eps),
                                               prep.img.data_ptr(), out.data_ptr(), _dense.stream_ptr(x.device)), "mixer_channel")
    calls["channel"] += 1
    return out


def mixer_forward(prep: Prepared, mixer, x):
    """MLPMixer.forward of x [n, K, C] with dropout as identity, as a new tensor: two launches."""
    return mixer_channel(prep, mixer, mixer_token(mixer, x))


def _check_token_input(ls, x, what):
    K, _, C, _ = _dims(ls)
    if x.dtype != torch.float32 or x.dim() != 3 or tuple(x.shape[1:]) != (K, C) or not x.is_contiguous() \
            or x.device != ls.token_norm.weight.device:
        raise ValueError(f"{what}: x must be a contiguous float32 [n, K, C] on the mixer's device")


def _rate_and_key(p, key, what):
    """(p, key) as the training calls take them: 0 <= p < 1, and a 64-bit key.  key None: 64 bits from torch's default CPU generator
    (no device synchronisation, reproducible under torch.manual_seed) -- at p = 0 nothing is drawn from it, the key is 0."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{what}: 0 <= p < 1")
    if key is None:
        key = 0
        if p > 0.0:
            hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
            key = hi << 32 | lo
    return p, int(key) & (1 << 64) - 1


class _TokenTrain(torch.autograd.Function):
    """Forward: tpnet_mixer_token_train.  Saved: x and the six Parameters.  Backward: tpnet_mixer_token_bwd + the fixed-order sum of
    its partials."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w1, b1, w2, b2, eps, p, key):
        n, K, C = x.shape
        Kh = w1.shape[0]
        out = torch.empty_like(x)
        _lib.check(_lib.load().tpnet_mixer_token_train(x.data_ptr(), n, K, C, gamma.data_ptr(), beta.data_ptr(), eps, w1.data_ptr(),
                                                       b1.data_ptr(), Kh, w2.data_ptr(), b2.data_ptr(), p, key, out.data_ptr(),
                                                       _dense.stream_ptr(x.device)), "mixer_token_train")
        calls["token_train"] += 1
        ctx.save_for_backward(x, gamma, beta, w1, b1, w2, b2)
        ctx.consts = (eps, p, key)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, gamma, beta, w1, b1, w2, b2 = ctx.saved_tensors
        eps, p, key = ctx.consts
        n, K, C = x.shape
        Kh = w1.shape[0]
        gy = gy.contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        tot = None
        if n > 0:
            lib = _lib.load()
            part = _dense.partial_buffer(x.device, MAX_PARTIALS, lib.tpnet_mixer_token_bwd_partial_floats(K, Kh))
            rc = lib.tpnet_mixer_token_bwd(x.data_ptr(), gy.data_ptr(), n, K, C, gamma.data_ptr(), beta.data_ptr(), eps, w1.data_ptr(),
                                           b1.data_ptr(), Kh, w2.data_ptr(), b2.data_ptr(), p, key,
                                           None if gx is None else gx.data_ptr(), part.data_ptr(), part.shape[0],
                                           _dense.stream_ptr(x.device))
            tot = _dense.sum_partials(rc, part, "mixer_token_bwd")
            calls["token_bwd"] += 1
        return (gx, *_dense.split_grads(tot, (gamma, beta, w1, b1, w2, b2), ctx.needs_input_grad[1:7]), None, None, None)


def token_train(mixer, x, p, key=None):
    """x + token_feedforward(token_norm(x^T))^T of x [n, K, C] float32 (contiguous, on the Parameters' device) with both dropouts of
    the token FFN at rate `p` (0 <= p < 1; 0: none), differentiable with respect to x and the six Parameters: one launch forward,
    one launch backward (+ the sum of at most MAX_PARTIALS partial results), no synchronisation.  `key`: the 64-bit key of this
    call's dropout draws; None draws one from torch's default CPU generator, so torch.manual_seed makes a run reproducible.  The
    masks are nn.Dropout's probabilities from the device's counter-based generator (token_masks returns them), NOT torch's
    dropout stream."""
    ls = layers_of(mixer)
    _check_token_input(ls, x, "token_train")
    p, key = _rate_and_key(p, key, "token_train")
    return _TokenTrain.apply(x, *_params(ls)[:6], float(ls.token_norm.eps), p, key)


def token_masks(mixer, n, C, p, key):
    """The keep masks token_train(mixer, x [n, K, C], p, key) applies, as bool tensors: m1 [n, C, Kh] (behind the GELU) and
    m2 [n, K, C] (behind the second Linear)."""
    ls = layers_of(mixer)
    K, Kh = _dims(ls)[:2]
    dev = ls.token_norm.weight.device
    m1 = torch.empty((n, C, Kh), dtype=torch.uint8, device=dev)
    m2 = torch.empty((n, K, C), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().tpnet_mixer_token_masks(n, K, Kh, C, float(p), int(key) & (1 << 64) - 1, m1.data_ptr(), m2.data_ptr(),
                                                   _dense.stream_ptr(dev)), "mixer_token_masks")
    return m1.bool(), m2.bool()


class _ChannelTrain(torch.autograd.Function):
    """Forward: tpnet_mixer_channel_train.  Saved: x and the six Parameters (the images are derived from them and looked up again in
    the backward: an in-place change in between raises as torch does).  Backward: tpnet_mixer_channel_bwd in a workspace of its
    own + the fixed-order sum of its partials."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w1, b1, w2, b2, mixer, eps, p, key):
        Ch, C = w1.shape
        prep = prepared(mixer, backward=True)
        out = torch.empty_like(x)
        if x.numel() > 0:                                       # (an empty tensor has no pointer to give)
            _lib.check(_lib.load().tpnet_mixer_channel_train(x.data_ptr(), x.numel() // C, C, Ch, gamma.data_ptr(), beta.data_ptr(), eps,
                                                             prep.img.data_ptr(), p, key, out.data_ptr(), _dense.stream_ptr(x.device)),
                       "mixer_channel_train")
            calls["channel_train"] += 1
        ctx.save_for_backward(x, gamma, beta, w1, b1, w2, b2)
        ctx.mixer = mixer
        ctx.consts = (eps, p, key)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, gamma, beta, w1, b1, w2, b2 = ctx.saved_tensors
        eps, p, key = ctx.consts
        Ch, C = w1.shape
        n = x.numel() // C
        gy = gy.contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        tot = None
        if n > 0:
            lib = _lib.load()
            prep = prepared(ctx.mixer, backward=True)           # (current: the saved Parameters are unchanged, or torch has raised)
            part = _dense.partial_buffer(x.device, CHANNEL_PARTIALS, lib.tpnet_mixer_channel_bwd_partial_floats(C, Ch))
            ws = torch.empty(int(lib.tpnet_mixer_channel_bwd_workspace_bytes(n, C, Ch)), dtype=torch.uint8, device=x.device)
            rc = lib.tpnet_mixer_channel_bwd(x.data_ptr(), gy.data_ptr(), n, C, Ch, gamma.data_ptr(), beta.data_ptr(), eps,
                                             prep.bimg.data_ptr(), p, key, ws.data_ptr(),
                                             None if gx is None else gx.data_ptr(), part.data_ptr(), part.shape[0],
                                             _dense.stream_ptr(x.device))
            tot = _dense.sum_partials(rc, part, "mixer_channel_bwd")
            calls["channel_bwd"] += 1
            del ws                                              # (the caching allocator keeps it alive for the stream's launches)
        return (gx, *_dense.split_grads(tot, (gamma, beta, w1, b1, w2, b2), ctx.needs_input_grad[1:7]), None, None, None, None)


def channel_train(mixer, x, p, key=None):
    """x + channel_feedforward(channel_norm(x)) of x [..., C] float32 (contiguous, on the Parameters' device) with both dropouts of
    the channel FFN at rate `p` (0 <= p < 1; 0: none), differentiable with respect to x and the six Parameters: one launch forward,
    two backward (+ the sum of at most CHANNEL_PARTIALS partial results), no synchronisation, on the matrix cores in the
    project's fp32 class.  `key`: the 64-bit key of this call's dropout draws; None draws one from torch's default CPU generator,
    so torch.manual_seed makes a run reproducible.  The masks are nn.Dropout's probabilities from the device's counter-based
    generator (channel_masks returns them), NOT torch's dropout stream."""
    ls = layers_of(mixer)
    C = _dims(ls)[2]
    if x.dtype != torch.float32 or x.dim() < 1 or x.shape[-1] != C or not x.is_contiguous() \
            or x.device != ls.channel_norm.weight.device:
        raise ValueError("channel_train: x must be a contiguous float32 [..., C] on the mixer's device")
    p, key = _rate_and_key(p, key, "channel_train")
    if prepared(mixer, backward=True) is None:
        raise ValueError("channel_train: the kernels do not serve this mixer")
    return _ChannelTrain.apply(x, *_params(ls)[6:], mixer, float(ls.channel_norm.eps), p, key)


def channel_masks(mixer, n_rows, p, key):
    """The keep masks channel_train(mixer, x [n_rows, C], p, key) applies, as bool tensors: m1 [n_rows, Ch] (behind the GELU) and
    m2 [n_rows, C] (behind the second Linear)."""
    ls = layers_of(mixer)
    C, Ch = _dims(ls)[2:]
    dev = ls.channel_norm.weight.device
    m1 = torch.empty((n_rows, Ch), dtype=torch.uint8, device=dev)
    m2 = torch.empty((n_rows, C), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().tpnet_mixer_channel_masks(n_rows, C, Ch, float(p), int(key) & (1 << 64) - 1, m1.data_ptr(), m2.data_ptr(),
                                                     _dense.stream_ptr(dev)), "mixer_channel_masks")
    return m1.bool(), m2.bool()
