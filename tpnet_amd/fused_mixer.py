"""One MLP-Mixer layer in two launches (C ABI: tpnet_mixer_*, csrc/mixer.hip): token mixing as an exact-fp32 kernel, channel mixing
(LayerNorm -> Linear(C, Ch) -> GELU -> Linear(Ch, C) -> + residual, models/TPNet.py:371-416) on the matrix cores in the project's
fp32 class, dropout as identity.  Forward only and opt-in: the caller (tpnet_amd/encoder.py, TPNetEmbedding.fused_mixer) takes it
when no gradient is recorded and no dropout is active.  The split weights of the channel FFN are kept per mixer like
fused_input.prepared() keeps projection_layer's: rewritten by one launch when a Parameter's (data_ptr, _version) changed.  The
LayerNorms' and the token FFN's Parameters are read in place at every call and need no image."""
import weakref
from typing import NamedTuple

import torch

from . import _dense, _lib

_PREPARED = weakref.WeakKeyDictionary()                 # mixer -> Prepared
calls = {"token": 0, "channel": 0, "prepare": 0}        # launches made through this binding (tests assert the dispatch through it)

layers_of = _dense.mixer_layers                         # the structural test: MixerLayers, or None for another module


class Prepared(NamedTuple):
    key: tuple          # dims + (data_ptr, _version) of the channel FFN's w1, b1, w2, b2 when the image was last written
    dims: tuple         # K, Kh, C, Ch
    img: torch.Tensor   # the channel FFN's weight image (uint8)
    storage: tuple      # device + the Parameters' data_ptr()s + dims: the same storage keeps the image buffer


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


def prepared(mixer):
    """The Prepared record of `mixer`, or None where the kernels do not serve it.  The image is rewritten in place, on the current
    stream, when a Parameter of the channel FFN changed through a versioned op (optimizer step, load_state_dict, copy_())."""
    ls = layers_of(mixer)
    if ls is None:
        return None
    w1, b1, w2, b2 = ls.channel[0].weight, ls.channel[0].bias, ls.channel[1].weight, ls.channel[1].bias
    d = _dims(ls)

    def build(previous):
        if not supported(mixer):
            return None
        lib = _lib.load()
        if previous is not None:
            img = previous.img
        else:
            img = torch.empty(int(lib.tpnet_mixer_channel_image_bytes(d[2], d[3])), dtype=torch.uint8, device=w1.device)
        _lib.check(lib.tpnet_mixer_channel_prepare(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), d[2], d[3], img.data_ptr(),
                                                   _dense.stream_ptr(w1.device)), "mixer_channel_prepare")
        calls["prepare"] += 1
        return Prepared(key, d, img, storage)

    key = d + _dense.param_key(w1, b1, w2, b2)
    storage = (w1.device, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()) + d
    return _dense.cached(_PREPARED, mixer, key, storage, build)


def mixer_token(mixer, x):
    """x + token_feedforward(token_norm(x^T))^T of x [n, K, C] float32 (contiguous, on the Parameters' device) as a new tensor: one
    launch on the current stream, no synchronisation."""
    ls = layers_of(mixer)
    K, Kh, C, _ = _dims(ls)
    if x.dtype != torch.float32 or x.dim() != 3 or tuple(x.shape[1:]) != (K, C) or not x.is_contiguous() \
            or x.device != ls.token_norm.weight.device:
        raise ValueError("mixer_token: x must be a contiguous float32 [n, K, C] on the mixer's device")
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
