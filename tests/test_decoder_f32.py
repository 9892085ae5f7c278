"""LinkPredictor_v1 in the fp32 class (`fused = "f32"`; tpnet_amd/fused_decoder.py, C ABI tpnet_decoder_f32*, csrc/decoder_train.hip):
one launch forward, two backward, the ReLU's decisions recomputed with the forward's bits.

CPU tier: the symbols, the size queries against hand arithmetic, bad arguments, the switch's default and its fall-through to the torch
layers.  GPU tier: direct ABI calls into views whose surroundings are NaN, against a float64 evaluation on the host that uses the
decisions the kernel used; per entry |got - want| <= 4e-5 mag + 1e-6 max|want| (the project's bound for an fp32-class stage,
tests/test_encoder_input_training.py::_check), mag the same expression over the absolute values of its terms.  Then the module and
one step of the training loop.  Every test prints its largest err / bound per tensor."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tpnet_amd import fused_decoder as fd  # noqa: E402
from tpnet_amd.callers import LinkPredictor_v1  # noqa: E402

PAD = 64                                       # floats of NaN either side of a guarded view (a multiple of 4: the view stays 16-byte aligned)
NEW = ("tpnet_decoder_f32_supported", "tpnet_decoder_f32_partial_floats", "tpnet_decoder_f32_bwd_workspace_bytes", "tpnet_decoder_f32",
       "tpnet_decoder_f32_bwd")
UNSERVED = [(170, 64, 172), (260, 64, 172), (172, 6, 172), (172, 104, 172), (172, 64, 0), (172, 64, 257), (0, 0, 172)]


def pad32(v):
    return (v + 31) // 32 * 32


# ---------------------------------------------------------------------------------------------------------------------- CPU tier
def test_new_symbols_in_library_binding_and_header(hip_lib):
    from tpnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "tpnet_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert hasattr(raw, s) and s in _lib.SIGNATURES and s + "(" in header, s
    assert hip_lib.tpnet_abi_version() == 7


def test_size_queries_are_hand_arithmetic(hip_lib):
    for D, F, H in [(172, 64, 172), (4, 0, 1)]:
        K = 2 * D + F
        assert hip_lib.tpnet_decoder_f32_supported(D, F, H) == 1
        assert hip_lib.tpnet_decoder_f32_partial_floats(D, F, H) == H * K + 2 * H + 1
        for n in (0, 1, 200, 1000, 2 ** 31 - 1):
            tiles = (n + 31) // 32
            assert hip_lib.tpnet_decoder_f32_bwd_workspace_bytes(n, D, F, H) == tiles * 32 * (2 * pad32(H) + pad32(K) + 1) * 4
        assert hip_lib.tpnet_decoder_f32_bwd_workspace_bytes(-1, D, F, H) == 0
        assert hip_lib.tpnet_decoder_f32_bwd_workspace_bytes(2 ** 31, D, F, H) == 0
    assert hip_lib.tpnet_decoder_f32_partial_floats(172, 64, 172) == 70521
    assert hip_lib.tpnet_decoder_f32_bwd_workspace_bytes(200, 172, 64, 172) == 7 * 32 * (2 * 192 + 416 + 1) * 4
    for D, F, H in UNSERVED:
        assert hip_lib.tpnet_decoder_f32_supported(D, F, H) == 0, (D, F, H)
        assert hip_lib.tpnet_decoder_f32_partial_floats(D, F, H) == 0
        assert hip_lib.tpnet_decoder_f32_bwd_workspace_bytes(200, D, F, H) == 0
    for D, F, H in [(0, 16, 33), (20, 36, 64), (256, 100, 256), (8, 100, 256), (256, 0, 1)]:
        assert hip_lib.tpnet_decoder_f32_supported(D, F, H) == 1, (D, F, H)


def test_bad_arguments_return_minus_one_and_nothing_is_launched(hip_lib):
    """Every check comes before any GPU call: this runs without a GPU, on addresses that are never read."""
    A = 1 << 20                                                            # an aligned address that is never dereferenced
    D, F, H, n = 8, 4, 5, 10
    fwd = dict(src=A, dst=A, D=D, feat=A, F=F, n=n, w1=A, b1=A, w2=A, b2=A, H=H, out=A, hidden=None, stream=None)
    bwd = dict(src=A, dst=A, D=D, feat=A, F=F, n=n, w1=A, b1=A, w2=A, H=H, gout=A, ws=A, gsrc=A, gdst=A, gfeat=A, partial=A, parts=1,
               stream=None)

    def f(**kw):
        return hip_lib.tpnet_decoder_f32(*{**fwd, **kw}.values())

    def b(**kw):
        return hip_lib.tpnet_decoder_f32_bwd(*{**bwd, **kw}.values())

    assert f(n=0) == 0 and b(n=0) == 0                                      # no rows: nothing to do
    for name in ("w1", "b1", "w2", "b2", "out", "src", "dst", "feat"):      # (one of src / dst alone, a feature missing at F > 0)
        assert f(**{name: None}) == -1, name
    for name in ("w1", "b1", "w2", "gout", "ws", "partial", "src", "dst", "feat"):
        assert b(**{name: None}) == -1, name
    assert b(src=None, dst=None) == -1                                      # a gradient for embeddings that are not read
    assert b(src=None, dst=None, gsrc=None, gdst=None, n=0) == 0
    assert f(src=None, dst=None, feat=None, F=0) == -1                      # no source at all
    assert f(feat=A, F=0, D=8) == -1                                        # a feature array at F = 0
    for name in ("src", "dst", "feat", "w1"):
        assert f(**{name: A + 4}) == -1 and b(**{name: A + 4}) == -1, name
    for name in ("b1", "w2", "b2", "out", "hidden"):
        assert f(**{name: A + 2}) == -1, name
    for name in ("gsrc", "gdst", "gfeat", "ws"):
        assert b(**{name: A + 4}) == -1, name
    for name in ("b1", "w2", "gout", "partial"):
        assert b(**{name: A + 2}) == -1, name
    for bad in (-1, 2 ** 31, 2 ** 40):
        assert f(n=bad) == -1 and b(n=bad) == -1
    assert b(parts=0) == -1 and b(parts=-3) == -1
    for D_, F_, H_ in UNSERVED:
        kw = dict(D=D_, F=F_, H=H_) if F_ else dict(D=D_, F=F_, H=H_, feat=None)
        assert f(**kw) == -1 and b(**kw) == -1, (D_, F_, H_)


class _FeatStub(torch.nn.Module):
    """stands in for RandomProjectionModule: hands out a fixed feature matrix (a Parameter: it takes a gradient; else a buffer)"""

    def __init__(self, feat, grad=True):
        super().__init__()
        self.pair_wise_feature_dim = feat.shape[1]
        if grad:
            self.feat = torch.nn.Parameter(feat)
        else:
            self.register_buffer("feat", feat)

    def get_pair_wise_feature(self, src_node_ids, dst_node_ids):
        return self.feat[: len(src_node_ids)]


def _quarters_(lin, rng, lo=-4, hi=5):
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(rng.randint(lo, hi, tuple(lin.weight.shape)).astype(np.float32)) / 4.0)
        lin.bias.copy_(torch.from_numpy(rng.randint(lo, hi, tuple(lin.bias.shape)).astype(np.float32)) / 2.0)


def _ints(rng, shape, lo=-3, hi=4):
    return torch.from_numpy(rng.randint(lo, hi, shape).astype(np.float32))


def test_switch_defaults_to_false_and_a_cpu_module_keeps_the_torch_layers():
    rng = np.random.RandomState(5)
    n, D, F, H = 9, 8, 16, 12
    dec = LinkPredictor_v1(D, D, H, 1, _FeatStub(torch.from_numpy(rng.standard_normal((n, F)).astype(np.float32))), False)
    assert dec.fused is False
    ids = np.arange(n)
    src = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).requires_grad_(True)
    dst = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).requires_grad_(True)
    g = torch.from_numpy(rng.standard_normal((n, 1)).astype(np.float32))
    inputs = list(dec.parameters()) + [src, dst]
    before = dict(fd.calls)
    for not_encode in (False, True):
        dec.not_encode = not_encode
        dec.fused = False
        ref = dec(ids, ids, src, dst)
        gr = torch.autograd.grad(ref, inputs, g, allow_unused=True)
        dec.fused = "f32"
        out = dec(ids, ids, src, dst)
        gf = torch.autograd.grad(out, inputs, g, allow_unused=True)
        assert torch.equal(out, ref)
        for a, b in zip(gf, gr):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    assert fd.calls == before
    with pytest.raises(ValueError):
        dec.fused = "bf16"
        dec(ids, ids, src, dst)


def test_true_still_means_the_bf16_kernel():
    """`fused = True` on a CPU module: the bf16 route's own `supported` still takes the shape it took (F % 16 == 0) and refuses
    F = 36, which only the fp32 class serves; its packed weights are what they were."""
    fc1, fc2 = torch.nn.Linear(2 * 20 + 64, 20), torch.nn.Linear(20, 1)
    assert fd.supported(fc1, fc2, 20, 64)
    assert not fd.supported(torch.nn.Linear(2 * 20 + 36, 20), fc2, 20, 36)
    assert not fd.supported_f32(fc1, fc2, 20, 64)                            # (CPU Parameters: the fp32 class is the GPU's)
    w1p, b1p, w2p, b2, HT = fd.pack_weights(fc1, fc2, 20, 64)
    assert w1p.dtype == torch.bfloat16 and tuple(w1p.shape) == (32, 2 * 32 + 64) and HT == 1
    assert set(fd.calls) >= {"bf16_forward", "f32_forward", "f32_train_forward", "f32_backward"}


# ---------------------------------------------------------------------------------------------------------------------- GPU tier
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU (the product has no CPU fallback)")


DEV = "cuda:0"


def _guarded(t=None, shape=None):
    """(buffer, view): the view holds `t` (or NaN, of `shape`) inside a buffer that is NaN on either side."""
    shape = tuple(t.shape) if t is not None else tuple(shape)
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * PAD,), float("nan"), device=DEV)
    view = buf[PAD:PAD + numel].view(shape)
    if t is not None:
        view.copy_(t)
    return buf, view


def _intact(*bufs):
    return all(bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[-PAD:]).all()) for b in bufs)


_CASES = {}


def _case(D, F, H, n, kind="normal", not_encode=False):
    """The inputs of one call (host float32, made once) and what the float64 reference needs of them: x64 = the concat, a64 and its
    magnitude.  kind: "normal" draws, or "edge": b1 = -W1 . x of row 0 rounded, so every a of row 0 (and of its copies, rows 1, 2)
    lies within a few ulp of 0."""
    key = (D, F, H, n, kind, not_encode)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.RandomState(1000 * D + 10 * F + H + n)
    K = 2 * D + F
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    c = dict(D=D, F=F, H=H, n=n, K=K, not_encode=not_encode, src=f32(n, D), dst=f32(n, D), feat=np.abs(f32(n, F)) * 1.5,
             w1=f32(H, K) / np.float32(np.sqrt(K)), b1=0.1 * f32(H), w2=0.3 * f32(H), b2=f32(1), g=f32(n) / n)
    if kind == "edge":
        for a in ("src", "dst", "feat"):
            c[a][1:3] = c[a][0]
    x = np.concatenate([c["src"] * (0 if not_encode else 1), c["dst"] * (0 if not_encode else 1), c["feat"]], axis=1).astype(np.float64)
    if kind == "edge":
        c["b1"] = (-(c["w1"].astype(np.float64) @ x[0])).astype(np.float32)
    w1 = c["w1"].astype(np.float64)
    c["x64"] = x
    c["a64"] = x @ w1.T + c["b1"].astype(np.float64)
    c["amag"] = np.abs(x) @ np.abs(w1).T + np.abs(c["b1"].astype(np.float64))
    _CASES[key] = c
    return c


def _device(c):
    """The case's arrays in guarded device views: (buffers, views)."""
    bufs, v = [], {}
    for name in ("src", "dst", "feat", "w1", "b1", "w2", "b2", "g"):
        t = torch.from_numpy(c[name])
        if t.numel() == 0:
            v[name] = None
            continue
        b, v[name] = _guarded(t.to(DEV))
        bufs.append(b)
    if c["not_encode"]:
        v["src"] = v["dst"] = None
    return bufs, v


def _ptr(t):
    return None if t is None else t.data_ptr()


def _forward(c, v, hidden=True):
    from tpnet_amd import _dense, _lib
    n, H = c["n"], c["H"]
    ob, out = _guarded(shape=(n,))
    hb, hid = _guarded(shape=(n, H)) if hidden else (None, None)
    rc = _lib.load().tpnet_decoder_f32(_ptr(v["src"]), _ptr(v["dst"]), c["D"], _ptr(v["feat"]), c["F"], n, _ptr(v["w1"]), _ptr(v["b1"]),
                                       _ptr(v["w2"]), _ptr(v["b2"]), H, _ptr(out), _ptr(hid), _dense.stream_ptr(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    assert _intact(ob) and (hb is None or _intact(hb))
    return out, hid


def _backward(c, v, parts, want=(True, True, True), max_parts=None):
    """-> dict: rc, the summed partial cut into gw1, gb1, gw2, gb2, the input gradients (None where not asked for or not there), the
    parked relu(a) [n][H], and the raw partial buffer."""
    from tpnet_amd import _dense, _lib
    lib = _lib.load()
    n, D, F, H, K = c["n"], c["D"], c["F"], c["H"], c["K"]
    pf = int(lib.tpnet_decoder_f32_partial_floats(D, F, H))
    wsf = int(lib.tpnet_decoder_f32_bwd_workspace_bytes(n, D, F, H)) // 4
    assert pf == H * K + 2 * H + 1 and wsf > 0
    wb, ws = _guarded(shape=(wsf,))
    room = parts if max_parts is None else max_parts
    pb, part = _guarded(shape=(room, pf))
    outs, bufs = {}, [wb, pb]
    for name, src_name, width, w in (("gsrc", "src", D, want[0]), ("gdst", "dst", D, want[1]), ("gfeat", "feat", F, want[2])):
        outs[name] = None
        if w and v[src_name] is not None:
            b, outs[name] = _guarded(shape=(n, width))
            bufs.append(b)
    rc = lib.tpnet_decoder_f32_bwd(_ptr(v["src"]), _ptr(v["dst"]), D, _ptr(v["feat"]), F, n, _ptr(v["w1"]), _ptr(v["b1"]), _ptr(v["w2"]), H,
                                   _ptr(v["g"]), _ptr(ws), _ptr(outs["gsrc"]), _ptr(outs["gdst"]), _ptr(outs["gfeat"]), _ptr(part), parts,
                                   _dense.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert 1 <= rc <= min(parts, (n + 31) // 32)
    assert _intact(*bufs)
    assert bool(torch.isnan(part[rc:]).all())                               # partials beyond the returned count are not written
    assert not bool(torch.isnan(ws).any())                                  # the whole workspace is the call's, padding included
    tot = part[:rc].double().sum(0).cpu()
    T, HP = (n + 31) // 32, pad32(H)
    hT = ws[:T * HP * 32].view(T, HP, 32).permute(0, 2, 1).reshape(T * 32, HP)
    assert bool((hT[n:] == 0).all()) and bool((hT[:, H:] == 0).all())       # rows >= n and units >= H park selected zeros
    outs.update(rc=rc, gw1=tot[:H * K].view(H, K), gb1=tot[H * K:H * K + H], gw2=tot[H * K + H:H * K + 2 * H], gb2=tot[-1:],
                h=hT[:n, :H].contiguous(), part=part)
    return outs


def _ratio(name, got, want, mag, worst):
    """The largest |got - want| / (4e-5 mag + 1e-6 max|want|) over the entries into worst[name] (a bound of 0 asks for err = 0)."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    err = np.abs(got.reshape(want.shape) - want)
    bound = 4e-5 * mag + 1e-6 * (np.abs(want).max() if want.size else 0.0)
    ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err == 0, 0.0, np.inf))
    worst[name] = max(worst.get(name, 0.0), float(ratio.max()) if ratio.size else 0.0)


def _report(tag, worst):
    print(f"{tag}: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(np.isfinite(x) and x <= 1.0 for x in worst.values()), worst


def _logits64(c, on):
    w2 = c["w2"].astype(np.float64)
    want = (np.where(on, c["a64"], 0.0) * w2).sum(1) + float(c["b2"][0])
    mag = (np.where(on, c["amag"], 0.0) * np.abs(w2)).sum(1) + abs(float(c["b2"][0]))
    return want, mag


def _grads64(c, on):
    """name -> (want, mag) of the seven gradients in float64 with the decisions `on` [n][H]."""
    g, w2, w1, x = c["g"].astype(np.float64), c["w2"].astype(np.float64), c["w1"].astype(np.float64), c["x64"]
    D = c["D"]
    ga = np.where(on, g[:, None] * w2[None, :], 0.0)
    gx, gxm = ga @ w1, np.abs(ga) @ np.abs(w1)
    r = dict(gw1=(ga.T @ x, np.abs(ga).T @ np.abs(x)), gb1=(ga.sum(0), np.abs(ga).sum(0)),
             gw2=((g[:, None] * np.where(on, c["a64"], 0.0)).sum(0), (np.abs(g)[:, None] * np.where(on, c["amag"], 0.0)).sum(0)),
             gb2=(g.sum(keepdims=True), np.abs(g).sum(keepdims=True)),
             gsrc=(gx[:, :D], gxm[:, :D]), gdst=(gx[:, D:2 * D], gxm[:, D:2 * D]), gfeat=(gx[:, 2 * D:], gxm[:, 2 * D:]))
    return r


SHAPES_N = [(4, 0, 1, 1), (4, 0, 1, 33), (0, 16, 33, 31), (0, 16, 33, 129), (20, 36, 64, 33), (20, 36, 64, 200), (172, 64, 172, 129),
            (172, 64, 172, 200), (256, 100, 256, 1), (256, 100, 256, 31)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,F,H,n", SHAPES_N)
def test_forward_against_float64(D, F, H, n):
    """Test 1.  The logits and the hidden layer within the bound, with the decisions this launch took; the launch without `hidden`
    (what the no_grad route and the training forward both are) gives the same bits, and so does a second call."""
    _need_gpu()
    c = _case(D, F, H, n)
    bufs, v = _device(c)
    out, hid = _forward(c, v)
    on = (hid > 0).cpu().numpy()
    far = np.abs(c["a64"]) > 4e-5 * c["amag"]                               # where a is clear of 0 the decision is float64's
    assert ((c["a64"] > 0) == on)[far].all()
    worst = {}
    _ratio("logit", out, *_logits64(c, on), worst)
    _ratio("hidden", hid, np.where(on, c["a64"], 0.0), np.where(on, c["amag"], 0.0), worst)
    _report(f"forward {D, F, H} n={n}", worst)
    out2, _ = _forward(c, v, hidden=False)
    out3, hid3 = _forward(c, v)
    assert torch.equal(out, out2) and torch.equal(out, out3) and torch.equal(hid, hid3) and _intact(*bufs)


@pytest.mark.gpu
def test_module_routes_give_the_bits_of_the_direct_call():
    """Test 1, second half: `fused = "f32"` under no_grad ("f32_forward") and with a gradient recorded ("f32_train_forward") are the
    direct call's launch: equal bits, counted by route."""
    _need_gpu()
    c = _case(20, 36, 64, 33)
    bufs, v = _device(c)
    out, _ = _forward(c, v, hidden=False)
    dec = _module_of(c)
    ids = np.arange(c["n"])
    src, dst = torch.from_numpy(c["src"]).to(DEV), torch.from_numpy(c["dst"]).to(DEV)
    before = dict(fd.calls)
    with torch.no_grad():
        a = dec(ids, ids, src, dst)
    b = dec(ids, ids, src, dst)
    assert a.shape == (c["n"], 1) and not a.requires_grad and b.requires_grad
    assert torch.equal(a[:, 0], out) and torch.equal(b[:, 0], out)
    assert fd.calls["f32_forward"] == before["f32_forward"] + 1 and fd.calls["f32_train_forward"] == before["f32_train_forward"] + 1
    assert fd.calls["f32_backward"] == before["f32_backward"] and fd.calls["bf16_forward"] == before["bf16_forward"]
    b.sum().backward()
    assert fd.calls["f32_backward"] == before["f32_backward"] + 1


def _module_of(c, fused="f32", feat_grad=True):
    """A LinkPredictor_v1 on the GPU with the case's weights and feature."""
    rp = _FeatStub(torch.from_numpy(c["feat"]), feat_grad) if c["F"] else None
    dec = LinkPredictor_v1(c["D"], c["D"], c["H"], 1, rp, c["not_encode"]).to(DEV)
    with torch.no_grad():
        dec.fc1.weight.copy_(torch.from_numpy(c["w1"])); dec.fc1.bias.copy_(torch.from_numpy(c["b1"]))
        dec.fc2.weight.copy_(torch.from_numpy(c["w2"])[None]); dec.fc2.bias.copy_(torch.from_numpy(c["b2"]))
    dec.fused = fused
    return dec


def _integer_decoder(D, F, H, n, seed):
    """(decoder on the CPU, src, dst, g): weights in quarters, biases in halves, inputs in -3..3, output gradients in -2..2."""
    rng = np.random.RandomState(seed)
    rp = _FeatStub(_ints(rng, (n, F), 0, 5)) if F else None
    dec = LinkPredictor_v1(D, D, H, 1, rp, False)
    _quarters_(dec.fc1, rng, -2, 3); _quarters_(dec.fc2, rng, -2, 3)
    return dec, _ints(rng, (n, D)), _ints(rng, (n, D)), _ints(rng, (n, 1), -2, 3)


def _exact_zeros(dec, src, dst):
    with torch.no_grad():
        x = torch.cat([src, dst] + ([dec.random_projections.feat] if dec.random_projections is not None else []), dim=1)
        return int((x @ dec.fc1.weight.t() + dec.fc1.bias == 0).sum())


INTEGER_CASES = [(20, 36, 64, 200, 1), (172, 64, 172, 129, 1), (4, 0, 1, 33, 1), (0, 16, 33, 31, 1)]      # D, F, H, n, seed


@pytest.mark.parametrize("D,F,H,n,seed", INTEGER_CASES)
def test_integer_cases_hold_pre_activations_that_are_exactly_zero(D, F, H, n, seed):
    """The seeds of test 2 are chosen so that some unit sits exactly on the ReLU's corner (checked here without a GPU)."""
    assert _exact_zeros(*_integer_decoder(D, F, H, n, seed)[:3]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("D,F,H,n,seed", INTEGER_CASES)
def test_small_integers_are_exact(D, F, H, n, seed):
    """Test 2.  Weights in quarters, biases in halves, inputs in -3..3, output gradients in -2..2: every product and every partial sum
    is representable, so logits and all gradients are torch.equal to the torch layers and their autograd -- units whose
    pre-activation is exactly 0 included (they exist; their gradient is 0, torch's rule)."""
    _need_gpu()
    ids = np.arange(n)
    dec, src, dst, g = _integer_decoder(D, F, H, n, seed)
    zeros = _exact_zeros(dec, src, dst)
    print(f"integers {D, F, H} n={n}: {zeros} pre-activations are exactly 0")
    assert zeros > 0
    dec = dec.to(DEV)
    rp = dec.random_projections
    src, dst, g = src.to(DEV).requires_grad_(True), dst.to(DEV).requires_grad_(True), g.to(DEV)
    inputs = list(dec.fc1.parameters()) + list(dec.fc2.parameters()) + ([rp.feat] if F else []) + ([src, dst] if D else [])
    ref = dec(ids, ids, src, dst)
    gr = torch.autograd.grad(ref, inputs, g)
    dec.fused = "f32"
    before = dict(fd.calls)
    out = dec(ids, ids, src, dst)
    gf = torch.autograd.grad(out, inputs, g)
    assert fd.calls["f32_train_forward"] == before["f32_train_forward"] + 1 and fd.calls["f32_backward"] == before["f32_backward"] + 1
    assert torch.equal(out, ref)
    for a, b, p in zip(gf, gr, inputs):
        assert a.shape == p.shape and torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("D,F,H,n,parts", [(4, 0, 1, 1, 1), (4, 0, 1, 33, 2), (0, 16, 33, 31, 1), (0, 16, 33, 129, 3), (20, 36, 64, 33, 1),
                                           (20, 36, 64, 200, 2), (172, 64, 172, 129, 1), (172, 64, 172, 200, 3), (256, 100, 256, 1, 1),
                                           (256, 100, 256, 31, 4)])
def test_backward_against_float64(D, F, H, n, parts):
    """Test 3.  The seven gradients within the bound, with the decisions the backward parked; two calls give equal bits."""
    _need_gpu()
    c = _case(D, F, H, n)
    bufs, v = _device(c)
    r = _backward(c, v, parts)
    assert r["rc"] == min(parts, (n + 31) // 32)
    on = (r["h"] > 0).cpu().numpy()
    worst = {}
    for name, (want, mag) in _grads64(c, on).items():
        if want.size:
            assert r[name] is not None, name
            _ratio(name, r[name], want, mag, worst)
        else:
            assert r[name] is None or r[name].numel() == 0
    _report(f"backward {D, F, H} n={n} parts={parts}", worst)
    r2 = _backward(c, v, parts)
    assert torch.equal(r["part"][:r["rc"]], r2["part"][:r["rc"]]) and torch.equal(r["h"], r2["h"])
    for name in ("gsrc", "gdst", "gfeat"):
        assert r[name] is None or torch.equal(r[name], r2[name])
    assert _intact(*bufs)


@pytest.mark.gpu
def test_row_parts_at_six_tiles():
    """Test 3, the parts: n = 161 is 6 row tiles; 1, 2, 4 and 6 parts asked for (4 gives 3 parts of 2 tiles), in a buffer with room
    for two more than asked for, which stay NaN.  Every sum is within the bound of the float64 reference, so the sums are independent of the parts up to the
    bound; the input gradients and the parked layer do not depend on the parts at all."""
    _need_gpu()
    c = _case(20, 36, 64, 161)
    bufs, v = _device(c)
    first, ref = None, None
    for parts, want_rc in ((1, 1), (2, 2), (4, 3), (6, 6)):
        r = _backward(c, v, parts, max_parts=parts + 2)
        assert r["rc"] == want_rc
        if first is None:
            first, ref = r, _grads64(c, (r["h"] > 0).cpu().numpy())
        worst = {}
        for name, (want, mag) in ref.items():
            _ratio(name, r[name], want, mag, worst)
        _report(f"row parts {parts} -> {r['rc']}", worst)
        assert torch.equal(r["h"], first["h"])
        for name in ("gsrc", "gdst", "gfeat"):
            assert torch.equal(r[name], first[name])
    assert _intact(*bufs)


@pytest.mark.gpu
def test_the_decisions_are_the_forwards():
    """Test 4.  The kernels recompute a in the backward.  Rows 0..2 have b1 = -W1 . x rounded, so all their pre-activations are
    rounding noise around 0 (the float64 value is below 4e-5 of its magnitude), where any other instruction sequence would decide
    differently: the backward's parked relu(a) equals the forward's `hidden` bit for bit, over those rows and all the others."""
    _need_gpu()
    for D, F, H, n in ((172, 64, 172, 129), (20, 36, 64, 33)):
        c = _case(D, F, H, n, kind="edge")
        bufs, v = _device(c)
        _, hid = _forward(c, v)
        r = _backward(c, v, 2)
        near = np.abs(c["a64"][:3]) <= 4e-5 * c["amag"][:3]
        assert near.all()
        on = (hid[:3] > 0).cpu().numpy()
        print(f"decisions {D, F, H}: {int(on.sum())} of {on.size} near-zero units are on, largest |a| there {float(hid[:3].abs().max()):.3e}")
        assert 0 < on.sum() < on.size                                       # (noise: both signs occur)
        assert torch.equal(hid.view(torch.int32), r["h"].view(torch.int32))
        assert _intact(*bufs)


@pytest.mark.gpu
def test_not_encode():
    """Test 5.  The embeddings count as zeros and are never read (they hold NaN here): logits equal the unfused module's, src.grad and
    dst.grad stay None, fc1.weight.grad[:, :2 D] is exactly 0, the rest equals autograd of the torch layers (integer data)."""
    _need_gpu()
    rng = np.random.RandomState(17)
    n, D, F, H = 70, 20, 36, 40
    ids = np.arange(n)
    rp = _FeatStub(_ints(rng, (n, F), 0, 5)).to(DEV)
    dec = LinkPredictor_v1(D, D, H, 1, rp, True).to(DEV)
    _quarters_(dec.fc1, rng, -2, 3); _quarters_(dec.fc2, rng, -2, 3)
    twin = copy.deepcopy(dec)
    dec.fused = "f32"
    g = _ints(rng, (n, 1), -2, 3).to(DEV)
    src = torch.full((n, D), float("nan"), device=DEV, requires_grad=True)
    dst = torch.full((n, D), float("nan"), device=DEV, requires_grad=True)
    before = dict(fd.calls)
    out = dec(ids, ids, src, dst)
    ref = twin(ids, ids, src, dst)
    assert fd.calls["f32_train_forward"] == before["f32_train_forward"] + 1
    assert torch.equal(out, ref)
    out.backward(g)
    ref.backward(g)
    assert src.grad is None and dst.grad is None
    assert bool((dec.fc1.weight.grad[:, :2 * D] == 0).all())
    for a, b in zip(list(dec.parameters()), list(twin.parameters())):
        assert torch.equal(a.grad, b.grad)
    # the direct call: gw1's embedding columns are zeros in every partial, and a gradient for the embeddings is refused
    c = _case(20, 36, 64, 33, not_encode=True)
    bufs, v = _device(c)
    r = _backward(c, v, 2)
    assert bool((r["part"][:r["rc"], :64 * 76].view(-1, 64, 76)[:, :, :40] == 0).all()) and r["gsrc"] is None and r["gdst"] is None
    worst = {}
    for name, (want, mag) in _grads64(c, (r["h"] > 0).cpu().numpy()).items():
        if name not in ("gsrc", "gdst"):
            _ratio(name, r[name], want, mag, worst)
    _report("not_encode, direct", worst)


@pytest.mark.gpu
def test_other_calling_modes():
    """Test 6.  A decoder without a pair feature; a feature that takes no gradient (its product columns are skipped: the call gets
    no gfeat array); embeddings that take none either (no product at all).  Integer data: everything asked for is torch.equal to the
    torch layers' autograd."""
    _need_gpu()
    rng = np.random.RandomState(23)
    n, D, H = 45, 12, 33
    ids = np.arange(n)
    g = _ints(rng, (n, 1), -2, 3).to(DEV)
    for F, feat_grad, emb_grad in ((0, False, True), (16, False, True), (16, False, False), (16, True, False)):
        rp = _FeatStub(_ints(rng, (n, F), 0, 5), feat_grad).to(DEV) if F else None
        dec = LinkPredictor_v1(D, D, H, 1, rp, False).to(DEV)
        _quarters_(dec.fc1, rng, -2, 3); _quarters_(dec.fc2, rng, -2, 3)
        src = _ints(rng, (n, D)).to(DEV).requires_grad_(emb_grad)
        dst = _ints(rng, (n, D)).to(DEV).requires_grad_(emb_grad)
        inputs = list(dec.fc1.parameters()) + list(dec.fc2.parameters()) + ([rp.feat] if feat_grad else []) + ([src, dst] if emb_grad else [])
        gr = torch.autograd.grad(dec(ids, ids, src, dst), inputs, g)
        dec.fused = "f32"
        before = dict(fd.calls)
        out = dec(ids, ids, src, dst)
        gf = torch.autograd.grad(out, inputs, g)
        assert fd.calls["f32_train_forward"] == before["f32_train_forward"] + 1 and fd.calls["f32_backward"] == before["f32_backward"] + 1
        for a, b in zip(gf, gr):
            assert torch.equal(a, b)
        # frozen Parameters: only the inputs' gradients are asked for
        if emb_grad:
            for p in dec.parameters():
                p.requires_grad_(False)
            a, = torch.autograd.grad(dec(ids, ids, src, dst), [src], g)
            assert torch.equal(a, gr[-2])
    # a shape the kernels do not serve (F = 6) and another dtype keep the torch layers: same outputs as fused = False, no launch counted
    rp = _FeatStub(_ints(rng, (n, 6), 0, 5)).to(DEV)
    dec = LinkPredictor_v1(D, D, H, 1, rp, False).to(DEV)
    src, dst = _ints(rng, (n, D)).to(DEV), _ints(rng, (n, D)).to(DEV)
    ref = dec(ids, ids, src, dst)
    dec.fused = "f32"
    before = dict(fd.calls)
    assert torch.equal(dec(ids, ids, src, dst), ref)
    dec64 = LinkPredictor_v1(D, D, H, 1, None, False).to(DEV).double()
    ref64 = dec64(ids, ids, src.double(), dst.double())
    dec64.fused = "f32"
    assert torch.equal(dec64(ids, ids, src.double(), dst.double()), ref64)
    nc = torch.zeros(n, 2 * D, device=DEV)[:, ::2]                          # not contiguous
    dec2 = LinkPredictor_v1(D, D, H, 1, None, False).to(DEV)
    ref2 = dec2(ids, ids, nc, dst)
    dec2.fused = "f32"
    assert torch.equal(dec2(ids, ids, nc, dst), ref2)
    assert fd.calls == before


@pytest.mark.gpu
def test_skipped_sources_may_hold_nan():
    """Test 6, the NaN: with gsrc / gdst / gfeat not asked for, and in not_encode, what is skipped is never multiplied -- a NaN in a
    row >= n cannot exist (there is no such row), so the NaN sits where the code does not look: the embeddings of a not_encode
    call, and the guards around every array.  No output and no partial holds a NaN."""
    _need_gpu()
    c = _case(20, 36, 64, 33, not_encode=True)
    bufs, v = _device(c)
    out, hid = _forward(c, v)
    r = _backward(c, v, 1, want=(False, False, True))
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(hid).any())
    assert not bool(torch.isnan(r["part"][:r["rc"]]).any()) and not bool(torch.isnan(r["gfeat"]).any())
    c = _case(20, 36, 64, 33)
    bufs, v = _device(c)
    r = _backward(c, v, 1, want=(False, False, False))
    assert r["gsrc"] is None and r["gdst"] is None and r["gfeat"] is None and not bool(torch.isnan(r["part"][:1]).any())
    full = _backward(c, v, 1)
    assert torch.equal(r["part"][:1], full["part"][:1])                     # the weight gradients do not depend on what else is asked for
    some = _backward(c, v, 1, want=(False, True, False))
    assert some["gsrc"] is None and some["gfeat"] is None and torch.equal(some["gdst"], full["gdst"])


@pytest.mark.gpu
def test_module_on_fixture_g7(golden_dir):
    """Test 7.  D = 20, F = 64, H = 20, 12 pairs, a real RandomProjectionModule: the "f32" logits against fused = False of the same
    module within the bound (mag from the module's own feature and weights in float64), through the f32 route, twice with equal bits."""
    _need_gpu()
    from tpnet_amd import RandomProjectionModule
    g = np.load(os.path.join(golden_dir, "g7_decoder.npz"))
    L, N, d = int(g["L"]), int(g["N"]), int(g["d"])
    now = float(g["now_time"])
    rp = RandomProjectionModule(node_num=N, edge_num=100, dim_factor=10, num_layer=L, time_decay_weight=float(g["lam"]),
                                device=DEV, use_matrix=False, beginning_time=np.float64(now), not_scale=False, enforce_dim=d)
    rp.random_projections[0].data = torch.from_numpy(g["P"][0])
    dec = LinkPredictor_v1(input_dim1=20, input_dim2=20, hidden_dim=20, output_dim=1, random_projections=rp, not_encode=False).to(DEV)
    dec.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("dec.")})
    rp.reload_random_projections((torch.tensor(now, dtype=torch.float64, device=DEV),
                                  [torch.from_numpy(g["P"][i]).to(DEV) for i in range(1, L + 1)]))
    src, dst = torch.from_numpy(g["src_emb"]).to(DEV), torch.from_numpy(g["dst_emb"]).to(DEV)
    call = lambda: dec(src_node_ids=g["u"], dst_node_ids=g["v"], src_node_embeddings=src, dst_node_embeddings=dst)
    with torch.no_grad():
        ref = call()
        feat = rp.get_pair_wise_feature(src_node_ids=g["u"], dst_node_ids=g["v"])
        assert feat.shape == (12, 64)
        dec.fused = "f32"
        before = dict(fd.calls)
        out, again = call(), call()
    assert fd.calls["f32_forward"] == before["f32_forward"] + 2 and fd.calls["bf16_forward"] == before["bf16_forward"]
    assert torch.equal(out, again) and out.shape == ref.shape == (12, 1)
    np.testing.assert_allclose(out.cpu().numpy(), g["logits"], rtol=1e-4, atol=1e-5)     # (and the reference's own logits)
    x = torch.cat([src, dst, feat], dim=1).double().cpu().numpy()
    w1, b1 = dec.fc1.weight.detach().double().cpu().numpy(), dec.fc1.bias.detach().double().cpu().numpy()
    w2, b2 = dec.fc2.weight.detach().double().cpu().numpy()[0], float(dec.fc2.bias.detach()[0])
    a, amag = x @ w1.T + b1, np.abs(x) @ np.abs(w1).T + np.abs(b1)
    mag = (np.where(a > 0, amag, 0.0) * np.abs(w2)).sum(1) + abs(b2)
    worst = {}
    _ratio("logit", out[:, 0], ref[:, 0].double().cpu().numpy(), mag, worst)
    _report("G7", worst)


class _Encoder(torch.nn.Module):
    def __init__(self, width, dim):
        super().__init__()
        self.lin = torch.nn.Linear(width, dim)

    def forward(self, features, node_ids, times):                          # [2B, K, 2F] -> [2B, D]
        return self.lin(features.mean(dim=1))


class _Snapshot:
    """An optimizer that never moves a Parameter and keeps the gradients it is handed at its first step."""

    def __init__(self, params):
        self.params, self.first = list(params), None

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self):
        if self.first is None:
            self.first = [None if p.grad is None else p.grad.detach().clone() for p in self.params]


@pytest.mark.gpu
def test_one_training_step_of_the_epoch_loop(golden_dir):
    """Test 8.  callers.train_link_prediction_epoch on the toy stream, 87 edges in batches of 50 (the tail has 37), the decoder on
    "f32" against a deep copy on False with its own module (same mlp), encoder and negatives.  The gradients the optimizer is handed
    at its FIRST step (after the first batch's backward; later ones are not compared) agree per Parameter -- fc1, fc2, the encoder's
    and rp.mlp's -- within 4e-5 mag + 1e-6 max|want| with mag = max|want| of that Parameter's gradient, its own magnitude: the two
    logits differ by <= 4e-5 of their magnitude, the loss's derivative has slope <= 1/4 in a logit, and every gradient is linear in
    the logits' gradients and in the decoder's own products, each fp32 class, so entries move by a few 1e-5 of the tensor's scale."""
    _need_gpu()
    import tpnet_amd
    from tpnet_amd.callers import RandomNegativeSampler, train_link_prediction_epoch
    from test_negative_sampler import _module, g13
    g = g13(golden_dir)
    src, dst, t = g["src"][:87], g["dst"][:87], g["t"][:87]
    nbr = tpnet_amd.GpuRecentNeighborSampler(g["src"], g["dst"], g["t"], device=DEV, num_nodes=41)
    rp, twin = _module(41), _module(41)
    twin.mlp.load_state_dict(rp.mlp.state_dict())
    torch.manual_seed(3)
    enc = _Encoder(2 * rp.pair_wise_feature_dim, 16).to(DEV)
    dec = LinkPredictor_v1(16, 16, 24, 1, rp, False).to(DEV)
    enc2 = copy.deepcopy(enc)
    dec2 = LinkPredictor_v1(16, 16, 24, 1, twin, False).to(DEV)
    dec2.fc1.load_state_dict(dec.fc1.state_dict()); dec2.fc2.load_state_dict(dec.fc2.state_dict())
    dec.fused = "f32"
    assert dec2.fused is False
    grads = []
    before = dict(fd.calls)
    for r_, e_, d_ in ((rp, enc, dec), (twin, enc2, dec2)):
        params = list(e_.parameters()) + list(d_.fc1.parameters()) + list(d_.fc2.parameters()) + list(r_.mlp.parameters())
        opt = _Snapshot(params)
        torch.manual_seed(77)                                              # (the reset draws P[0] from torch's generator)
        losses, _ = train_link_prediction_epoch(r_, nbr, RandomNegativeSampler(src, dst, seed=3), src, dst, t, 50, 4, e_, d_, opt)
        assert len(losses) == 2 and all(np.isfinite(losses))
        grads.append(opt.first)
    assert fd.calls["f32_train_forward"] == before["f32_train_forward"] + 4 and fd.calls["f32_backward"] == before["f32_backward"] + 4
    assert torch.equal(rp.random_projections[0].detach(), twin.random_projections[0].detach())
    worst = {}
    for i, (a, b) in enumerate(zip(*grads)):
        assert a is not None and b is not None and float(b.abs().max()) > 0
        want = b.double().cpu().numpy()
        _ratio(f"p{i}{tuple(b.shape)}", a, want, np.full(want.shape, np.abs(want).max()), worst)
    _report("training step", worst)
