"""tpnet_mlp_l4_* (csrc/mlp_l4.hip): self.mlp = Linear(100, 400) -> ReLU -> Linear(400, 100) of num_layer 4 on the matrix cores in the
project's fp32 class, forward (with and without the recorded ReLU decisions) and backward -- the kernels through the C entries, then
through fused_feature.mlp_l4 and RandomProjectionModule.mlp_l4.

Bounds: bit equality on small integers (every product and partial sum is exact in two bf16 pieces and an fp32 accumulator); against
float64 evaluations |err| <= 4e-5 mag + 1e-6 max|want| per entry, mag the sum of the absolute values of the entry's terms (the
project's constant for a chain of two fp32-class products: tests/test_encoder_input_training.py).  The recorded decisions equal
a64 > 0 outside the band |a64| <= 2e-5 (|W1||x| + |b1|), which may hold at most 1 % of the units.

Every buffer of a direct call is a view into a larger one whose remainder is NaN (inputs) or a sentinel (outputs).  A row of x that
holds a NaN: nothing is asserted about THAT row (include/tpnet_hip.h), only that every other row keeps its bits."""
import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, _module, _need_gpu, _random_stream

pytestmark = pytest.mark.gpu

F, H, NW = 100, 400, 13
# one row; either side of a 32-row tile and of a 128-row workgroup; 4 099 rows = 129 tiles: more than 32 row parts, a one-row last tile
N = (1, 31, 32, 33, 127, 128, 129, 1000, 4099)
N_BWD = (1, 33, 129, 1000, 4099)
PAD = 64                                         # floats on either side of a view (keeps 16-byte alignment)
SENTINEL = 0x5A5A5A5A


def _layers(seed=None, dev=DEV):
    if seed is not None:
        torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(F, H), torch.nn.ReLU(), torch.nn.Linear(H, F)).to(dev)


def _int_layers():
    g = torch.Generator().manual_seed(F)
    mlp = _layers()
    with torch.no_grad():
        mlp[0].weight.copy_(torch.randint(-3, 4, (H, F), generator=g).float())
        mlp[0].bias.copy_(torch.randint(-8, 9, (H,), generator=g).float())
        mlp[2].weight.copy_((torch.randint(-3, 4, (F, H), generator=g) * (torch.rand(F, H, generator=g) < 0.5)).float())
        mlp[2].bias.copy_(torch.randint(-8, 9, (F,), generator=g).float())
    return mlp, g


def _features(n, seed):
    """test_mlp_rows.py's recipe: log1p of values in [0, e^20) with 10 % exact zeros."""
    g = torch.Generator().manual_seed(seed)
    v = torch.expm1(torch.rand(n, F, generator=g, dtype=torch.float64) * 20.0) * (torch.rand(n, F, generator=g) < 0.9)
    return torch.log1p(v).float()


def _guarded(t=None, shape=None):
    """(buffer, view): the view holds `t` (or NaN, of `shape`) inside a buffer that is NaN on either side."""
    shape = tuple(t.shape) if t is not None else tuple(shape)
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * PAD,), float("nan"), device=DEV)
    view = buf[PAD:PAD + numel].view(shape)
    if t is not None:
        view.copy_(t)
    return buf, view


def _guards_intact(buf):
    if buf.dtype == torch.int32:
        return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[-PAD:]).all())


def _images(mlp, backward=False):
    from tpnet_amd import fused_feature as ff
    rec = ff.l4_images(mlp, backward=backward)
    assert rec is not None and (rec.bimg is not None or not backward)
    return rec


def _fwd(mlp, x, bits=True, finite=True):
    """tpnet_mlp_l4_f32 itself on a guarded copy of x into guarded outputs: (y [n, 100], relu_bits [n, 13] int32 or None)."""
    from tpnet_amd import _dense, _lib
    n = x.shape[0]
    rec = _images(mlp)
    xbuf, xv = _guarded(x.to(DEV))
    ybuf, y = _guarded(shape=(n, F))
    bbuf = torch.full((n * NW + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    bv = bbuf[PAD:PAD + n * NW].view(n, NW)
    rc = _lib.load().tpnet_mlp_l4_f32(xv.data_ptr(), n, rec.img.data_ptr(), y.data_ptr(), bv.data_ptr() if bits else None,
                                      _dense.stream_ptr(y.device))
    assert rc == 0 and _guards_intact(ybuf) and _guards_intact(bbuf) and _guards_intact(xbuf)
    assert not finite or bool(torch.isfinite(y).all())
    if not bits:
        assert bool((bv == SENTINEL).all())
    return y, (bv if bits else None)


def _unpack(bits):
    """relu_bits [n, 13] int32 -> bool [n, 400] on the host, and the check that the bits of the padded units 400..415 are 0."""
    b = bits.cpu().numpy().view(np.uint32)
    full = ((b[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(b.shape[0], -1).astype(bool)
    assert full.shape[1] == 32 * NW and not full[:, H:].any()
    return torch.from_numpy(full[:, :H].copy())


def _p64(mlp):
    return tuple(t.detach().double().cpu() for t in (mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias))


def _fwd64(mlp, x):
    """float64 on the host: (y64, its bound per entry, a64, am = |W1||x| + |b1|)."""
    w1, b1, w2, b2 = _p64(mlp)
    x = x.detach().double().cpu()
    a, am = x @ w1.t() + b1, x.abs() @ w1.abs().t() + b1.abs()
    y = torch.relu(a) @ w2.t() + b2
    mag = am @ w2.abs().t() + b2.abs()
    return y, 4e-5 * mag + 1e-6 * float(y.abs().max()), a, am


def _bwd64(mlp, x, gy, m):
    """The kernel file's expressions in float64 on the host with the decisions m [n, 400] (bool): (gw1, gb1, gw2, gb2) and for each the
    sum of the absolute values of its terms."""
    w1, b1, w2, _ = _p64(mlp)
    x, g, m = x.detach().double().cpu(), gy.detach().double().cpu(), m.double()
    a, am = x @ w1.t() + b1, x.abs() @ w1.abs().t() + b1.abs()
    h, hm = a * m, am * m
    ga, gam = (g @ w2) * m, (g.abs() @ w2.abs()) * m
    return ((ga.t() @ x, ga.sum(0), g.t() @ h, g.sum(0)), (gam.t() @ x.abs(), gam.sum(0), g.abs().t() @ hm, g.abs().sum(0)))


NAMES = ("gw1", "gb1", "gw2", "gb2")


def _check(tag, got, ref, keep=None):
    """|err| <= 4e-5 mag + 1e-6 max|want| per entry of the four gradients; prints the largest err / bound per tensor.  keep[name]: a
    bool mask of the entries to compare (all without one)."""
    want, mags = ref
    worst = {}
    for name, gt, wt, mg in zip(NAMES, got, want, mags):
        err = (gt.detach().double().cpu() - wt).abs()
        bound = 4e-5 * mg + 1e-6 * float(wt.abs().max())
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
        if keep is not None and name in keep:
            ratio = ratio[keep[name]]
        worst[name] = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{tag}: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(np.isfinite(v) and v <= 1.0 for v in worst.values()), worst


def _bwd(mlp, x, bits, gy, n_partial):
    """tpnet_mlp_l4_bwd_f32 itself on guarded copies of x, gy and bits: (rc, the four summed gradients);
    partial buffer and workspace prefilled with NaN, the partials beyond rc and all guards still NaN behind the call."""
    from tpnet_amd import _dense, _lib
    lib = _lib.load()
    rec = _images(mlp, backward=True)
    n = x.shape[0]
    pf = int(lib.tpnet_mlp_l4_bwd_partial_floats())
    xbuf, xv = _guarded(x.to(DEV))
    gbuf, gv = _guarded(gy.to(DEV))
    bbuf = torch.full((n * NW + 2 * PAD,), -1, dtype=torch.int32, device=DEV)      # (all ones: a NaN's pattern, every decision on)
    bits = bbuf[PAD:PAD + n * NW].view(n, NW).copy_(bits)
    pbuf, part = _guarded(shape=(n_partial, pf))
    wbuf, ws = _guarded(shape=(int(lib.tpnet_mlp_l4_bwd_workspace_bytes(n)) // 4,))
    rc = lib.tpnet_mlp_l4_bwd_f32(xv.data_ptr(), bits.data_ptr(), gv.data_ptr(), n, rec.bimg.data_ptr(), ws.data_ptr(), part.data_ptr(),
                                  n_partial, _dense.stream_ptr(part.device))
    tiles = (n + 31) // 32
    per_part = (tiles + n_partial - 1) // n_partial
    assert 1 <= rc <= n_partial and rc == (tiles + per_part - 1) // per_part           # equal parts, none empty
    assert _guards_intact(pbuf) and _guards_intact(wbuf) and _guards_intact(xbuf) and _guards_intact(gbuf)
    assert bool(torch.isnan(part[rc:]).all()) and bool(torch.isfinite(part[:rc]).all())
    tot = part[:rc].sum(0)
    return rc, [tot[:H * F].view(H, F), tot[H * F:H * F + H], tot[H * F + H:2 * H * F + H].view(F, H), tot[2 * H * F + H:]]


_CASES = {}


def _case(n):
    """Default-initialised layers (shared), the features of n rows, gy, the train forward's (y, bits) and the float64 forward,
    computed once per n and shared."""
    if "mlp" not in _CASES:
        _CASES["mlp"] = _layers(seed=F)
    if n not in _CASES:
        mlp = _CASES["mlp"]
        x = _features(n, 100 + n)
        gy = torch.randn(n, F, generator=torch.Generator().manual_seed(700 + n))
        y, bits = _fwd(mlp, x)
        _CASES[n] = dict(mlp=mlp, x=x, gy=gy, y=y, bits=bits, m=_unpack(bits), ref=_fwd64(mlp, x))
    return _CASES[n]


# ---------------------------------------------------------------------------------------------------------------- the C entries

def test_forward_exact_on_small_integers():
    """Weights in [-3, 3] (W2 half zeros), biases in [-8, 8], x in {0..3}: |hidden| <= 908 and |out| < 2^21, every product and sum is
    exact -- y equals the torch layers bit for bit and relu_bits equals a > 0 at every n, with and without the bits."""
    _need_gpu()
    mlp, g = _int_layers()
    for n in N:
        x = torch.randint(0, 4, (n, F), generator=g).float()
        with torch.no_grad():
            a = torch.addmm(mlp[0].bias, x.to(DEV), mlp[0].weight.t())
            want = mlp(x.to(DEV))
        assert float(a.abs().max()) <= 908 and float(want.abs().max()) < 2 ** 21
        y, bits = _fwd(mlp, x)
        assert torch.equal(y, want), f"n={n}: max |delta| {(y - want).abs().max().item()}"
        assert torch.equal(_unpack(bits), (a > 0).cpu()), n
        plain, _ = _fwd(mlp, x, bits=False)
        assert torch.equal(plain, want), n


@pytest.mark.parametrize("n", N)
def test_forward_fp32_class_bits_and_decisions(n):
    """nn.Linear's default init on the readout's kind of features against float64: y within the bound per entry; a second launch and
    the launch without relu_bits give equal bits; the decisions equal a64 > 0 outside the band, which holds at most 1 % of the units."""
    _need_gpu()
    c = _case(n)
    mlp, x = c["mlp"], c["x"]
    y64, bound, a, am = c["ref"]
    err = (c["y"].double().cpu() - y64).abs()
    print(f"n={n}: largest err / bound against float64 {float((err / bound).max()):.3f}")
    with torch.no_grad():
        t = mlp(x.to(DEV))
    d, scale = float((c["y"] - t).abs().max()), max(1.0, float(t.abs().max()))
    print(f"n={n}: against the torch layers max |delta| {d:.3e} = {d / scale:.3e} of the scale {scale:.3f}")
    assert bool((err <= bound).all())
    y2, bits2 = _fwd(mlp, x)
    assert torch.equal(y2, c["y"]) and torch.equal(bits2, c["bits"])
    plain, _ = _fwd(mlp, x, bits=False)
    assert torch.equal(plain, c["y"])
    band = a.abs() <= 2e-5 * am
    share = float(band.double().mean())
    print(f"n={n}: {int(band.sum())} of {band.numel()} units inside the band ({share:.2e})")
    assert share <= 0.01
    assert torch.equal(c["m"][~band], (a > 0)[~band])


@pytest.mark.parametrize("n", [33, 1000])
def test_a_nan_row_stays_in_its_row(n):
    """(Nothing written past row n, NaN behind x: _fwd's guards, in every test.)  A NaN row, interior or last, leaves every other
    row's y and relu_bits unchanged."""
    _need_gpu()
    c = _case(n)
    for bad in (n // 2, n - 1):
        x = c["x"].clone()
        x[bad] = float("nan")
        y, bits = _fwd(c["mlp"], x, finite=False)
        keep = torch.ones(n, dtype=torch.bool, device=DEV)
        keep[bad] = False
        assert torch.equal(y[keep], c["y"][keep]) and torch.equal(bits[keep], c["bits"][keep]), bad


def test_rows_are_independent():
    """The first 1 / 33 / 129 rows of a 300-row call give the shorter calls' bits."""
    _need_gpu()
    mlp = _case(1)["mlp"]
    x = _features(300, 300)
    y, bits = _fwd(mlp, x)
    for m in (1, 33, 129):
        ys, bs = _fwd(mlp, x[:m])
        assert torch.equal(ys, y[:m]) and torch.equal(bs, bits[:m]), m


@pytest.mark.parametrize("n_partial", [1, 3, 32])
@pytest.mark.parametrize("n", N_BWD)
def test_backward_against_float64(n, n_partial):
    """The four partial-summed gradients against the float64 evaluation with the exported bits: |err| <= 4e-5 mag + 1e-6 max|want|.
    A second call gives equal bits.  Guards, the sentinel of the partials beyond the returned count: _bwd."""
    _need_gpu()
    c = _case(n)
    rc, got = _bwd(c["mlp"], c["x"], c["bits"], c["gy"], n_partial)
    _check(f"n={n} in {rc} parts", got, _bwd64(c["mlp"], c["x"], c["gy"], c["m"]))
    rc2, again = _bwd(c["mlp"], c["x"], c["bits"], c["gy"], n_partial)
    assert rc2 == rc and all(torch.equal(a, b) for a, b in zip(again, got))


@pytest.mark.parametrize("n", [1, 33, 129, 1000])
def test_backward_exact_on_small_integers(n):
    """Small-integer weights, x and gy in {-2..2}, n <= 1 000: every sum is below 2^24 and every gradient has the bits of torch
    autograd through the torch layers."""
    _need_gpu()
    mlp, g = _int_layers()
    x = torch.randint(0, 4, (n, F), generator=g).float()
    gy = torch.randint(-2, 3, (n, F), generator=g).float()
    params = [mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias]
    want = torch.autograd.grad(mlp(x.to(DEV)), params, gy.to(DEV))
    y, bits = _fwd(mlp, x)
    _, mags = _bwd64(mlp, x, gy, _unpack(bits))
    assert all(float(mg.max()) < 2 ** 24 for mg in mags)
    rc, got = _bwd(mlp, x, bits, gy, 3)
    for nm, gt, wt in zip(NAMES, got, want):
        assert torch.equal(gt, wt), (nm, float((gt - wt).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- the module

def _updated_module(L, d=64, N_=300):
    rp = _module(N_, d, L, 2e-6, 1.0e6)
    src, dst, _, t = _random_stream(np.random.RandomState(10 * L + d), N_, 600, 3.0e5)
    for a in range(0, 600, 200):                                         # three updates of 200 edges
        rp.update(src[a:a + 200], dst[a:a + 200], t[a:a + 200])
    return rp


def _pairs(n=9000, seed=4):
    rng = np.random.RandomState(seed)
    return torch.from_numpy(rng.randint(0, 300, n)).to(DEV), torch.from_numpy(rng.randint(0, 300, n)).to(DEV)


def _within_forward_bound(mlp, feats, got):
    y64, bound, _, _ = _fwd64(mlp, feats)
    err = (got.detach().double().cpu() - y64).abs()
    print(f"module: largest err / bound against float64 {float((err / bound).max()):.3f}")
    return bool((err <= bound).all())


def test_default_switch_keeps_the_torch_route():
    _need_gpu()
    from tpnet_amd import fused_feature as ff
    rp = _updated_module(4)
    assert rp.mlp_l4 is False
    u, v = _pairs()
    before = dict(ff.calls)
    with torch.no_grad():
        feats = rp.pair_gram(u, v)
        assert feats.shape == (9000, F)
        assert torch.equal(rp._apply_mlp(feats), rp.mlp(feats))
        assert torch.equal(rp.get_pair_wise_feature(u, v), rp.mlp(feats))
    assert ff.calls == before
    rp.check_device_errors()


def test_switch_routes_the_forward(monkeypatch):
    """rp.mlp_l4 with MLP_L4_FROM = 1 000: one launch per call, within the forward's bound of the float64 layers -- _apply_mlp,
    get_pair_wise_feature from device ids and from host arrays, get_pair_wise_feature_anchored."""
    _need_gpu()
    from tpnet_amd import fused_feature as ff
    rp = _updated_module(4)
    rp.mlp_l4 = True
    monkeypatch.setattr(ff, "MLP_L4_FROM", 1000)
    u, v = _pairs()
    with torch.no_grad():
        feats = rp.pair_gram(u, v)
        for call in (lambda: rp._apply_mlp(feats), lambda: rp.get_pair_wise_feature(u, v),
                     lambda: rp.get_pair_wise_feature(u.cpu().numpy(), v.cpu().numpy())):
            before = dict(ff.calls)
            got = call()
            assert ff.calls["l4"] == before["l4"] + 1 and ff.calls["l4_bwd"] == before["l4_bwd"]
            assert _within_forward_bound(rp.mlp, feats, got)
        rng = np.random.RandomState(9)
        neigh = torch.from_numpy(rng.randint(0, 300, (60, 20))).to(DEV)
        a1, a2 = torch.from_numpy(rng.randint(1, 300, 60)).to(DEV), torch.from_numpy(rng.randint(1, 300, 60)).to(DEV)
        before = dict(ff.calls)
        got = rp.get_pair_wise_feature_anchored(neigh, a1, a2)
        assert ff.calls["l4"] == before["l4"] + 1 and got.shape == (2400, F)
        pre = rp.pair_gram(neigh.reshape(-1).repeat(2), torch.cat([a1.repeat_interleave(20), a2.repeat_interleave(20)]))
        assert _within_forward_bound(rp.mlp, pre, got)
    rp.check_device_errors()


def test_autograd_through_the_module_and_an_optimizer_step(monkeypatch):
    """Under autograd the gradients of the four Parameters against float64 through the layers (ReLU deciding on a64 > 0), within the
    backward's bound for every unit outside the band: rows of gw1 / gb1 and columns of gw2 of a unit with a row inside the band are
    not compared.  Two backward launches.  After an Adam step the images are rebuilt once and the next call runs on the new weights."""
    _need_gpu()
    from tpnet_amd import fused_feature as ff
    rp = _updated_module(4)
    rp.mlp_l4 = True
    monkeypatch.setattr(ff, "MLP_L4_FROM", 1000)
    monkeypatch.setattr(ff, "MLP_L4_BWD_FROM", 1000)
    u, v = _pairs()
    params = list(rp.mlp.parameters())
    gy = torch.randn(9000, F, generator=torch.Generator().manual_seed(4)).to(DEV)
    opt = torch.optim.Adam(params, lr=1e-2)
    with torch.no_grad():
        feats = rp.pair_gram(u, v)
    before = dict(ff.calls)
    out = rp.get_pair_wise_feature(u, v)
    assert out.requires_grad and ff.calls["l4"] == before["l4"] + 1 and ff.calls["l4_prepare"] == before["l4_prepare"] + 1
    assert _within_forward_bound(rp.mlp, feats, out)
    out.backward(gy)
    assert ff.calls["l4_bwd"] == before["l4_bwd"] + 2 and ff.calls["l4_prepare"] == before["l4_prepare"] + 1
    _, _, a, am = _fwd64(rp.mlp, feats)
    band = a.abs() <= 2e-5 * am
    clean = ~band.any(0)
    print(f"{int(band.sum())} units inside the band, {int(clean.sum())} of {H} hidden units compared")
    keep = {"gw1": clean[:, None].expand(H, F), "gb1": clean, "gw2": clean[None, :].expand(F, H)}
    _check("autograd through the module", [p.grad for p in params], _bwd64(rp.mlp, feats, gy, a > 0), keep)
    # an optimizer step: both images rebuilt once, the next call on the new weights
    opt.step()
    rp.mlp.zero_grad(set_to_none=True)
    after = rp.get_pair_wise_feature(u, v)
    assert ff.calls["l4_prepare"] == before["l4_prepare"] + 2 and not torch.equal(after, out)
    assert _within_forward_bound(rp.mlp, feats, after)
    after.backward(gy)
    assert ff.calls["l4_prepare"] == before["l4_prepare"] + 2 and ff.calls["l4_bwd"] == before["l4_bwd"] + 4
    _, _, a, am = _fwd64(rp.mlp, feats)
    clean = ~(a.abs() <= 2e-5 * am).any(0)
    keep = {"gw1": clean[:, None].expand(H, F), "gb1": clean, "gw2": clean[None, :].expand(F, H)}
    _check("after an Adam step", [p.grad for p in params], _bwd64(rp.mlp, feats, gy, a > 0), keep)
    with torch.no_grad():
        rp.get_pair_wise_feature(u, v)
    assert ff.calls["l4_prepare"] == before["l4_prepare"] + 2
    ff.invalidate(rp.mlp)
    assert ff._L4.get(rp.mlp) is None
    rp.check_device_errors()


def test_calls_that_keep_the_torch_route(monkeypatch):
    """mlp_backward = "torch", an x that requires a gradient, a list below the threshold, a CPU module and L = 3: no launch."""
    _need_gpu()
    from tpnet_amd import fused_feature as ff
    monkeypatch.setattr(ff, "MLP_L4_FROM", 1000)
    monkeypatch.setattr(ff, "MLP_L4_BWD_FROM", 1000)
    rp = _updated_module(4)
    rp.mlp_l4 = True
    u, v = _pairs()
    with torch.no_grad():
        feats = rp.pair_gram(u, v)
        want = rp.mlp(feats)
    before = dict(ff.calls)
    params = list(rp.mlp.parameters())
    gy = torch.randn(9000, F, generator=torch.Generator().manual_seed(5)).to(DEV)
    want_g = torch.autograd.grad(rp.mlp(feats), params, gy)
    # the torch backward asked for: the torch layers, forward and backward, bit for bit
    rp.mlp.mlp_backward = "torch"
    y = rp._apply_mlp(feats)
    assert torch.equal(y, want) and all(torch.equal(a, b) for a, b in zip(torch.autograd.grad(y, params, gy), want_g))
    del rp.mlp.mlp_backward
    # a caller's own x that requires a gradient gets it from the torch layers
    x = feats.clone().requires_grad_(True)
    y = rp._apply_mlp(x)
    assert torch.equal(y, want)
    gx, = torch.autograd.grad(y, [x], gy)
    x2 = feats.clone().requires_grad_(True)
    gx_want, = torch.autograd.grad(rp.mlp(x2), [x2], gy)
    assert torch.equal(gx, gx_want)
    # a list below the threshold
    with torch.no_grad():
        assert torch.equal(rp._apply_mlp(feats[:999]), rp.mlp(feats[:999]))
    assert ff.calls == before
    # a CPU module
    from tpnet_amd import RandomProjectionModule
    cpu = RandomProjectionModule(node_num=50, edge_num=100, dim_factor=10, num_layer=4, time_decay_weight=2e-6, device="cpu",
                                 use_matrix=False, beginning_time=np.float64(0.0), not_scale=False, enforce_dim=16)
    cpu.mlp_l4 = True
    xc = _features(1200, 3)
    with torch.no_grad():
        assert torch.equal(cpu._apply_mlp(xc), cpu.mlp(xc))
    # L = 3
    rp3 = _updated_module(3)
    rp3.mlp_l4 = True
    with torch.no_grad():
        f3 = rp3.pair_gram(u, v)
        got3 = rp3._apply_mlp(f3)
    rp3.mlp_l4 = False
    with torch.no_grad():
        assert torch.equal(got3, rp3._apply_mlp(f3))
    assert ff.calls == before
    rp.check_device_errors()
    rp3.check_device_errors()
