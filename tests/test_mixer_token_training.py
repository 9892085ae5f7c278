"""The token-mixing half of an MLP-Mixer layer in a training step (tpnet_amd/fused_mixer.py: token_train / token_masks,
csrc/mixer_token_train.hip, TPNetEmbedding.fused_token_training): forward with dropout against the torch layers with the exported
masks, backward against float64 evaluations of the expressions at the top of the kernel file, the draws against a numpy Philox."""
import numpy as np
import pytest
import torch

from test_encoder_module import _g11, _model, _need_gpu
from test_fused_mixer import _mixer, _stage, _token_input, _token_torch
from test_sampler_strategies import philox4x32

DEV = "cuda:0"
SHAPES = [(20, 172), (6, 20), (2, 4), (32, 256), (10, 100)]
NS = [1, 7, 300]
TAG = 0x4D58544B
NAMES = ("ggamma", "gbeta", "gw1", "gb1", "gw2", "gb2")
U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- CPU tier

def test_partial_floats_are_host_arithmetic(hip_lib):
    L = hip_lib
    assert L.tpnet_mixer_token_bwd_partial_floats(20, 10) == 470
    assert L.tpnet_mixer_token_bwd_partial_floats(2, 1) == 11            # 3 K + 2 K Kh + Kh: 2 + 2 + 2 + 1 + 2 + 2
    assert L.tpnet_mixer_token_bwd_partial_floats(32, 32) == 2176
    for K, Kh in ((1, 1), (33, 10), (20, 0), (20, 33), (0, 0), (-1, 4)):
        assert L.tpnet_mixer_token_bwd_partial_floats(K, Kh) == 0, (K, Kh)


def test_bad_arguments_return_without_a_gpu(hip_lib):
    """Null pointers, p outside [0, 1), n_partial < 1, misaligned arrays, out == x and unserved sizes: -1 (TPNET_ERR_BAD_ARG),
    nothing launched; no nodes: 0."""
    L = hip_lib
    #      x   n  K   C    g   b   eps   w1  b1  Kh  w2  b2  p    key out stream
    fwd = [16, 5, 20, 172, 16, 16, 1e-5, 16, 16, 10, 16, 16, 0.1, 7, 32, None]
    for i in (0, 4, 5, 7, 8, 10, 11, 14):                                                # every pointer null in turn
        a = list(fwd)
        a[i] = None
        assert L.tpnet_mixer_token_train(*a) == -1, i
    for i, v in ((14, 16), (0, 20), (14, 40), (4, 18), (11, 6), (12, 1.0), (12, -0.1), (12, float("nan")), (1, -1), (2, 1), (2, 33),
                 (9, 0), (9, 33), (3, 174), (3, 0), (1, 1 << 40)):
        a = list(fwd)
        a[i] = v
        assert L.tpnet_mixer_token_train(*a) == -1, (i, v)
    #      x   gy  n  K   C    g   b   eps   w1  b1  Kh  w2  b2  p    key gx  part np stream
    bwd = [16, 32, 5, 20, 172, 16, 16, 1e-5, 16, 16, 10, 16, 16, 0.1, 7, 48, 64, 4, None]
    for i in (0, 1, 5, 6, 8, 9, 11, 12, 16):                                             # (gx, 15, may be null)
        a = list(bwd)
        a[i] = None
        assert L.tpnet_mixer_token_bwd(*a) == -1, i
    for i, v in ((15, 16), (15, 32), (0, 20), (1, 36), (15, 52), (16, 66), (5, 18), (13, 1.0), (13, -0.1), (17, 0), (17, -3), (2, -1),
                 (3, 1), (3, 33), (10, 0), (10, 33), (4, 174), (2, 1 << 40)):
        a = list(bwd)
        a[i] = v
        assert L.tpnet_mixer_token_bwd(*a) == -1, (i, v)
    #      n  K   Kh  C    p    key m1  m2  stream
    msk = [5, 20, 10, 172, 0.1, 7, 16, 32, None]
    for i in (6, 7):
        a = list(msk)
        a[i] = None
        assert L.tpnet_mixer_token_masks(*a) == -1, i
    for i, v in ((4, 1.0), (4, -0.1), (0, -1), (1, 1), (1, 33), (2, 0), (2, 33), (3, 174), (0, 1 << 40)):
        a = list(msk)
        a[i] = v
        assert L.tpnet_mixer_token_masks(*a) == -1, (i, v)
    fwd[1], bwd[2], msk[0] = 0, 0, 0                                                     # nothing to do, nothing launched
    assert L.tpnet_mixer_token_train(*fwd) == 0 and L.tpnet_mixer_token_bwd(*bwd) == 0 and L.tpnet_mixer_token_masks(*msk) == 0
    bwd[15] = None
    assert L.tpnet_mixer_token_bwd(*bwd) == 0


def test_switch_defaults_to_off_and_a_cpu_model_ignores_it(golden_dir):
    import tpnet_amd
    from tpnet_amd import fused_mixer as fm
    assert tpnet_amd.TPNetEmbedding.fused_token_training is False
    assert "token_train" in fm.calls and "token_bwd" in fm.calls
    g = _g11(golden_dir)
    model, _ = _model(g, "cpu", dropout=0.0)
    model.train()
    emb = model.embedding_module
    args = (g["c0_neigh"], g["c0_eids"], g["c0_tn"], np.tile(g["c0_t"], 2), torch.from_numpy(g["c0_feat"]))
    before = dict(fm.calls)
    off = emb.embed_from_features(*args)
    emb.fused_token_training = True
    on = emb.embed_from_features(*args)
    assert on.requires_grad and torch.equal(on, off) and fm.calls == before


# ---------------------------------------------------------------------------------------------------------------- references

def _scale(p):
    """1 / (1 - p) in float, as the kernels take it."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def _numpy_masks(n, K, Kh, C, p, key):
    """The header's counter layout with the test-side Philox: m1 [n, C, Kh], m2 [n, K, C]."""
    M32 = np.uint64(0xFFFFFFFF)
    nd = Kh + K
    nb = (nd + 3) // 4
    col = np.arange(n * C, dtype=np.uint64)[:, None].repeat(nb, 1)
    blk = np.arange(nb, dtype=np.uint64)[None, :].repeat(n * C, 0)
    ctr = np.stack([col & M32, col >> np.uint64(32), blk, np.full_like(col, TAG)], axis=-1)
    k = np.array([key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    words = philox4x32(ctr, np.broadcast_to(k, ctr.shape[:-1] + (2,))).reshape(n * C, nb * 4)[:, :nd].astype(np.uint64)
    keep = words >= np.uint64(int(np.floor(float(np.float32(p)) * 2.0 ** 32)))
    return keep[:, :Kh].reshape(n, C, Kh), keep[:, Kh:].reshape(n, C, K).transpose(0, 2, 1)


def _token_torch_masked(m, x, m1, m2, s):
    """_token_torch with the given keep masks in place of nn.Dropout: m1 [n, C, Kh], m2 [n, K, C], s = 1 / (1 - p)."""
    ffn = m.token_feedforward.ffn
    a = ffn[0](m.token_norm(x.permute(0, 2, 1)))
    h = torch.nn.functional.gelu(a) * m1 * s
    return (ffn[3](h) * m2.permute(0, 2, 1) * s).permute(0, 2, 1) + x


def _ref64(m, x, gy, m1=None, m2=None, s=1.0):
    """The kernel file's expressions in float64 on the host: (y, gx, the six parameter gradients, their magnitudes: the sums over
    the columns of the terms' absolute values)."""
    D = lambda t: t.detach().double().cpu()
    ffn = m.token_feedforward.ffn
    gamma, beta, eps = D(m.token_norm.weight), D(m.token_norm.bias), float(m.token_norm.eps)
    w1, b1, w2, b2 = D(ffn[0].weight), D(ffn[0].bias), D(ffn[3].weight), D(ffn[3].bias)
    v, g = D(x).permute(0, 2, 1), D(gy).permute(0, 2, 1)                              # [n, C, K]
    K = v.shape[-1]
    m1 = torch.ones(v.shape[:2] + (w1.shape[0],), dtype=torch.float64) if m1 is None else D(m1)
    m2 = torch.ones_like(v) if m2 is None else D(m2).permute(0, 2, 1)
    mean = v.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (v - mean) * rstd
    ln = xh * gamma + beta
    a = ln @ w1.t() + b1
    h = 0.5 * a * (1.0 + torch.erf(a / np.sqrt(2.0))) * m1 * s
    y = (h @ w2.t() + b2) * m2 * s + v
    go = g * m2 * s
    gh = go @ w2
    ga = gh * m1 * s * (0.5 * (1.0 + torch.erf(a / np.sqrt(2.0))) + a * torch.exp(-0.5 * a * a) / np.sqrt(2.0 * np.pi))
    gln = ga @ w1
    gxh = gln * gamma
    gx = rstd * (gxh - gxh.mean(-1, keepdim=True) - xh * (gxh * xh).mean(-1, keepdim=True)) + g
    grads = ((gln * xh).sum((0, 1)), gln.sum((0, 1)), torch.einsum("ncj,nck->jk", ga, ln), ga.sum((0, 1)),
             torch.einsum("nck,ncj->kj", go, h), go.sum((0, 1)))
    mags = ((gln * xh).abs().sum((0, 1)), gln.abs().sum((0, 1)), torch.einsum("ncj,nck->jk", ga.abs(), ln.abs()), ga.abs().sum((0, 1)),
            torch.einsum("nck,ncj->kj", go.abs(), h.abs()), go.abs().sum((0, 1)))
    assert all(gr.shape == t.shape for gr, t in zip(grads, (gamma, beta, w1, b1, w2, b2)))
    return y.permute(0, 2, 1), gx.permute(0, 2, 1), grads, mags


def _bwd_call(m, x, gy, p=0.0, key=0, n_partial=256, want_gx=True, part=None):
    """tpnet_mixer_token_bwd itself: (rc, partial buffer [rows, floats] prefilled with NaN, gx or None)."""
    from tpnet_amd import _dense, _lib
    lib = _lib.load()
    ffn = m.token_feedforward.ffn
    n, K, C = x.shape
    Kh = ffn[0].out_features
    pf = int(lib.tpnet_mixer_token_bwd_partial_floats(K, Kh))
    if part is None:
        part = torch.full((n_partial, pf), float("nan"), device=x.device)
    gx = torch.full_like(x, float("nan")) if want_gx else None
    ptr = lambda t: t.data_ptr()
    rc = lib.tpnet_mixer_token_bwd(ptr(x), ptr(gy), n, K, C, ptr(m.token_norm.weight), ptr(m.token_norm.bias), float(m.token_norm.eps),
                                   ptr(ffn[0].weight), ptr(ffn[0].bias), Kh, ptr(ffn[3].weight), ptr(ffn[3].bias), float(p), int(key),
                                   None if gx is None else ptr(gx), ptr(part), n_partial, _dense.stream_ptr(x.device))
    return rc, part, gx


def _split(m, tot):
    """A summed partial as the six gradients, in the layout ggamma | gbeta | gw1 | gb1 | gw2 | gb2."""
    ffn = m.token_feedforward.ffn
    out, off = [], 0
    for t in (m.token_norm.weight, m.token_norm.bias, ffn[0].weight, ffn[0].bias, ffn[3].weight, ffn[3].bias):
        out.append(tot[off:off + t.numel()].view(t.shape))
        off += t.numel()
    assert off == tot.numel()
    return out


def _batches(n, K, C, Kh):
    cols = 256 if 256 * (4 * K + 2 * Kh + 1) * 4 <= 160 * 1024 else 128
    return (n * C + cols - 1) // cols


def _check_param_grads(tag, got, want, mags):
    """|err| <= 64 * 2^-24 * mag + 1e-6 * max|want| per entry; prints the largest err / bound per tensor."""
    worst = {}
    for name, gt, wt, mg in zip(NAMES, got, want, mags):
        err = (gt.detach().double().cpu() - wt).abs()
        bound = 64 * U * mg + 1e-6 * float(wt.abs().max())
        worst[name] = float((err / bound).max())
    print(f"{tag}: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(np.isfinite(v) and v <= 1.0 for v in worst.values()), worst


# ---------------------------------------------------------------------------------------------------------------- GPU tier

@pytest.mark.gpu
@pytest.mark.parametrize("K,C", SHAPES)
@pytest.mark.parametrize("n", NS)
def test_forward_without_dropout_has_the_bits_of_mixer_token(n, K, C):
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(K, C, seed=K + C).to(DEV)
    x = _token_input(n, K, C, seed=n)
    before = dict(fm.calls)
    with torch.no_grad():
        got = fm.token_train(m, x, 0.0)
    assert fm.calls["token_train"] == before["token_train"] + 1 and fm.calls["token"] == before["token"]
    assert got.data_ptr() != x.data_ptr() and torch.equal(got, fm.mixer_token(m, x))
    assert torch.equal(got, fm.token_train(m, x, 0.0, key=12345))                       # p = 0 draws nothing: the key is not read


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", [(20, 172), (6, 20)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_masks_follow_the_counter_layout(K, C, p):
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(K, C, seed=K + C).to(DEV)
    n, Kh, key = 7, K // 2, 0x0123456789ABCDEF
    m1, m2 = fm.token_masks(m, n, C, p, key)
    assert m1.shape == (n, C, Kh) and m2.shape == (n, K, C) and m1.dtype == torch.bool
    w1, w2 = _numpy_masks(n, K, Kh, C, p, key)
    assert np.array_equal(m1.cpu().numpy(), w1) and np.array_equal(m2.cpu().numpy(), w2)
    a1, a2 = fm.token_masks(m, n, C, p, key)
    assert torch.equal(a1, m1) and torch.equal(a2, m2)
    o1, o2 = fm.token_masks(m, n, C, p, key + 1)
    assert not torch.equal(o1, m1) and not torch.equal(o2, m2)
    z1, z2 = fm.token_masks(m, n, C, 0.0, key)
    assert bool(z1.all()) and bool(z2.all())


@pytest.mark.gpu
def test_kept_share_of_the_draws():
    """(300, 20, 172) at p = 0.1: the kept share of the 516 000 m1 draws (sigma = sqrt(0.09 / 516 000) = 4.2e-4) and of the
    1 032 000 m2 draws is within 5 sigma of 0.9."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(20, 172, seed=192).to(DEV)
    m1, m2 = fm.token_masks(m, 300, 172, 0.1, 99)
    assert m1.numel() == 516000
    for name, mk in (("m1", m1), ("m2", m2)):
        share, sigma = float(mk.double().mean()), float(np.sqrt(0.09 / mk.numel()))
        print(f"kept share of {name}: {share:.6f} ({(share - 0.9) / sigma:+.2f} sigma of {sigma:.2e})")
        assert abs(share - 0.9) <= 5 * sigma


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", SHAPES)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_forward_with_dropout_matches_torch_with_the_exported_masks(p, n, K, C):
    """The project's true-fp32 tolerance (rtol 1e-4, atol 1e-5), test_token_kernel_matches_torch's, twice: on standard normal input
    against the torch layers in fp32 on the device, and on _token_input's constant columns and +1000 node against the same
    expression in float64.  The second reference is float64 because torch's fp32 LayerNorm is itself off there (a constant
    column does not normalise to exactly beta, and 1 / sqrt(eps) = 316 stands in front), and s^2 = 4 at p = 0.5 scales that:
    measured on an MI355X at (7, 20, 172), p = 0.5, torch's fp32 result has 2 elements beyond this tolerance of the float64 one
    (largest difference 2.1e-4), the kernel's none (3.1e-5, at values of 1000)."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(K, C, seed=K + C).to(DEV)
    key = 1000 * n + K
    m1, m2 = fm.token_masks(m, n, C, p, key)
    x = torch.randn(n, K, C, generator=torch.Generator().manual_seed(n + K)).to(DEV)
    with torch.no_grad():
        want = _token_torch_masked(m, x, m1, m2, _scale(p))
        got = fm.token_train(m, x, p, key)
        assert not torch.equal(got, fm.token_train(m, x, 0.0)) and torch.equal(got, fm.token_train(m, x, p, key))
    print(f"token_train n {n} K {K} C {C} p {p}: max abs diff from torch fp32 {float((got - want).abs().max()):.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-5)
    x = _token_input(n, K, C, seed=n)
    with torch.no_grad():
        got = fm.token_train(m, x, p, key)
    want = _ref64(m, x, x, m1, m2, _scale(p))[0]
    print(f"token_train n {n} K {K} C {C} p {p}, ill-conditioned: max abs diff from float64 {float((got.double().cpu() - want).abs().max()):.3e}")
    np.testing.assert_allclose(got.double().cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", [s for s in SHAPES if s[0] >= 6])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_backward_on_well_conditioned_inputs(p, n, K, C):
    """x and gy standard normal, against the float64 expressions with the exported masks: gx element-wise at rtol 1e-4 / atol 1e-5,
    every parameter gradient at |err| <= 64 * 2^-24 * mag + 1e-6 * max|want| (mag: the float64 sum over the columns of the terms'
    absolute values).  64: a term carries the roundings of a LayerNorm, two dot products of at most 32 terms and erff / expf, and the
    blocked sum adds its depth; torch's own fp32 autograd stays at or below 3.5 * 2^-24 * mag on these inputs.  Measured on an
    MI355X: the largest err / bound of any tensor and case is 0.049 (profiles/mixer_token_training.md)."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(K, C, seed=K + C).to(DEV)
    gen = torch.Generator().manual_seed(100 * n + K)
    x, gy = torch.randn(n, K, C, generator=gen).to(DEV), torch.randn(n, K, C, generator=gen).to(DEV)
    key = 77 + n
    m1, m2 = fm.token_masks(m, n, C, p, key)
    _, want_gx, want, mags = _ref64(m, x, gy, m1, m2, _scale(p))
    rc, part, gx = _bwd_call(m, x, gy, p, key)
    assert rc == min(256, _batches(n, K, C, K // 2))
    print(f"bwd n {n} K {K} C {C} p {p}: gx max abs diff {float((gx.double().cpu() - want_gx).abs().max()):.3e}")
    np.testing.assert_allclose(gx.cpu().numpy(), want_gx.numpy(), rtol=1e-4, atol=1e-5)
    _check_param_grads(f"bwd n {n} K {K} C {C} p {p}", _split(m, part[:rc].sum(0)), want, mags)


ILL = [(K, C, n, "token_input") for K, C in SHAPES for n in NS] + [(2, 4, n, "normal") for n in NS]


@pytest.mark.gpu
@pytest.mark.parametrize("K,C,n,kind", ILL)
def test_backward_on_ill_conditioned_inputs(K, C, n, kind):
    """K = 2, and _token_input's constant columns (1 / sqrt(eps) = 316 in front of gx) and +1000 node: torch's fp32 autograd is itself
    off the float64 result there, so it is the yardstick.  Per tensor, the kernel's scaled error max|err| / max(1, max|want|)
    against float64 is at most 4 x that of torch's fp32 autograd on the same device and inputs, + 1e-6 (both are fp32 evaluations
    of one ill-conditioned expression in different summation orders).  Measured on an MI355X: the kernel's scaled error is at most
    1.0e-6 in every case and tensor, torch's up to 7.4e-5 (profiles/mixer_token_training.md)."""
    _need_gpu()
    m = _mixer(K, C, seed=K + C).to(DEV)
    gen = torch.Generator().manual_seed(31 * n + K)
    x = _token_input(n, K, C, seed=n) if kind == "token_input" else torch.randn(n, K, C, generator=gen).to(DEV)
    gy = torch.randn(n, K, C, generator=gen).to(DEV)
    _, want_gx, want, _ = _ref64(m, x, gy)
    ffn = m.token_feedforward.ffn
    params = (m.token_norm.weight, m.token_norm.bias, ffn[0].weight, ffn[0].bias, ffn[3].weight, ffn[3].bias)
    xr = x.clone().requires_grad_(True)
    torch_grads = torch.autograd.grad(_token_torch(m, xr), (xr,) + params, gy)
    rc, part, gx = _bwd_call(m, x, gy)
    got = [gx] + _split(m, part[:rc].sum(0))
    scaled = lambda t, w: float((t.detach().double().cpu() - w).abs().max() / max(1.0, float(w.abs().max())))
    bad = []
    for name, gt, tg, wt in zip(("gx",) + NAMES, got, torch_grads, (want_gx,) + tuple(want)):
        assert bool(torch.isfinite(gt).all()), name
        ek, et = scaled(gt, wt), scaled(tg, wt)
        print(f"ill-conditioned {kind} n {n} K {K} C {C} {name}: kernel {ek:.3e}, torch fp32 autograd {et:.3e}")
        if not ek <= 4 * et + 1e-6:
            bad.append((name, ek, et))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", SHAPES)
@pytest.mark.parametrize("n", NS)
def test_backward_is_deterministic_and_independent_of_the_geometry(n, K, C):
    """Two calls: equal partials and gx.  n_partial = 4 (at n = 300 every workgroup walks many batches) and 256: equal gx, summed
    gradients within test_backward_on_well_conditioned_inputs' bound of the float64 result and of each other; partials beyond the
    returned count keep their NaN prefill; a null gx leaves the partials' bits."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(K, C, seed=K + C).to(DEV)
    Kh = K // 2
    gen = torch.Generator().manual_seed(7 * n + K)
    x, gy = torch.randn(n, K, C, generator=gen).to(DEV), torch.randn(n, K, C, generator=gen).to(DEV)
    p, key = 0.1, 5 + n
    m1, m2 = fm.token_masks(m, n, C, p, key)
    _, _, want, mags = _ref64(m, x, gy, m1, m2, _scale(p))
    nb = _batches(n, K, C, Kh)
    sums = {}
    for n_partial in (4, 256):
        rc, part, gx = _bwd_call(m, x, gy, p, key, n_partial)
        rc2, part2, gx2 = _bwd_call(m, x, gy, p, key, n_partial)
        assert rc == rc2 == min(n_partial, nb)
        assert bool(torch.isfinite(part[:rc]).all()) and bool(torch.isnan(part[rc:]).all())
        assert torch.equal(part[:rc], part2[:rc]) and torch.equal(gx, gx2) and bool(torch.isfinite(gx).all())
        rc3, part3, none = _bwd_call(m, x, gy, p, key, n_partial, want_gx=False)
        assert rc3 == rc and none is None and torch.equal(part3[:rc], part[:rc]) and bool(torch.isnan(part3[rc:]).all())
        sums[n_partial] = (gx, _split(m, part[:rc].sum(0)))
        if K >= 6:
            _check_param_grads(f"n_partial {n_partial} n {n} K {K} C {C}", sums[n_partial][1], want, mags)
    assert torch.equal(sums[4][0], sums[256][0])
    for name, a, b, mg, wt in zip(NAMES, sums[4][1], sums[256][1], mags, want):
        bound = 64 * U * mg + 1e-6 * float(wt.abs().max())
        assert bool(((a.double().cpu() - b.double().cpu()).abs() <= bound).all()), name
    # a window inside a larger NaN buffer: nothing is written in front of the first or behind the last partial
    pf = sum(t.numel() for t in sums[4][1])
    buf = torch.full((6, pf), float("nan"), device=DEV)
    rc, _, _ = _bwd_call(m, x, gy, p, key, 4, part=buf[1:])
    assert rc == min(4, nb) and bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[1 + rc:]).all())
    assert bool(torch.isfinite(buf[1:1 + rc]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", [s for s in SHAPES if s[0] >= 6])
@pytest.mark.parametrize("n", NS)
def test_autograd_through_token_train(n, K, C):
    """torch.autograd.grad through token_train at p = 0 against float64 autograd through the torch layers, at
    test_backward_on_well_conditioned_inputs' bounds; a Parameter that requires no gradient gets None."""
    _need_gpu()
    import copy
    from tpnet_amd import fused_mixer as fm
    m = _mixer(K, C, seed=K + C).to(DEV)
    gen = torch.Generator().manual_seed(13 * n + K)
    x, gy = torch.randn(n, K, C, generator=gen).to(DEV), torch.randn(n, K, C, generator=gen).to(DEV)
    ffn = m.token_feedforward.ffn
    params = (m.token_norm.weight, m.token_norm.bias, ffn[0].weight, ffn[0].bias, ffn[3].weight, ffn[3].bias)
    m64 = copy.deepcopy(m).double().cpu()
    f64 = m64.token_feedforward.ffn
    p64 = (m64.token_norm.weight, m64.token_norm.bias, f64[0].weight, f64[0].bias, f64[3].weight, f64[3].bias)
    x64 = x.double().cpu().requires_grad_(True)
    want = torch.autograd.grad(_token_torch(m64, x64), (x64,) + p64, gy.double().cpu())
    _, ref_gx, ref, mags = _ref64(m, x, gy)
    assert float((want[0] - ref_gx).abs().max()) <= 1e-9                                # the expressions ARE the layers' gradient
    for a, b in zip(want[1:], ref):
        assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max()))
    before = dict(fm.calls)
    xr = x.clone().requires_grad_(True)
    y = fm.token_train(m, xr, 0.0)
    assert y.requires_grad and fm.calls["token_train"] == before["token_train"] + 1 and fm.calls["token_bwd"] == before["token_bwd"]
    got = torch.autograd.grad(y, (xr,) + params, gy)
    assert fm.calls["token_bwd"] == before["token_bwd"] + 1
    assert all(fm.calls[k] == before[k] for k in ("token", "channel", "prepare"))
    np.testing.assert_allclose(got[0].cpu().numpy(), want[0].numpy(), rtol=1e-4, atol=1e-5)
    _check_param_grads(f"autograd n {n} K {K} C {C}", got[1:], [w.detach() for w in want[1:]], mags)
    # frozen Parameters and a plain input: None for those, the same bits for the others
    ffn[0].weight.requires_grad_(False)
    m.token_norm.bias.requires_grad_(False)
    y = fm.token_train(m, x, 0.0)
    y.backward(gy)
    assert ffn[0].weight.grad is None and m.token_norm.bias.grad is None
    for i in (0, 3, 4, 5):
        assert torch.equal(params[i].grad, got[1 + i]), NAMES[i]


def _training_stage(g, dropout, train):
    """G11's embedding module (test_fused_mixer._stage: fused_mixer on) with fused_token_training on."""
    emb, arrays = _stage(g, dropout)
    emb.fused_token_training = True
    emb.train(train)
    return emb, arrays


def _grads_of(emb, arrays):
    emb.zero_grad(set_to_none=True)
    emb.embed_from_features(*arrays).sum().backward()
    return {k: p.grad.clone() for k, p in emb.named_parameters() if p.grad is not None}


@pytest.mark.gpu
def test_routing_and_gradients_on_g11(golden_dir):
    """Call counters: a grad-enabled call moves token_train by the layer count and its backward token_bwd by the same; no_grad and
    the switch off move neither; the other counters never move on the new route.  Every gradient of the module's Parameters is within
    rtol 1e-4 / atol 1e-5 of the run with the switch off (test_g11_end_to_end_gradients' tolerance)."""
    _need_gpu()
    g = _g11(golden_dir)
    from tpnet_amd import fused_mixer as fm
    emb, arrays = _training_stage(g, 0.0, train=True)
    layers = len(emb.mlp_mixers)
    c0 = dict(fm.calls)
    out = emb.embed_from_features(*arrays)
    assert out.requires_grad and fm.calls["token_train"] == c0["token_train"] + layers and fm.calls["token_bwd"] == c0["token_bwd"]
    out.sum().backward()
    assert fm.calls["token_bwd"] == c0["token_bwd"] + layers
    assert all(fm.calls[k] == c0[k] for k in ("token", "channel", "prepare"))
    on = _grads_of(emb, arrays)
    emb.eval()                                                                          # eval mode with a gradient: rate 0, same route
    c1 = dict(fm.calls)
    on_eval = _grads_of(emb, arrays)
    assert fm.calls["token_train"] == c1["token_train"] + layers and fm.calls["token_bwd"] == c1["token_bwd"] + layers
    emb.train()
    emb.fused_token_training = False
    c2 = dict(fm.calls)
    off = _grads_of(emb, arrays)
    assert fm.calls == c2                                                               # the switch off: torch, as before
    emb.fused_token_training = True
    with torch.no_grad():
        emb.embed_from_features(*arrays)                                                # no gradient: fused_mixer's kernels
    assert fm.calls["token_train"] == c2["token_train"] and fm.calls["token_bwd"] == c2["token_bwd"]
    assert fm.calls["token"] == c2["token"] + layers
    assert set(on) == set(off) == set(on_eval) and any(k.startswith("mlp_mixers.0.token_norm") for k in on)
    for k in off:
        np.testing.assert_allclose(on_eval[k].cpu().numpy(), off[k].cpu().numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
        print(f"G11 {k}: largest difference {float((on[k] - off[k]).abs().max()):.3e} at scale {float(off[k].abs().max()):.3f}")
    for k in off:
        np.testing.assert_allclose(on[k].cpu().numpy(), off[k].cpu().numpy(), rtol=1e-4, atol=1e-5, err_msg=k)


@pytest.mark.gpu
def test_dropout_in_train_mode_is_reproducible_under_manual_seed(golden_dir):
    _need_gpu()
    g = _g11(golden_dir)
    from tpnet_amd import fused_mixer as fm
    emb, arrays = _training_stage(g, 0.1, train=True)
    layers = len(emb.mlp_mixers)
    runs = []
    for seed in (11, 11, 12):
        torch.manual_seed(seed)                     # (the channel FFN's dropouts are torch's and follow the seed as well)
        c0 = dict(fm.calls)
        emb.zero_grad(set_to_none=True)
        out = emb.embed_from_features(*arrays)
        out.sum().backward()
        assert fm.calls["token_train"] == c0["token_train"] + layers and fm.calls["token_bwd"] == c0["token_bwd"] + layers
        assert all(fm.calls[k] == c0[k] for k in ("token", "channel", "prepare"))
        runs.append((out.detach().clone(), {k: p.grad.clone() for k, p in emb.named_parameters() if p.grad is not None}))
    assert bool(torch.isfinite(runs[0][0]).all())
    assert torch.equal(runs[0][0], runs[1][0]) and not torch.equal(runs[0][0], runs[2][0])
    for k in runs[0][1]:                            # (the torch layers between the kernels may sum their weight gradients atomically)
        np.testing.assert_allclose(runs[0][1][k].cpu().numpy(), runs[1][1][k].cpu().numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
    emb.eval()
    with torch.no_grad():
        plain = emb.embed_from_features(*arrays)
    assert not torch.equal(plain, runs[0][0])                                           # the dropout was active


@pytest.mark.gpu
def test_parameter_updates_are_seen_by_the_next_call(golden_dir):
    """The Parameters are read in place: after an optimiser step the next call runs on the new weights (against the torch layers)."""
    _need_gpu()
    g = _g11(golden_dir)
    emb, arrays = _training_stage(g, 0.0, train=True)
    first = emb.embed_from_features(*arrays)
    opt = torch.optim.SGD(emb.mlp_mixers.parameters(), lr=0.05)
    first.square().sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in emb.mlp_mixers.parameters())
    opt.step()
    after = emb.embed_from_features(*arrays)
    emb.fused_token_training = False
    want = emb.embed_from_features(*arrays)
    assert not torch.equal(after, first)
    np.testing.assert_allclose(after.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
