"""The channel-mixing half of an MLP-Mixer layer in a training step (tpnet_amd/fused_mixer.py: channel_train / channel_masks,
csrc/mixer_channel_train.hip, TPNetEmbedding.fused_channel_training): forward with dropout against the torch layers with the
exported masks, backward against float64 evaluations of the expressions at the top of the kernel file, the draws against a numpy
Philox.  x, gy and every output of a direct call are views into larger buffers whose remainder is NaN."""
import numpy as np
import pytest
import torch

from test_encoder_module import _g11, _model, _need_gpu, _scaled_err
from test_fused_mixer import _channel_input, _channel_torch, _mixer, _stage
from test_sampler_strategies import philox4x32

DEV = "cuda:0"
SHAPES = [(172, 688), (20, 80), (100, 353), (256, 1024), (4, 1)]
# (rows, partials offered to the backward): one tile; two; five tiles in five parts; five tiles in two parts (3 + 2: a part of several
# tiles, the last one short); ten tiles in four parts (3 + 3 + 3 + 1)
ROWS = [(1, 32), (33, 32), (129, 32), (129, 2), (300, 4)]
BIG = [(172, 688), (20, 80)]                     # + 6000 rows: 188 tiles in 32 parts of 6, the last one of 2
TAG = 0x4D584348
NAMES = ("ggamma", "gbeta", "gw1", "gb1", "gw2", "gb2")
PAD = 64                                         # floats of NaN on either side of a view (keeps 16-byte alignment)
# test_g11_end_to_end_gradients: 3 x the worst scaled difference of a Parameter's gradient between the switch on and off measured on an
# MI355X (6.9e-6, mlp_mixers.1.channel_feedforward.ffn.0.bias; profiles/mixer_channel_training.md); the file's neighbours allow 1e-4
G11_BOUND = 3 * 6.9e-6


# ---------------------------------------------------------------------------------------------------------------- CPU tier

def test_partial_floats_are_host_arithmetic(hip_lib):
    L = hip_lib
    assert L.tpnet_mixer_channel_bwd_partial_floats(172, 688) == 237876
    assert L.tpnet_mixer_channel_bwd_partial_floats(4, 1) == 21             # 2 C + 2 C Ch + Ch + C: 8 + 8 + 1 + 4
    for C, Ch in ((174, 688), (260, 688), (172, 1025), (0, 8), (172, 0), (-4, 4)):
        assert L.tpnet_mixer_channel_bwd_partial_floats(C, Ch) == 0, (C, Ch)
        assert L.tpnet_mixer_channel_bwd_image_bytes(C, Ch) == 0 and L.tpnet_mixer_channel_bwd_workspace_bytes(100, C, Ch) == 0
    assert L.tpnet_mixer_channel_bwd_image_bytes(172, 688) % 16 == 0
    assert L.tpnet_mixer_channel_bwd_image_bytes(172, 688) >= L.tpnet_mixer_channel_image_bytes(172, 688)
    # 32-row tiles of 2 ceil(Ch / 32) 32 + 4 ceil(C / 32) 32 floats per row
    assert L.tpnet_mixer_channel_bwd_workspace_bytes(33, 172, 688) == 2 * 32 * (2 * 704 + 4 * 192) * 4
    assert L.tpnet_mixer_channel_bwd_workspace_bytes(0, 172, 688) == 0 and L.tpnet_mixer_channel_bwd_workspace_bytes(-1, 172, 688) == 0


def test_bad_arguments_return_without_a_gpu(hip_lib):
    """Null pointers, p outside [0, 1) or NaN, n_partial < 1, misaligned arrays, out == x, gx == x or gy and unserved sizes: -1
    (TPNET_ERR_BAD_ARG), nothing launched; no rows: 0."""
    L = hip_lib
    #      x   n  C    Ch   g   b   eps   img p    key out stream
    fwd = [16, 5, 172, 688, 32, 48, 1e-5, 64, 0.1, 7, 80, None]
    for i in (0, 4, 5, 7, 10):                                                           # every pointer null in turn
        a = list(fwd)
        a[i] = None
        assert L.tpnet_mixer_channel_train(*a) == -1, i
    for i, v in ((10, 16), (0, 20), (10, 40), (4, 36), (5, 8), (7, 24), (8, 1.0), (8, -0.1), (8, float("nan")), (1, -1), (2, 174),
                 (2, 260), (2, 0), (3, 1025), (3, 0), (1, 1 << 40)):
        a = list(fwd)
        a[i] = v
        assert L.tpnet_mixer_channel_train(*a) == -1, (i, v)
    #      x   gy  n  C    Ch   g   b   eps   bimg p    key ws   gx   part np stream
    bwd = [16, 32, 5, 172, 688, 48, 64, 1e-5, 96, 0.1, 7, 112, 128, 144, 4, None]
    for i in (0, 1, 5, 6, 8, 11, 13):                                                    # (gx, 12, may be null)
        a = list(bwd)
        a[i] = None
        assert L.tpnet_mixer_channel_bwd(*a) == -1, i
    for i, v in ((12, 16), (12, 32), (0, 20), (1, 36), (12, 132), (13, 146), (5, 52), (6, 72), (8, 100), (11, 120), (9, 1.0),
                 (9, -0.1), (9, float("nan")), (14, 0), (14, -3), (2, -1), (3, 174), (3, 260), (4, 1025), (4, 0), (2, 1 << 40)):
        a = list(bwd)
        a[i] = v
        assert L.tpnet_mixer_channel_bwd(*a) == -1, (i, v)
    for a in ((None, 16, 32, 172, 688, 48, None), (16, None, 32, 172, 688, 48, None), (16, 32, None, 172, 688, 48, None),
              (16, 32, 48, 172, 688, None, None), (16, 32, 48, 172, 688, 40, None), (16, 32, 48, 174, 688, 64, None)):
        assert L.tpnet_mixer_channel_bwd_prepare(*a) == -1, a
    #      n  C    Ch   p    key m1  m2  stream
    msk = [5, 172, 688, 0.1, 7, 16, 32, None]
    for i in (5, 6):
        a = list(msk)
        a[i] = None
        assert L.tpnet_mixer_channel_masks(*a) == -1, i
    # (0, 1 << 31): a served row count, but 215 blocks of draws per row are more threads than one launch has
    for i, v in ((3, 1.0), (3, -0.1), (3, float("nan")), (0, -1), (1, 174), (1, 260), (2, 0), (2, 1025), (0, 1 << 40), (0, 1 << 31)):
        a = list(msk)
        a[i] = v
        assert L.tpnet_mixer_channel_masks(*a) == -1, (i, v)
    fwd[1], bwd[2], msk[0] = 0, 0, 0                                                     # nothing to do, nothing launched
    assert L.tpnet_mixer_channel_train(*fwd) == 0 and L.tpnet_mixer_channel_bwd(*bwd) == 0 and L.tpnet_mixer_channel_masks(*msk) == 0
    bwd[12] = None
    assert L.tpnet_mixer_channel_bwd(*bwd) == 0


def test_switch_defaults_to_off_and_a_cpu_model_ignores_it(golden_dir):
    import tpnet_amd
    from tpnet_amd import fused_mixer as fm
    assert tpnet_amd.TPNetEmbedding.fused_channel_training is False
    assert "channel_train" in fm.calls and "channel_bwd" in fm.calls
    g = _g11(golden_dir)
    model, _ = _model(g, "cpu", dropout=0.0)
    model.train()
    emb = model.embedding_module
    args = (g["c0_neigh"], g["c0_eids"], g["c0_tn"], np.tile(g["c0_t"], 2), torch.from_numpy(g["c0_feat"]))
    before = dict(fm.calls)
    off = emb.embed_from_features(*args)
    emb.fused_channel_training = True
    on = emb.embed_from_features(*args)
    emb.fused_token_training = True
    both = emb.embed_from_features(*args)
    assert on.requires_grad and torch.equal(on, off) and torch.equal(both, off) and fm.calls == before


# ---------------------------------------------------------------------------------------------------------------- references

def _scale(p):
    """1 / (1 - p) in float, as the kernels take it."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def _numpy_masks(n, C, Ch, p, key):
    """The header's counter layout with the test-side Philox: m1 [n, Ch], m2 [n, C]."""
    M32 = np.uint64(0xFFFFFFFF)
    nb1 = (Ch + 3) // 4
    nb = nb1 + C // 4
    row = np.arange(n, dtype=np.uint64)[:, None].repeat(nb, 1)
    blk = np.arange(nb, dtype=np.uint64)[None, :].repeat(n, 0)
    ctr = np.stack([row & M32, row >> np.uint64(32), blk, np.full_like(row, TAG)], axis=-1)
    k = np.array([key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    words = philox4x32(ctr, np.broadcast_to(k, ctr.shape[:-1] + (2,))).reshape(n, nb * 4).astype(np.uint64)
    keep = words >= np.uint64(int(np.floor(float(np.float32(p)) * 2.0 ** 32)))
    return keep[:, :Ch], keep[:, 4 * nb1:]


def _channel_torch_masked(m, x, m1, m2, s):
    """_channel_torch with the given keep masks in place of nn.Dropout: m1 [n, Ch], m2 [n, C], s = 1 / (1 - p)."""
    ffn = m.channel_feedforward.ffn
    h = torch.nn.functional.gelu(ffn[0](m.channel_norm(x))) * m1 * s
    return ffn[3](h) * m2 * s + x


def _params(m):
    ffn = m.channel_feedforward.ffn
    return (m.channel_norm.weight, m.channel_norm.bias, ffn[0].weight, ffn[0].bias, ffn[3].weight, ffn[3].bias)


def _ref64(m, x, gy, m1=None, m2=None, s=1.0):
    """The kernel file's expressions in float64 on the host: (y, gx, the six parameter gradients, gx's magnitude, the six
    gradients' magnitudes), the magnitudes as test_backward_against_float64 derives them."""
    D = lambda t: t.detach().double().cpu()
    gamma, beta, w1, b1, w2, b2 = (D(t) for t in _params(m))
    eps = float(m.channel_norm.eps)
    v, g = D(x), D(gy)
    m1 = torch.ones(v.shape[0], w1.shape[0], dtype=torch.float64) if m1 is None else D(m1)
    m2 = torch.ones_like(v) if m2 is None else D(m2)
    mean = v.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (v - mean) * rstd
    ln = xh * gamma + beta
    a = ln @ w1.t() + b1
    Phi, phi = 0.5 * (1.0 + torch.erf(a / np.sqrt(2.0))), torch.exp(-0.5 * a * a) / np.sqrt(2.0 * np.pi)
    d = m1 * s
    h = a * Phi * d
    y = (h @ w2.t() + b2) * m2 * s + v
    go = g * m2 * s
    gh = go @ w2
    gd = Phi + a * phi
    ga = gh * d * gd
    gln = ga @ w1
    gt = gln * gamma
    gx = g + rstd * (gt - gt.mean(-1, keepdim=True) - xh * (gt * xh).mean(-1, keepdim=True))
    grads = ((gln * xh).sum(0), gln.sum(0), ga.t() @ ln, ga.sum(0), go.t() @ h, go.sum(0))
    am = ln.abs() @ w1.abs().t() + b1.abs()
    gom = go.abs()
    ghm = gom @ w2.abs()
    gam = (ghm * gd.abs() + 0.8 * gh.abs() * am) * d
    hm = 1.13 * am * d
    glnm = gam @ w1.abs()
    gtm = glnm * gamma.abs()
    gxm = rstd * (gtm + gtm.mean(-1, keepdim=True) + xh.abs() * (gtm * xh.abs()).mean(-1, keepdim=True)) + g.abs()
    mags = ((glnm * xh.abs()).sum(0), glnm.sum(0), gam.t() @ ln.abs(), gam.sum(0), gom.t() @ hm, gom.sum(0))
    assert all(gr.shape == t.shape for gr, t in zip(grads, (gamma, beta, w1, b1, w2, b2)))
    return y, gx, grads, gxm, mags


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
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[-PAD:]).all())


def _inputs(n, C, seed):
    """_channel_input rows and a standard normal gy, both as views into NaN buffers."""
    gen = torch.Generator().manual_seed(1000 + seed)
    x = _guarded(_channel_input(n, C, seed=seed))[1]
    gy = _guarded(torch.randn(n, C, generator=gen).to(DEV))[1]
    return x, gy


def _fwd_call(m, x, p=0.0, key=0):
    """tpnet_mixer_channel_train itself into a guarded output."""
    from tpnet_amd import _dense, _lib, fused_mixer as fm
    prep = fm.prepared(m, backward=True)
    n, C = x.shape
    Ch = m.channel_feedforward.ffn[0].out_features
    buf, out = _guarded(shape=x.shape)
    g, b = m.channel_norm.weight, m.channel_norm.bias
    rc = _lib.load().tpnet_mixer_channel_train(x.data_ptr(), n, C, Ch, g.data_ptr(), b.data_ptr(), float(m.channel_norm.eps),
                                               prep.img.data_ptr(), float(p), int(key), out.data_ptr(), _dense.stream_ptr(x.device))
    assert rc == 0 and _guards_intact(buf)
    return out


def _bwd_call(m, x, gy, p=0.0, key=0, n_partial=32, want_gx=True):
    """tpnet_mixer_channel_bwd itself: (rc, summed partials, gx or None); partial buffer, workspace and gx prefilled with NaN, the
    partials beyond rc and all guards still NaN behind the call."""
    from tpnet_amd import _dense, _lib, fused_mixer as fm
    lib = _lib.load()
    prep = fm.prepared(m, backward=True)
    n, C = x.shape
    Ch = m.channel_feedforward.ffn[0].out_features
    pf = int(lib.tpnet_mixer_channel_bwd_partial_floats(C, Ch))
    pbuf, part = _guarded(shape=(n_partial, pf))
    wbuf, ws = _guarded(shape=(int(lib.tpnet_mixer_channel_bwd_workspace_bytes(n, C, Ch)) // 4,))
    gbuf, gx = _guarded(shape=x.shape) if want_gx else (None, None)
    g, b = m.channel_norm.weight, m.channel_norm.bias
    rc = lib.tpnet_mixer_channel_bwd(x.data_ptr(), gy.data_ptr(), n, C, Ch, g.data_ptr(), b.data_ptr(), float(m.channel_norm.eps),
                                     prep.bimg.data_ptr(), float(p), int(key), ws.data_ptr(),
                                     None if gx is None else gx.data_ptr(), part.data_ptr(), n_partial, _dense.stream_ptr(x.device))
    tiles = (n + 31) // 32
    per_part = (tiles + n_partial - 1) // n_partial
    assert 1 <= rc <= n_partial and rc == (tiles + per_part - 1) // per_part          # equal parts, none empty
    assert _guards_intact(pbuf) and _guards_intact(wbuf) and (gbuf is None or _guards_intact(gbuf))
    assert bool(torch.isnan(part[rc:]).all()) and bool(torch.isfinite(part[:rc]).all())
    return rc, part[:rc].sum(0), gx


def _split(m, tot):
    out, off = [], 0
    for t in _params(m):
        out.append(tot[off:off + t.numel()].view(t.shape))
        off += t.numel()
    assert off == tot.numel()
    return out


def _check(tag, got_gx, got, ref):
    """|err| <= 4e-5 mag + 1e-6 max|want| per entry of gx and of the six gradients; prints the largest err / bound per tensor."""
    _, want_gx, want, gxm, mags = ref
    worst = {}
    pairs = list(zip(NAMES, got, want, mags))
    if got_gx is not None:
        pairs.append(("gx", got_gx, want_gx, gxm))
    for name, gt, wt, mg in pairs:
        err = (gt.detach().double().cpu() - wt).abs()
        bound = 4e-5 * mg + 1e-6 * float(wt.abs().max())
        worst[name] = float((err / bound).max())
    print(f"{tag}: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(np.isfinite(v) and v <= 1.0 for v in worst.values()), worst


def _cases(shapes=SHAPES):
    return [(C, Ch, n, npart) for C, Ch in shapes for n, npart in ROWS + ([(6000, 32)] if (C, Ch) in BIG else [])]


# ---------------------------------------------------------------------------------------------------------------- GPU tier

@pytest.mark.gpu
@pytest.mark.parametrize("C,Ch", SHAPES)
def test_forward_without_dropout_has_the_bits_of_mixer_channel(C, Ch):
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(4, C, Ch=Ch, seed=C + Ch).to(DEV)
    for n in [1, 33, 129, 300] + ([6000] if (C, Ch) in BIG else []):
        x, _ = _inputs(n, C, seed=n)
        want = fm.mixer_channel(fm.prepared(m), m, x)
        assert torch.equal(_fwd_call(m, x), want), n
        before = dict(fm.calls)
        got = fm.channel_train(m, x.clone().requires_grad_(True), 0.0)
        assert got.requires_grad and torch.equal(got, want) and fm.calls["channel_train"] == before["channel_train"] + 1


@pytest.mark.gpu
@pytest.mark.parametrize("C,Ch", [(172, 688), (20, 80), (100, 353), (4, 1)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_masks_follow_the_counter_layout(C, Ch, p):
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(4, C, Ch=Ch, seed=1).to(DEV)
    n, key = 70, 0x9E3779B97F4A7C15
    m1, m2 = fm.channel_masks(m, n, p, key)
    w1, w2 = _numpy_masks(n, C, Ch, p, key)
    assert m1.shape == (n, Ch) and m2.shape == (n, C) and m1.dtype == torch.bool
    assert np.array_equal(m1.cpu().numpy(), w1) and np.array_equal(m2.cpu().numpy(), w2)
    a1, a2 = fm.channel_masks(m, n, 0.0, key)
    assert bool(a1.all()) and bool(a2.all())
    o1, _ = fm.channel_masks(m, n, p, key + 1)
    assert Ch * n < 200 or not torch.equal(o1, m1)


@pytest.mark.gpu
def test_kept_share_of_the_draws():
    """6000 rows at 172 -> 688 -> 172, p = 0.1: the kept share of either mask is within 5 sigma of 0.9."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(4, 172, Ch=688, seed=1).to(DEV)
    for mask in fm.channel_masks(m, 6000, 0.1, 12345):
        N = mask.numel()
        share = float(mask.float().mean())
        sigma = np.sqrt(0.1 * 0.9 / N)
        print(f"kept share of {N} draws: {share:.6f} ({(share - 0.9) / sigma:+.2f} sigma)")
        assert abs(share - 0.9) <= 5 * sigma


@pytest.mark.gpu
@pytest.mark.parametrize("C,Ch", SHAPES)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_forward_with_dropout_matches_torch_with_the_exported_masks(p, C, Ch):
    """Scaled error <= 2e-5 (test_fused_mixer.test_channel_kernel_matches_torch's bound, from mfma_split.hpp) against the torch layers
    with the masks channel_masks returns; the rows of mean 0 are also scored alone."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(4, C, Ch=Ch, seed=C + Ch).to(DEV)
    worst = 0.0
    for n in [1, 33, 129] + ([6000] if (C, Ch) in BIG else []):
        key = 77 * n + C
        x, _ = _inputs(n, C, seed=n)
        m1, m2 = fm.channel_masks(m, n, p, key)
        with torch.no_grad():
            want = _channel_torch_masked(m, x, m1, m2, _scale(p))
        got = _fwd_call(m, x, p, key)
        err = _scaled_err(got.cpu().numpy(), want.cpu().numpy())
        plain = _scaled_err(got[:n // 2].cpu().numpy(), want[:n // 2].cpu().numpy()) if n > 1 else 0.0
        print(f"channel_train C {C} Ch {Ch} p {p} rows {n}: scaled err {err:.3e} (rows of mean 0 alone: {plain:.3e})")
        worst = max(worst, err, plain)
        if Ch * n >= 200:
            assert not torch.equal(got, _fwd_call(m, x, p, key + 1))                    # the key matters
        assert torch.equal(got, fm.channel_train(m, x, p, key))
    assert worst <= 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("C,Ch", SHAPES)
def test_rows_are_independent_and_the_backward_is_deterministic(C, Ch):
    """The first n rows of the forward and of gx on 300 rows have the bits of the call on n rows; two backward calls give equal bits
    in gx and in the summed partials."""
    _need_gpu()
    m = _mixer(4, C, Ch=Ch, seed=C + Ch).to(DEV)
    p, key = 0.1, 4242
    X, GY = _inputs(300, C, seed=3)
    y_all = _fwd_call(m, X, p, key)
    _, tot_all, gx_all = _bwd_call(m, X, GY, p, key, n_partial=4)
    _, tot_again, gx_again = _bwd_call(m, X, GY, p, key, n_partial=4)
    assert torch.equal(tot_all, tot_again) and torch.equal(gx_all, gx_again)
    for n in (1, 33, 129):
        x, gy = _guarded(X[:n])[1], _guarded(GY[:n])[1]
        assert torch.equal(_fwd_call(m, x, p, key), y_all[:n]), n
        _, _, gx = _bwd_call(m, x, gy, p, key)
        assert torch.equal(gx, gx_all[:n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("C,Ch,n,npart", _cases())
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_backward_against_float64(p, C, Ch, n, npart):
    """Every tensor within tol = 4e-5 mag + 1e-6 max|want| of the float64 evaluation of the kernel file's expressions on the host,
    with the exported masks.  4e-5 is the project's fp32-class coefficient (test_mlp_rows_bwd.py); the magnitudes are the first-order
    propagation of 2^-16 per two-piece product: am = |ln| |W1|^T + |b1|, gom = |go|, ghm = gom |W2|, d = m1 s,
    gam = (ghm |gelu'(a)| + 0.8 |gh| am) d (0.8 >= max |gelu''| = 2 phi(0)), hm = 1.13 am d (1.13 >= max |gelu'|), glnm = gam |W1|,
    gtm = glnm |gamma|; gW1: gam^T |ln|, gb1: sum gam, gW2: gom^T hm, gb2: sum gom, ggamma: sum glnm |xh|, gbeta: sum glnm,
    gx: rstd (gtm + mean(gtm) + |xh| mean(gtm |xh|)) + |gy|.  gx = None leaves the partial sums' bits unchanged."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(4, C, Ch=Ch, seed=C + Ch).to(DEV)
    key = 31 * n + Ch
    x, gy = _inputs(n, C, seed=n)
    m1, m2 = fm.channel_masks(m, n, p, key)
    ref = _ref64(m, x, gy, m1, m2, _scale(p))
    rc, tot, gx = _bwd_call(m, x, gy, p, key, n_partial=npart)
    _check(f"channel_bwd C {C} Ch {Ch} rows {n} p {p} parts {rc}", gx, _split(m, tot), ref)
    _, tot2, none = _bwd_call(m, x, gy, p, key, n_partial=npart, want_gx=False)
    assert none is None and torch.equal(tot, tot2)


@pytest.mark.gpu
@pytest.mark.parametrize("C,Ch", SHAPES)
@pytest.mark.parametrize("n", [1, 33, 129])
def test_autograd_through_channel_train(n, C, Ch):
    """torch.autograd.grad through channel_train at p = 0 against float64 autograd through the module's layers, at
    test_backward_against_float64's bounds; a Parameter that requires no gradient gets None, and so does a plain input."""
    _need_gpu()
    import copy
    from tpnet_amd import fused_mixer as fm
    m = _mixer(4, C, Ch=Ch, seed=C + Ch).to(DEV)
    x, gy = _inputs(n, C, seed=n)
    x, gy = x.reshape(1, n, C), gy.reshape(1, n, C)                                     # [..., C]
    params = _params(m)
    m64 = copy.deepcopy(m).double().cpu()
    x64 = x.double().cpu().requires_grad_(True)
    want = torch.autograd.grad(_channel_torch(m64, x64), (x64,) + _params(m64), gy.double().cpu())
    ref = _ref64(m, x[0], gy[0])
    assert float((want[0][0] - ref[1]).abs().max()) <= 1e-9 * max(1.0, float(ref[1].abs().max()))   # the expressions ARE the gradient
    for a, b in zip(want[1:], ref[2]):
        assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max()))
    ref = (None, want[0][0].detach(), [w.detach() for w in want[1:]], ref[3], ref[4])
    before = dict(fm.calls)
    xr = x.clone().requires_grad_(True)
    y = fm.channel_train(m, xr, 0.0)
    assert y.shape == x.shape and y.requires_grad and fm.calls["channel_train"] == before["channel_train"] + 1
    assert fm.calls["channel_bwd"] == before["channel_bwd"]
    got = torch.autograd.grad(y, (xr,) + params, gy)
    assert fm.calls["channel_bwd"] == before["channel_bwd"] + 1
    assert all(fm.calls[k] == before[k] for k in ("token", "channel", "token_train", "token_bwd"))
    _check(f"autograd C {C} Ch {Ch} rows {n}", got[0][0], got[1:], ref)
    # frozen Parameters and a plain input: None for those, the same bits for the others
    ffn = m.channel_feedforward.ffn
    ffn[0].weight.requires_grad_(False)
    m.channel_norm.bias.requires_grad_(False)
    y = fm.channel_train(m, x, 0.0)
    y.backward(gy)
    assert ffn[0].weight.grad is None and m.channel_norm.bias.grad is None and x.grad is None
    for i in (0, 3, 4, 5):
        assert torch.equal(params[i].grad, got[1 + i]), NAMES[i]


@pytest.mark.gpu
def test_parameter_updates_are_seen_by_the_next_call():
    """After an optimiser step both images are rewritten (calls["prepare"] moves once) and the next forward and backward run on the
    new weights; an in-place change between forward and backward raises as torch does."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    C, Ch, n = 20, 80, 129
    m = _mixer(4, C, Ch=Ch, seed=5).to(DEV)
    x, gy = _inputs(n, C, seed=9)
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    c0 = dict(fm.calls)
    first = fm.channel_train(m, x, 0.0)
    assert fm.calls["prepare"] == c0["prepare"] + 1
    first.backward(gy)
    assert fm.calls["prepare"] == c0["prepare"] + 1 and fm.cached(m).bimg is not None
    opt.step()
    m.zero_grad(set_to_none=True)
    after = fm.channel_train(m, x, 0.0)
    assert fm.calls["prepare"] == c0["prepare"] + 2 and not torch.equal(after, first)
    with torch.no_grad():
        want = _channel_torch(m, x)
    assert _scaled_err(after.detach().cpu().numpy(), want.cpu().numpy()) <= 2e-5
    after.backward(gy)
    got = [t.grad for t in _params(m)]
    _check("after an optimiser step", None, got, _ref64(m, x, gy))
    y = fm.channel_train(m, x, 0.0)
    with torch.no_grad():
        m.channel_feedforward.ffn[0].weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(gy)


@pytest.mark.gpu
def test_no_rows_and_a_changed_partial_count(monkeypatch):
    """An empty input gives an empty output, an empty gx and zeros for the six Parameters, with nothing launched; raising
    fused_mixer.CHANNEL_PARTIALS after a backward sizes a new partial buffer (63 parts of 188 tiles) and gives gradients at the
    same bounds."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    C, Ch = 20, 80
    m = _mixer(4, C, Ch=Ch, seed=3).to(DEV)
    x = torch.empty(0, C, device=DEV).requires_grad_(True)
    c0 = dict(fm.calls)
    y = fm.channel_train(m, x, 0.1)
    assert y.shape == (0, C) and y.requires_grad
    y.backward(torch.empty(0, C, device=DEV))
    assert x.grad.shape == (0, C) and fm.calls["channel_train"] == c0["channel_train"] and fm.calls["channel_bwd"] == c0["channel_bwd"]
    for t in _params(m):
        assert t.grad is not None and t.grad.shape == t.shape and not bool(t.grad.any())
    x, gy = _inputs(6000, C, seed=4)
    ref = _ref64(m, x, gy)
    for parts in (32, 64):
        monkeypatch.setattr(fm, "CHANNEL_PARTIALS", parts)
        m.zero_grad(set_to_none=True)
        fm.channel_train(m, x, 0.0).backward(gy)
        _check(f"CHANNEL_PARTIALS {parts}", None, [t.grad for t in _params(m)], ref)


def _grads_of(emb, arrays):
    emb.zero_grad(set_to_none=True)
    emb.embed_from_features(*arrays).sum().backward()
    return {k: p.grad.clone() for k, p in emb.named_parameters() if p.grad is not None}


@pytest.mark.gpu
def test_dispatch_on_g11(golden_dir):
    """Call counters on G11's embedding module: channel_train / channel_bwd serve exactly when the switch is on and a gradient is
    recorded, with fused_token_training on and off; never under no_grad, never on the default switches."""
    _need_gpu()
    g = _g11(golden_dir)
    from tpnet_amd import fused_mixer as fm
    emb, arrays = _stage(g, 0.0)
    emb.train()
    layers = len(emb.mlp_mixers)
    moved = lambda c0: {k: fm.calls[k] - c0[k] for k in fm.calls if fm.calls[k] != c0[k]}
    c0 = dict(fm.calls)
    _grads_of(emb, arrays)                                                              # the default switches: torch
    assert moved(c0) == {}
    emb.fused_channel_training = True
    for token in (False, True):
        emb.fused_token_training = token
        c0 = dict(fm.calls)
        out = emb.embed_from_features(*arrays)
        want = {"channel_train": layers, **({"token_train": layers} if token else {})}
        assert out.requires_grad and {k: v for k, v in moved(c0).items() if k != "prepare"} == want
        assert moved(c0).get("prepare", 0) in (0, layers)                               # (the images, on the first call only)
        c1 = dict(fm.calls)
        out.sum().backward()
        assert moved(c1) == {"channel_bwd": layers, **({"token_bwd": layers} if token else {})}
        c2 = dict(fm.calls)
        with torch.no_grad():
            emb.embed_from_features(*arrays)                                            # no gradient: fused_mixer's kernels
        assert moved(c2) == {"token": layers, "channel": layers}
    emb.eval()                                                                          # eval mode with a gradient: rate 0, same route
    c3 = dict(fm.calls)
    _grads_of(emb, arrays)
    assert moved(c3) == {"channel_train": layers, "channel_bwd": layers, "token_train": layers, "token_bwd": layers}
    emb.fused_channel_training = False
    emb.fused_token_training = False
    c4 = dict(fm.calls)
    _grads_of(emb, arrays)
    assert moved(c4) == {}


@pytest.mark.gpu
def test_g11_end_to_end_gradients(golden_dir):
    """G11 at dropout 0: the gradients of embeddings.sum() for all 30 Parameters with the switch on against off (the torch layers
    are the reference), scaled as test_encoder_module._scaled_err scales: within G11_BOUND."""
    _need_gpu()
    g = _g11(golden_dir)
    emb, arrays = _stage(g, 0.0)
    emb.train()
    off = _grads_of(emb, arrays)
    emb.fused_channel_training = True
    on = _grads_of(emb, arrays)
    print(f"G11: {len(off)} Parameters with a gradient")
    assert set(on) == set(off) and len(off) == 30
    worst = {k: _scaled_err(on[k].cpu().numpy(), off[k].cpu().numpy()) for k in off}
    top = max(worst, key=worst.get)
    print(f"G11 gradients, fused_channel_training on against off: worst scaled difference {worst[top]:.3e} ({top})")
    assert G11_BOUND < 1e-4 and worst[top] <= G11_BOUND
