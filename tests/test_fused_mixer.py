"""The opt-in two-launch MLP-Mixer layer (tpnet_amd/fused_mixer.py, csrc/mixer.hip, TPNetEmbedding.fused_mixer) against the
module's own torch layers on the same device, and end to end against fixture G11."""
import numpy as np
import pytest
import torch

from test_encoder_module import _fixture_stage, _g11, _model, _need_gpu, _replay, _samplers, _scaled_err

DEV = "cuda:0"


def _mixer(K, C, Kh=None, Ch=None, eps=1e-5, dropout=0.0, seed=0):
    """tpnet_amd.MLPMixer(K, C) with hidden widths Kh / Ch (default: the reference's K / 2 and 4 C), LayerNorms of `eps`, and
    non-trivial gamma / beta."""
    import tpnet_amd
    nn = torch.nn
    torch.manual_seed(seed)
    m = tpnet_amd.MLPMixer(num_tokens=K, num_channels=C, dropout=dropout)
    ffn = lambda a, b: nn.Sequential(nn.Linear(a, b), nn.GELU(), nn.Dropout(dropout), nn.Linear(b, a), nn.Dropout(dropout))
    if Kh is not None:
        m.token_feedforward.ffn = ffn(K, Kh)
    if Ch is not None:
        m.channel_feedforward.ffn = ffn(C, Ch)
    m.token_norm, m.channel_norm = nn.LayerNorm(K, eps=eps), nn.LayerNorm(C, eps=eps)
    with torch.no_grad():
        for ln in (m.token_norm, m.channel_norm):
            ln.weight.uniform_(0.5, 1.5)
            ln.bias.normal_(0, 0.3)
    return m.eval()


def _token_torch(m, x):
    return m.token_feedforward(m.token_norm(x.permute(0, 2, 1))).permute(0, 2, 1) + x


def _channel_torch(m, x):
    return m.channel_feedforward(m.channel_norm(x)) + x


# ---------------------------------------------------------------------------------------------------------------- CPU tier

def test_supported_and_image_bytes_are_host_arithmetic(hip_lib):
    L = hip_lib
    for dims in ((20, 10, 172, 688), (6, 3, 20, 80), (2, 1, 4, 1), (32, 16, 256, 1024)):
        assert L.tpnet_mixer_supported(*dims) == 1, dims
        nbytes = L.tpnet_mixer_channel_image_bytes(dims[2], dims[3])
        assert nbytes > 0 and nbytes % 16 == 0, dims
    for dims in ((1, 10, 172, 688), (20, 0, 172, 688), (33, 10, 172, 688), (20, 10, 174, 688), (20, 10, 260, 688), (20, 10, 172, 1025)):
        assert L.tpnet_mixer_supported(*dims) == 0, dims
    for C, Ch in ((174, 688), (260, 688), (172, 1025), (0, 8), (172, 0)):
        assert L.tpnet_mixer_channel_image_bytes(C, Ch) == 0, (C, Ch)
    # 172 -> 688 -> 172: 3 passes of 8 hidden slices over 11 k-steps, 6 output tiles, chunks of 1 536 16-byte elements, padded biases
    assert L.tpnet_mixer_channel_image_bytes(172, 688) == 3 * (11 + 8) * 1536 * 16 + (24 + 6) * 32 * 4
    assert L.tpnet_mixer_channel_image_bytes(20, 80) == (2 + 11) * 1536 * 16 + (11 + 6) * 32 * 4
    assert L.tpnet_mixer_channel_image_bytes(256, 1024) == 4 * (16 + 8) * 2048 * 16 + (32 + 8) * 32 * 4


def test_bad_arguments_return_without_a_gpu(hip_lib):
    """Null pointers, out == x, misaligned arrays and unserved sizes: -1 (TPNET_ERR_BAD_ARG), nothing launched."""
    L = hip_lib
    assert L.tpnet_mixer_channel_prepare(None, 16, 16, 16, 172, 688, 16, None) == -1
    assert L.tpnet_mixer_channel_prepare(16, 16, 16, 16, 172, 688, None, None) == -1
    assert L.tpnet_mixer_channel_prepare(16, 16, 16, 16, 172, 688, 24, None) == -1      # image not 16-byte aligned
    assert L.tpnet_mixer_channel_prepare(16, 16, 16, 16, 174, 688, 16, None) == -1
    tok = [16, 5, 20, 172, 16, 16, 1e-5, 16, 16, 10, 16, 16, 32, None]
    for i in (0, 4, 5, 7, 8, 10, 11, 12):                                                # every pointer null in turn
        a = list(tok)
        a[i] = None
        assert L.tpnet_mixer_token(*a) == -1, i
    for i, v in ((12, 16), (0, 20), (4, 18), (1, -1), (2, 1), (2, 33), (9, 0), (9, 33), (3, 174), (1, 1 << 40)):
        a = list(tok)
        a[i] = v
        assert L.tpnet_mixer_token(*a) == -1, (i, v)
    ch = [16, 100, 172, 688, 16, 16, 1e-5, 16, 32, None]
    for i in (0, 4, 5, 7, 8):
        a = list(ch)
        a[i] = None
        assert L.tpnet_mixer_channel(*a) == -1, i
    for i, v in ((8, 16), (0, 24), (4, 20), (7, 8), (1, -1), (2, 174), (2, 260), (3, 1025), (3, 0), (1, 1 << 40)):
        a = list(ch)
        a[i] = v
        assert L.tpnet_mixer_channel(*a) == -1, (i, v)
    tok[1], ch[1] = 0, 0                                                                 # nothing to do: TPNET_OK, nothing launched
    assert L.tpnet_mixer_token(*tok) == 0 and L.tpnet_mixer_channel(*ch) == 0


def test_layers_of_is_a_structural_test():
    import tpnet_amd
    from tpnet_amd import fused_mixer as fm
    nn = torch.nn
    ls = fm.layers_of(tpnet_amd.MLPMixer(20, 172, dropout=0.1))
    assert ls is not None and ls.dropout == 0.1
    assert (ls.token[0].in_features, ls.token[0].out_features, ls.channel[0].in_features, ls.channel[0].out_features) == (20, 10, 172, 688)
    assert fm.layers_of(_mixer(6, 20, Kh=5, Ch=33)) is not None

    class Duck(nn.Module):                       # another class with the four attributes: accepted
        def __init__(self):
            super().__init__()
            src = tpnet_amd.MLPMixer(6, 20)
            self.token_norm, self.token_feedforward = src.token_norm, src.token_feedforward
            self.channel_norm, self.channel_feedforward = src.channel_norm, src.channel_feedforward
    assert fm.layers_of(Duck()) is not None
    m = tpnet_amd.MLPMixer(20, 172)
    m.channel_feedforward.ffn[1] = nn.GELU(approximate="tanh")
    assert fm.layers_of(m) is None
    m = tpnet_amd.MLPMixer(20, 172)
    m.token_norm = nn.LayerNorm(20, elementwise_affine=False)
    assert fm.layers_of(m) is None
    m = tpnet_amd.MLPMixer(20, 172)
    m.token_feedforward.ffn[3] = nn.Linear(10, 20, bias=False)
    assert fm.layers_of(m) is None
    m = tpnet_amd.MLPMixer(20, 172)
    m.channel_feedforward.ffn[3] = nn.Linear(680, 172)                                   # hidden width 688 != 680
    assert fm.layers_of(m) is None
    m = tpnet_amd.MLPMixer(20, 172)
    m.channel_norm = nn.LayerNorm(100)                                                   # a norm of another width
    assert fm.layers_of(m) is None
    assert fm.layers_of(nn.Identity()) is None and fm.prepared(nn.Identity()) is None
    assert not fm.supported(tpnet_amd.MLPMixer(20, 172))                                 # CPU Parameters
    assert fm.prepared(tpnet_amd.MLPMixer(20, 172)) is None and fm.cached(m) is None


def test_switch_defaults_to_off_and_a_cpu_model_ignores_it(golden_dir):
    import tpnet_amd
    from tpnet_amd import fused_mixer as fm
    assert tpnet_amd.TPNetEmbedding.fused_mixer is False
    g = _g11(golden_dir)
    model, _ = _model(g, "cpu")
    model.eval()
    emb = model.embedding_module
    args = (g["c0_neigh"], g["c0_eids"], g["c0_tn"], np.tile(g["c0_t"], 2), torch.from_numpy(g["c0_feat"]))
    before = dict(fm.calls)
    with torch.no_grad():
        off = emb.embed_from_features(*args)
        emb.fused_mixer = True
        on = emb.embed_from_features(*args)
    assert torch.equal(on, off) and fm.calls == before


# ---------------------------------------------------------------------------------------------------------------- GPU tier

def _token_input(n, K, C, seed):
    """[n, K, C] normal; the columns of one node constant over the tokens (variance 0), one node offset by +1000 (with a single
    node: half of its channels each)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, K, C, generator=gen)
    if n == 1:
        x[0, :, :C // 2] = x[0, :1, :C // 2]
        x[0, :, C // 2:] += 1000.0
    else:
        x[0] = x[0, :1]
        x[n - 1] += 1000.0
    return x.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("K,C", [(20, 172), (6, 20), (2, 4), (32, 256), (10, 100)])
@pytest.mark.parametrize("n", [1, 7, 300])
def test_token_kernel_matches_torch(n, K, C):
    """Exact fp32 against the torch layers: the project's true-fp32 tolerance (rtol 1e-4, atol 1e-5); a repeated call is bitwise
    equal."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(K, C, seed=K + C).to(DEV)
    x = _token_input(n, K, C, seed=n)
    with torch.no_grad():
        want = _token_torch(m, x)
    before = fm.calls["token"]
    got = fm.mixer_token(m, x)
    assert fm.calls["token"] == before + 1 and got.shape == want.shape and got.data_ptr() != x.data_ptr()
    print(f"token kernel n {n} K {K} C {C}: scaled err {_scaled_err(got.cpu().numpy(), want.cpu().numpy()):.3e}, "
          f"max abs diff {float((got - want).abs().max()):.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-5)
    assert torch.equal(got, fm.mixer_token(m, x))


CHANNEL_SHAPES = [(172, 688), (20, 80), (64, 256), (100, 353), (256, 1024), (4, 1)]


def _channel_input(n, C, seed):
    """[n, C] normal; from the middle on rows of mean 50 and spread 1; with more than one row, row 0 constant (variance 0).  The
    constant is 0.0 because the exact answer, beta, is then also what every summation order gives: torch's LayerNorm on the GPU
    combines partial means as (nA / n) mean_A + (nB / n) mean_B with rounded weights, which need not return 3.0 for a row of 3.0,
    and 1 / sqrt(eps) = 316 turns one ulp of the reference's mean (2.4e-7) into 7.5e-5 of a normalised value.  Measured on an
    MI355X at C = 100, rows of 3.0: torch's LayerNorm is 3.4e-4 off beta and its layer 1.2e-4 off an fp64 evaluation, the kernel
    1.2e-6; at the other widths of this file torch returns beta exactly (profiles/mixer.md).
    The kernel's own handling of constant rows of other values: test_channel_kernel_constant_rows."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=gen)
    x[n // 2:] += 50.0
    if n > 1:
        x[0] = 0.0
    return x.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("C,Ch", CHANNEL_SHAPES)
def test_channel_kernel_matches_torch(C, Ch):
    """fp32 class against the torch layers, every row count of tile and workgroup tails: err <= 2e-5 * max(1, max|want|), the bound
    mfma_split.hpp states.  The worst per shape is printed (profiles/mixer.md keeps the figures)."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(4, C, Ch=Ch, seed=C + Ch).to(DEV)
    prep = fm.prepared(m)
    assert prep is not None and prep.dims == (4, 2, C, Ch)
    worst = 0.0
    for n in (1, 33, 127, 128, 129, 6000):
        x = _channel_input(n, C, seed=n)
        with torch.no_grad():
            want = _channel_torch(m, x)
        got = fm.mixer_channel(prep, m, x)
        assert got.shape == want.shape and got.data_ptr() != x.data_ptr()
        err = _scaled_err(got.cpu().numpy(), want.cpu().numpy())
        plain = _scaled_err(got[:n // 2].cpu().numpy(), want[:n // 2].cpu().numpy()) if n > 1 else 0.0
        print(f"channel kernel C {C} Ch {Ch} rows {n}: scaled err {err:.3e} (rows of mean 0 alone: {plain:.3e})")
        worst = max(worst, err, plain)
        assert torch.equal(got, fm.mixer_channel(prep, m, x))
    print(f"channel kernel C {C} Ch {Ch}: worst scaled err {worst:.3e}")
    assert worst <= 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("C,Ch", CHANNEL_SHAPES)
def test_channel_kernel_constant_rows(C, Ch):
    """A constant row of any value v normalises to beta, so its output is v + FFN(beta): against the row of zeros (which
    test_channel_kernel_matches_torch compares with torch) the only difference allowed is the rounding of the final + v, half an ulp
    of the output.  The values' row sums are exact in fp32 (few significant bits, C <= 256)."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(4, C, Ch=Ch, seed=C + Ch).to(DEV)
    values = torch.tensor([0.0, 3.0, -7.25, 50.0, 1000.0])
    x = values[:, None].expand(-1, C).contiguous().to(DEV)
    got = fm.mixer_channel(fm.prepared(m), m, x).cpu().double()
    dev = ((got - values[:, None].double()) - got[:1]).abs()
    print(f"channel kernel C {C} Ch {Ch}, constant rows: worst deviation from the row of zeros {float(dev.max()):.3e}")
    assert bool((dev <= 2.0 ** -24 * got.abs()).all())


@pytest.mark.gpu
def test_layernorm_eps_is_honoured():
    """LayerNorms with eps = 1e-3 on inputs of spread 0.03 (variance 9e-4: the eps term halves the normalised values)."""
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    gen = torch.Generator().manual_seed(5)
    x = (0.03 * torch.randn(40, 20, 172, generator=gen)).to(DEV)
    m, m5 = _mixer(20, 172, eps=1e-3, seed=1).to(DEV), _mixer(20, 172, eps=1e-5, seed=1).to(DEV)
    with torch.no_grad():
        want_t, want_c = _token_torch(m, x), _channel_torch(m, x)
        other_t, other_c = _token_torch(m5, x), _channel_torch(m5, x)
    assert float((want_t - other_t).abs().max()) > 1e-2 and float((want_c - other_c).abs().max()) > 1e-2
    got_t, got_c = fm.mixer_token(m, x), fm.mixer_channel(fm.prepared(m), m, x)
    np.testing.assert_allclose(got_t.cpu().numpy(), want_t.cpu().numpy(), rtol=1e-4, atol=1e-5)
    err = _scaled_err(got_c.cpu().numpy(), want_c.cpu().numpy())
    print(f"eps 1e-3, channel kernel: scaled err {err:.3e}")
    assert err <= 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,C", [(50, 20, 172), (9, 6, 20)])
def test_whole_layer_matches_torch(n, K, C):
    _need_gpu()
    from tpnet_amd import fused_mixer as fm
    m = _mixer(K, C, seed=3).to(DEV)
    x = torch.randn(n, K, C, generator=torch.Generator().manual_seed(n)).to(DEV)
    with torch.no_grad():
        want = m(x)
    before = dict(fm.calls)
    prep = fm.prepared(m)
    got = fm.mixer_forward(prep, m, x)
    assert fm.calls["token"] == before["token"] + 1 and fm.calls["channel"] == before["channel"] + 1
    assert fm.calls["prepare"] == before["prepare"] + 1 and fm.cached(m) is prep
    err = _scaled_err(got.cpu().numpy(), want.cpu().numpy())
    print(f"whole layer n {n} K {K} C {C}: scaled err {err:.3e}")
    assert err <= 2e-5
    assert torch.equal(got, fm.mixer_forward(fm.prepared(m), m, x)) and fm.calls["prepare"] == before["prepare"] + 1
    fm.invalidate(m)
    assert fm.cached(m) is None


# The bound on the embeddings of G11's two calls with the fused mixers on (both sampler kinds, fused_input on and off) is, as in
# test_encoder_module.py, 3x the worst scaled deviation measured on an MI355X -- the kernels are deterministic, the margin covers
# compiler and machine differences -- and may not exceed 1e-4.  G11_MIXER_MEASURED is that measurement: 8.73e-6 with fused_input
# on, 2.68e-6 with it off, the same for both sampler kinds (the input-stage kernel with torch mixers behind it measured 7.97e-6).
G11_MIXER_MEASURED = 8.73e-6
G11_MIXER_BOUND = 3 * G11_MIXER_MEASURED


@pytest.mark.gpu
@pytest.mark.parametrize("fused_input", [True, False])
@pytest.mark.parametrize("kind", ["host", "device"])
def test_g11_end_to_end_with_fused_mixers(golden_dir, kind, fused_input):
    """Under no_grad in eval mode both mixers of both calls take the two kernels (call counters); embeddings against the fixture."""
    _need_gpu()
    assert G11_MIXER_BOUND <= 1e-4
    g = _g11(golden_dir)
    from tpnet_amd import fused_mixer as fm
    model, rp = _model(g, DEV, _samplers(g, kind))
    model.embedding_module.fused_input = fused_input
    model.embedding_module.fused_mixer = True
    model.eval()
    before = dict(fm.calls)
    outs = _replay(g, model, rp, 1)
    layers = int(g["mixers"])
    assert fm.calls["token"] == before["token"] + 2 * layers and fm.calls["channel"] == before["channel"] + 2 * layers
    assert fm.calls["prepare"] == before["prepare"] + layers
    worst = 0.0
    for c, (es, ed) in enumerate(outs):
        worst = max(worst, _scaled_err(es.cpu().numpy(), g[f"c{c}_emb_src"]), _scaled_err(ed.cpu().numpy(), g[f"c{c}_emb_dst"]))
    print(f"G11 with fused mixers, {kind} sampler, fused_input {fused_input}: worst scaled err {worst:.3e} (bound {G11_MIXER_BOUND:.3e})")
    assert worst <= G11_MIXER_BOUND
    model.embedding_module.check_device_errors()


@pytest.mark.gpu
def test_default_switch_moves_no_counter(golden_dir):
    _need_gpu()
    g = _g11(golden_dir)
    from tpnet_amd import fused_mixer as fm
    model, rp = _model(g, DEV, _samplers(g, "device"))
    model.eval()
    before = dict(fm.calls)
    _replay(g, model, rp, 1)
    assert fm.calls == before


def _stage(g, dropout):
    """G11's embedding module with `dropout` (eval mode, fused_mixer on) and the recorded arrays of call 1 on the device."""
    model, _ = _model(g, DEV, dropout=dropout)
    model.eval()
    emb = model.embedding_module
    emb.fused_mixer = True
    return emb, _fixture_stage(g, 1)[1]


@pytest.mark.gpu
def test_dispatch_by_grad_mode_and_dropout(golden_dir):
    """Call counters, not timing: gradients recorded or an active dropout take the torch layers; train mode with dropout 0 under
    no_grad takes the kernels."""
    _need_gpu()
    g = _g11(golden_dir)
    from tpnet_amd import fused_mixer as fm
    emb, arrays = _stage(g, 0.1)
    layers = len(emb.mlp_mixers)
    with torch.no_grad():
        emb.embed_from_features(*arrays)
    with torch.inference_mode():
        emb.embed_from_features(*arrays)
    c0 = dict(fm.calls)
    e = emb.embed_from_features(*arrays)                                   # grad enabled: the torch layers
    assert fm.calls == c0 and e.requires_grad
    emb.train()
    with torch.no_grad():
        emb.embed_from_features(*arrays)                                   # dropout 0.1 in train mode: torch's dropout
    assert fm.calls == c0
    emb.eval()
    with torch.no_grad():
        emb.embed_from_features(*arrays)
    assert fm.calls["token"] == c0["token"] + layers and fm.calls["channel"] == c0["channel"] + layers
    emb, arrays = _stage(g, 0.0)
    emb.train()
    c0 = dict(fm.calls)
    with torch.no_grad():
        emb.embed_from_features(*arrays)                                   # dropout 0 in train mode: nothing to keep
    assert fm.calls["token"] == c0["token"] + layers and fm.calls["channel"] == c0["channel"] + layers


@pytest.mark.gpu
def test_parameter_updates_are_seen(golden_dir):
    """After an optimiser step over all mixer Parameters the next no_grad call prepares each layer's image once more and runs on
    the new weights -- the token FFN's and the LayerNorms', read in place, included; a call without a change re-prepares nothing."""
    _need_gpu()
    g = _g11(golden_dir)
    from tpnet_amd import fused_mixer as fm
    emb, arrays = _stage(g, 0.0)
    layers = len(emb.mlp_mixers)
    with torch.no_grad():
        first = emb.embed_from_features(*arrays)
        emb.embed_from_features(*arrays)
    p0 = fm.calls["prepare"]
    emb.train()
    opt = torch.optim.SGD(emb.mlp_mixers.parameters(), lr=0.05)
    emb.embed_from_features(*arrays).square().sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in emb.mlp_mixers.parameters())
    opt.step()
    emb.eval()
    assert fm.calls["prepare"] == p0
    with torch.no_grad():
        after = emb.embed_from_features(*arrays)
        assert fm.calls["prepare"] == p0 + layers
        again = emb.embed_from_features(*arrays)
        assert fm.calls["prepare"] == p0 + layers
        emb.fused_mixer = False
        want = emb.embed_from_features(*arrays)
    assert not torch.equal(after, first) and torch.equal(after, again)
    err = _scaled_err(after.cpu().numpy(), want.cpu().numpy())
    print(f"fused mixers vs torch layers after an optimiser step: scaled err {err:.3e}")
    assert err <= 2e-5
