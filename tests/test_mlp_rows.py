"""tpnet_mlp_rows_f32 (csrc/mlp_rows.hip): self.mlp = Linear(F, 4F) -> ReLU -> Linear(4F, F) on the matrix cores for num_layer 1 and 2
(F = 16 and 36), in the project's fp32 class -- the kernel through the C entry, then through RandomProjectionModule._apply_mlp.

Bounds: bit equality on small integers (every product and partial sum is exact in two bf16 pieces and an fp32 accumulator); 2e-5 of
the output scale against the torch layers on real-valued data (C_DENSE: mfma_split.hpp, tests/test_host_routes.py).

A row of x that holds a NaN: nothing is asserted about THAT row of y -- relu_split16 maps a NaN hidden unit to 0 where torch's
ReLU keeps it -- only that every other row keeps its bits."""
import os

import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, _module, _need_gpu, _random_stream

pytestmark = pytest.mark.gpu

C_DENSE = 2e-5
WIDTHS = [(1, 16), (2, 36)]
# The launch's grid rule (launch_mlp_rows_l): at most 512 workgroups of 8 waves, one 32-row tile per wave and round -- a wave walks
# more than one tile from 512 * 8 * 32 = 131 072 rows on.  140 001 rows are 4 376 tiles: 280 waves walk two, the last tile holds one row.
N_LIST = (1, 31, 32, 33, 1000, 4099, 140001)


def _layers(F, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(F, 4 * F), torch.nn.ReLU(), torch.nn.Linear(4 * F, F)).to(DEV)


def _call(mlp, x, y=None):
    """tpnet_mlp_rows_f32 on x [n, F] (any view whose data_ptr is the first row); returns (rc, y)."""
    from tpnet_amd import _dense, _lib
    from tpnet_amd import fused_feature as ff
    n, F = x.shape
    prep = ff.prepared(mlp, F)
    assert prep is not None and prep.st.F == F and not prep.st.w1 and not prep.st.w2f and not prep.st.wimg
    if y is None:
        y = torch.empty((n, F), dtype=torch.float32, device=x.device)
    rc = _lib.load().tpnet_mlp_rows_f32(x.data_ptr(), n, prep.ref, y.data_ptr(), _dense.stream_ptr(x.device))
    return rc, y


@pytest.mark.parametrize("L,F", WIDTHS)
def test_exact_on_small_integers(L, F):
    """Asymmetric small-integer weights and inputs: the kernel must equal the fp32 torch layers bit for bit -- pins the lane, register
    and slice mapping, the zero padding of the weight image and the masks of the loads and stores."""
    _need_gpu()
    g = torch.Generator().manual_seed(F)
    mlp = _layers(F)
    with torch.no_grad():
        mlp[0].weight.copy_(torch.randint(-3, 4, (4 * F, F), generator=g).float())
        mlp[0].bias.copy_(torch.randint(-8, 9, (4 * F,), generator=g).float())
        mlp[2].weight.copy_((torch.randint(-3, 4, (F, 4 * F), generator=g) * (torch.rand(F, 4 * F, generator=g) < 0.5)).float())
        mlp[2].bias.copy_(torch.randint(-8, 9, (F,), generator=g).float())
    # |hidden| <= 36 * 9 + 8 = 332 (9 bits: exact in two bf16 pieces), |output| <= 144 * 332 * 3 + 8 < 2^18: far below 2^24
    for n in N_LIST:
        x = torch.randint(0, 4, (n, F), generator=g).float().to(DEV)
        with torch.no_grad():
            want = mlp(x)
        rc, got = _call(mlp, x)
        assert rc == 0
        assert torch.equal(got, want), f"n={n}: max |delta| {(got - want).abs().max().item()}"


@pytest.mark.parametrize("L,F", WIDTHS)
def test_fp32_class_and_run_to_run_bits(L, F):
    _need_gpu()
    mlp = _layers(F, seed=F)                                             # nn.Linear's default init
    g = torch.Generator().manual_seed(100 + F)
    for n in N_LIST:
        # the readout's features are log1p of non-negative Gram entries: 0 .. 20 here, with exact zeros
        v = torch.expm1(torch.rand(n, F, generator=g, dtype=torch.float64) * 20.0) * (torch.rand(n, F, generator=g) < 0.9)
        x = torch.log1p(v).float().to(DEV)
        with torch.no_grad():
            want = mlp(x)
        rc, got = _call(mlp, x)
        rc2, again = _call(mlp, x)
        assert rc == 0 and rc2 == 0
        err, scale = (got - want).abs().max().item(), max(1.0, want.abs().max().item())
        print(f"F={F} n={n}: max |delta| {err:.3e} = {err / scale:.3e} of the scale {scale:.3f}")
        assert err <= C_DENSE * scale, (n, err, scale)
        assert torch.equal(got, again), n


@pytest.mark.parametrize("L,F", WIDTHS)
@pytest.mark.parametrize("n", [33, 1000])
def test_nothing_is_read_past_a_row_or_the_list_and_nothing_written_past_it(L, F, n):
    _need_gpu()
    mlp = _layers(F, seed=7 * F)
    g = torch.Generator().manual_seed(n + F)
    plain = (torch.rand(n, F, generator=g) * 12.0).to(DEV)
    _, want = _call(mlp, plain)
    assert torch.isfinite(want).all()
    # x = the first n * F floats of a larger tensor whose remaining floats are NaN; y = the first n rows of a tensor of sentinels
    big = torch.full(((n + 40) * F,), float("nan"), device=DEV)
    big[: n * F] = plain.reshape(-1)
    ybig = torch.full((n + 40, F), -777.25, device=DEV)
    rc, _ = _call(mlp, big[: n * F].view(n, F), ybig)
    assert rc == 0
    assert torch.isfinite(ybig[:n]).all() and torch.equal(ybig[:n], want)
    assert (ybig[n:] == -777.25).all()
    # a NaN row stays in its row: an interior one, then the last one (the row itself: see the header)
    for bad in (n // 2, n - 1):
        x = plain.clone()
        x[bad] = float("nan")
        rc, got = _call(mlp, x)
        assert rc == 0
        keep = torch.ones(n, dtype=torch.bool, device=DEV)
        keep[bad] = False
        assert torch.equal(got[keep], want[keep]), bad


def _updated_module(L, d, N=300):
    rp = _module(N, d, L, 2e-6, 1.0e6)
    src, dst, _, t = _random_stream(np.random.RandomState(10 * L + d), N, 600, 3.0e5)
    for a in range(0, 600, 200):                                         # three updates of 200 edges
        rp.update(src[a:a + 200], dst[a:a + 200], t[a:a + 200])
    return rp


def _recorded(monkeypatch):
    """Wrap the bound library function: the list of row counts it served, without touching the product."""
    from tpnet_amd import _lib
    lib = _lib.load()
    real, seen = lib.tpnet_mlp_rows_f32, []

    def recorder(x, n, mlp, y, stream):
        rc = real(x, n, mlp, y, stream)
        seen.append((int(n), int(rc)))
        return rc

    monkeypatch.setattr(lib, "tpnet_mlp_rows_f32", recorder, raising=True)
    return seen


def _encoder_pattern(rng, N, K=17, rows=241):
    neigh = rng.randint(0, N, (rows, K)).astype(np.int64)
    a1, a2 = rng.randint(1, N, rows).astype(np.int64), rng.randint(1, N, rows).astype(np.int64)
    return np.tile(neigh.reshape(-1), 2), np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])


@pytest.mark.parametrize("L,d", [(1, 64), (2, 64), (1, 140)])
def test_through_the_module(L, d, monkeypatch):
    _need_gpu()
    from tpnet_amd import fused_feature as ff
    F = (2 * L + 2) ** 2
    rp = _updated_module(L, d)
    u, v = _encoder_pattern(np.random.RandomState(L + d), 300)           # 2 * 241 * 17 = 8 194 pairs
    assert len(u) == 8194
    ud, vd = torch.from_numpy(u).to(DEV), torch.from_numpy(v).to(DEV)
    seen = _recorded(monkeypatch)
    with torch.no_grad():
        want = rp.mlp(rp.pair_gram(ud, vd))
        scale = max(1.0, want.abs().max().item())
        # the threshold above n: the unchanged path, bit for bit
        monkeypatch.setitem(ff.MLP_ROWS_FROM, F, len(u) + 1)
        assert torch.equal(rp.get_pair_wise_feature(ud, vd), want)
        monkeypatch.setitem(ff.MLP_ROWS_FROM, F, None)
        assert torch.equal(rp.get_pair_wise_feature(ud, vd), want)
        assert seen == []
        # routed: host arrays in the encoder's pattern, then device ids
        monkeypatch.setitem(ff.MLP_ROWS_FROM, F, 0)
        for a, b in ((u, v), (ud, vd)):
            del seen[:]
            got = rp.get_pair_wise_feature(a, b)
            assert seen == [(8194, 0)], seen
            err = (got - want).abs().max().item()
            print(f"L={L} d={d}: max |delta| {err:.3e} of scale {scale:.3f}")
            assert err <= C_DENSE * scale, (err, scale)
    rp.check_device_errors()


def test_golden_post_mlp_features(golden_dir):
    _need_gpu()
    g = np.load(os.path.join(golden_dir, "g3g4_readout_d140_L1.npz"))
    mlp = _layers(16)
    mlp.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("mlp.")})
    for pre, post in (("gram_scaled", "feat_mlp_scaled"), ("gram_raw", "feat_mlp_raw")):
        x, want = torch.from_numpy(g[pre]).to(DEV), torch.from_numpy(g[post]).to(DEV)
        rc, got = _call(mlp, x)
        assert rc == 0
        err, scale = (got - want).abs().max().item(), max(1.0, want.abs().max().item())
        print(f"{post}: max |delta| {err:.3e} of scale {scale:.3f}")
        assert err <= C_DENSE * scale, (post, err, scale)


@pytest.mark.parametrize("L", [1, 2])
def test_gradients_through_the_module_route(L, monkeypatch):
    """The backward behind the kernel's forward is the fp32 torch expressions on the saved pre-mlp features: the bar of
    tests/test_fused_mlp.py for them (rtol 1e-4, atol 1e-3 against autograd of the torch layers)."""
    _need_gpu()
    from tpnet_amd import fused_feature as ff
    F = (2 * L + 2) ** 2
    rp = _updated_module(L, 64)
    rng = np.random.RandomState(L)
    u, v = torch.from_numpy(rng.randint(0, 300, 1000)).to(DEV), torch.from_numpy(rng.randint(0, 300, 1000)).to(DEV)
    monkeypatch.setitem(ff.MLP_ROWS_FROM, F, 0)
    seen = _recorded(monkeypatch)
    params = list(rp.mlp.parameters())
    gy = torch.randn(1000, F, generator=torch.Generator().manual_seed(L)).to(DEV)
    got = torch.autograd.grad(rp.get_pair_wise_feature(u, v), params, gy)
    assert seen == [(1000, 0)]
    feats = rp.pair_gram(u, v)
    want = torch.autograd.grad(rp.mlp(feats), params, gy)
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-3)
    # a caller's own x that requires grad gets its gradient too
    x = feats.detach().clone().requires_grad_(True)
    y = rp._apply_mlp(x)
    assert seen[-1] == (1000, 0) and len(seen) == 2
    gx, = torch.autograd.grad(y, [x], gy)
    x2 = feats.detach().clone().requires_grad_(True)
    gx_want, = torch.autograd.grad(rp.mlp(x2), [x2], gy)
    torch.testing.assert_close(gx, gx_want, rtol=1e-4, atol=1e-3)
    rp.check_device_errors()


@pytest.mark.parametrize("L", [3, 4])
def test_unserved_widths_keep_their_route(L, monkeypatch):
    _need_gpu()
    from tpnet_amd import _dense, _lib
    from tpnet_amd import fused_feature as ff
    F = (2 * L + 2) ** 2
    rp = _updated_module(L, 64)
    seen = _recorded(monkeypatch)
    rng = np.random.RandomState(L)
    u, v = torch.from_numpy(rng.randint(0, 300, 9000)).to(DEV), torch.from_numpy(rng.randint(0, 300, 9000)).to(DEV)
    with torch.no_grad():
        feats = rp.pair_gram(u, v)
        got = rp._apply_mlp(feats)
        assert seen == []
        if L == 4:
            # (100, 400): the C entry refuses, and the module's output is torch's, bit for bit
            assert torch.equal(got, rp.mlp(feats))
            prep = ff.prepared(rp.mlp, F)
            y = torch.empty_like(feats)
            assert _lib.load().tpnet_mlp_rows_f32(feats.data_ptr(), feats.shape[0], prep.ref, y.data_ptr(), _dense.stream_ptr(feats.device)) == -1
    rp.check_device_errors()
