"""tpnet_mlp_rows_bwd_f32 (csrc/mlp_rows_bwd.hip): the weight gradients of self.mlp = Linear(F, 4F) -> ReLU -> Linear(4F, F) on the
matrix cores for num_layer 1 and 2 (F = 16 and 36), in the project's fp32 class -- the kernel through the C entry, then through
fused_feature.weight_grads_f32 behind autograd and RandomProjectionModule.

Bounds: bit equality on small integers (every product and partial sum is exact in two bf16 pieces and an fp32 accumulator); on
real-valued data the bound of tests/test_fused_mlp.py::test_mlp_backward_in_the_fp32_class against the float64 expressions --
4e-5 of the sum of the terms' magnitudes (2^-16 per product of two-piece operands, in gH = W2^T gY and in the contractions over
the rows; the pre-activations are exact f32), plus what a ReLU that flips at a pre-activation that is zero up to rounding moves,
plus 1e-6 of the largest entry.  Observed on an MI355X (profiles/mlp_rows.md): at most 0.125 of that bound at F = 16 and 0.176 at F = 36 (n = 33,
gW1); through autograd against the torch layers at most 0.118 of the two-sided bound (F = 36, mlp_f32)."""
import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, _module, _need_gpu, _random_stream

pytestmark = pytest.mark.gpu

WIDTHS = [(1, 16), (2, 36)]
NAMES = ("gW1", "gb1", "gW2", "gb2")


def _layers(F, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(F, 4 * F), torch.nn.ReLU(), torch.nn.Linear(4 * F, F)).to(DEV)


def _partial_floats(F):
    from tpnet_amd import _lib
    pf = int(_lib.load().tpnet_mlp_rows_bwd_partial_floats(F, 4 * F))
    assert pf == 2 * 4 * F * F + 4 * F == {16: 2112, 36: 10512}[F]
    return pf


def _call(mlp, x, gy, n_partial=256, part=None, n=None, x_ptr=None, ref=None):
    """tpnet_mlp_rows_bwd_f32 on x, gy [n, F] (any views whose data_ptr is the first row); returns (rc, partial [n_partial, pf])."""
    from tpnet_amd import _dense, _lib
    from tpnet_amd import fused_feature as ff
    F = x.shape[1]
    if ref is None:
        prep = ff.prepared(mlp, F)
        assert prep is not None and prep.st.F == F and not prep.st.w1
        ref = prep.ref
    if part is None:
        part = torch.full((max(n_partial, 1), _partial_floats(F)), float("nan"), device=x.device)
    rc = _lib.load().tpnet_mlp_rows_bwd_f32(x.data_ptr() if x_ptr is None else x_ptr, gy.data_ptr(), x.shape[0] if n is None else n, ref,
                                            part.data_ptr(), n_partial, _dense.stream_ptr(x.device))
    return rc, part


def _grads(part, rc, gy, F):
    """(gW1, gb1, gW2, gb2) from the first rc partials, summed as _dense.mlp64_bwd sums them."""
    H = 4 * F
    tot = part[:rc].sum(0)
    return tot[:H * F].view(H, F), tot[2 * H * F:], tot[H * F:2 * H * F].view(F, H), gy.sum(0)


def _float64_checks(mlp, x, gy):
    """[(want, magnitude, ReLU-flip allowance)] of gW1, gb1, gW2, gb2 from the float64 expressions: the construction of
    test_mlp_backward_in_the_fp32_class (near, ghm, hm)."""
    w1, b1, w2 = mlp[0].weight.detach().double(), mlp[0].bias.detach().double(), mlp[2].weight.detach().double()
    xd, gd = x.double(), gy.double()
    pre = xd @ w1.t() + b1
    on = (pre > 0).double()
    hid = pre * on
    gh = (gd @ w2) * on
    near = (pre.abs() < 1e-4 * (1.0 + xd.abs().max())).double()           # a flip there moves row `unit` of the first layer's gradients
    gha = (gd @ w2).abs()
    ghm = (gd.abs() @ w2.abs()) * on
    hm = (xd.abs() @ w1.abs().t() + b1.abs()) * on
    zero = torch.zeros(x.shape[1], device=x.device, dtype=torch.float64)
    return [(gh.t() @ xd, ghm.t() @ xd.abs(), (gha * near).t() @ xd.abs()),
            (gh.sum(0), ghm.sum(0), (gha * near).sum(0)),
            (gd.t() @ hid, gd.abs().t() @ hm, gd.abs().t() @ (pre.abs() * near)),
            (gd.sum(0), gd.abs().sum(0), zero)]


@pytest.mark.parametrize("L,F", WIDTHS)
def test_exact_on_small_integers(L, F):
    """Small-integer weights, features and output gradients: the four gradients equal autograd's through the fp32 torch layers bit
    for bit, around the 32-row tile and beyond one pass of a 256-partial grid (9 000 rows = 282 tiles); two calls give equal bits."""
    _need_gpu()
    from tpnet_amd import _dense
    g = torch.Generator().manual_seed(3 + F)
    mlp = _layers(F)
    with torch.no_grad():
        mlp[0].weight.copy_(torch.randint(-1, 2, (4 * F, F), generator=g).float())
        mlp[0].bias.copy_(torch.randint(-8, 9, (4 * F,), generator=g).float())
        mlp[2].weight.copy_(torch.randint(-2, 3, (F, 4 * F), generator=g).float())
        mlp[2].bias.copy_(torch.randint(-8, 9, (F,), generator=g).float())
    cpu = [p.detach().cpu() for p in (mlp[0].weight, mlp[0].bias, mlp[2].weight)]
    for n in (1, 31, 32, 33, 1000, 9000):
        x = torch.randint(0, 3, (n, F), generator=g).float()
        x[:, 8:] *= (torch.rand(n, F - 8, generator=g) < 0.2).float()            # sparse: |pre| stays small
        gy = torch.randint(-1, 2, (n, F), generator=g).float()
        gy *= (torch.rand(n, F, generator=g) < 0.3).float()
        # every sum stays an exact integer: the float32 and the float64 expressions agree exactly
        for a, b in zip(_dense.layer_grads(x, gy, *cpu), _dense.layer_grads(x.double(), gy.double(), *[p.double() for p in cpu])):
            assert torch.equal(a.double(), b), n
        x, gy = x.to(DEV), gy.to(DEV)
        want = torch.autograd.grad(mlp(x), list(mlp.parameters()), gy)
        tiles = (n + 31) // 32
        rc, part = _call(mlp, x, gy)
        rc2, part2 = _call(mlp, x, gy)
        assert rc == rc2 == min(256, tiles)
        got, again = _grads(part, rc, gy, F), _grads(part2, rc2, gy, F)
        for a, b, c, name in zip(got, want, again, NAMES):
            assert torch.equal(a, c), name
            assert torch.equal(a, b), f"{name}, n={n}: max |delta| {(a - b).abs().max().item()}"


@pytest.mark.parametrize("L,F", WIDTHS)
@pytest.mark.parametrize("n", [33, 5000, 80000])
def test_fp32_class_on_real_valued_data(L, F, n):
    _need_gpu()
    torch.manual_seed(n + F)
    mlp = _layers(F)                                                     # nn.Linear's default init
    x = torch.rand(n, F, device=DEV) * 9.0
    x[:, 5] = 0.0
    gy = torch.randn(n, F, device=DEV)
    nblk = min(256, (n + 31) // 32)
    rc, part = _call(mlp, x, gy)
    rc2, part2 = _call(mlp, x, gy)
    assert rc == rc2 == nblk
    assert torch.equal(part[:rc].sum(0), part2[:rc].sum(0))
    got = _grads(part, rc, gy, F)
    for (want, mag, amb), a, name in list(zip(_float64_checks(mlp, x, gy), got, NAMES))[:3]:
        tol = 4e-5 * mag + amb + 1e-6 * float(want.abs().max())
        err = (a.double() - want).abs()
        print(f"F={F} n={n} {name}: largest error / bound {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all()), (name, float((err / tol).max()))


@pytest.mark.parametrize("L,F", WIDTHS)
@pytest.mark.parametrize("n", [33, 1000])
def test_nothing_is_read_or_written_outside_the_lists_and_the_partials(L, F, n):
    _need_gpu()
    mlp = _layers(F, seed=7 * F)
    g = torch.Generator().manual_seed(n + F)
    x = (torch.rand(n, F, generator=g) * 9.0).to(DEV)
    gy = torch.randn(n, F, generator=g).to(DEV)
    pf, tiles, pad = _partial_floats(F), (n + 31) // 32, 64              # (64 floats: the windows stay 16-byte aligned)

    def window(t):
        big = torch.full((pad + n * F + pad,), float("nan"), device=DEV)
        big[pad:pad + n * F] = t.reshape(-1)
        return big[pad:pad + n * F].view(n, F)

    xv, gv = window(x), window(gy)
    for n_partial in (1, 3, 256):
        rc0, plain = _call(mlp, x, gy, n_partial)
        buf = torch.full((n_partial + 2, pf), float("nan"), device=DEV)
        rc, _ = _call(mlp, xv, gv, n_partial, part=buf[1:])
        assert rc == rc0 == min(n_partial, tiles)
        assert torch.isfinite(buf[1:1 + rc]).all()
        assert torch.equal(buf[1:1 + rc], plain[:rc])
        for a, b in zip(_grads(buf[1:], rc, gv, F), _grads(plain, rc0, gy, F)):
            assert torch.isfinite(a).all() and torch.equal(a, b)
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[1 + rc:]).all()
        assert torch.isnan(plain[rc:]).all()


def test_refusals():
    _need_gpu()
    from tpnet_amd import fused_feature as ff
    mlp = _layers(16, seed=1)
    x, gy = torch.rand(64, 16, device=DEV), torch.rand(64, 16, device=DEV)
    part = torch.full((4, _partial_floats(16)), float("nan"), device=DEV)
    from tpnet_amd import _dense, _lib
    lib, stream = _lib.load(), _dense.stream_ptr(x.device)
    ref = ff.prepared(mlp, 16).ref
    for F in (64, 100):                                                  # widths of other kernels / of none
        other = _layers(F, seed=F)
        assert lib.tpnet_mlp_rows_bwd_partial_floats(F, 4 * F) == 0
        xo = torch.rand(64, F, device=DEV)
        assert _call(other, xo, xo, 4, part=part, ref=ff.prepared(other, F).ref)[0] == -1
    assert lib.tpnet_mlp_rows_bwd_partial_floats(16, 144) == 0
    assert lib.tpnet_mlp_rows_bwd_f32(None, gy.data_ptr(), 64, ref, part.data_ptr(), 4, stream) == -1
    assert lib.tpnet_mlp_rows_bwd_f32(x.data_ptr(), None, 64, ref, part.data_ptr(), 4, stream) == -1
    assert lib.tpnet_mlp_rows_bwd_f32(x.data_ptr(), gy.data_ptr(), 64, None, part.data_ptr(), 4, stream) == -1
    assert lib.tpnet_mlp_rows_bwd_f32(x.data_ptr(), gy.data_ptr(), 64, ref, None, 4, stream) == -1
    assert _call(mlp, x[:63], gy, 4, part=part, x_ptr=x.data_ptr() + 4)[0] == -1          # a misaligned x
    assert _call(mlp, x, gy, 0, part=part)[0] == -1
    assert _call(mlp, x, gy, 4, part=part, n=-1)[0] == -1
    assert _call(mlp, x, gy, 4, part=part, n=0)[0] == 0
    torch.cuda.synchronize()
    assert torch.isnan(part).all()
    assert _call(mlp, x, gy, 4, part=part)[0] == 2 and torch.isfinite(part[:2]).all() and torch.isnan(part[2:]).all()


def _backward(out, gy, params):
    for p in params:
        p.grad = None
    out.backward(gy)
    return [p.grad.clone() for p in params]


def _assert_two_sided(mlp_before, x, gy, got, want, what):
    """Two evaluations of the same gradients, each with its own rounding and its own side of a ReLU at a zero pre-activation: the
    two-sided bound of test_mlp_backward_in_the_fp32_class."""
    worst = 0.0
    for a, b, (_, mag, amb), name in zip(got, want, _float64_checks(mlp_before, x, gy), NAMES):
        tol = 5e-5 * mag + 2 * amb + 1e-5
        err = (a.double() - b.double()).abs()
        worst = max(worst, float((err / tol).max()))
        assert bool((err <= tol).all()), (what, name, float((err / tol).max()))
    print(f"{what}: largest error / two-sided bound {worst:.3f}")


@pytest.mark.parametrize("L,F", WIDTHS)
def test_through_autograd(L, F, monkeypatch):
    _need_gpu()
    from tpnet_amd import fused_feature as ff
    monkeypatch.setitem(ff.MLP_ROWS_FROM, F, 0)
    monkeypatch.setitem(ff.MLP_ROWS_BWD_FROM, F, 1000)
    torch.manual_seed(F)
    mlp = _layers(F)
    params = list(mlp.parameters())
    n = 2000
    x = torch.rand(n, F, device=DEV) * 9.0
    x[:, 5] = 0.0
    gy = torch.randn(n, F, device=DEV)
    seen = ff.calls["rows_bwd"]
    got = _backward(ff.mlp_f32(mlp, x), gy, params)
    assert ff.calls["rows_bwd"] == seen + 1
    _assert_two_sided(mlp, x, gy, got, _backward(mlp(x), gy, params), f"F={F} mlp_f32")
    # below the threshold, switched off for the module or for the process, or with a gradient for x: the torch expressions
    seen = ff.calls["rows_bwd"]
    _backward(ff.mlp_f32(mlp, x[:999]), gy[:999], params)
    monkeypatch.setitem(ff.MLP_ROWS_BWD_FROM, F, None)
    _backward(ff.mlp_f32(mlp, x), gy, params)
    monkeypatch.setitem(ff.MLP_ROWS_BWD_FROM, F, 1000)
    mlp.mlp_backward = "torch"
    _backward(ff.mlp_f32(mlp, x), gy, params)
    del mlp.mlp_backward
    monkeypatch.setattr(ff, "mlp_backward", "torch")
    _backward(ff.mlp_f32(mlp, x), gy, params)
    monkeypatch.setattr(ff, "mlp_backward", "mfma")
    xg = x.clone().requires_grad_(True)
    _backward(ff.mlp_f32(mlp, xg), gy, params)
    assert xg.grad is not None
    assert ff.calls["rows_bwd"] == seen
    _backward(ff.mlp_f32(mlp, x), gy, params)
    assert ff.calls["rows_bwd"] == seen + 1


@pytest.mark.parametrize("L,F", WIDTHS)
def test_through_the_module_and_an_optimizer_step(L, F, monkeypatch):
    _need_gpu()
    from tpnet_amd import fused_feature as ff
    monkeypatch.setitem(ff.MLP_ROWS_FROM, F, 0)
    monkeypatch.setitem(ff.MLP_ROWS_BWD_FROM, F, 1000)
    N = 300
    rp = _module(N, 64, L, 2e-6, 1.0e6)
    src, dst, _, t = _random_stream(np.random.RandomState(10 * L), N, 600, 3.0e5)
    for a in range(0, 600, 200):
        rp.update(src[a:a + 200], dst[a:a + 200], t[a:a + 200])
    rng = np.random.RandomState(L)
    u, v = torch.from_numpy(rng.randint(0, N, 2000)).to(DEV), torch.from_numpy(rng.randint(0, N, 2000)).to(DEV)
    params = list(rp.mlp.parameters())
    gy = torch.randn(2000, F, generator=torch.Generator().manual_seed(L)).to(DEV)
    feats = rp.pair_gram(u, v).detach()
    opt = torch.optim.Adam(params, lr=0.05)
    first = None
    for step in range(2):
        seen = ff.calls["rows_bwd"]
        got = _backward(rp.get_pair_wise_feature(u, v), gy, params)
        assert ff.calls["rows_bwd"] == seen + 1, step
        want = _backward(rp.mlp(feats), gy, params)
        _assert_two_sided(rp.mlp, feats, gy, got, want, f"L={L} module, step {step}")
        if first is None:
            first = got
            for p, g_ in zip(params, got):
                p.grad = g_
            opt.step()                                                   # the prepared key changes: the weights are re-read
        else:
            assert not torch.equal(first[0], got[0]) and not torch.equal(first[2], got[2])
    rp.check_device_errors()
