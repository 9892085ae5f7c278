"""The encoder's readout (models/TPNet.py:311-324, 129) on rows that are only 8-byte aligned: dim % 4 == 2, 38 <= dim <= 158 -- the
widths 110 / 130 / 150 of the reference's default rule dim = 10 * floor(ln(2 * edge_num)) (models/TPNet.py:30-33) -- behind the
opt-in switch RandomProjectionModule.rows8_readout (TPNET_FLAG_ROWS8, csrc/encoder_mfma.hip: every 16-byte piece of a row as two
8-byte halves, a half past the row's end supplied as zeros).  Helpers, cases and tolerances of test_encoder_widths.py /
test_fused_feature.py; the widths cover every shape of the last 32-deep step:

    d    KS  floats in the last step
    38   2    6   one piece + a half piece
    66   3    2   only a half piece
    110  4   14   three pieces + a half piece
    130  5    2   only a half piece
    150  5   22   five pieces + a half piece
    158  5   30   the last piece half valid
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_encoder_widths import _alternating_state, _even_queries, _raw_bound
from test_fused_feature import _assert_mlp_grads_close, _module, _stream

WIDTHS = (38, 66, 110, 130, 150, 158)
DEFAULT_WIDTHS = (110, 130, 150)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _switched_on(N, d, L=3, **kw):
    rp = _module(N, d, L, **kw)
    rp.rows8_readout = True
    return rp


def _rows8_supported(rp, n, K, with_mlp=True):
    from tpnet_amd import _lib
    rp._ensure_engine()
    prep = rp._overlapped_mlp() if with_mlp else None
    assert prep is not None or not with_mlp
    return _lib.load().tpnet_encoder_rows8_supported(rp._st_ref(), n, K, prep.ref if with_mlp else None)


def _pairs(neigh, a1, a2):
    K = neigh.shape[1]
    return np.tile(neigh.reshape(-1), 2), np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.gpu
def test_support_and_switch():
    """tpnet_encoder_rows8_supported: 1 for the six widths (readout alone and with self.mlp, K = 20 and K = 4), 0 for K = 3, odd d,
    d = 34, d = 162 and L = 2; the two older queries keep answering 0 at 110 / 130; without the switch pair_gram_anchored raises at
    d = 110 and the C calls answer TPNET_ERR_BAD_ARG without the flag -- and with it wherever only the vector-ALU walk could have
    served (K < 4, unaligned outputs, TPNET_FLAG_NO_MFMA_READOUT)."""
    _need_gpu()
    from tpnet_amd import _lib
    lib = _lib.load()
    for d in WIDTHS:
        rp = _module(300, d, 3)
        for mlp in (False, True):
            assert _rows8_supported(rp, 50, 20, mlp) == 1, (d, mlp)
            assert _rows8_supported(rp, 50, 4, mlp) == 1, (d, mlp)
            assert _rows8_supported(rp, 50, 3, mlp) == 0, (d, mlp)
    for d in (37, 34, 162, 120):
        rp = _module(300, d, 3)
        assert _rows8_supported(rp, 50, 20, False) == 0 and _rows8_supported(rp, 50, 20, True) == 0, d
    assert _rows8_supported(_module(300, 110, 2), 50, 20, False) == 0
    for d in (110, 130):
        rp = _module(300, d, 3)
        rp._ensure_engine()
        prep = rp._overlapped_mlp()
        assert lib.tpnet_pair_gram_anchored_supported(rp._st_ref()) == 0, d
        assert lib.tpnet_encoder_fused_supported(rp._st_ref(), 50, 20, prep.ref) == 0, d
    # the switch is off by default: today's answers
    rng = np.random.RandomState(1)
    N, d, n, K = 300, 110, 9, 5
    rp = _module(N, d, 3)
    assert rp.rows8_readout is False and type(rp).rows8_readout is False
    neigh = rng.randint(0, N, (n, K)).astype(np.int64)
    a1, a2 = rng.randint(1, N, n).astype(np.int64), rng.randint(1, N, n).astype(np.int64)
    with pytest.raises(_lib.TPNetHipError):
        rp.pair_gram_anchored(neigh, a1, a2)
    rp.rows8_readout = True
    with pytest.raises(_lib.TPNetHipError):
        rp.pair_gram_anchored(neigh, a1, a2, matrix_cores=False)       # (no vector-ALU walk at these widths)
    assert tuple(rp.pair_gram_anchored(neigh, a1, a2).shape) == (2, n * K, 64)
    # the C calls
    prep = rp._overlapped_mlp()
    wd, d1, d2 = _dev(neigh.reshape(-1)), _dev(a1), _dev(a2)
    out = torch.empty((2 * n * K * 64 + 4,), dtype=torch.float32, device="cuda:0")
    gram = torch.empty((2 * n * K, 64), dtype=torch.float32, device="cuda:0")
    now, lam, s = rp._now_host, float(rp.time_decay_weight), rp._stream()
    half = n * K * 64 * 4

    def gram_call(flags, K_=K, base=out.data_ptr()):
        return lib.tpnet_pair_gram_anchored(rp._st_ref(), wd.data_ptr(), d1.data_ptr(), d2.data_ptr(), (n * K) // K_, K_, now, lam, flags,
                                            base, base + ((n * K) // K_) * K_ * 256, s)

    def feature_call(flags):
        return lib.tpnet_anchored_features(rp._st_ref(), wd.data_ptr(), d1.data_ptr(), d2.data_ptr(), n, K, now, lam, flags, prep.ref,
                                           gram.data_ptr(), out.data_ptr(), s)
    BAD = -1
    assert half % 16 == 0 and out.data_ptr() % 16 == 0
    assert gram_call(0) == BAD and feature_call(0) == BAD
    assert gram_call(_lib.FLAG_NO_MFMA_READOUT) == BAD and feature_call(_lib.FLAG_NO_MFMA_READOUT) == BAD
    assert gram_call(_lib.FLAG_ROWS8) == 0 and feature_call(_lib.FLAG_ROWS8) == 0
    assert gram_call(_lib.FLAG_ROWS8 | _lib.FLAG_NO_MFMA_READOUT) == BAD
    assert feature_call(_lib.FLAG_ROWS8 | _lib.FLAG_NO_MFMA_READOUT) == BAD
    assert gram_call(_lib.FLAG_ROWS8, K_=3) == BAD                                           # K < 4
    assert gram_call(_lib.FLAG_ROWS8, base=out.data_ptr() + 8) == BAD                        # outputs not 16-byte aligned
    torch.cuda.synchronize()
    rp.check_device_errors()
    # d % 4 == 0: the flag changes nothing
    rp4 = _module(N, 120, 3)
    a = rp4.pair_gram_anchored(neigh, a1, a2)
    rp4.rows8_readout = True
    assert torch.equal(rp4.pair_gram_anchored(neigh, a1, a2), a)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.gpu
@pytest.mark.parametrize("K,n", [(20, 37), (4, 9), (5, 13), (33, 3), (20, 2000)])
@pytest.mark.parametrize("d", WIDTHS)
def test_readout_against_the_oracle(d, K, n):
    """tpnet_pair_gram_anchored with TPNET_FLAG_ROWS8 against the oracle on the reference's pair list and against the general pair
    kernel: three update batches, 20 % padding ids, one row with coinciding anchors; random ids, so rows at 0 and at 8 mod 16 bytes
    both occur.  Scaled features by relative tolerance, raw entries (not_scale) inside 1e-6 |R_a| |R_b| + 2e-7 |G| of the float64
    Gram (test_encoder_widths.py::test_readout_against_the_oracle)."""
    _need_gpu()
    from oracle import tpnet_oracle as O
    rng = np.random.RandomState(K * 131 + d + n)
    N, L = 260, 3
    for not_scale in (False, True):
        rp = _switched_on(N, d, L, not_scale=not_scale)
        st = O.OracleState(rp.random_projections[0].detach().cpu().numpy(), L, 1e-6, 0.0)
        for src, dst, t in _stream(rng, N, 150, 3):
            rp.update(src, dst, t)
            O.update(st, src, dst, t)
        neigh = rng.randint(0, N, (n, K)).astype(np.int64)
        neigh[rng.rand(n, K) < 0.2] = 0
        a1 = rng.randint(1, N, n).astype(np.int64)
        a2 = rng.randint(1, N, n).astype(np.int64)
        a2[n // 2] = a1[n // 2]
        u, v = _pairs(neigh, a1, a2)
        got = rp.pair_gram_anchored(neigh, a1, a2).view(-1, 64).cpu().numpy()
        gen = rp.pair_gram(u, v).cpu().numpy()
        if not_scale:
            want = O.pair_gram(st, u, v, not_scale=True, accumulate=np.float64).reshape(-1, 8, 8)
            bound = _raw_bound(want)
            e_mc = np.abs(got.reshape(-1, 8, 8) - want)
            print("raw entries / bound: matrix cores %.3f" % float(np.max(e_mc / (bound + 1e-30))))
            assert np.all(e_mc <= bound), float(np.max(e_mc / (bound + 1e-30)))
            assert np.all(np.abs(gen.reshape(-1, 8, 8) - want) <= bound)
        else:
            want = O.pair_gram(st, u, v)
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(got, gen, rtol=2e-5, atol=2e-6)
        rp.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 3
def _oracle_state(P, L):
    from oracle import tpnet_oracle as O
    st = O.OracleState(P[0], L, 1e-6, 0.0)
    for i in range(1, L + 1):
        st.P[i] = P[i].copy()
    return st


def test_the_raw_bound_exposes_half_a_piece_too_many_or_too_few():
    """The oracle alone, on the CPU: with the rows of odd nodes 1e3 times the rows of even nodes and queries on even ids, a Gram
    that reads TWO floats past each row's end misses the raw-entry bound by more than 100 x wherever a row follows, and a Gram that
    drops each row's last two floats (a mask left at 4-float granularity) misses it by more than 100 x everywhere -- so the GPU
    test below cannot hide either mask inside its tolerance.  (Smallest ratios seen: about 7.7e9 and 3.4e3.)"""
    from oracle import tpnet_oracle as O
    rng = np.random.RandomState(5)
    N, L = 41, 3
    for d in (38, 110, 130, 150, 158):
        P = _alternating_state(rng, N, d, L)
        st = _oracle_state(P, L)
        neigh, a1, a2 = _even_queries(rng, N, 6, 5)
        u, v = _pairs(neigh, a1, a2)
        want = O.pair_gram(st, u, v, not_scale=True, accumulate=np.float64).reshape(-1, 8, 8)
        bound = _raw_bound(want)
        # rows of d + 2 floats that run on into the next node's row (the last node's: zeros, nothing follows)
        flat = [np.concatenate([p.reshape(-1), np.zeros(2, np.float32)]) for p in P]
        wide = [np.stack([f[i * d: i * d + d + 2] for i in range(N)]) for f in flat]
        R = np.stack([w[u] for w in wide] + [w[v] for w in wide], axis=1).astype(np.float64)
        over = np.einsum('nad,nbd->nab', R, R)
        ratio = (np.abs(over - want) / (bound + 1e-30)).max(axis=(1, 2))
        follows = (u != N - 1) | (v != N - 1)
        assert follows.sum() > 40 and np.all(ratio[follows] > 100.0), (d, float(ratio[follows].min()))
        assert np.all(ratio[~follows] <= 1.0)
        # rows cut to d - 2 floats
        R = np.stack([p[u, : d - 2] for p in P] + [p[v, : d - 2] for p in P], axis=1).astype(np.float64)
        under = np.einsum('nad,nbd->nab', R, R)
        ratio = (np.abs(under - want) / (bound + 1e-30)).max(axis=(1, 2))
        assert np.all(ratio > 100.0), (d, float(ratio.min()))


@pytest.mark.gpu
@pytest.mark.parametrize("d", DEFAULT_WIDTHS)
def test_a_mask_that_is_off_by_half_a_piece_shows(d):
    """Rows lie back to back in memory (P[0] is [N][d]): with the rows of odd nodes 1e3 times the rows of even nodes, queries on
    even ids only (the table's last even node among them) hold the raw-entry bound only if no half piece past a row's end is read
    and none inside it is dropped (test_the_raw_bound_exposes_half_a_piece_too_many_or_too_few)."""
    _need_gpu()
    from oracle import tpnet_oracle as O
    rng = np.random.RandomState(d)
    N, L, n, K = 261, 3, 40, 20
    P = _alternating_state(rng, N, d, L)
    rp = _switched_on(N, d, L, not_scale=True)
    rp.random_projections[0].data = torch.from_numpy(P[0]).cuda()
    rp.reload_random_projections((torch.tensor(0.0, dtype=torch.float64, device="cuda:0"),
                                  [torch.from_numpy(P[i]).cuda() for i in range(1, L + 1)]))
    st = _oracle_state(P, L)
    neigh, a1, a2 = _even_queries(rng, N, n, K)
    u, v = _pairs(neigh, a1, a2)
    want = O.pair_gram(st, u, v, not_scale=True, accumulate=np.float64).reshape(-1, 8, 8)
    bound = _raw_bound(want)
    got = rp.pair_gram_anchored(neigh, a1, a2).view(-1, 8, 8).cpu().numpy()
    ratio = float(np.max(np.abs(got - want) / (bound + 1e-30)))
    print("raw entries / bound %.3f" % ratio)
    assert np.all(np.abs(got - want) <= bound), ratio
    rp.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.gpu
@pytest.mark.parametrize("K,n", [(20, 200), (5, 13), (4, 1), (7, 3), (20, 2000)])
@pytest.mark.parametrize("d", DEFAULT_WIDTHS)
def test_readout_and_dense_layers_in_one_launch(d, K, n):
    """k_encoder_fused on 8-byte rows against self.mlp on the general kernel's features: fp32 class; with gradients recorded the
    outputs keep their bits and the gradients of self.mlp's four tensors match autograd on the torch layers."""
    _need_gpu()
    rng = np.random.RandomState(K * 17 + d + n)
    N = 300
    rp = _switched_on(N, d, 3)
    for src, dst, t in _stream(rng, N, 150, 3):
        rp.update(src, dst, t)
    neigh = rng.randint(0, N, (n, K)).astype(np.int64)
    neigh[rng.rand(n, K) < 0.2] = 0
    a1, a2 = rng.randint(1, N, n).astype(np.int64), rng.randint(1, N, n).astype(np.int64)
    u, v = _pairs(neigh, a1, a2)
    assert _rows8_supported(rp, n, K) == 1
    with torch.no_grad():
        got = rp.get_pair_wise_feature_anchored(_dev(neigh), _dev(a1), _dev(a2))
        feats = rp.pair_gram(_dev(u), _dev(v))
        want = rp.mlp(feats)
    scale = float(want.abs().max())
    err = (got - want).abs()
    print("error / scale %.3g" % (float(err.max()) / scale))
    assert bool((err <= 2e-5 * scale + 1e-4 * want.abs()).all()), (float(err.max()), scale)
    got2 = rp.get_pair_wise_feature_anchored(_dev(neigh), _dev(a1), _dev(a2))
    assert got2.requires_grad and torch.equal(got2.detach(), got)
    gy = torch.from_numpy(rng.randn(*got.shape).astype(np.float32)).cuda()
    got2.backward(gy)
    grads = [p.grad.clone() for p in rp.mlp.parameters()]
    for p in rp.mlp.parameters():
        p.grad = None
    ref = rp.mlp(feats)
    ref.backward(gy)
    want_g = [p.grad.clone() for p in rp.mlp.parameters()]
    _assert_mlp_grads_close(rp.mlp, feats, gy, grads, want_g)
    rp.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.gpu
@pytest.mark.parametrize("d", [110, 130])
def test_encoder_call_from_the_sampler(d):
    """encoder_pair_features (row set-up + device sampler + readout + self.mlp) with the switch on, device ids and host arrays,
    against the reference's call sequence restated with the host sampler and get_pair_wise_feature(u, v) with the switch off
    (models/TPNet.py:280-316).  Shapes and tolerances of test_encoder_widths.py::test_encoder_call_from_the_sampler."""
    _need_gpu()
    from tpnet_amd.callers import RecentNeighborSampler, encoder_pair_indices
    from tpnet_amd.sampler import GpuRecentNeighborSampler
    K = 20
    rng = np.random.RandomState(d + K)
    N, E, B = 300, 900, 60
    src = rng.randint(1, N, E).astype(np.int64)
    dst = rng.randint(1, N, E).astype(np.int64)
    t = np.sort(rng.uniform(1.0e6, 1.4e6, E))
    rp = _module(N, d, 3)
    host = RecentNeighborSampler(src, dst, t)
    gpu = GpuRecentNeighborSampler(src, dst, t, device="cuda:0", num_nodes=N)
    for b0 in range(0, E - B, B):
        s = slice(b0, b0 + B)
        if b0 >= 5 * B:
            other = rng.randint(1, N, B).astype(np.int64)
            neigh_h, _, _ = host.get_historical_neighbors(np.concatenate([src[s], other]), np.tile(t[s], 2), K)
            u, v = encoder_pair_indices(neigh_h, src[s], other)
            rp.rows8_readout = False
            want = rp.get_pair_wise_feature(u, v).detach().cpu().numpy()
            rp.rows8_readout = True
            assert _rows8_supported(rp, 2 * B, K) == 1
            got, neigh_d = rp.encoder_pair_features(gpu, _dev(src[s]), _dev(other), _dev(t[s]), K)
            np.testing.assert_array_equal(neigh_d.cpu().numpy(), neigh_h)
            np.testing.assert_allclose(got.detach().cpu().numpy(), want, rtol=2e-4, atol=2e-4)
            got_h, neigh_dh = rp.encoder_pair_features(gpu, src[s], other, t[s], K)
            np.testing.assert_array_equal(neigh_dh.cpu().numpy(), neigh_h)
            np.testing.assert_allclose(got_h.detach().cpu().numpy(), want, rtol=2e-4, atol=2e-4)
        rp.update(src[s], dst[s], t[s])
    rp.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.gpu
def test_route_5_of_get_pair_wise_feature(monkeypatch):
    """get_pair_wise_feature on the encoder's pattern from host arrays (K = 4, just above fused_feature.MAX_PAIRS) at d = 130:
    with the switch on the one crossing serves it (route 5, as test_host_routes.py tells routes), with the switch off today's route
    (5 declines, the shared readout answers); both against the oracle within that file's post-mlp bound, and within C_DENSE of scale
    of each other."""
    _need_gpu()
    import test_host_routes as H
    rp, st, layers, th = H._table(**H._D130)
    N = rp.node_num
    n = H._above(th["MAX_PAIRS"], 4)
    u, v = H._pattern_pairs(np.random.RandomState(130), N, n, 4)
    rec = H._Recorder(rp, monkeypatch)
    outs = {}
    try:
        for on, expected in ((False, ("7", "shared, 5 declined")), (True, ("5", "one crossing"))):
            rp.rows8_readout = on
            rec.clear()
            with torch.no_grad():
                got = rp.get_pair_wise_feature(u, v)
            assert rec.feature_route() == expected, (on, rec.feature_route(), rec.events)
            rp.check_device_errors()
            outs[on] = got.cpu().numpy()
            H._check_outputs(outs[on], layers, st, H._wrapped(u, N), H._wrapped(v, N), rp.not_scale, H.C_DENSE, f"d130 switch {on}")
    finally:
        rp.__dict__.pop("rows8_readout", None)
    scale = max(1.0, float(np.abs(outs[False]).max()))
    err = float(np.abs(outs[True] - outs[False]).max())
    print("switch on against off: %.3e of scale" % (err / scale))
    assert err <= H.C_DENSE * scale


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.gpu
def test_ids_out_of_range_answer_nan_and_are_counted():
    """d = 110: NaN rows exactly for the pairs that hold an id out of range; check_device_errors raises IndexError."""
    _need_gpu()
    rng = np.random.RandomState(110)
    N, d, n, K = 260, 110, 37, 20
    rp = _switched_on(N, d, 3)
    neigh = rng.randint(1, N, (n, K)).astype(np.int64)
    a1 = rng.randint(1, N, n).astype(np.int64)
    a2 = rng.randint(1, N, n).astype(np.int64)
    neigh[0, K - 1] = N + 5
    bad_row = n - 1
    a2[bad_row] = -3
    got = rp.pair_gram_anchored(_dev(neigh), _dev(a1), _dev(a2)).cpu().numpy()          # [2, n*K, 64]
    nanrow = np.isnan(got).all(axis=2)
    exp = np.zeros((2, n * K), dtype=bool)
    exp[:, K - 1] = True
    exp[:, bad_row * K:(bad_row + 1) * K] = True
    assert np.array_equal(nanrow, exp)
    assert not np.isnan(got[~exp]).any()
    with pytest.raises(IndexError):
        rp.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.gpu
def test_a_module_built_by_the_default_rule_takes_the_one_launch_call(monkeypatch):
    """59 836 edges give dim = 110 by the reference's rule.  A tpnet_amd.TPNet on such a module (K = 20, a batch of 60) gives the same
    embeddings with the switch on (the anchored call, one launch: no feature buffer) and off (general pair readout + torch layers):
    within 1e-4 * max(1, max|want|), the bound of test_encoder_module.py::test_anchored_readout_branch_end_to_end."""
    _need_gpu()
    import tpnet_amd
    from tpnet_amd.sampler import GpuRecentNeighborSampler
    N, K, B, E = 300, 20, 60, 900
    rp = _module(N, -1, 3, edge_num=59836, dim_factor=10)
    assert rp.dim == 110
    rng = np.random.RandomState(59836)
    src = rng.randint(1, N, E).astype(np.int64)
    dst = rng.randint(1, N, E).astype(np.int64)
    t = np.sort(rng.uniform(1.0e6, 1.4e6, E))
    torch.manual_seed(110)
    model = tpnet_amd.TPNet(node_raw_features=rng.randn(N, 32).astype(np.float32), edge_raw_features=rng.randn(E + 1, 32).astype(np.float32),
                            neighbor_sampler=GpuRecentNeighborSampler(src, dst, t, device="cuda:0", num_nodes=N), time_feat_dim=20,
                            dropout=0.1, random_projections=rp, num_layers=2, num_neighbors=K, device="cuda:0").to("cuda:0")
    model.eval()
    for b0 in range(0, 600, 150):
        rp.update(src[b0:b0 + 150], dst[b0:b0 + 150], t[b0:b0 + 150])
    launches = []
    inner = rp._anchored_launch

    def spy(*a, **kw):
        launch = inner(*a, **kw)

        def recorded(gram):
            launches.append((kw.get("rows8", a[6] if len(a) > 6 else 0), gram is None))
            return launch(gram)
        return recorded
    monkeypatch.setitem(rp.__dict__, "_anchored_launch", spy)
    s = slice(600, 600 + B)
    embs = {}
    for on in (False, True):
        rp.rows8_readout = on
        with torch.no_grad():
            es, ed = model.compute_src_dst_node_temporal_embeddings(src[s], dst[s], t[s])
        embs[on] = torch.cat([es, ed]).cpu().numpy()
        if not on:
            assert launches == []
    from tpnet_amd import _lib
    assert launches == [(_lib.FLAG_ROWS8, True)], launches
    want = embs[False].astype(np.float64)
    err = float(np.abs(embs[True] - want).max() / max(1.0, np.abs(want).max()))
    print("embeddings, switch on against off: %.3e of scale" % err)
    assert err <= 1e-4
    rp.check_device_errors()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 9
@pytest.mark.gpu
def test_one_launch_encoder_call_on_random_shapes_and_widths():
    """k_encoder_fused on 8-byte rows over forty seeded (rows, K, d) shapes, d from the six widths, against the general pair kernel +
    torch layers at 2e-5 of scale."""
    _need_gpu()
    rng = np.random.RandomState(2026)
    N = 500
    mods = {}
    for d in WIDTHS:
        rp = _switched_on(N, d, 3)
        for src, dst, t in _stream(rng, N, 200, 2):
            rp.update(src, dst, t)
        mods[d] = rp
    for trial in range(40):
        d = int(rng.choice(WIDTHS))
        rp = mods[d]
        K = int(rng.randint(4, 46))
        n = int(rng.choice([1, 2, 3, 5, 17, 64, 257, 1000, 3000]))
        neigh = rng.randint(0, N, (n, K)).astype(np.int64)
        a1, a2 = rng.randint(1, N, n).astype(np.int64), rng.randint(1, N, n).astype(np.int64)
        u, v = _pairs(neigh, a1, a2)
        assert _rows8_supported(rp, n, K) == 1
        with torch.no_grad():
            got = rp.get_pair_wise_feature_anchored(_dev(neigh), _dev(a1), _dev(a2))
            want = rp.mlp(rp.pair_gram(_dev(u), _dev(v)))
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        assert err <= 2e-5 * scale + 1e-6, (trial, d, K, n, err, scale)
    for rp in mods.values():
        rp.check_device_errors()
