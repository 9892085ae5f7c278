"""The encoder's readout (models/TPNet.py:311-324, 129) at the row widths the reference produces by default: dim =
10 * floor(ln(2 * edge_num)) (models/TPNet.py:30-33) = 120 / 140 / 160, and every other width of whole 16-byte vectors in
36..160 -- rows that do not fill the last 32-deep step of the matrix-core kernels (csrc/encoder_mfma.hip: the pieces past a row's
end are supplied as zeros) nor the chunk of the vector-ALU walk (csrc/readout.hpp::gram_anchored).  Same helpers, cases and
tolerances as the d = 64 / 128 tests of test_fused_feature.py."""
import numpy as np
import pytest
import torch

from test_fused_feature import _assert_mlp_grads_close, _module, _stream

WIDTHS = (120, 140, 160, 36, 100)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")


def _raw_bound(want):
    """|delta| <= 1e-6 |R_a| |R_b| + 2e-7 |G| per raw entry of the float64 Gram `want` [n, 8, 8] (the bound of
    test_fused_feature.py::test_encoder_readout_on_the_matrix_cores)."""
    diag = np.sqrt(np.abs(want[:, np.arange(8), np.arange(8)]))
    return 1e-6 * diag[:, :, None] * diag[:, None, :] + 2e-7 * np.abs(want)


def _fused_supported(rp, n, K):
    from tpnet_amd import _lib
    prep = rp._overlapped_mlp()
    assert prep is not None
    rp._ensure_engine()
    return _lib.load().tpnet_encoder_fused_supported(rp._st_ref(), n, K, prep[2])


@pytest.mark.gpu
def test_supported_widths():
    """Rows of whole 16-byte vectors are served (walk: 36 <= d <= 512; one launch with self.mlp: 36 <= d <= 160, K >= 4, L = 3);
    rows that are only 8-byte aligned (d % 4 == 2) are not."""
    _need_gpu()
    from tpnet_amd import _lib
    lib = _lib.load()
    for d in WIDTHS:
        rp = _module(300, d, 3)
        rp._ensure_engine()
        assert lib.tpnet_pair_gram_anchored_supported(rp._st_ref()) == 1, d
        assert _fused_supported(rp, 50, 20) == 1, d
        assert _fused_supported(rp, 50, 4) == 1, d
    for d in (110, 130):
        rp = _module(300, d, 3)
        rp._ensure_engine()
        assert lib.tpnet_pair_gram_anchored_supported(rp._st_ref()) == 0, d
        assert _fused_supported(rp, 50, 20) == 0, d


@pytest.mark.gpu
@pytest.mark.parametrize("edge_num,dim", [(157474, 120), (672447, 140)])
def test_the_references_default_rule_takes_the_one_launch_path(edge_num, dim):
    """A module built as the reference's scripts build it (no --enforce_dim: utils/load_configs.py:70-84) gets dim 120 / 140
    from the rule and the encoder's call as one launch."""
    _need_gpu()
    rp = _module(300, -1, 3, edge_num=edge_num, dim_factor=10)
    assert rp.dim == dim
    assert _fused_supported(rp, 2000, 20) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("K,n", [(20, 37), (4, 9), (5, 13), (33, 3), (20, 2000)])
@pytest.mark.parametrize("d", WIDTHS)
def test_readout_against_the_oracle(d, K, n):
    """tpnet_pair_gram_anchored on the matrix cores (masked last step) and on the vector ALUs (zero tail lanes) against the
    oracle on the reference's pair list, against each other and against the general pair kernel: three update batches, 20 %
    padding ids, one row with coinciding anchors; scaled features by relative tolerance, raw entries (not_scale) inside
    1e-6 |R_a| |R_b| + 2e-7 |G| of the float64 Gram, as test_fused_feature.py::test_encoder_readout_on_the_matrix_cores."""
    _need_gpu()
    from oracle import tpnet_oracle as O
    rng = np.random.RandomState(K * 131 + d + n)
    N, L = 260, 3
    for not_scale in (False, True):
        rp = _module(N, d, L, not_scale=not_scale)
        st = O.OracleState(rp.random_projections[0].detach().cpu().numpy(), L, 1e-6, 0.0)
        for src, dst, t in _stream(rng, N, 150, 3):
            rp.update(src, dst, t)
            O.update(st, src, dst, t)
        neigh = rng.randint(0, N, (n, K)).astype(np.int64)
        neigh[rng.rand(n, K) < 0.2] = 0
        a1 = rng.randint(1, N, n).astype(np.int64)
        a2 = rng.randint(1, N, n).astype(np.int64)
        a2[n // 2] = a1[n // 2]
        u = np.tile(neigh.reshape(-1), 2)
        v = np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])
        got = rp.pair_gram_anchored(neigh, a1, a2).view(-1, 64).cpu().numpy()
        valu = rp.pair_gram_anchored(neigh, a1, a2, matrix_cores=False).view(-1, 64).cpu().numpy()
        gen = rp.pair_gram(u, v).cpu().numpy()
        if not_scale:
            # raw entries against the float64 Gram.  (No relative comparison between two fp32 summation orders here: an inner
            # product that nearly cancels is only known to 1e-6 |R_a| |R_b| in either of them, which is what this bound says.)
            want = O.pair_gram(st, u, v, not_scale=True, accumulate=np.float64).reshape(-1, 8, 8)
            bound = _raw_bound(want)
            e_mc = np.abs(got.reshape(-1, 8, 8) - want)
            e_va = np.abs(valu.reshape(-1, 8, 8) - want)
            print("raw entries / bound: matrix cores %.3f, vector ALUs %.3f" % (float(np.max(e_mc / (bound + 1e-30))),
                                                                               float(np.max(e_va / (bound + 1e-30)))))
            assert np.all(e_mc <= bound), float(np.max(e_mc / (bound + 1e-30)))
            assert np.all(e_va <= bound), float(np.max(e_va / (bound + 1e-30)))
        else:
            want = O.pair_gram(st, u, v)
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(valu, want, rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(got, valu, rtol=2e-5, atol=2e-6)
            np.testing.assert_allclose(got, gen, rtol=2e-5, atol=2e-6)
            np.testing.assert_allclose(valu, gen, rtol=2e-5, atol=2e-6)
        rp.check_device_errors()


def _alternating_state(rng, N, d, L):
    """Layers 0..L in which the rows of odd node ids are 1e3 times the O(1) rows of even ids: what follows an even node's row
    in memory is a row a thousand times larger."""
    scale = np.where(np.arange(N) % 2 == 1, 1e3, 1.0).astype(np.float32)[:, None]
    return [(rng.randn(N, d).astype(np.float32) * scale) for _ in range(L + 1)]


def _even_queries(rng, N, n, K):
    last_even = (N - 1) - ((N - 1) % 2)
    neigh = (2 * rng.randint(0, (N + 1) // 2, (n, K))).astype(np.int64)
    a1 = (2 * rng.randint(0, (N + 1) // 2, n)).astype(np.int64)
    a2 = (2 * rng.randint(0, (N + 1) // 2, n)).astype(np.int64)
    neigh[0, 0] = neigh[n - 1, K - 1] = last_even             # the table's last even row among neighbours and anchors
    a1[1] = a2[n - 1] = last_even
    assert neigh.max() < N and a1.max() < N and a2.max() < N
    return neigh, a1, a2


def test_the_raw_bound_exposes_one_piece_too_many():
    """The oracle alone, on the CPU: a readout that took ONE 16-byte piece past the end of an even node's row (the first four
    floats of the next, 1e3 times larger row) misses the raw-entry bound by orders of magnitude, so the GPU test below cannot
    hide such a mask inside its tolerance."""
    from oracle import tpnet_oracle as O
    rng = np.random.RandomState(5)
    N, L = 41, 3
    for d in (120, 140):
        P = _alternating_state(rng, N, d, L)
        st = O.OracleState(P[0], L, 1e-6, 0.0)
        for i in range(1, L + 1):
            st.P[i] = P[i].copy()
        neigh, a1, a2 = _even_queries(rng, N, 6, 5)
        K = neigh.shape[1]
        u = np.tile(neigh.reshape(-1), 2)
        v = np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])
        want = O.pair_gram(st, u, v, not_scale=True, accumulate=np.float64).reshape(-1, 8, 8)
        bound = _raw_bound(want)
        # the same Gram from rows of d + 4 floats that run on into the next node's row (the last node's: zeros, nothing follows)
        flat = [np.concatenate([p.reshape(-1), np.zeros(4, np.float32)]) for p in P]
        wide = [np.stack([f[i * d: i * d + d + 4] for i in range(N)]) for f in flat]
        R = np.stack([w[u] for w in wide] + [w[v] for w in wide], axis=1).astype(np.float64)
        over = np.einsum('nad,nbd->nab', R, R)
        ratio = (np.abs(over - want) / (bound + 1e-30)).max(axis=(1, 2))
        follows = (u != N - 1) | (v != N - 1)                     # (nothing follows the table's last row)
        assert follows.sum() > 40 and np.all(ratio[follows] > 100.0), float(ratio[follows].min())
        assert np.all(ratio[~follows] <= 1.0)                     # (only the oracle's own rounding of the entry to fp32)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [120, 140])
def test_a_mask_that_is_off_by_one_piece_shows(d):
    """Rows lie back to back in memory (P[0] is [N][d]): with the rows of odd nodes 1e3 times the rows of even nodes, queries on
    even ids only (the table's last even node among them) hold the raw-entry bound only if no piece past a row's end is read
    (test_the_raw_bound_exposes_one_piece_too_many: one piece too many misses it by more than 100 x)."""
    _need_gpu()
    from oracle import tpnet_oracle as O
    rng = np.random.RandomState(d)
    N, L, n, K = 261, 3, 40, 20
    P = _alternating_state(rng, N, d, L)
    rp = _module(N, d, L, not_scale=True)
    rp.random_projections[0].data = torch.from_numpy(P[0]).cuda()
    rp.reload_random_projections((torch.tensor(0.0, dtype=torch.float64, device="cuda:0"),
                                  [torch.from_numpy(P[i]).cuda() for i in range(1, L + 1)]))
    st = O.OracleState(P[0], L, 1e-6, 0.0)
    for i in range(1, L + 1):
        st.P[i] = P[i].copy()
    neigh, a1, a2 = _even_queries(rng, N, n, K)
    u = np.tile(neigh.reshape(-1), 2)
    v = np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])
    want = O.pair_gram(st, u, v, not_scale=True, accumulate=np.float64).reshape(-1, 8, 8)
    bound = _raw_bound(want)
    for mc in (True, False):
        got = rp.pair_gram_anchored(neigh, a1, a2, matrix_cores=mc).view(-1, 8, 8).cpu().numpy()
        ratio = float(np.max(np.abs(got - want) / (bound + 1e-30)))
        print("matrix_cores=%s: raw entries / bound %.3f" % (mc, ratio))
        assert np.all(np.abs(got - want) <= bound), (mc, ratio)
    rp.check_device_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("K,n", [(20, 200), (5, 13), (4, 1), (7, 3), (20, 2000)])
@pytest.mark.parametrize("d", [120, 140, 160])
def test_readout_and_dense_layers_in_one_launch(d, K, n):
    """k_encoder_fused with a masked last step against self.mlp on the general kernel's features: fp32 class; with gradients
    recorded the outputs keep their bits and the gradients of self.mlp's four tensors match autograd on the torch layers."""
    _need_gpu()
    rng = np.random.RandomState(K * 17 + d + n)
    N = 300
    rp = _module(N, d, 3)
    for src, dst, t in _stream(rng, N, 150, 3):
        rp.update(src, dst, t)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    neigh = rng.randint(0, N, (n, K)).astype(np.int64)
    neigh[rng.rand(n, K) < 0.2] = 0
    a1, a2 = rng.randint(1, N, n).astype(np.int64), rng.randint(1, N, n).astype(np.int64)
    u = np.tile(neigh.reshape(-1), 2)
    v = np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])
    assert _fused_supported(rp, n, K) == 1
    with torch.no_grad():
        got = rp.get_pair_wise_feature_anchored(dev(neigh), dev(a1), dev(a2))
        feats = rp.pair_gram(dev(u), dev(v))
        want = rp.mlp(feats)
    scale = float(want.abs().max())
    err = (got - want).abs()
    print("error / scale %.3g" % (float(err.max()) / scale))
    assert bool((err <= 2e-5 * scale + 1e-4 * want.abs()).all()), (float(err.max()), scale)
    got2 = rp.get_pair_wise_feature_anchored(dev(neigh), dev(a1), dev(a2))
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


@pytest.mark.gpu
@pytest.mark.parametrize("d", [140, 120])
def test_encoder_call_from_the_sampler(d):
    """encoder_pair_features (row set-up + device sampler + readout + self.mlp), device ids and host arrays, against the
    reference's call sequence restated with the host sampler and get_pair_wise_feature(u, v) (models/TPNet.py:280-316)."""
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
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for b0 in range(0, E - B, B):
        s = slice(b0, b0 + B)
        if b0 >= 5 * B:
            other = rng.randint(1, N, B).astype(np.int64)
            neigh_h, _, _ = host.get_historical_neighbors(np.concatenate([src[s], other]), np.tile(t[s], 2), K)
            u, v = encoder_pair_indices(neigh_h, src[s], other)
            want = rp.get_pair_wise_feature(u, v)
            got, neigh_d = rp.encoder_pair_features(gpu, dev(src[s]), dev(other), dev(t[s]), K)
            np.testing.assert_array_equal(neigh_d.cpu().numpy(), neigh_h)
            np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=2e-4, atol=2e-4)
            got_h, neigh_dh = rp.encoder_pair_features(gpu, src[s], other, t[s], K)
            np.testing.assert_array_equal(neigh_dh.cpu().numpy(), neigh_h)
            np.testing.assert_allclose(got_h.detach().cpu().numpy(), want.detach().cpu().numpy(), rtol=2e-4, atol=2e-4)
        rp.update(src[s], dst[s], t[s])
    rp.check_device_errors()


@pytest.mark.gpu
def test_ids_out_of_range_answer_nan_and_are_counted():
    """d = 140: NaN rows exactly for the pairs that hold an id out of range; check_device_errors raises IndexError."""
    _need_gpu()
    rng = np.random.RandomState(140)
    N, d, n, K = 260, 140, 37, 20
    for mc in (True, False):
        rp = _module(N, d, 3)
        neigh = rng.randint(1, N, (n, K)).astype(np.int64)
        a1 = rng.randint(1, N, n).astype(np.int64)
        a2 = rng.randint(1, N, n).astype(np.int64)
        neigh[0, K - 1] = N + 5
        bad_row = n - 1
        a2[bad_row] = -3
        dev = lambda x: torch.from_numpy(x).cuda()
        got = rp.pair_gram_anchored(dev(neigh), dev(a1), dev(a2), matrix_cores=mc).cpu().numpy()          # [2, n*K, 64]
        nanrow = np.isnan(got).all(axis=2)
        exp = np.zeros((2, n * K), dtype=bool)
        exp[:, K - 1] = True
        exp[:, bad_row * K:(bad_row + 1) * K] = True
        assert np.array_equal(nanrow, exp)
        assert not np.isnan(got[~exp]).any()
        with pytest.raises(IndexError):
            rp.check_device_errors()


@pytest.mark.gpu
def test_one_launch_encoder_call_on_random_shapes_and_widths():
    """k_encoder_fused over forty seeded (rows, K, d) shapes, d from (72, 120, 140, 160) (KS = 3, 4, 5, 5 steps, the last one
    masked), against the vector-ALU walk + torch layers."""
    _need_gpu()
    rng = np.random.RandomState(2025)
    N = 500
    widths = (72, 120, 140, 160)
    mods = {}
    for d in widths:
        rp = _module(N, d, 3)
        for src, dst, t in _stream(rng, N, 200, 2):
            rp.update(src, dst, t)
        mods[d] = rp
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for trial in range(40):
        d = int(rng.choice(widths))
        rp = mods[d]
        K = int(rng.randint(4, 46))
        n = int(rng.choice([1, 2, 3, 5, 17, 64, 257, 1000, 3000]))
        neigh = rng.randint(0, N, (n, K)).astype(np.int64)
        a1, a2 = rng.randint(1, N, n).astype(np.int64), rng.randint(1, N, n).astype(np.int64)
        assert _fused_supported(rp, n, K) == 1
        with torch.no_grad():
            got = rp.get_pair_wise_feature_anchored(dev(neigh), dev(a1), dev(a2))
            want = rp.mlp(rp.pair_gram_anchored(neigh, a1, a2, matrix_cores=False).view(-1, 64))
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        assert err <= 2e-5 * scale + 1e-6, (trial, d, K, n, err, scale)
    for rp in mods.values():
        rp.check_device_errors()
