"""The encoder's call (models/TPNet.py:311-324, 129) on rows of 164..512 floats in ONE launch (csrc/anchored_feature.hip:
k_anchored_feature -- the vector-ALU anchored walk with self.mlp on the matrix cores inside), reached through the explicit entry
tpnet_anchored_features_wide whatever the default route of tpnet_anchored_features is.  Both geometries (32 lanes x 2 vectors up
to d = 256, 64 x 2 from d = 260), full and masked rows, the class boundaries; helpers, cases and tolerances of
test_fused_feature.py / test_encoder_widths.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_encoder_widths import _alternating_state, _even_queries, _raw_bound
from test_fused_feature import _assert_mlp_grads_close, _module, _stream

WIDTHS = (164, 200, 256, 260, 508, 512)
# (rows, K): one unit and one partial tile | K a multiple of nothing | few rows: chunks of 4, the last one short | K beyond 32
# lanes: the walk's second id fetch | the same beyond 64 lanes | the workload's K, partly filled workgroups | several grid strides
SHAPES = ((1, 4), (3, 7), (1, 45), (2, 33), (5, 70), (37, 20), (2000, 20))
N_NODES = 300


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _prep(rp):
    prep = rp._overlapped_mlp()
    assert prep is not None
    rp._ensure_engine()
    return prep


def _wide_supported(rp, n, K):
    from tpnet_amd import _lib
    return _lib.load().tpnet_encoder_wide_supported(rp._st_ref(), n, K, _prep(rp).ref)


def _wide(rp, neigh, a1, a2, want_gram=True):
    """tpnet_anchored_features_wide on device ids -> (out [2 n K, 64], gram [2, n K, 64] or None)."""
    from tpnet_amd import _lib
    prep = _prep(rp)
    n, K = neigh.shape
    out = torch.empty((2 * n * K, 64), dtype=torch.float32, device="cuda:0")
    gram = torch.empty((2, n * K, 64), dtype=torch.float32, device="cuda:0") if want_gram else None
    rc = _lib.load().tpnet_anchored_features_wide(rp._st_ref(), neigh.data_ptr(), a1.data_ptr(), a2.data_ptr(), n, K, rp._now_host,
                                                  float(rp.time_decay_weight), rp._readout_flags(), prep.ref,
                                                  gram.data_ptr() if want_gram else None, out.data_ptr(),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "anchored_features_wide")
    return out, gram


def _queries(rng, n, K):
    neigh = rng.randint(0, N_NODES, (n, K)).astype(np.int64)
    neigh[rng.rand(n, K) < 0.2] = 0                             # 20 % padding ids
    a1 = rng.randint(1, N_NODES, n).astype(np.int64)
    a2 = rng.randint(1, N_NODES, n).astype(np.int64)
    a2[n // 2] = a1[n // 2]                                     # one row with coinciding anchors
    return neigh, a1, a2


@functools.lru_cache(maxsize=None)
def _case(d, not_scale):
    """Module + oracle after three update batches, and the queries of every shape: built once per (width, not_scale), shared by
    the tests below and left unchanged by them.  The raw (not_scale) table is grown by _stream's hub nodes, whose rows reach
    norms of several units: the raw-entry bound scales with |R_a| |R_b| and holds there.  The scaled features are compared at
    atol 1e-5, which ANY fp32 summation misses on such rows (an inner product is known to 1e-6 |R_a| |R_b|, and log(x + 1) ~ x
    passes that on: numpy's own fp32 einsum against the float64 oracle sits at 1.0 x this bound on a hub-grown table and at
    0.01 x on one without hubs), so the scaled table is grown by the same stream without hubs."""
    from oracle import tpnet_oracle as O
    rng = np.random.RandomState(977 * d + int(not_scale))
    rp = _module(N_NODES, d, 3, not_scale=not_scale)
    st = O.OracleState(rp.random_projections[0].detach().cpu().numpy(), 3, 1e-6, 0.0)
    for src, dst, t in _stream(rng, N_NODES, 150, 3, hubs=not_scale):
        rp.update(src, dst, t)
        O.update(st, src, dst, t)
    return rp, st, {s: _queries(rng, *s) for s in SHAPES}


def _oracle_gram(st, u, v, **kw):
    from oracle import tpnet_oracle as O
    return np.concatenate([O.pair_gram(st, u[i: i + 8192], v[i: i + 8192], **kw) for i in range(0, u.size, 8192)])


@pytest.mark.gpu
def test_supported_shapes():
    """Served: L = 3, d % 4 == 0, 164 <= d <= 512, K >= 4.  Not: rows that are only 8-byte aligned, the narrow kernel's widths,
    K = 3."""
    _need_gpu()
    for d in WIDTHS:
        rp = _module(N_NODES, d, 3)
        for K in (4, 20):
            assert _wide_supported(rp, 50, K) == 1, (d, K)
        assert _wide_supported(rp, 50, 3) == 0, d
    for d in (258, 160):
        assert _wide_supported(_module(N_NODES, d, 3), 50, 20) == 0, d
    # an unserved shape through the explicit entry: refused, nothing launched
    from tpnet_amd import _lib
    rp = _module(N_NODES, 160, 3)
    neigh, a1, a2 = _queries(np.random.RandomState(0), 3, 7)
    with pytest.raises(_lib.TPNetHipError):
        _wide(rp, _dev(neigh), _dev(a1), _dev(a2))


@pytest.mark.gpu
@pytest.mark.parametrize("not_scale", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_features_are_the_walks_bits(d, not_scale):
    """`gram` as the kernel leaves it = pair_gram_anchored(..., matrix_cores=False), bit for bit, at every shape; scaled features
    also against the oracle on the reference's pair list (rtol 1e-4, atol 1e-5, as test_encoder_widths.py), raw entries inside
    1e-6 |R_a| |R_b| + 2e-7 |G| of the float64 Gram."""
    _need_gpu()
    rp, st, queries = _case(d, not_scale)
    for (n, K), (neigh, a1, a2) in queries.items():
        assert _wide_supported(rp, n, K) == 1
        _, gram = _wide(rp, _dev(neigh), _dev(a1), _dev(a2))
        walk = rp.pair_gram_anchored(neigh, a1, a2, matrix_cores=False)
        assert torch.equal(gram, walk), (n, K)
        u = np.tile(neigh.reshape(-1), 2)
        v = np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])
        got = gram.view(-1, 64).cpu().numpy()
        if not_scale:
            want = _oracle_gram(st, u, v, not_scale=True, accumulate=np.float64).reshape(-1, 8, 8)
            bound = _raw_bound(want)
            e = np.abs(got.reshape(-1, 8, 8) - want)
            assert np.all(e <= bound), (n, K, float(np.max(e / (bound + 1e-30))))
        else:
            # (the oracle's Gram accumulated in float64, so that only the kernel's rounding is measured)
            want = _oracle_gram(st, u, v, accumulate=np.float64)
            print("d=%d n=%d K=%d: max |got - want| / (1e-5 + 1e-4 |want|) = %.3f"
                  % (d, n, K, float(np.max(np.abs(got - want) / (1e-5 + 1e-4 * np.abs(want))))))
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
    rp.check_device_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("d", WIDTHS)
def test_outputs_in_the_fp32_class(d):
    """Outputs against the torch layers on the walk's features: err <= 2e-5 scale + 1e-6 (the bound of
    test_one_launch_encoder_call_on_random_shapes_and_widths); the same bits with and without `gram`, and run to run."""
    _need_gpu()
    rp, _, queries = _case(d, False)
    for (n, K), (neigh, a1, a2) in queries.items():
        ids = _dev(neigh), _dev(a1), _dev(a2)
        out, gram = _wide(rp, *ids)
        out_nogram, _ = _wide(rp, *ids, want_gram=False)
        out_again, _ = _wide(rp, *ids)
        with torch.no_grad():
            want = rp.mlp(rp.pair_gram_anchored(neigh, a1, a2, matrix_cores=False).view(-1, 64))
        scale = float(want.abs().max())
        err = float((out - want).abs().max())
        print("d=%d n=%d K=%d: error / scale %.3g" % (d, n, K, err / scale))
        assert err <= 2e-5 * scale + 1e-6, (n, K, err, scale)
        assert torch.equal(out_nogram, out), (n, K)
        assert torch.equal(out_again, out), (n, K)
    rp.check_device_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [200, 508])
def test_a_mask_that_is_off_by_one_piece_shows(d):
    """Masked tails: rows of odd nodes 1e3 times the rows of even nodes, queries on even ids only -- the raw-entry bound holds only
    if no piece past a row's end is read (test_encoder_widths.py::test_the_raw_bound_exposes_one_piece_too_many: one piece too
    many misses it by more than 100 x)."""
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
    _, gram = _wide(rp, _dev(neigh), _dev(a1), _dev(a2))
    got = gram.view(-1, 8, 8).cpu().numpy()
    ratio = float(np.max(np.abs(got - want) / (bound + 1e-30)))
    print("raw entries / bound %.3f" % ratio)
    assert np.all(np.abs(got - want) <= bound), ratio
    rp.check_device_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [256, 512])
def test_ids_out_of_range_answer_nan_and_are_counted(d):
    """One bad neighbour, one bad anchor: NaN output (and feature) rows exactly for the pairs that hold them -- none in the other
    columns of the same tiles -- and check_device_errors raises IndexError."""
    _need_gpu()
    rng = np.random.RandomState(d)
    n, K = 37, 20
    rp = _module(N_NODES, d, 3)
    neigh = rng.randint(1, N_NODES, (n, K)).astype(np.int64)
    a1 = rng.randint(1, N_NODES, n).astype(np.int64)
    a2 = rng.randint(1, N_NODES, n).astype(np.int64)
    neigh[0, K - 1] = N_NODES + 5
    bad_row = n - 1
    a2[bad_row] = -3
    out, gram = _wide(rp, _dev(neigh), _dev(a1), _dev(a2))
    exp = np.zeros((2, n * K), dtype=bool)
    exp[:, K - 1] = True
    exp[:, bad_row * K:(bad_row + 1) * K] = True
    for got in (out.view(2, n * K, 64).cpu().numpy(), gram.cpu().numpy()):
        assert np.array_equal(np.isnan(got).all(axis=2), exp)
        assert not np.isnan(got[~exp]).any()
    with pytest.raises(IndexError):
        rp.check_device_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [256, 512])
def test_gradients_through_the_module(d):
    """get_pair_wise_feature_anchored with gradients recorded: the outputs keep the no-grad bits, and the gradients of self.mlp's
    four tensors match autograd on the torch layers."""
    _need_gpu()
    rng = np.random.RandomState(d + 1)
    n, K = 37, 20
    rp = _module(N_NODES, d, 3)
    for src, dst, t in _stream(rng, N_NODES, 150, 3):
        rp.update(src, dst, t)
    neigh, a1, a2 = _queries(rng, n, K)
    with torch.no_grad():
        got = rp.get_pair_wise_feature_anchored(_dev(neigh), _dev(a1), _dev(a2))
        feats = rp.pair_gram_anchored(neigh, a1, a2, matrix_cores=False).view(-1, 64)
        want = rp.mlp(feats)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 2e-5 * scale + 1e-6
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


@pytest.mark.gpu
def test_encoder_callers_at_256():
    """encoder_pair_features (device ids and host arrays) and the host-array pattern of get_pair_wise_feature at d = 256 against
    the reference's call sequence restated with the host sampler (comparison and tolerances of
    test_encoder_widths.py::test_encoder_call_from_the_sampler)."""
    _need_gpu()
    from tpnet_amd.callers import RecentNeighborSampler, encoder_pair_indices
    from tpnet_amd.sampler import GpuRecentNeighborSampler
    d, K = 256, 20
    rng = np.random.RandomState(d + K)
    N, E, B = 300, 1200, 120                                  # 4 B K = 9 600 pairs: a list long enough for the host-array pattern
    src = rng.randint(1, N, E).astype(np.int64)
    dst = rng.randint(1, N, E).astype(np.int64)
    t = np.sort(rng.uniform(1.0e6, 1.4e6, E))
    rp = _module(N, d, 3)
    host = RecentNeighborSampler(src, dst, t)
    gpu = GpuRecentNeighborSampler(src, dst, t, device="cuda:0", num_nodes=N)
    for b0 in range(0, E - B, B):
        s = slice(b0, b0 + B)
        if b0 >= 7 * B:
            other = rng.randint(1, N, B).astype(np.int64)
            neigh_h, _, _ = host.get_historical_neighbors(np.concatenate([src[s], other]), np.tile(t[s], 2), K)
            u, v = encoder_pair_indices(neigh_h, src[s], other)
            with torch.no_grad():
                want = rp.mlp(rp.pair_gram(_dev(u), _dev(v))).cpu().numpy()          # the general kernel + the torch layers
                got_p = rp.get_pair_wise_feature(u, v)                                  # the pattern on host arrays
                got, neigh_d = rp.encoder_pair_features(gpu, _dev(src[s]), _dev(other), _dev(t[s]), K)
                got_h, neigh_dh = rp.encoder_pair_features(gpu, src[s], other, t[s], K)
            np.testing.assert_array_equal(neigh_d.cpu().numpy(), neigh_h)
            np.testing.assert_array_equal(neigh_dh.cpu().numpy(), neigh_h)
            for g in (got_p, got, got_h):
                np.testing.assert_allclose(g.cpu().numpy(), want, rtol=2e-4, atol=2e-4)
        rp.update(src[s], dst[s], t[s])
    rp.check_device_errors()
