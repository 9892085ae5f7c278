"""The encoder's readout (models/TPNet.py:311-324) on the matrix cores for num_layer 1, 2 and 4, behind the opt-in switch
RandomProjectionModule.layers_readout (TPNET_FLAG_LAYERS_MFMA, csrc/encoder_layers.hip).  Helpers, cases and tolerances of
test_encoder_widths.py / test_encoder_even_widths.py; the raw-entry bound is theirs on (2L+2)^2 entries.

Tile geometry (LT = L + 1 rows per node, NB = 16 // LT neighbours per tile, the anchor operand holds 16 // (2 LT) nodes): the
enumeration is one function shared by the kernel and the host (tpnet_encoder_layers_tile), walked exhaustively on the CPU below; the
K values of the readout test (4, 5, 7: a node boundary at every tile offset for NB = 8, 5, 3) cover its use in the kernel.

Inputs: two update batches of 150 edges and a third, later one among the table's last three nodes, with time_decay_weight 2e-6 --
the rows every query touches then carry a PENDING decay (applied on read) between about 0.35 and 0.85, so a block that carries the
wrong power of it cannot hide."""
import ctypes as C

import numpy as np
import pytest
import torch

LAYERS = (1, 2, 4)
LAM = 2e-6
N_TABLE = 260


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _raw_bound(want):
    """|delta| <= 1e-6 |R_a| |R_b| + 2e-7 |G| per raw entry of the float64 Gram `want` [n, W, W] (test_encoder_widths.py::_raw_bound)."""
    W = want.shape[1]
    diag = np.sqrt(np.abs(want[:, np.arange(W), np.arange(W)]))
    return 1e-6 * diag[:, :, None] * diag[:, None, :] + 2e-7 * np.abs(want)


def _pairs(neigh, a1, a2):
    K = neigh.shape[1]
    return np.tile(neigh.reshape(-1), 2), np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])


def _layer_stream(rng, N):
    """Three batches: two of 150 edges with hubs (test_fused_feature.py::_stream), then 6 edges among nodes N-3 .. N-1 half a
    decay length later.  Returns the batches and, per node, the time of its last update (0: never)."""
    out, t0 = [], 0.0
    last = np.zeros(N)
    for b in range(3):
        if b < 2:
            src = rng.randint(1, N - 3, 150)
            dst = rng.randint(1, N - 3, 150)
            src[rng.rand(150) < 0.3] = 3
            dst[rng.rand(150) < 0.1] = 5
            t = np.sort(rng.uniform(t0, t0 + 2e5, 150))
        else:
            src = rng.randint(N - 3, N, 6)
            dst = rng.randint(N - 3, N, 6)
            t = np.sort(rng.uniform(t0 + 0.8e5, t0 + 1.0e5, 6))
        t0 = t[-1]
        last[src] = t0
        last[dst] = t0
        out.append((src.astype(np.int64), dst.astype(np.int64), t))
    return out, last


def _queries(rng, N, n, K):
    """n rows x K neighbours among the nodes the third batch left alone, 20 % id 0, one row with coinciding anchors."""
    neigh = rng.randint(0, N - 3, (n, K)).astype(np.int64)
    neigh[rng.rand(n, K) < 0.2] = 0
    a1 = rng.randint(1, N - 3, n).astype(np.int64)
    a2 = rng.randint(1, N - 3, n).astype(np.int64)
    a2[n // 2] = a1[n // 2]
    return neigh, a1, a2


def _pending(last, now, ids):
    return np.exp(-LAM * (now - last[ids]))


def _module(N, d, L, **kw):
    from test_fused_feature import _module as module
    return module(N, d, L, lam=LAM, **kw)


def _switched_on(N, d, L, **kw):
    rp = _module(N, d, L, **kw)
    rp.layers_readout = True
    return rp


def _layers_supported(rp, n, K):
    from tpnet_amd import _lib
    rp._ensure_engine()
    return _lib.load().tpnet_encoder_layers_supported(rp._st_ref(), n, K)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("L", LAYERS)
def test_the_raw_bound_exposes_a_wrong_power_a_wrong_row_and_a_block_left_unmirrored(L):
    """The oracle alone, on the CPU, on the readout test's inputs: the raw-entry bound is missed by more than 100 x when (a) a
    neighbour's rows carry the decay power of the adjacent layer (layer i: g^(i+1)), (b) a neighbour is paired with the NEXT row's
    anchors, (c) the anchor.w block is the w.anchor block copied, not transposed -- while the vector-ALU route's float32 model stays
    inside it.  The pending decay factors of the queried nodes spread over [0.3, 0.95]."""
    from oracle import tpnet_oracle as O
    rng = np.random.RandomState(40 + L)
    N, d, n, K = N_TABLE, 64, 37, 20
    LT, W = L + 1, 2 * L + 2
    st = O.OracleState(rng.randn(N, d).astype(np.float32), L, LAM, 0.0)
    batches, last = _layer_stream(rng, N)
    for src, dst, t in batches:
        O.update(st, src, dst, t)
    neigh, a1, a2 = _queries(rng, N, n, K)
    u, v = _pairs(neigh, a1, a2)
    g = _pending(last, float(st.now_time), np.concatenate([u, v]))
    print("pending decay factors: %.3f .. %.3f" % (g.min(), g.max()))
    assert 0.3 <= g.min() < 0.45 and 0.75 < g.max() <= 0.95
    want = O.pair_gram(st, u, v, not_scale=True, accumulate=np.float64).reshape(-1, W, W).astype(np.float64)
    bound = _raw_bound(want)

    def ratio(x):
        return (np.abs(x - want) / (bound + 1e-30)).max(axis=(1, 2))
    f32 = O.pair_gram(st, u, v, not_scale=True, accumulate=np.float32).reshape(-1, W, W)
    assert np.all(ratio(f32) <= 1.0), float(ratio(f32).max())
    # (a) w rows with one power of g too many: every pair shows it (layer 0's |R|^2 becomes g^2 |R|^2)
    gw = _pending(last, float(st.now_time), u)
    s = np.ones((u.size, W))
    s[:, :LT] = gw[:, None]
    r = ratio(want * s[:, :, None] * s[:, None, :])
    print("wrong decay power: smallest ratio %.3g" % r.min())
    assert np.all(r > 100.0), float(r.min())
    # (b) the next row's anchors
    vn = np.concatenate([np.repeat(np.roll(a1, -1), K), np.repeat(np.roll(a2, -1), K)])
    r = ratio(O.pair_gram(st, u, vn, not_scale=True, accumulate=np.float64).reshape(-1, W, W))
    differs = vn != v
    print("next row's anchors: smallest ratio %.3g over %d pairs" % (r[differs].min(), differs.sum()))
    assert differs.sum() > 0.9 * u.size and np.all(r[differs] > 100.0), float(r[differs].min())
    # (c) un-mirrored: where neighbour and anchor are distinct nodes with a history, the block is not symmetric
    x = want.copy()
    x[:, LT:, :LT] = want[:, :LT, LT:]
    r = ratio(x)
    live = (last[u] > 0) & (last[v] > 0) & (u != v)
    # (two inner products of unrelated rows differ by about |R_a| |R_b| / sqrt(d), 1e5 bounds; a pair whose two happen to agree
    # to 1e-4 of that is a coincidence of the draw, so the claim is about the bulk of the pairs, not about every one)
    print("un-mirrored block: ratio median %.3g, smallest %.3g, %.1f %% of %d pairs above 100" %
          (np.median(r[live]), r[live].min(), 100.0 * np.mean(r[live] > 100.0), live.sum()))
    assert live.sum() > 0.4 * u.size and np.mean(r[live] > 100.0) > 0.95 and np.median(r[live]) > 1e4, float(np.median(r[live]))


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("L", LAYERS)
def test_every_slot_is_in_one_tile_and_no_tile_outgrows_the_anchor_operand(L):
    """tpnet_encoder_layers_tile (the kernel's own enumeration, on the host) for K = 4..40 and enough rows that a tile starts at
    every offset of a row that tiles of NB slots reach (the multiples of gcd(NB, K) in 0..K-1): the tiles partition the slots in order, none is empty or longer than NB, and none touches more
    rows than the anchor operand holds (16 // (2 LT): 4, 2, 1)."""
    from tpnet_amd import _lib
    lib = _lib.load()
    LT = L + 1
    NB, NA = 16 // LT, 16 // (2 * LT)
    s0, cnt = C.c_int64(0), C.c_int32(0)
    for K in range(4, 41):
        n_rows = 2 * NB + 3
        T = n_rows * K
        nt = int(lib.tpnet_encoder_layers_tiles(L, n_rows, K))
        assert nt > 0
        nxt, offsets = 0, set()
        for t in range(nt):
            assert lib.tpnet_encoder_layers_tile(L, n_rows, K, t, C.byref(s0), C.byref(cnt)) == 0
            assert s0.value == nxt and 1 <= cnt.value <= NB, (K, t, s0.value, cnt.value)
            nxt = s0.value + cnt.value
            offsets.add(s0.value % K)
            spanned = (nxt - 1) // K - s0.value // K + 1
            assert spanned <= NA, (K, t, spanned)
        assert nxt == T
        if L != 4:
            assert offsets == set(range(0, K, int(np.gcd(NB, K)))), (K, sorted(offsets))   # every offset tiles of NB slots can reach
        else:
            assert offsets == set(range(0, K, NB)), (K, sorted(offsets))      # tiles end at row ends: short last tile
        assert lib.tpnet_encoder_layers_tile(L, n_rows, K, nt, C.byref(s0), C.byref(cnt)) != 0
    assert lib.tpnet_encoder_layers_tiles(3, 10, 20) == 0 and lib.tpnet_encoder_layers_tiles(L, 10, 3) == 0


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.gpu
def test_support_and_switch():
    """tpnet_encoder_layers_supported: 1 at L = 1, 2, 4 for d = 64 / 120 / 128 / 160 and K = 4 / 20; 0 for K = 3, d = 34 / 164 / 110 and
    L = 3.  The switch is off by default and then every call keeps its bits; with it, matrix_cores=False and
    TPNET_FLAG_NO_MFMA_READOUT give the walk's bits, L = 3 is untouched, and shapes the kernel declines (K = 3, unaligned
    outputs) take the walk with TPNET_OK."""
    _need_gpu()
    from tpnet_amd import _lib
    lib = _lib.load()
    assert _lib.FLAG_LAYERS_MFMA == 1024
    for L in LAYERS:
        for d in (64, 120, 128, 160):
            rp = _module(300, d, L)
            assert _layers_supported(rp, 50, 20) == 1 and _layers_supported(rp, 50, 4) == 1, (L, d)
            assert _layers_supported(rp, 50, 3) == 0, (L, d)
        for d in (34, 164, 110):
            assert _layers_supported(_module(300, d, L), 50, 20) == 0, (L, d)
    assert _layers_supported(_module(300, 128, 3), 50, 20) == 0
    rp110 = _module(300, 110, 2)
    rp110._ensure_engine()
    assert lib.tpnet_encoder_rows8_supported(rp110._st_ref(), 50, 20, None) == 0
    rng = np.random.RandomState(3)
    N, d, n, K = N_TABLE, 128, 9, 5
    rp = _module(N, d, 2)
    assert rp.layers_readout is False and type(rp).layers_readout is False
    batches, _ = _layer_stream(rng, N)
    for src, dst, t in batches:
        rp.update(src, dst, t)
    neigh, a1, a2 = _queries(rng, N, n, K)
    walk = rp.pair_gram_anchored(neigh, a1, a2, matrix_cores=False)
    assert torch.equal(rp.pair_gram_anchored(neigh, a1, a2), walk)                            # switch off: the walk
    rp.layers_readout = True
    assert rp._readout_flags() & _lib.FLAG_LAYERS_MFMA and not rp._readout_flags(matrix_cores=False) & _lib.FLAG_LAYERS_MFMA
    assert torch.equal(rp.pair_gram_anchored(neigh, a1, a2, matrix_cores=False), walk)
    mc = rp.pair_gram_anchored(neigh, a1, a2)
    assert not torch.equal(mc, walk)                                                          # another summation order: other bits
    torch.testing.assert_close(mc, walk, rtol=2e-5, atol=2e-6)
    # the C call
    F = rp.pair_wise_feature_dim
    # (the K = 3 call below reads the same 45 slots as 15 rows: anchors for 15 rows, the first 9 the call's own)
    wd, d1, d2 = _dev(neigh.reshape(-1)), _dev(np.concatenate([a1, a2[:6]])), _dev(np.concatenate([a2, a1[:6]]))
    out = torch.zeros((2 * n * K * F + 4,), dtype=torch.float32, device="cuda:0")
    now, lam, s = rp._now_host, float(rp.time_decay_weight), rp._stream()

    def gram_call(flags, K_=K, off=0):
        rows = (n * K) // K_
        out.zero_()
        base = out.data_ptr() + off
        rc = lib.tpnet_pair_gram_anchored(rp._st_ref(), wd.data_ptr(), d1.data_ptr(), d2.data_ptr(), rows, K_, now, lam, flags, base,
                                          base + rows * K_ * F * 4, s)
        torch.cuda.synchronize()
        return rc, out[off // 4: off // 4 + 2 * rows * K_ * F].clone()
    base_flags = rp._readout_flags(matrix_cores=False) & ~_lib.FLAG_NO_MFMA_READOUT
    rc, ref = gram_call(base_flags)
    assert rc == 0 and torch.equal(ref, walk.view(-1))
    rc, got = gram_call(base_flags | _lib.FLAG_LAYERS_MFMA)
    assert rc == 0 and torch.equal(got, mc.view(-1))
    rc, got = gram_call(base_flags | _lib.FLAG_LAYERS_MFMA | _lib.FLAG_NO_MFMA_READOUT)
    assert rc == 0 and torch.equal(got, ref)
    rc, got = gram_call(base_flags | _lib.FLAG_LAYERS_MFMA, off=8)                            # outputs not 16-byte aligned: the walk
    assert rc == 0 and torch.equal(got, ref)
    rc3, ref3 = gram_call(base_flags, K_=3)
    rc, got = gram_call(base_flags | _lib.FLAG_LAYERS_MFMA, K_=3)                             # K < 4: the walk
    assert rc3 == 0 and rc == 0 and torch.equal(got, ref3)
    rp.check_device_errors()
    # L = 3: the flag changes nothing
    rp3 = _module(N, d, 3)
    for src, dst, t in batches:
        rp3.update(src, dst, t)
    a = rp3.pair_gram_anchored(neigh, a1, a2)
    rp3.layers_readout = True
    assert rp3._readout_flags() & _lib.FLAG_LAYERS_MFMA == 0
    assert torch.equal(rp3.pair_gram_anchored(neigh, a1, a2), a)
    F3 = rp3.pair_wise_feature_dim
    o3 = torch.empty((2, 2 * n * K * F3), dtype=torch.float32, device="cuda:0")
    for i, fl in enumerate((0, _lib.FLAG_LAYERS_MFMA)):
        assert lib.tpnet_pair_gram_anchored(rp3._st_ref(), wd.data_ptr(), d1.data_ptr(), d2.data_ptr(), n, K, rp3._now_host, lam, fl,
                                            o3[i].data_ptr(), o3[i].data_ptr() + n * K * F3 * 4, rp3._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(o3[0], o3[1]) and torch.equal(o3[0], a.view(-1))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.gpu
@pytest.mark.parametrize("K,n", [(4, 9), (5, 13), (7, 3), (20, 37), (33, 3), (20, 2000)])
@pytest.mark.parametrize("d", (64, 120, 128, 140))
@pytest.mark.parametrize("L", LAYERS)
def test_readout_against_the_oracle(L, d, K, n):
    """tpnet_pair_gram_anchored with TPNET_FLAG_LAYERS_MFMA against the oracle on the reference's pair list, against the vector-ALU
    walk and the general pair kernel: the three update batches and the queries of the header; scaled features by relative
    tolerance, raw entries (not_scale) inside 1e-6 |R_a| |R_b| + 2e-7 |G| of the float64 Gram on both routes."""
    _need_gpu()
    from oracle import tpnet_oracle as O
    rng = np.random.RandomState(K * 131 + d + n + 7 * L)
    N, W = N_TABLE, 2 * L + 2
    for not_scale in (False, True):
        rp = _switched_on(N, d, L, not_scale=not_scale)
        assert _layers_supported(rp, n, K) == 1
        st = O.OracleState(rp.random_projections[0].detach().cpu().numpy(), L, LAM, 0.0)
        batches, _ = _layer_stream(rng, N)
        for src, dst, t in batches:
            rp.update(src, dst, t)
            O.update(st, src, dst, t)
        neigh, a1, a2 = _queries(rng, N, n, K)
        u, v = _pairs(neigh, a1, a2)
        got = rp.pair_gram_anchored(neigh, a1, a2).view(-1, W * W).cpu().numpy()
        valu = rp.pair_gram_anchored(neigh, a1, a2, matrix_cores=False).view(-1, W * W).cpu().numpy()
        gen = rp.pair_gram(u, v).cpu().numpy()
        if not_scale:
            want = O.pair_gram(st, u, v, not_scale=True, accumulate=np.float64).reshape(-1, W, W)
            bound = _raw_bound(want)
            e_mc = np.abs(got.reshape(-1, W, W) - want)
            e_va = np.abs(valu.reshape(-1, W, W) - want)
            print("raw entries / bound: matrix cores %.3f, vector ALUs %.3f" % (float(np.max(e_mc / (bound + 1e-30))),
                                                                               float(np.max(e_va / (bound + 1e-30)))))
            assert np.all(e_mc <= bound), float(np.max(e_mc / (bound + 1e-30)))
            assert np.all(e_va <= bound), float(np.max(e_va / (bound + 1e-30)))
        else:
            want = O.pair_gram(st, u, v)
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(got, valu, rtol=2e-5, atol=2e-6)
            np.testing.assert_allclose(got, gen, rtol=2e-5, atol=2e-6)
        rp.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.gpu
@pytest.mark.parametrize("d", (120, 140))
@pytest.mark.parametrize("L", LAYERS)
def test_a_mask_that_is_off_by_one_piece_shows(L, d):
    """The table of test_encoder_widths.py::test_a_mask_that_is_off_by_one_piece_shows (rows of odd nodes 1e3 times the rows of even
    nodes, queries on even ids only, the table's last even node among them): the raw-entry bound holds only if the masked last
    step reads nothing past a row's end and drops nothing inside it."""
    _need_gpu()
    from oracle import tpnet_oracle as O
    from test_encoder_widths import _alternating_state, _even_queries
    rng = np.random.RandomState(d + L)
    N, n, K, W = 261, 40, 20, 2 * L + 2
    P = _alternating_state(rng, N, d, L)
    rp = _switched_on(N, d, L, not_scale=True)
    rp.random_projections[0].data = torch.from_numpy(P[0]).cuda()
    rp.reload_random_projections((torch.tensor(0.0, dtype=torch.float64, device="cuda:0"),
                                  [torch.from_numpy(P[i]).cuda() for i in range(1, L + 1)]))
    st = O.OracleState(P[0], L, LAM, 0.0)
    for i in range(1, L + 1):
        st.P[i] = P[i].copy()
    neigh, a1, a2 = _even_queries(rng, N, n, K)
    u, v = _pairs(neigh, a1, a2)
    want = O.pair_gram(st, u, v, not_scale=True, accumulate=np.float64).reshape(-1, W, W)
    bound = _raw_bound(want)
    assert _layers_supported(rp, n, K) == 1
    got = rp.pair_gram_anchored(neigh, a1, a2).view(-1, W, W).cpu().numpy()
    ratio = float(np.max(np.abs(got - want) / (bound + 1e-30)))
    print("raw entries / bound %.3f" % ratio)
    assert np.all(np.abs(got - want) <= bound), ratio
    rp.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.gpu
@pytest.mark.parametrize("L", LAYERS)
def test_ids_out_of_range_answer_nan_and_are_counted(L):
    """NaN rows exactly for the pairs that hold an id out of range (a neighbour: its two pairs; an anchor: its row's 2 K pairs);
    check_device_errors raises IndexError -- as at L = 3."""
    _need_gpu()
    rng = np.random.RandomState(110 + L)
    N, d, n, K = N_TABLE, 120, 37, 20
    rp = _switched_on(N, d, L)
    neigh = rng.randint(1, N, (n, K)).astype(np.int64)
    a1 = rng.randint(1, N, n).astype(np.int64)
    a2 = rng.randint(1, N, n).astype(np.int64)
    neigh[0, K - 1] = N + 5
    neigh[7, 3] = -1
    bad_row = n - 1
    a2[bad_row] = -3
    a1[11] = N
    assert _layers_supported(rp, n, K) == 1
    got = rp.pair_gram_anchored(_dev(neigh), _dev(a1), _dev(a2)).cpu().numpy()
    nanrow = np.isnan(got).all(axis=2)
    exp = np.zeros((2, n * K), dtype=bool)
    exp[:, K - 1] = True
    exp[:, 7 * K + 3] = True
    exp[:, bad_row * K:(bad_row + 1) * K] = True
    exp[:, 11 * K:12 * K] = True
    assert np.array_equal(nanrow, exp)
    assert not np.isnan(got[~exp]).any()
    with pytest.raises(IndexError):
        rp.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 7
class _Served:
    """Counts the C readouts that took the matrix cores: tpnet_pair_gram_anchored / tpnet_encoder_gram called with
    TPNET_FLAG_LAYERS_MFMA and without TPNET_FLAG_NO_MFMA_READOUT on a shape tpnet_encoder_layers_supported accepts."""

    def __init__(self, monkeypatch):
        from tpnet_amd import _lib
        self.lib, self.calls = _lib.load(), []
        for name, i_rows, i_k, i_flags, twice in (("tpnet_pair_gram_anchored", 4, 5, 8, 1), ("tpnet_encoder_gram", 7, 8, 11, 2)):
            inner = getattr(self.lib, name)

            def spy(*a, _inner=inner, _name=name, _r=i_rows, _k=i_k, _f=i_flags, _m=twice):
                on = bool(a[_f] & _lib.FLAG_LAYERS_MFMA) and not a[_f] & _lib.FLAG_NO_MFMA_READOUT
                self.calls.append((_name, on and self.lib.tpnet_encoder_layers_supported(a[0], _m * a[_r], a[_k]) == 1))
                return _inner(*a)
            monkeypatch.setattr(self.lib, name, spy)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.mark.gpu
@pytest.mark.parametrize("L", LAYERS)
def test_routes(L, monkeypatch):
    """With the switch on, get_pair_wise_feature_anchored (device ids), encoder_pair_features (device ids and host arrays, recent
    sampler) and get_pair_wise_feature on the encoder's host pattern equal self.mlp on the oracle's features (rtol = atol = 2e-4, the
    tolerance of test_encoder_even_widths.py for the same routes), and each is served by ONE C readout on the matrix cores."""
    _need_gpu()
    from oracle import tpnet_oracle as O
    from tpnet_amd.callers import RecentNeighborSampler, encoder_pair_indices
    from tpnet_amd.sampler import GpuRecentNeighborSampler
    rng = np.random.RandomState(70 + L)
    N, d, K, B, E = 300, 128, 20, 60, 600
    src = rng.randint(1, N, E).astype(np.int64)
    dst = rng.randint(1, N, E).astype(np.int64)
    t = np.sort(rng.uniform(1.0e5, 4.0e5, E))
    rp = _switched_on(N, d, L)
    st = O.OracleState(rp.random_projections[0].detach().cpu().numpy(), L, LAM, 0.0)
    for b0 in range(0, 450, 150):
        s = slice(b0, b0 + 150)
        rp.update(src[s], dst[s], t[s])
        O.update(st, src[s], dst[s], t[s])
    served = _Served(monkeypatch)

    def want_of(u, v):
        with torch.no_grad():
            return rp.mlp(_dev(O.pair_gram(st, u, v))).cpu().numpy()

    def check(got, u, v, calls, what):
        np.testing.assert_allclose(got.detach().cpu().numpy(), want_of(u, v), rtol=2e-4, atol=2e-4, err_msg=what)
        assert len(calls) == 1 and calls[0][1], (what, calls)
    # the anchored call, device ids
    neigh = rng.randint(0, N, (37, K)).astype(np.int64)
    a1, a2 = rng.randint(1, N, 37).astype(np.int64), rng.randint(1, N, 37).astype(np.int64)
    u, v = _pairs(neigh, a1, a2)
    with torch.no_grad():
        got = rp.get_pair_wise_feature_anchored(_dev(neigh), _dev(a1), _dev(a2))
    check(got, u, v, served.take(), "anchored")
    # the sampler's call, device ids and host arrays
    s = slice(450, 450 + B)
    other = rng.randint(1, N, B).astype(np.int64)
    host = RecentNeighborSampler(src, dst, t)
    gpu = GpuRecentNeighborSampler(src, dst, t, device="cuda:0", num_nodes=N)
    neigh_h, _, _ = host.get_historical_neighbors(np.concatenate([src[s], other]), np.tile(t[s], 2), K)
    u, v = encoder_pair_indices(neigh_h, src[s], other)
    with torch.no_grad():
        got, neigh_d = rp.encoder_pair_features(gpu, _dev(src[s]), _dev(other), _dev(t[s]), K)
    np.testing.assert_array_equal(neigh_d.cpu().numpy(), neigh_h)
    calls = [c for c in served.take() if c[0] == "tpnet_encoder_gram"]
    check(got, u, v, calls, "encoder_pair_features, device ids")
    with torch.no_grad():
        got, neigh_d = rp.encoder_pair_features(gpu, src[s], other, t[s], K)
    np.testing.assert_array_equal(neigh_d.cpu().numpy(), neigh_h)
    calls = [c for c in served.take() if c[0] == "tpnet_encoder_gram"]
    check(got, u, v, calls, "encoder_pair_features, host arrays")
    # get_pair_wise_feature on the host pattern, longer than every staged route takes
    from tpnet_amd import fused_feature
    K4 = 4
    rows = max(rp._eng["stage"].max_pairs, fused_feature.MAX_PAIRS) // (2 * K4) + 1
    neigh = rng.randint(0, N, (rows, K4)).astype(np.int64)
    a1 = (1 + (np.arange(rows) % (N - 1))).astype(np.int64)                   # consecutive anchors differ: the pattern's K is 4
    a2 = (1 + ((np.arange(rows) + 7) % (N - 1))).astype(np.int64)
    u, v = _pairs(neigh, a1, a2)
    with torch.no_grad():
        got = rp.get_pair_wise_feature(u, v)
    check(got, u, v, served.take(), "get_pair_wise_feature, host pattern")
    rp.layers_readout = False
    with torch.no_grad():
        off = rp.get_pair_wise_feature(u, v)
    assert not any(c[1] for c in served.take())
    np.testing.assert_allclose(off.cpu().numpy(), got.cpu().numpy(), rtol=2e-4, atol=2e-4)
    rp.check_device_errors()


@pytest.mark.gpu
def test_a_training_step_at_two_layers(monkeypatch):
    """One tpnet_amd.TPNet forward and backward at num_layer 2 with the switch on: the matrix-core readout serves, the gradients of
    random_projections.mlp's four tensors are finite and equal the switch-off step's within 1e-4 of their scale."""
    _need_gpu()
    import tpnet_amd
    from tpnet_amd.sampler import GpuRecentNeighborSampler
    N, K, B, E = 300, 20, 60, 900
    rp = _module(N, 128, 2)
    rng = np.random.RandomState(222)
    src = rng.randint(1, N, E).astype(np.int64)
    dst = rng.randint(1, N, E).astype(np.int64)
    t = np.sort(rng.uniform(1.0e5, 4.0e5, E))
    torch.manual_seed(22)
    model = tpnet_amd.TPNet(node_raw_features=rng.randn(N, 32).astype(np.float32), edge_raw_features=rng.randn(E + 1, 32).astype(np.float32),
                            neighbor_sampler=GpuRecentNeighborSampler(src, dst, t, device="cuda:0", num_nodes=N), time_feat_dim=20,
                            dropout=0.0, random_projections=rp, num_layers=2, num_neighbors=K, device="cuda:0").to("cuda:0")
    model.train()
    for b0 in range(0, 600, 150):
        rp.update(src[b0:b0 + 150], dst[b0:b0 + 150], t[b0:b0 + 150])
    served = _Served(monkeypatch)
    s = slice(600, 600 + B)
    grads = {}
    for on in (False, True):
        rp.layers_readout = on
        for p in model.parameters():
            p.grad = None
        es, ed = model.compute_src_dst_node_temporal_embeddings(src[s], dst[s], t[s])
        (es * ed).sum().backward()
        grads[on] = [p.grad.detach().double().cpu().numpy() for p in rp.mlp.parameters()]
        calls = served.take()
        assert any(c[1] for c in calls) == on, (on, calls)
    assert len(grads[True]) == 4
    for g_on, g_off in zip(grads[True], grads[False]):
        assert np.all(np.isfinite(g_on))
        scale = max(float(np.abs(g_off).max()), 1e-30)
        err = float(np.abs(g_on - g_off).max()) / scale
        print("gradient, switch on against off: %.3e of scale" % err)
        assert err <= 1e-4
    rp.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.gpu
def test_readout_on_random_shapes_and_widths():
    """Twenty seeded (L, d, K, n) shapes, d % 4 == 0 in 36..160, K in 4..40, n in 1..300: the matrix-core Gram against the general
    pair kernel's at 2e-5 of scale (the bound of test_encoder_even_widths.py::test_one_launch_encoder_call_on_random_shapes_and_widths,
    here on the features before self.mlp)."""
    _need_gpu()
    rng = np.random.RandomState(2027)
    N = N_TABLE
    for trial in range(20):
        L = int(rng.choice(LAYERS))
        d = 4 * int(rng.randint(9, 41))
        K = int(rng.randint(4, 41))
        n = int(rng.randint(1, 301))
        rp = _switched_on(N, d, L)
        batches, _ = _layer_stream(rng, N)
        for src, dst, t in batches[:2]:
            rp.update(src, dst, t)
        neigh = rng.randint(0, N, (n, K)).astype(np.int64)
        a1, a2 = rng.randint(1, N, n).astype(np.int64), rng.randint(1, N, n).astype(np.int64)
        u, v = _pairs(neigh, a1, a2)
        assert _layers_supported(rp, n, K) == 1
        got = rp.pair_gram_anchored(_dev(neigh), _dev(a1), _dev(a2)).view(-1, rp.pair_wise_feature_dim)
        want = rp.pair_gram(_dev(u), _dev(v))
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        assert err <= 2e-5 * scale + 1e-6, (trial, L, d, K, n, err, scale)
        rp.check_device_errors()
