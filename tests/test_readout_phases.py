"""The finish phase of the readout (clamp, log, NaN for a bad id, the store) per store path, as a matrix of row width x L.

csrc/readout.hpp has three tails behind a one-pair Gram (reduction through LDS; recursive halving with an LDS-staged whole-line
store at 4 and 8 lanes per row; recursive halving with a direct store) and the slot picks of the two-output kernels; which one
serves a call depends on the row width d and on L.  The widths below take every one of them:

    d = 12    4 lanes, not exact fit, staged store        d = 100   32 lanes, tail predicate
    d = 16    4 lanes, exact fit                          d = 256   32 lanes x 2 vectors
    d = 32    8 lanes, exact fit                          d = 260   64 lanes x 2 vectors, chunk loop
    d = 64    16 lanes: LDS reduction at L <= 3,          d = 30    one float per lane
              halving + direct store at L = 4

at L = 1..4: packed rows of 10, 21, 36 and 55 floats, so only L = 3 takes the 16-byte store of the staged path.

Fixture: N = 64 nodes, update() batches of 40 seeded edges, lambda = 1e-6, n = 37 pairs (a partly filled workgroup at 64, 32, 16,
8 and 4 lane groups per 256 threads).  An update reads the rows of BEFORE its batch, so layer i is filled by the i-th batch at the
earliest: the fixture applies max(2, L) batches (two where two suffice, L at L = 3 and 4), so that every layer 1..L is non-zero and
every entry of the Gram is a number that a wrong slot, mirror or decay power would change.  Nodes are split into two halves with
rows of opposite sign and edges stay inside a half: every inner product of two non-zero rows is far from zero (no entry of the
float64 Gram within 1e-3 * ||R_a|| ||R_b|| of it -- test_fixture_has_no_entry_near_the_clamp checks that without a GPU), so the
log tolerance never decides a result at the clamp, and pairs across the halves are negative: the clamp is taken.

Tolerances and helpers are test_gpu_parity's (_assert_features; raw Gram within _gram_bound at 1e-4).  Cells another test
already asserts and that are left out here: pair_gram_shared against the oracle at (d, L) = (64, 2), (256, 3), (30, 4) --
test_gpu_parity.py::test_shared_first_node_readout.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import tpnet_oracle as O
from test_gpu_parity import DEV, _assert_features, _gram_bound, _module, _need_gpu

WIDTHS = [12, 16, 32, 64, 100, 256, 260, 30]
LAYERS = [1, 2, 3, 4]
N, EB, NP, K, LAM = 64, 40, 37, 5, 1e-6
SHARED_ELSEWHERE = {(64, 2), (256, 3), (30, 4)}
SEED = 7


@functools.lru_cache(maxsize=None)
def _batches(L):
    return max(2, L)


@functools.lru_cache(maxsize=None)
def _inputs(d, L):
    """Seeded inputs and the oracle's state after the batches (computed once per cell, never modified)."""
    nb = _batches(L)
    rng = np.random.RandomState(SEED + 1000 * d + L)
    half = rng.permutation(N) < N // 2                                # the half of each node
    sign = np.where(half, 1.0, -1.0)[:, None]
    P0 = (sign * rng.uniform(0.5, 1.5, (N, d)) / np.sqrt(d)).astype(np.float32)
    src = rng.randint(0, N, nb * EB).astype(np.int64)
    same = [np.flatnonzero(half == half[s]) for s in src]
    dst = np.array([m[rng.randint(len(m))] for m in same], dtype=np.int64)      # an edge stays inside its half
    t = np.sort(rng.uniform(1.0, 2.0e5, nb * EB))
    st = O.OracleState(P0, L, LAM, 0.0)
    for b in range(nb):
        s = slice(b * EB, (b + 1) * EB)
        O.update(st, src[s], dst[s], t[s])
    full = np.flatnonzero(np.all([np.abs(st.P[i]).max(axis=1) > 0 for i in range(1, L + 1)], axis=0))
    u = full[rng.randint(0, len(full), NP)]                           # first nodes: every layer filled; the others: any node
    v = rng.randint(0, N, NP).astype(np.int64)
    v2 = rng.randint(0, N, NP).astype(np.int64)
    neigh = rng.randint(0, N, (NP, K)).astype(np.int64)
    return dict(P0=P0, src=src, dst=dst, t=t, st=st, u=u, v=v, v2=v2, neigh=neigh)


def _near_clamp(st, u, v):
    """Entries of the float64 Gram of two NON-ZERO rows that lie within 1e-3 * ||R_a|| ||R_b|| of zero."""
    g64 = O.pair_gram(st, u, v, not_scale=True, accumulate=np.float64).astype(np.float64)
    bound = _gram_bound(st.P, u, v, st.L, 1e-3)
    return int(((bound > 1e-20) & (np.abs(g64) <= bound)).sum())


@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("d", WIDTHS)
def test_fixture_has_no_entry_near_the_clamp(d, L):
    f = _inputs(d, L)
    w = f["neigh"].reshape(-1)
    pairs = [(f["u"], f["v"]), (f["u"], f["v2"]), (w, np.repeat(f["u"], K)), (w, np.repeat(f["v"], K))]
    assert sum(_near_clamp(f["st"], a, b) for a, b in pairs) == 0
    raw = O.pair_gram(f["st"], f["u"], f["v"], not_scale=True)
    assert (raw < 0).any() and (raw > 0).any()                        # both sides of the clamp are in the fixture
    rows = np.concatenate([f["u"], f["v"], f["v2"], w])
    for i in range(1, L + 1):
        assert np.abs(f["st"].P[i]).max() > 0                         # every layer is filled ...
        assert (np.abs(f["st"].P[i][f["u"]]).max(axis=1) > 0).all()            # ... for every first node ...
        assert (np.abs(f["st"].P[i][rows]).max(axis=1) > 0).mean() > 0.25     # ... and for many of the other nodes that are read


@functools.lru_cache(maxsize=None)
def _cell(d, L):
    """The module after the batches, ids on the device, and the clean outputs the out-of-range test compares with."""
    f = _inputs(d, L)
    rp = _module(N, d, L, LAM, 0.0, P0=f["P0"])
    for b in range(_batches(L)):
        s = slice(b * EB, (b + 1) * EB)
        rp.update(f["src"][s], f["dst"][s], f["t"][s])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    ids = {k: dev(f[k]) for k in ("u", "v", "v2")}
    ids["neigh"] = dev(f["neigh"])
    anchored = bool(d % 4 == 0 and 36 <= d <= 512)
    from tpnet_amd import _lib
    assert bool(_lib.load().tpnet_pair_gram_anchored_supported(rp._st_ref())) == anchored
    return rp, f, ids, anchored


def _calls(rp, ids, anchored, u, v, neigh):
    """Every variant of the three readouts on device ids, as numpy arrays."""
    out = {"default": rp.pair_gram(u, v), "raw": rp.pair_gram(u, v, raw=True), "packed": rp.pair_gram(u, v, packed=True)}
    out["shared1"], out["shared2"] = rp.pair_gram_shared(u, v, ids["v2"])
    if anchored:
        a = rp.pair_gram_anchored(neigh, u, v, matrix_cores=False)
        out["anchored1"], out["anchored2"] = a[0], a[1]
    return {k: x.cpu().numpy() for k, x in out.items()}


@functools.lru_cache(maxsize=None)
def _clean(d, L):
    rp, f, ids, anchored = _cell(d, L)
    got = _calls(rp, ids, anchored, ids["u"], ids["v"], ids["neigh"])
    rp.check_device_errors()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("d", WIDTHS)
def test_pair_gram_default_raw_packed(d, L):
    _need_gpu()
    f = _inputs(d, L)
    got = _clean(d, L)
    st, u, v = f["st"], f["u"], f["v"]
    NN = 2 * L + 2
    _assert_features(got["default"], st, u, v, f"d={d} L={L} default")
    want = O.pair_gram(st, u, v, not_scale=True)
    err = np.abs(got["raw"] - want)
    bound = _gram_bound(st.P, u, v, L, 1e-4)
    print(f"d={d} L={L}: raw worst |delta| / bound = {(err / bound).max():.3e}")
    assert np.all(err <= bound), f"d={d} L={L} raw: worst |delta| / bound {(err / bound).max():.3e}"
    a, b = np.triu_indices(NN)                                        # row-major upper triangle
    assert got["packed"].shape == (NP, NN * (NN + 1) // 2)
    assert np.array_equal(got["packed"].view(np.uint32), got["raw"].reshape(NP, NN, NN)[:, a, b].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("d", WIDTHS)
def test_shared_and_anchored(d, L):
    _need_gpu()
    f = _inputs(d, L)
    got = _clean(d, L)
    st, u, v, v2 = f["st"], f["u"], f["v"], f["v2"]
    if (d, L) not in SHARED_ELSEWHERE:
        _assert_features(got["shared1"], st, u, v, f"d={d} L={L} shared 1")
        _assert_features(got["shared2"], st, u, v2, f"d={d} L={L} shared 2")
    if "anchored1" in got:
        w = f["neigh"].reshape(-1)
        _assert_features(got["anchored1"], st, w, np.repeat(u, K), f"d={d} L={L} anchored 1")
        _assert_features(got["anchored2"], st, w, np.repeat(v, K), f"d={d} L={L} anchored 2")


@pytest.mark.gpu
@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("d", WIDTHS)
def test_out_of_range_id_gives_nan_rows_and_one_error(d, L):
    """One pair holds the id N (for the anchored readout: one neighbour, then one anchor, whose K outputs all go): its rows are NaN
    in every variant, every other row is the clean call's bit for bit, and the error is reported once."""
    _need_gpu()
    rp, f, ids, anchored = _cell(d, L)
    clean = _clean(d, L)
    bad_pair, bad_row, bad_k = 11, 23, 3
    v_bad = ids["v"].clone()
    v_bad[bad_pair] = N
    neigh_bad = ids["neigh"].clone()
    neigh_bad[bad_row, bad_k] = N

    def check(got, names, bad):
        for name in names:
            x, c = got[name], clean[name]
            assert np.isnan(x[bad]).all(), f"d={d} L={L} {name}: the bad pair's row is not all NaN"
            keep = np.ones(len(x), dtype=bool)
            keep[bad] = False
            assert np.array_equal(x[keep].view(np.uint32), c[keep].view(np.uint32)), f"d={d} L={L} {name}: another row moved"

    def reported_once():
        with pytest.raises(IndexError):
            rp.check_device_errors()
        rp.check_device_errors()

    rp.check_device_errors()
    u = ids["u"]
    got = {"default": rp.pair_gram(u, v_bad), "raw": rp.pair_gram(u, v_bad, raw=True),
           "packed": rp.pair_gram(u, v_bad, packed=True)}
    check({k: x.cpu().numpy() for k, x in got.items()}, ("default", "raw", "packed"), bad_pair)
    reported_once()
    s1, s2 = rp.pair_gram_shared(u, v_bad, ids["v2"])
    check({"shared1": s1.cpu().numpy(), "shared2": s2.cpu().numpy()}, ("shared1", "shared2"), bad_pair)
    reported_once()
    if anchored:
        a = rp.pair_gram_anchored(neigh_bad, u, ids["v"], matrix_cores=False).cpu().numpy()
        check({"anchored1": a[0], "anchored2": a[1]}, ("anchored1", "anchored2"), bad_row * K + bad_k)
        reported_once()
        a = rp.pair_gram_anchored(ids["neigh"], u, v_bad, matrix_cores=False).cpu().numpy()
        check({"anchored1": a[0], "anchored2": a[1]}, ("anchored1", "anchored2"), np.arange(bad_pair * K, bad_pair * K + K))
        reported_once()
