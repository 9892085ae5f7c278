"""The one-vs-many ranking evaluation on the GPU: the fan-out readout (tpnet_pair_gram_fanout, csrc/fanout.hip) against the oracle on
the expanded pairs, the per-query candidates (tpnet_neg_sample_many) against the Python restatement bit for bit, the ranking record
(tpnet_lp_ranking) against the host rule, and `evaluate_link_ranking` against a straight-line restatement.

Readout tolerances are the project's own: test_gpu_parity._assert_features for the scaled features, _gram_bound at 1e-4 for the raw
Gram, C_DENSE = 2e-5 of the output scale for self.mlp behind it (tests/test_mlp_rows.py, tests/test_host_routes.py).  The fixture
of the readout matrix is test_readout_phases' (its _inputs: N = 64 nodes in two halves of opposite sign, every layer filled, no
entry near the clamp): B = 37 rows of C = 5 candidates = its `u` against its `neigh`.

The loop's tolerance (test_loop_against_a_straight_line_restatement) is worked out there."""
import functools

import numpy as np
import pytest
import torch

from oracle import tpnet_oracle as O
from test_fused_feature import _assert_mlp_grads_close
from test_gpu_parity import DEV, _assert_features, _gram_bound, _layers, _module, _need_gpu
from test_link_ranking_host import (FLAG_EMPTY, FLAG_NAN, FLAG_NO_QUERY, assert_record, assert_row_promises, batch_of, graph,
                                    record_cases, restated_rows)
from test_readout_phases import EB, K, LAM, N, NP, _batches, _inputs

pytestmark = pytest.mark.gpu

C_DENSE = 2e-5
WIDTHS = [64, 100, 128, 256, 260]
LAYERS = [1, 2, 3, 4]


def _dev(x, dt=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dt)


@functools.lru_cache(maxsize=None)
def _cell(d, L):
    """The module after the fixture's batches (readouts do not change it)."""
    f = _inputs(d, L)
    rp = _module(N, d, L, LAM, 0.0, P0=f["P0"])
    for b in range(_batches(L)):
        s = slice(b * EB, (b + 1) * EB)
        rp.update(f["src"][s], f["dst"][s], f["t"][s])
    rp.FANOUT_PAIRS_FROM = 0                                             # every list the geometry serves takes the fan-out kernel
    return rp, f


def _raw(rp, src, cand):
    """pair_gram_one_to_many without the clamp / log tail (the module's not_scale switch, put back afterwards)."""
    was = rp.not_scale
    rp.not_scale = True
    try:
        return rp.pair_gram_one_to_many(src, cand)
    finally:
        rp.not_scale = was


def _supported(rp):
    from tpnet_amd import _lib
    return bool(_lib.load().tpnet_pair_gram_fanout_supported(rp._st_ref()))


# ------------------------------------------------------------------------------------------------------------ fan-out readout

@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("d", WIDTHS)
def test_fanout_against_the_oracle(d, L):
    _need_gpu()
    rp, f = _cell(d, L)
    assert _supported(rp)
    st, u, neigh = f["st"], f["u"], f["neigh"]
    eu, ec = np.repeat(u, K), neigh.reshape(-1)
    NG = (2 * L + 2) ** 2
    got = rp.pair_gram_one_to_many(_dev(u), _dev(neigh))
    assert got.shape == (NP, K, NG) and got.dtype == torch.float32 and got.is_cuda
    _assert_features(got.view(-1, NG).cpu().numpy(), st, eu, ec, f"d={d} L={L} fan-out")
    raw = _raw(rp, _dev(u), _dev(neigh)).view(-1, NG).cpu().numpy()
    want = O.pair_gram(st, eu, ec, not_scale=True)
    err, bound = np.abs(raw - want), _gram_bound(st.P, eu, ec, L, 1e-4)
    print(f"d={d} L={L}: raw worst |delta| / bound = {(err / bound).max():.3e}")
    assert np.all(err <= bound), f"d={d} L={L} raw: worst |delta| / bound {(err / bound).max():.3e}"
    # host arrays take the same kernel: the same bits
    assert torch.equal(rp.pair_gram_one_to_many(u, neigh), got)
    rp.check_device_errors()


def test_route_threshold(monkeypatch):
    """FANOUT_PAIRS_FROM: None (the default) -- the expanded ids through pair_gram, bit for bit, and the fan-out entry is not called;
    a number -- lists of at least that many pairs take it."""
    _need_gpu()
    from tpnet_amd import RandomProjectionModule, _lib
    assert RandomProjectionModule.FANOUT_PAIRS_FROM is None
    rp, f = _cell(128, 3)
    lib = _lib.load()
    calls, real = [], lib.tpnet_pair_gram_fanout

    def counted(*a):
        calls.append((a[3], a[4]))
        return real(*a)
    monkeypatch.setattr(lib, "tpnet_pair_gram_fanout", counted)
    u, neigh = _dev(f["u"]), _dev(f["neigh"])
    want = rp.pair_gram(u.repeat_interleave(K), neigh.reshape(-1))
    for thr, served in ((None, False), (NP * K + 1, False), (NP * K, True), (0, True)):
        monkeypatch.setattr(rp, "FANOUT_PAIRS_FROM", thr)
        del calls[:]
        got = rp.pair_gram_one_to_many(u, neigh)
        assert calls == ([(NP, K)] if served else []), thr
        if not served:
            assert torch.equal(got.view(-1, 64), want)
    rp.check_device_errors()


def test_source_layers_come_first():
    """Where G(src, cand) and G(cand, src) differ (the blocks swap places), the output is the former: the decoder's order, not the
    anchored readout's."""
    _need_gpu()
    rp, f = _cell(64, 3)
    st, u, neigh = f["st"], f["u"], f["neigh"]
    eu, ec = np.repeat(u, K), neigh.reshape(-1)
    sc, cs = O.pair_gram(st, eu, ec), O.pair_gram(st, ec, eu)
    got = rp.pair_gram_one_to_many(_dev(u), _dev(neigh)).view(-1, 64).cpu().numpy()
    differ = np.abs(sc - cs) > 1e-2
    assert differ.any(axis=1).mean() > 0.5                               # most rows tell the two orders apart
    assert np.all(np.abs(got - sc)[differ] < 1e-3) and np.all(np.abs(got - cs)[differ] > 5e-3)
    # and the anchored readout of the same pairs holds the other order
    a = rp.pair_gram_anchored(_dev(neigh), _dev(u), _dev(u), matrix_cores=False)[0].cpu().numpy()
    assert np.all(np.abs(a - cs)[differ] < 1e-3)


@functools.lru_cache(maxsize=None)
def _long_list():
    rng = np.random.RandomState(11)
    return rng.randint(0, N, 8200).astype(np.int64), rng.randint(0, N, (8200, 5)).astype(np.int64)


@pytest.mark.parametrize("B,C", [(1, 1), (1, 3), (1, 4), (1, 21), (8200, 5)])
def test_fanout_chunking(B, C):
    """B = 1: the short-list rule cuts a row into chunks of 4 candidates (C = 1, 3: one partly filled chunk; 4: one whole; 21: five and
    a tail of one).  B = 8200, C = 5: more than 8192 units, the chunk is the whole row."""
    _need_gpu()
    rp, f = _cell(64, 3)
    if B == 1:
        src, cand = f["u"][5:6], np.resize(f["neigh"].reshape(-1), (1, C))
    else:
        src, cand = _long_list()
    got = rp.pair_gram_one_to_many(_dev(src), _dev(cand)).view(-1, 64).cpu().numpy()
    _assert_features(got, f["st"], np.repeat(src, C), cand.reshape(-1), f"B={B} C={C}")
    rp.check_device_errors()


def test_fanout_not_scale():
    _need_gpu()
    f = _inputs(100, 2)
    rp = _module(N, 100, 2, LAM, 0.0, P0=f["P0"], not_scale=True)
    rp.FANOUT_PAIRS_FROM = 0
    for b in range(_batches(2)):
        s = slice(b * EB, (b + 1) * EB)
        rp.update(f["src"][s], f["dst"][s], f["t"][s])
    eu, ec = np.repeat(f["u"], K), f["neigh"].reshape(-1)
    got = rp.pair_gram_one_to_many(f["u"], f["neigh"]).view(-1, 36).cpu().numpy()
    want = O.pair_gram(f["st"], eu, ec, not_scale=True)
    assert (want < 0).any()                                              # the clamp would show
    assert np.all(np.abs(got - want) <= _gram_bound(f["st"].P, eu, ec, 2, 1e-4))


@pytest.mark.parametrize("d", [16, 30])
def test_fallback_widths_take_pair_gram(d):
    _need_gpu()
    rp, f = _cell(d, 3)
    assert not _supported(rp)
    u, neigh = _dev(f["u"]), _dev(f["neigh"])
    got = rp.pair_gram_one_to_many(u, neigh)
    assert got.shape == (NP, K, 64)
    assert torch.equal(got.view(-1, 64), rp.pair_gram(u.repeat_interleave(K), neigh.reshape(-1)))
    _assert_features(got.view(-1, 64).cpu().numpy(), f["st"], np.repeat(f["u"], K), f["neigh"].reshape(-1), f"d={d} fallback")
    assert torch.equal(rp.pair_gram_one_to_many(f["u"], f["neigh"]), got)
    rp.check_device_errors()


@pytest.mark.parametrize("d,L", [(64, 3), (260, 4), (128, 1)])
def test_position_independence(d, L):
    """The row of a (src, cand) pair has the same bits whatever B, C and its position in the call."""
    _need_gpu()
    rp, f = _cell(d, L)
    u, neigh = f["u"], f["neigh"]
    base = rp.pair_gram_one_to_many(_dev(u), _dev(neigh))
    i, c = 4, 2
    one = rp.pair_gram_one_to_many(_dev(u[i:i + 1]), _dev(neigh[i:i + 1, c:c + 1]))
    assert torch.equal(one[0, 0], base[i, c])
    cand = np.resize(neigh.reshape(-1)[7:], (3, 23))
    cand[1, 22], cand[2, 0] = neigh[i, c], neigh[i, c]
    many = rp.pair_gram_one_to_many(_dev(u[[9, i, i]]), _dev(cand))
    assert torch.equal(many[1, 22], base[i, c]) and torch.equal(many[2, 0], base[i, c])
    src, long = _long_list()
    src, long = src.copy(), long.copy()
    src[8199], long[8199, 4] = u[i], neigh[i, c]
    assert torch.equal(rp.pair_gram_one_to_many(_dev(src), _dev(long))[8199, 4], base[i, c])


@pytest.mark.parametrize("d,L", [(64, 3), (100, 2), (256, 4)])
def test_out_of_range_ids_give_nan_rows_and_one_error(d, L):
    _need_gpu()
    rp, f = _cell(d, L)
    u, neigh = _dev(f["u"]), _dev(f["neigh"])
    rp.check_device_errors()
    clean = rp.pair_gram_one_to_many(u, neigh).cpu().numpy().view(np.uint32)

    def reported_once():
        with pytest.raises(IndexError):
            rp.check_device_errors()
        rp.check_device_errors()

    u_bad = u.clone()
    u_bad[11] = N
    got = rp.pair_gram_one_to_many(u_bad, neigh).cpu().numpy()
    keep = np.arange(NP) != 11
    assert np.isnan(got[11]).all() and np.array_equal(got[keep].view(np.uint32), clean[keep])
    reported_once()
    n_bad = neigh.clone()
    n_bad[23, 3] = -1
    got = rp.pair_gram_one_to_many(u, n_bad).cpu().numpy()
    keep = np.ones((NP, K), dtype=bool)
    keep[23, 3] = False
    assert np.isnan(got[23, 3]).all() and np.array_equal(got[keep].view(np.uint32), clean[keep])
    reported_once()


@pytest.mark.parametrize("d,L", [(64, 3), (128, 2)])
def test_feature_one_to_many_is_mlp_of_the_gram(d, L):
    """get_pair_wise_feature_one_to_many = _apply_mlp(pair_gram_one_to_many): within C_DENSE of the output scale of the torch layers
    on the same Gram, and the gradient reaches rp.mlp's four tensors."""
    _need_gpu()
    rp, f = _cell(d, L)
    NG = (2 * L + 2) ** 2
    u, neigh = _dev(f["u"]), _dev(f["neigh"])
    with torch.no_grad():
        want = rp.mlp(rp.pair_gram_one_to_many(u, neigh).view(-1, NG))
        got = rp.get_pair_wise_feature_one_to_many(u, neigh)
    assert got.shape == (NP * K, NG)
    err, scale = (got - want).abs().max().item(), max(1.0, want.abs().max().item())
    print(f"d={d} L={L}: max |delta| {err:.3e} of scale {scale:.3f}")
    assert err <= C_DENSE * scale
    params = list(rp.mlp.parameters())
    assert len(params) == 4
    gy = torch.randn(NP * K, NG, generator=torch.Generator().manual_seed(L)).to(DEV)
    got_g = torch.autograd.grad(rp.get_pair_wise_feature_one_to_many(u, neigh), params, gy)
    gram = rp.pair_gram_one_to_many(u, neigh).view(-1, NG)
    want_g = torch.autograd.grad(rp.mlp(gram), params, gy)
    for g in got_g:
        assert torch.isfinite(g).all() and g.abs().max() > 0               # the gradient reaches all four tensors
    _assert_mlp_grads_close(rp.mlp, gram, gy, got_g, want_g)
    rp.check_device_errors()


def test_decoder_forward_one_to_many_is_forward_on_the_expanded_pairs():
    _need_gpu()
    from tpnet_amd.callers import LinkPredictor_v1
    rp, f = _cell(64, 3)
    torch.manual_seed(3)
    u, neigh = _dev(f["u"]), _dev(f["neigh"])
    eu, ec = u.repeat_interleave(K), neigh.reshape(-1)
    with torch.no_grad():
        for not_encode in (True, False):
            dec = LinkPredictor_v1(8, 8, 16, 1, rp, not_encode=not_encode).to(DEV)
            es, ed = torch.randn(NP * K, 8, device=DEV), torch.randn(NP * K, 8, device=DEV)
            want = dec(eu, ec, es, ed).view(NP, K)
            got = dec.forward_one_to_many(u, neigh, es, ed)
            assert got.shape == (NP, K)
            scale = max(1.0, want.abs().max().item())
            assert (got - want).abs().max().item() <= 10 * C_DENSE * scale          # (C_DENSE of the features through 64 x 16 weights < 1)
            if not_encode:
                assert torch.equal(dec.forward_one_to_many(u, neigh), got)          # the embeddings are not looked at
            else:
                with pytest.raises(ValueError):
                    dec.forward_one_to_many(u, neigh)


# ------------------------------------------------------------------------------------------------------------------- sampler

_samplers, _lists = {}, {}


def _sampler(name, seed=1234):
    from tpnet_amd import GpuNegativeEdgeSampler
    if (name, seed) not in _samplers:
        g = graph(name)
        _samplers[(name, seed)] = GpuNegativeEdgeSampler(g.src, g.dst, g.t, negative_sample_strategy="historical", seed=seed, device=DEV)
    return _samplers[(name, seed)]


def _check_rows(name, B, Q, Qh, seed=1234):
    g, smp = graph(name), _sampler(name, seed)
    bs, bd, bt = batch_of(g, B)
    smp.reset_random_state()
    cand, n_hist = smp.sample_many_device(_dev(bs), _dev(bd), _dev(bt, torch.float64), Q, Qh)
    assert cand.shape == (B, Q) and cand.dtype == torch.int64 and n_hist.shape == (B,) and n_hist.dtype == torch.int32
    Qh = Q // 2 if Qh is None else Qh
    want, want_h = restated_rows(g, bs, bd, bt, Q, Qh, seed, 0, _lists.setdefault((name, B), {}))
    what = f"{name} B={B} Q={Q} Qh={Qh}"
    assert np.array_equal(n_hist.cpu().numpy(), want_h), what
    assert np.array_equal(cand.cpu().numpy(), want), what
    return bs, bd, bt, want, want_h


@pytest.mark.parametrize("B", [1, 65, 300])
def test_sample_many_equals_the_restated_rule(B):
    _need_gpu()
    for Q in (1, 2, 63, 64, 65, 100):
        _check_rows("mixed", B, Q, None)


@pytest.mark.parametrize("name,Q,Qh", [("hub", 100, None), ("hub", 250, 250), ("hub", 65, 64), ("seven", 10, None), ("seven", 10, 0),
                                       ("seven", 10, 10), ("mixed", 20, 0), ("mixed", 20, 20)])
def test_sample_many_hub_short_domain_and_split(name, Q, Qh):
    _need_gpu()
    bs, bd, bt, cand, n_hist = _check_rows(name, 40, Q, Qh)
    assert_row_promises(graph(name), bs, bd, bt, cand, n_hist, Q, Q // 2 if Qh is None else Qh, f"{name} Q={Q}")
    if name == "seven":
        assert (cand == -1).any(axis=1).all()
    if name == "hub":
        assert n_hist[bs == 1].max() >= min(Q // 2 if Qh is None else Qh, 65)          # R = 200: more than one wave step of 64


def test_sample_many_determinism_and_call_index():
    _need_gpu()
    from tpnet_amd import GpuNegativeEdgeSampler
    g = graph("mixed")
    bs, bd, bt = batch_of(g, 50)
    args = (_dev(bs), _dev(bd), _dev(bt, torch.float64), 20)
    a, b = (GpuNegativeEdgeSampler(g.src, g.dst, g.t, negative_sample_strategy="random", seed=77, device=DEV) for _ in range(2))
    first = [a.sample_many_device(*args) for _ in range(3)]
    again = [b.sample_many_device(*args) for _ in range(3)]
    for (c1, h1), (c2, h2) in zip(first, again):
        assert torch.equal(c1, c2) and torch.equal(h1, h2)               # the same seed and call replay the same output
    assert not torch.equal(first[0][0], first[1][0])                     # a call advances the call index
    for call in (0, 1, 2):
        want, _ = restated_rows(g, bs, bd, bt, 20, 10, 77, call)
        assert np.array_equal(first[call][0].cpu().numpy(), want)
    a.reset_random_state()
    c, h = a.sample_many_device(*args)
    assert torch.equal(c, first[0][0]) and torch.equal(h, first[0][1])   # reset_random_state restarts the sequence
    a.sample_device(10)                                                  # the two kinds of call share the call index
    assert np.array_equal(a.sample_many_device(*args)[0].cpu().numpy(), restated_rows(g, bs, bd, bt, 20, 10, 77, 2)[0])
    other = GpuNegativeEdgeSampler(g.src, g.dst, g.t, negative_sample_strategy="random", seed=78, device=DEV)
    assert not torch.equal(other.sample_many_device(*args)[0], first[0][0])


# --------------------------------------------------------------------------------------------------------------------- meter

def _record(rec):
    f = rec.view(np.float64)
    return dict(mrr=float(f[0]), hits=(float(f[1]), float(f[2]), float(f[3])), m_sum=int(rec[4]), n=int(rec[5]),
                n_valid_candidates=int(rec[6]), flags=int(rec[7]))


def _big_case():
    rng = np.random.RandomState(8)
    x = np.round(rng.randn(1000, 101) * 4).astype(np.float32) / 4         # a grid of quarters: ties with the positive are common
    v = rng.rand(1000, 100) < 0.9
    return x, v, (1, 3, 10)


@pytest.mark.parametrize("name", sorted(record_cases()) + ["B1000_C101"])
def test_record_equals_the_host_rule(name):
    _need_gpu()
    from tpnet_amd import LinkRankingMeter
    from tpnet_amd.metrics import link_ranking_metrics_host
    x, v, ks = _big_case() if name == "B1000_C101" else record_cases()[name]
    meter = LinkRankingMeter(4, DEV, hits_at=ks)
    cand = None if v is None else _dev(np.where(v, 5, -1))
    for _ in range(2):
        meter.add(_dev(x, torch.float32), cand)
    rec = meter.records()
    assert rec.shape == (2, 8) and np.array_equal(rec[0], rec[1])        # two runs: the same bits
    want = link_ranking_metrics_host(x, v, hits_at=ks)
    assert_record(_record(rec[0]), want, name)
    res = meter.results()
    assert res.flags == [want["flags"]] * 2 and list(res[0]) == ["mrr"] + [f"hits@{k}" for k in ks]
    if name == "B1000_C101":
        assert want["n"] == 1000 and want["flags"] == 0


def test_meter_totals_log_and_reset():
    _need_gpu()
    from tpnet_amd import LinkRankingMeter
    from tpnet_amd.metrics import link_ranking_metrics_host
    rng = np.random.RandomState(21)
    parts = [np.round(rng.randn(b, 9) * 2).astype(np.float32) / 2 for b in (50, 7, 300, 1)]
    parts[1][:] = np.nan                                                 # a batch in which nothing is counted
    meter = LinkRankingMeter(4, DEV)
    for k, x in enumerate(parts):
        assert meter.add(_dev(x, torch.float32)) == k
    with pytest.raises(IndexError):
        meter.add(_dev(parts[0], torch.float32))
    res = meter.results()
    assert len(res) == 4 and res.flags[1] == FLAG_NO_QUERY | FLAG_NAN and np.isnan(res[1]["mrr"])
    want = link_ranking_metrics_host(np.concatenate(parts))
    n = want["n"]
    assert res.totals["n"] == n == 351
    # each record's mrr is within n_b 2^-52 of its exact mean; the weighted mean adds a product, a sum and a quotient per record
    tol = (n + 3 * len(parts) + 2) * 2.0 ** -52
    assert abs(res.totals["mrr"] - want["mrr"]) <= tol * want["mrr"]
    for k, h in zip((1, 3, 10), want["hits"]):
        assert abs(res.totals[f"hits@{k}"] - h) <= tol * max(h, 1e-300)
    meter.reset()
    assert len(meter) == 0 and meter.add(_dev(parts[2], torch.float32)) == 0
    assert_record(_record(meter.records()[0]), link_ranking_metrics_host(parts[2]), "after reset")
    empty = LinkRankingMeter(1, DEV)
    empty.add(torch.empty((0, 5), dtype=torch.float32, device=DEV))
    r = _record(empty.records()[0])
    assert r["n"] == 0 and r["flags"] == FLAG_NO_QUERY and np.isnan(r["mrr"])
    assert FLAG_EMPTY == 4


# ---------------------------------------------------------------------------------------------------------------------- loop
# A toy stream: N = 64 nodes in two halves whose rows have opposite sign (test_readout_phases' construction), d = 64, L = 3,
# 6 batches of 4 edges with a ragged tail (E = 22), Q = 3 candidates per positive, decoder not_encode with 8 hidden units.
LOOP_SEED = 0          # of the seeds 0..39 most qualify (smallest gap / bound from 0.5 to 14.7); seed 0: 4.57
LOOP_E, LOOP_B, LOOP_Q = 22, 4, 3


@functools.lru_cache(maxsize=None)
def _toy(seed):
    rng = np.random.RandomState(1000 + seed)
    half = rng.permutation(N) < N // 2
    sign = np.where(half, 1.0, -1.0)[:, None]
    P0 = (sign * rng.uniform(0.5, 1.5, (N, 64)) / 8.0).astype(np.float32)
    warm = 120
    src = rng.randint(0, N, warm + LOOP_E).astype(np.int64)
    dst = np.array([rng.choice(np.flatnonzero(half == half[s])) for s in src], dtype=np.int64)
    t = np.sort(rng.uniform(1.0, 2.0e5, warm + LOOP_E))
    cand = rng.randint(0, N, (LOOP_E, LOOP_Q)).astype(np.int64)
    es, ed = src[warm:], dst[warm:]
    clash = cand == ed[:, None]
    cand[clash] = (cand[clash] + 1) % N                                  # a valid candidate is never the true destination
    cand[rng.rand(LOOP_E, LOOP_Q) < 0.15] = -1                           # absent slots
    cand[3] = -1                                                         # a query without candidates
    return dict(P0=P0, warm=(src[:warm], dst[:warm], t[:warm]), src=es, dst=ed, t=t[warm:], cand=cand)


def _toy_modules(seed):
    from tpnet_amd.callers import LinkPredictor_v1
    toy = _toy(seed)
    rp = _module(N, 64, 3, LAM, 0.0, P0=toy["P0"])
    rp.FANOUT_PAIRS_FROM = 0                                             # the loop's readout is the fan-out kernel
    gen = torch.Generator().manual_seed(500 + seed)
    dec = LinkPredictor_v1(4, 4, 8, 1, rp, not_encode=True)
    with torch.no_grad():
        for m in list(rp.mlp) + [dec.fc1, dec.fc2]:
            for p in m.parameters():
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * 4.0 / np.sqrt(m.in_features))
    dec = dec.to(DEV)
    for a in range(0, 120, 40):
        rp.update(toy["warm"][0][a:a + 40], toy["warm"][1][a:a + 40], toy["warm"][2][a:a + 40])
    return toy, rp, dec


def _sigma(w):
    """The largest singular value of a weight matrix, in float64: ||W x||_2 <= sigma ||x||_2."""
    return float(np.linalg.norm(w.detach().double().cpu().numpy(), 2))


def _restated_pass(seed):
    """The straight-line pass: per batch expand with numpy, get_pair_wise_feature -> decoder.forward, the host rule on the logits
    moved to the host, then update.  Next to it the oracle's state, for the tolerance of every logit.  -> per-batch (record, gap / tol
    per query), and the module afterwards."""
    from tpnet_amd.metrics import link_ranking_metrics_host
    toy, rp, dec = _toy_modules(seed)
    st = O.OracleState(toy["P0"], 3, LAM, 0.0)
    for a in range(0, 120, 40):
        O.update(st, toy["warm"][0][a:a + 40], toy["warm"][1][a:a + 40], toy["warm"][2][a:a + 40])
    s_mlp = _sigma(rp.mlp[0].weight) * _sigma(rp.mlp[2].weight)
    s_dec = _sigma(dec.fc1.weight[:, -64:]) * _sigma(dec.fc2.weight)
    out = []
    u24 = 2.0 ** -24
    with torch.no_grad():
        for b0 in range(0, LOOP_E, LOOP_B):
            s = slice(b0, min(b0 + LOOP_B, LOOP_E))
            src, dst, t, cand = toy["src"][s], toy["dst"][s], toy["t"][s], toy["cand"][s]
            b = len(src)
            ids = np.concatenate([dst[:, None], np.where(cand < 0, dst[:, None], cand)], axis=1)
            es, ed = np.repeat(src, LOOP_Q + 1), ids.reshape(-1)
            zeros = torch.zeros((len(es), 4), device=DEV)
            feat = rp.get_pair_wise_feature(es, ed)
            logits = dec(es, ed, zeros, zeros).view(b, LOOP_Q + 1)
            x = logits.cpu().numpy()
            valid = cand >= 0
            rec = link_ranking_metrics_host(x, valid)
            # ---- how far a logit of an fp32 implementation can lie from the exact one (the derivation: the test's docstring)
            raw = O.pair_gram(st, es, ed, not_scale=True).astype(np.float64)
            fx = np.log1p(np.maximum(raw, 0.0))
            tol_x = _gram_bound(st.P, es, ed, 3, (64 + 3) * u24) / (1.0 + np.maximum(raw, 0.0)) + 4 * u24 * fx
            tol_f = s_mlp * np.linalg.norm(tol_x, axis=1) + 8.0 * C_DENSE * max(1.0, feat.abs().max().item())     # ||delta f||_2, 64 entries
            tol_l = (s_dec * tol_f).reshape(b, LOOP_Q + 1) + C_DENSE * max(1.0, np.abs(x).max())
            gap = np.abs(x[:, 1:] - x[:, :1])
            ratio = np.where(valid, gap / (2 * (tol_l[:, 1:] + tol_l[:, :1])), np.inf).min(axis=1)
            out.append((rec, ratio))
            rp.update(src, dst, t)
            O.update(st, src, dst, t)
    return toy, rp, dec, out


def test_loop_against_a_straight_line_restatement():
    """`evaluate_link_ranking` with given candidates against the straight-line pass (_restated_pass), record by record.

    The two passes reach a logit through different kernels (the fan-out readout -- the toy's module sets FANOUT_PAIRS_FROM = 0 -- and
    the dense-layer route of its list length against the one-launch readout + self.mlp of host ids), so the integer words can only be compared where no comparison p ? q is decided
    inside the rounding error.  How far a logit of either pass can lie from the exact value of the same formula, per pair:
      Gram entry <a, b>, d = 64 products summed in fp32 in any order on rows scaled by their decay (one rounding each):
          |delta| <= (d + 3) 2^-24 ||a|| ||b||                                     (_gram_bound with rel = (d + 3) 2^-24)
      feature log(max(x, 0) + 1): the derivative is 1 / (1 + x) <= 1, logf is good to 2 ulp, twice that granted:
          tol_x = that / (1 + max(x, 0)) + 4 2^-24 log(1 + x)
      self.mlp and the decoder's two layers: ReLU does not expand a difference and ||W x||_2 <= sigma(W) ||x||_2 (sigma = the largest
      singular value), plus what the suite grants between two fp32-class implementations of dense layers (C_DENSE = 2e-5 of the
      output scale per entry, tests/test_host_routes.py; 64 entries of f: sqrt(64) = 8 of it as a vector):
          ||delta f||_2 <= sigma(W2) sigma(W1) ||tol_x||_2 + 8 C_DENSE max(1, |f|max) =: tol_f
          |delta logit| <= sigma(w2) sigma(W1[:, features]) tol_f + C_DENSE max(1, |logit|max) =: tol_logit
      (The weights of the toy's layers are drawn at 4 / sqrt(fan_in) so that features and logits are of order one and more: the two
      max(1, .) floors do not decide.)
    If the straight-line pass sees |p - q| > 2 (tol_p + tol_q), the exact values are more than tol_p + tol_q apart and the other pass
    orders them the same way.  LOOP_SEED is chosen so that EVERY query qualifies (asserted: nothing is skipped); then g, e and so
    m_sum, n, n_valid_candidates, flags and the hits words are equal, and mrr within the summation bound n 2^-52."""
    _need_gpu()
    from tpnet_amd import LinkRankingMeter
    from tpnet_amd.callers import evaluate_link_ranking, evaluate_with_restore
    toy, rp_ref, _, want = _restated_pass(LOOP_SEED)
    worst = min(r.min() for _, r in want)
    print(f"seed {LOOP_SEED}: smallest gap / (2 (tol_p + tol_q)) over all queries = {worst:.3f}")
    assert worst > 1.0, "a query of the toy stream does not qualify: choose another LOOP_SEED"
    ranks = sorted({rec["m_sum"] for rec, _ in want})
    assert len(ranks) > 1 and any(rec["m_sum"] > 2 * rec["n"] for rec, _ in want)          # not every positive ranks first
    _, rp, dec = _toy_modules(LOOP_SEED)
    meter = LinkRankingMeter(8, DEV)
    res = evaluate_link_ranking(rp, None, toy["src"], toy["dst"], toy["t"], LOOP_B, LOOP_Q, dec, candidates=toy["cand"], meter=meter)
    recs = meter.records()
    assert len(res) == len(want) == 6 and recs.shape == (6, 8)
    for k, (w, _) in enumerate(want):
        assert_record(_record(recs[k]), w, f"batch {k}")
        assert res[k]["mrr"] == _record(recs[k])["mrr"]
    assert want[0][0]["flags"] == FLAG_EMPTY and want[0][0]["n"] == LOOP_B - 1         # the query without candidates
    # ---- the state after the pass equals the state after plain update calls, bit for bit
    for a, b in zip(_layers(rp), _layers(rp_ref)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert float(rp.now_time) == float(rp_ref.now_time) == toy["t"][-1]
    # ---- composes with evaluate_with_restore (ids and candidates on the device this time): six more records, the state put back
    before = [p.detach().clone() for p in rp.random_projections]
    res2 = evaluate_with_restore(rp, lambda: evaluate_link_ranking(rp, None, _dev(toy["src"]), _dev(toy["dst"]), _dev(toy["t"], torch.float64),
                                                                    LOOP_B, LOOP_Q, dec, candidates=_dev(toy["cand"])))
    assert len(res2) == 6 and res2.totals["n"] == res.totals["n"]
    for a, b in zip(before, rp.random_projections):
        assert torch.equal(a, b.detach())
    rp.check_device_errors()


def test_loop_sampled_and_given_candidates_take_the_same_code():
    _need_gpu()
    from tpnet_amd import GpuNegativeEdgeSampler
    from tpnet_amd.callers import evaluate_link_ranking
    toy, rp, dec = _toy_modules(LOOP_SEED)
    hist = toy["warm"]
    mk = lambda: GpuNegativeEdgeSampler(np.concatenate([hist[0], toy["src"]]), np.concatenate([hist[1], toy["dst"]]),
                                        np.concatenate([hist[2], toy["t"]]), negative_sample_strategy="random", seed=5, device=DEV)
    saved = rp.backup_random_projections()
    sampled = evaluate_link_ranking(rp, mk(), toy["src"], toy["dst"], toy["t"], LOOP_B, LOOP_Q, dec, num_historical=2)
    rp.reload_random_projections(saved)
    smp, rows = mk(), []
    for b0 in range(0, LOOP_E, LOOP_B):
        s = slice(b0, min(b0 + LOOP_B, LOOP_E))
        rows.append(smp.sample_many_device(_dev(toy["src"][s]), _dev(toy["dst"][s]), _dev(toy["t"][s], torch.float64), LOOP_Q, 2)[0])
    given = evaluate_link_ranking(rp, None, toy["src"], toy["dst"], toy["t"], LOOP_B, LOOP_Q, dec, candidates=torch.cat(rows))
    assert [r for r in given] == [r for r in sampled] and given.flags == sampled.flags and given.totals == sampled.totals
    assert sampled.totals["n"] == LOOP_E and 0.0 < sampled.totals["mrr"] <= 1.0
    with pytest.raises(ValueError):
        evaluate_link_ranking(rp, None, toy["src"], toy["dst"], toy["t"], LOOP_B, LOOP_Q, dec, candidates=toy["cand"][:, :LOOP_Q - 1])   # not [E, Q]
