"""One source against many candidates in one launch, on the GPU: tpnet_score_one_to_many (csrc/score_fanout.hip) and what stands on it.

  features   the kernel's `gram` output against the fan-out readout (tpnet_pair_gram_fanout), bit for bit, list and range mode, lead
  logits     against score_one_to_many_host (float64) on the kernel's OWN features, per entry within the project's fp32-class bound
             4e-5 mag + 1e-6 max|want| (tests/test_decoder_f32.py) applied per stage and carried through the later stages by their
             absolute-value weights (test_score_fanout_host.score_bound)
  promises   one pair = one bit pattern whatever its position, chunk, mode or column; two calls = the same bits
  edges      column and row counts around the tile (32 columns) and the workgroup (GPB = 512 / LPP units), guarded output
  errors     ids out of range: NaN logits, one report, everything else untouched
  routing    LinkPredictor_v1.fused_scores, forward_one_to_all, the fallbacks
  record     tpnet_lp_ranking_skip against the host rule with the mask
  loop       evaluate_link_ranking_all and recommend_links on a toy stream

Fixture: test_readout_phases._inputs through test_link_ranking._cell (N = 64 nodes, B = 37 rows of C = 5 candidates), L = 3, widths
64 (16 lanes, exact fit), 100 (32 lanes, masked), 128 (32 lanes, exact fit), 256 (32 lanes x 2 vectors), 260 (64 lanes x 2, masked)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_decoder_f32 import _guarded, _intact
from test_gpu_parity import DEV, _layers, _module, _need_gpu
from test_link_ranking import LOOP_SEED, _cell, _dev, _raw, _record, _toy_modules
from test_link_ranking_host import FLAG_EMPTY, assert_record
from test_readout_phases import K, LAM, N, NP
from test_score_fanout_host import score_bound, skip_cases, skip_valid

pytestmark = pytest.mark.gpu

WIDTHS = [64, 100, 128, 256, 260]
GPB = {64: 32, 100: 16, 128: 16, 256: 16, 260: 8}               # units per workgroup: 512 / (lanes per unit)
SHAPES = [(172, 172), (8, 16), (4, 1), (4, 33), (4, 256)]       # the decoder's (D, H); the first is the reference's default


@functools.lru_cache(maxsize=None)
def _decoder(d, D=4, H=8, L=3):
    """A not_encode decoder on the cell's module, weights drawn at 4 / sqrt(fan_in) (logits of order one and more), never modified."""
    from tpnet_amd.callers import LinkPredictor_v1
    rp, _ = _cell(d, L)
    gen = torch.Generator().manual_seed(1000 * d + 10 * D + H)
    dec = LinkPredictor_v1(D, D, H, 1, rp, not_encode=True)
    with torch.no_grad():
        for m in (dec.fc1, dec.fc2):
            for p in m.parameters():
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * 4.0 / np.sqrt(m.in_features))
    dec = dec.to(DEV)
    for p in list(dec.fc1.parameters()) + list(dec.fc2.parameters()):
        p.requires_grad_(False)
    return dec


def _call(dec, src, cand=None, rng=None, lead=None, want_gram=True, flags=None):
    """tpnet_score_one_to_many itself, into guarded buffers -> (logits [B, C_1], gram [B, C_1, 64] or None, the buffers)."""
    from tpnet_amd import _lib
    from tpnet_amd import score_fanout as sf
    rp = dec.random_projections
    rp._ensure_engine()
    prep = sf._mlp_prepared(rp)
    assert prep is not None
    B = int(src.numel())
    Cn = int(cand.shape[1]) if cand is not None else rng[1] - rng[0]
    C1 = Cn + (1 if lead is not None else 0)
    obuf, out = _guarded(shape=(B, C1))
    gbuf, gram = _guarded(shape=(B, C1, 64)) if want_gram else (None, None)
    cand = None if cand is None else cand.contiguous()
    fc1, fc2 = dec.fc1, dec.fc2
    fl = (_lib.FLAG_NOT_SCALE if rp.not_scale else 0) if flags is None else flags
    rc = _lib.load().tpnet_score_one_to_many(
        rp._st_ref(), src.data_ptr(), None if cand is None else cand.data_ptr(), 0 if rng is None else rng[0],
        None if lead is None else lead.data_ptr(), B, Cn, rp._now_host, float(rp.time_decay_weight), fl, prep.ref,
        fc1.weight.data_ptr(), fc1.in_features, fc1.in_features - 64, fc1.bias.data_ptr(), fc2.weight.data_ptr(), fc2.bias.data_ptr(),
        fc1.out_features, None if gram is None else gram.data_ptr(), out.data_ptr(), rp._stream())
    assert rc == 0, rc
    return out, gram, [b for b in (obuf, gbuf) if b is not None]


def _want(dec, gram):
    """score_one_to_many_host on the kernel's own features -> (want, bound), both of gram's leading shape."""
    from tpnet_amd.score_fanout import score_one_to_many_host
    rp = dec.random_projections
    m = rp.mlp
    want, mags = score_one_to_many_host(gram.reshape(-1, 64), (m[0].weight, m[0].bias, m[2].weight, m[2].bias),
                                        (dec.fc1.weight, dec.fc1.bias), (dec.fc2.weight, dec.fc2.bias), dec.fc1.in_features - 64)
    return want.reshape(gram.shape[:-1]), score_bound(want, mags).reshape(gram.shape[:-1])


def _assert_in_bound(dec, out, gram, what):
    want, bound = _want(dec, gram)
    got = out.double().cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    ratio = np.abs(got - want) / bound
    print(f"{what}: worst |got - want| / bound = {ratio.max():.2e}, worst |got - want| = {np.abs(got - want).max():.2e} "
          f"(max |want| {np.abs(want).max():.3f})")
    assert (ratio <= 1.0).all(), f"{what}: {int((ratio > 1).sum())} entries beyond the bound, worst {ratio.max():.3f}"


# --------------------------------------------------------------------------------------------------------------------- features

@pytest.mark.parametrize("d", WIDTHS)
def test_features_are_the_fanout_readouts_bits(d):
    _need_gpu()
    rp, f = _cell(d, 3)
    dec = _decoder(d)
    u, neigh, v = _dev(f["u"]), _dev(f["neigh"]), _dev(f["v"])
    _, gram, bufs = _call(dec, u, cand=neigh)
    assert torch.equal(gram, rp.pair_gram_one_to_many(u, neigh))
    ids = torch.arange(3, 61, device=DEV)
    _, gram_r, bufs_r = _call(dec, u, rng=(3, 61))
    assert torch.equal(gram_r, rp.pair_gram_one_to_many(u, ids.unsqueeze(0).expand(NP, -1).contiguous()))
    _, gram_l, bufs_l = _call(dec, u, cand=neigh, lead=v)
    assert torch.equal(gram_l[:, 0], rp.pair_gram_one_to_many(u, v.unsqueeze(1))[:, 0])      # the lead column's row: (src, lead)
    assert torch.equal(gram_l[:, 1:], gram)
    assert _intact(*bufs, *bufs_r, *bufs_l)
    rp.check_device_errors()


def test_wide_rows_are_served():
    """The 64 x 2 class (rows of 260..512 floats) builds without scratch, so it is served: the Python route takes the kernel."""
    _need_gpu()
    from tpnet_amd import score_fanout as sf
    rp, f = _cell(260, 3)
    dec = _decoder(260)
    assert sf.serves(dec) is True
    u, neigh = _dev(f["u"]), _dev(f["neigh"])
    with torch.no_grad():
        dec.fused_scores = True
        n0 = sf.calls["score"]
        try:
            got = dec.forward_one_to_many(u, neigh)
        finally:
            dec.fused_scores = False
    assert sf.calls["score"] == n0 + 1 and torch.equal(got, _call(dec, u, cand=neigh, want_gram=False)[0])


# ----------------------------------------------------------------------------------------------------------------------- logits

@pytest.mark.parametrize("d,D,H", [(d, 172, 172) for d in WIDTHS] + [(128, D, H) for D, H in SHAPES[1:]])
def test_logits_against_float64(d, D, H):
    _need_gpu()
    rp, f = _cell(d, 3)
    dec = _decoder(d, D, H)
    u, neigh, v = _dev(f["u"]), _dev(f["neigh"]), _dev(f["v"])
    out, gram, bufs = _call(dec, u, cand=neigh, lead=v)
    _assert_in_bound(dec, out, gram, f"d={d} (D, H)=({D}, {H}) list + lead")
    out, gram, bufs_r = _call(dec, u, rng=(3, 61))
    _assert_in_bound(dec, out, gram, f"d={d} (D, H)=({D}, {H}) range [3, 61)")
    assert _intact(*bufs, *bufs_r)


# --------------------------------------------------------------------------------------------------------- position independence

@pytest.mark.parametrize("d", [64, 100, 256, 260])
def test_position_independence(d):
    """One pair (u, v): alone; at tile columns 31, 32 and 33 of a row of 65; as row 8199 of a list of 8200 x 5 (anchored_chunk cuts
    it differently); in range mode; as the lead column.  One bit pattern."""
    _need_gpu()
    rp, f = _cell(d, 3)
    dec = _decoder(d)
    rng = np.random.RandomState(d)
    u0, v0 = int(f["u"][5]), 3 + int(f["v"][5]) % 58                       # v0 inside [3, 61)
    one = lambda t: _dev(np.array(t, dtype=np.int64))
    base = _call(dec, one([u0]), cand=one([[v0]]), want_gram=False)[0][0, 0].clone()
    assert torch.isfinite(base)
    seen = {}
    row = rng.randint(0, N, (1, 65)).astype(np.int64)
    row[0, 31:34] = v0
    out = _call(dec, one([u0]), cand=_dev(row), want_gram=False)[0]
    seen.update({f"column {c}": out[0, c] for c in (31, 32, 33)})
    src = np.tile(f["u"], 8200 // NP + 1)[:8200].copy()
    cand = np.tile(f["neigh"], (8200 // NP + 1, 1))[:8200].copy()
    src[8199], cand[8199, 2] = u0, v0
    seen["row 8199 of 8200 x 5"] = _call(dec, _dev(src), cand=_dev(cand), want_gram=False)[0][8199, 2]
    seen["range mode"] = _call(dec, one([7, u0, 9]), rng=(3, 61), want_gram=False)[0][1, v0 - 3]
    seen["lead column"] = _call(dec, one([u0]), cand=one([[11, 12]]), lead=one([v0]), want_gram=False)[0][0, 0]
    seen["range mode with a lead"] = _call(dec, one([u0]), rng=(0, N), lead=one([4]), want_gram=False)[0][0, 1 + v0]
    for what, x in seen.items():
        assert torch.equal(x, base), f"{what}: {x.item()!r} against {base.item()!r}"
    rp.check_device_errors()


# ------------------------------------------------------------------------------------------------------------------------ edges

@pytest.mark.parametrize("d", WIDTHS)
def test_edges_of_the_tile_and_the_workgroup(d):
    _need_gpu()
    rp, f = _cell(d, 3)
    dec = _decoder(d)
    rng = np.random.RandomState(17 + d)
    for B in (1, GPB[d] - 1, GPB[d] + 1):
        for Cn in (1, 31, 32, 33, 65):
            src = _dev(f["u"][rng.randint(0, NP, B)])
            cand = _dev(rng.randint(0, N, (B, Cn)).astype(np.int64))
            out, gram, bufs = _call(dec, src, cand=cand)
            assert _intact(*bufs), (B, Cn)
            assert torch.equal(gram, rp.pair_gram_one_to_many(src, cand)), (B, Cn)
            _assert_in_bound(dec, out, gram, f"d={d} B={B} C={Cn}")
    rp.check_device_errors()


# ----------------------------------------------------------------------------------------------------------------------- errors

@pytest.mark.parametrize("d", [64, 256, 260])
def test_out_of_range_ids_give_nan_logits_and_one_error(d):
    _need_gpu()
    rp, f = _cell(d, 3)
    dec = _decoder(d)
    u, neigh, v = _dev(f["u"]), _dev(f["neigh"]), _dev(f["v"])
    rp.check_device_errors()
    clean = _call(dec, u, cand=neigh, lead=v, want_gram=False)[0].cpu().numpy().view(np.uint32)

    def reported_once():
        with pytest.raises(IndexError):
            rp.check_device_errors()
        rp.check_device_errors()

    u_bad = u.clone()
    u_bad[11] = N
    got = _call(dec, u_bad, cand=neigh, lead=v, want_gram=False)[0].cpu().numpy()
    keep = np.arange(NP) != 11
    assert np.isnan(got[11]).all() and np.array_equal(got[keep].view(np.uint32), clean[keep])
    reported_once()
    n_bad = neigh.clone()
    n_bad[23, 3] = -1
    got = _call(dec, u, cand=n_bad, lead=v, want_gram=False)[0].cpu().numpy()
    keep = np.ones((NP, K + 1), dtype=bool)
    keep[23, 4] = False
    assert np.isnan(got[23, 4]) and np.array_equal(got[keep].view(np.uint32), clean[keep])
    reported_once()
    v_bad = v.clone()
    v_bad[2] = N + 5
    got = _call(dec, u, cand=neigh, lead=v_bad, want_gram=False)[0].cpu().numpy()
    keep = np.ones((NP, K + 1), dtype=bool)
    keep[2, 0] = False
    assert np.isnan(got[2, 0]) and np.array_equal(got[keep].view(np.uint32), clean[keep])
    reported_once()


# ------------------------------------------------------------------------------------------------------ flags and determinism

def test_not_scale_is_honoured_and_two_calls_give_equal_bits():
    _need_gpu()
    from tpnet_amd import _lib
    rp, f = _cell(128, 3)
    dec = _decoder(128)
    u, neigh = _dev(f["u"]), _dev(f["neigh"])
    out_raw, gram_raw, _ = _call(dec, u, cand=neigh, flags=_lib.FLAG_NOT_SCALE)
    assert torch.equal(gram_raw, _raw(rp, u, neigh))
    out1, gram1, _ = _call(dec, u, cand=neigh)
    out2, gram2, _ = _call(dec, u, cand=neigh)
    assert torch.equal(out1, out2) and torch.equal(gram1, gram2) and not torch.equal(gram1, gram_raw)
    big1 = _call(dec, u, rng=(0, N), lead=_dev(f["v"]), want_gram=False)[0]
    big2 = _call(dec, u, rng=(0, N), lead=_dev(f["v"]), want_gram=False)[0]
    assert torch.equal(big1, big2)
    st = rp._state()
    assert _lib.load().tpnet_score_one_to_many_supported(ctypes.byref(st), None, 8, 8, 72) == 0


# ---------------------------------------------------------------------------------------------------------------------- routing

def test_routing_of_forward_one_to_many():
    _need_gpu()
    from tpnet_amd import score_fanout as sf
    rp, f = _cell(128, 3)
    dec = _decoder(128)
    u, neigh = _dev(f["u"]), _dev(f["neigh"])
    D = 4
    zeros = torch.zeros((NP * K, D), device=DEV)
    with torch.no_grad():
        n0 = sf.calls["score"]
        off = dec.forward_one_to_many(u, neigh)                              # the switch is off: today's path
        assert sf.calls["score"] == n0 and torch.equal(off, dec.forward_one_to_many(u, neigh, zeros, zeros))
        dec.fused_scores = True
        try:
            on = dec.forward_one_to_many(u, neigh)
            assert sf.calls["score"] == n0 + 1 and on.shape == (NP, K)
            assert torch.equal(on, _call(dec, u, cand=neigh, want_gram=False)[0])
            assert torch.equal(dec.forward_one_to_many(f["u"], f["neigh"]), on)          # host ids
            # ---- embeddings given: the composition
            assert torch.equal(dec.forward_one_to_many(u, neigh, zeros, zeros), off) and sf.calls["score"] == n0 + 2
        finally:
            dec.fused_scores = False
    # ---- a recorded gradient: the composition, with the graph
    dec.fused_scores = True
    for p in dec.fc1.parameters():
        p.requires_grad_(True)
    try:
        n1 = sf.calls["score"]
        g = dec.forward_one_to_many(u, neigh)
        assert g.requires_grad and sf.calls["score"] == n1 and torch.equal(g.detach(), off)
    finally:
        for p in dec.fc1.parameters():
            p.requires_grad_(False)
        dec.fused_scores = False


@pytest.mark.parametrize("what", ["use_matrix", "d30", "L2"])
def test_fallbacks_with_the_switch_on(what):
    _need_gpu()
    from tpnet_amd import score_fanout as sf
    from tpnet_amd.callers import LinkPredictor_v1
    if what == "use_matrix":
        rp = _module(30, 30, 3, LAM, 0.0, use_matrix=True)
        rng = np.random.RandomState(3)
        rp.update(rng.randint(0, 30, 40), rng.randint(0, 30, 40), np.sort(rng.uniform(1.0, 1e5, 40)))
        u, cand = _dev(rng.randint(0, 30, 9)), _dev(rng.randint(0, 30, (9, 4)))
    else:
        rp, f = _cell(30, 3) if what == "d30" else _cell(64, 2)
        u, cand = _dev(f["u"]), _dev(f["neigh"])
    torch.manual_seed(11)
    dec = LinkPredictor_v1(4, 4, 8, 1, rp, not_encode=True).to(DEV)
    with torch.no_grad():
        want = dec.forward_one_to_many(u, cand)
        want_all = dec.forward_one_to_all(u, 2, 20)
        dec.fused_scores = True
        n0 = sf.calls["score"]
        assert sf.serves(dec) is False
        assert torch.equal(dec.forward_one_to_many(u, cand), want) and torch.equal(dec.forward_one_to_all(u, 2, 20), want_all)
        assert sf.calls["score"] == n0


def test_forward_one_to_all_routes(monkeypatch):
    _need_gpu()
    from tpnet_amd import score_fanout as sf
    from tpnet_amd.callers import LinkPredictor_v1
    monkeypatch.setattr(LinkPredictor_v1, "SCORE_ALL_FUSED", False)          # the route is set here, whatever the measured default
    rp, f = _cell(128, 3)
    dec = _decoder(128)
    u, v = _dev(f["u"]), _dev(f["v"])
    ids = torch.arange(3, 61, device=DEV).unsqueeze(0).expand(NP, -1).contiguous()
    with torch.no_grad():
        n0 = sf.calls["score"]
        comp = dec.forward_one_to_all(u, 3, 61)                              # the composition route
        assert sf.calls["score"] == n0 and torch.equal(comp, dec.forward_one_to_many(u, ids))
        assert torch.equal(dec.forward_one_to_all(u, 3, 61, pairs_per_call=7), comp)
        # (slices of whole rows: rp.mlp's route depends on a list's length, so other slice sizes promise the class, not the bits)
        rows3 = dec.forward_one_to_all(u, 3, 61, pairs_per_call=3 * 58)
        assert rows3.shape == comp.shape and (rows3 - comp).abs().max().item() <= 1e-4 * max(1.0, comp.abs().max().item())
        lead = dec.forward_one_to_all(u, 3, 61, lead_node_ids=v)
        assert lead.shape == (NP, 59) and torch.equal(lead, dec.forward_one_to_many(u, torch.cat([v.unsqueeze(1), ids], dim=1)))
        dec.fused_scores = True
        try:
            fused = dec.forward_one_to_all(u, 3, 61, lead_node_ids=v)        # the kernel, range mode
            assert sf.calls["score"] == n0 + 1
            assert torch.equal(fused, _call(dec, u, rng=(3, 61), lead=v, want_gram=False)[0])
        finally:
            dec.fused_scores = False
        monkeypatch.setattr(LinkPredictor_v1, "SCORE_ALL_FUSED", True)       # the class constant alone routes forward_one_to_all ...
        assert torch.equal(dec.forward_one_to_all(u, 3, 61, lead_node_ids=v), fused) and sf.calls["score"] == n0 + 2
        assert torch.equal(dec.forward_one_to_many(u, ids), comp) and sf.calls["score"] == n0 + 2       # ... and nothing else
        monkeypatch.setattr(LinkPredictor_v1, "SCORE_ALL_FUSED", False)
        # the two routes agree within twice the bound of either against float64 (the composition is an fp32-class path too)
        out, gram, _ = _call(dec, u, rng=(3, 61), lead=v)
        _, bound = _want(dec, gram)
        assert ((fused - lead).abs().double().cpu().numpy() <= 2 * bound).all()
    with pytest.raises(ValueError):
        dec.forward_one_to_all(u, 5, 5)


# ----------------------------------------------------------------------------------------------------------------------- record

def _big_skip_case():
    rng = np.random.RandomState(8)
    x = np.round(rng.randn(1000, 101) * 4).astype(np.float32) / 4         # a grid of quarters: ties with the positive are common
    return x, rng.randint(-1, 100, 1000).astype(np.int64), (1, 3, 10), None


@pytest.mark.parametrize("name", sorted(skip_cases()) + ["B1000_C101"])
def test_skip_record_equals_the_host_rule(name):
    _need_gpu()
    from tpnet_amd import LinkRankingMeter
    from tpnet_amd.metrics import link_ranking_metrics_host
    x, skip, ks, _ = _big_skip_case() if name == "B1000_C101" else skip_cases()[name]
    meter = LinkRankingMeter(4, DEV, hits_at=ks)
    for _ in range(2):
        meter.add_skip(_dev(x, torch.float32).reshape(x.shape), _dev(skip))
    rec = meter.records()
    assert rec.shape == (2, 8) and np.array_equal(rec[0], rec[1])        # two runs: the same bits
    want = link_ranking_metrics_host(x, skip_valid(x.shape[0], x.shape[1] - 1, skip), hits_at=ks)
    assert_record(_record(rec[0]), want, name)
    if name == "B1000_C101":
        assert want["n"] == 1000 and want["n_valid_candidates"] == 1000 * 100 - int((skip >= 0).sum())
        meter.add(_dev(x, torch.float32))                                # tpnet_lp_ranking itself stays as it is
        assert_record(_record(meter.records()[2]), link_ranking_metrics_host(x, None, hits_at=ks), "no skip")
    with pytest.raises(TypeError):
        meter.add_skip(_dev(x, torch.float32).reshape(x.shape), _dev(skip).int())


# ------------------------------------------------------------------------------------------------------------------------- loop
LOOP_BATCH = 8                                                           # 22 edges: batches of 8, 8 and 6


@pytest.mark.parametrize("fused", [False, True])
def test_known_answer_with_a_zero_second_layer(fused, monkeypatch):
    """fc2.weight = 0: every logit is fc2.bias, every candidate ties with the lead, so every query has m = 2 + (N_c - 1) -- its own
    destination's copy is skipped -- and the MRR follows exactly."""
    _need_gpu()
    from tpnet_amd.callers import LinkPredictor_v1, evaluate_link_ranking_all
    monkeypatch.setattr(LinkPredictor_v1, "SCORE_ALL_FUSED", False)          # fused = False is the composition, whatever the default
    toy, rp, dec = _toy_modules(LOOP_SEED)
    with torch.no_grad():
        dec.fc2.weight.zero_()
    dec.fused_scores = fused
    res = evaluate_link_ranking_all(rp, toy["src"], toy["dst"], toy["t"], LOOP_BATCH, dec, candidate_range=(0, N))
    m = 2 + (N - 1)
    assert len(res) == 3 and res.flags == [0, 0, 0] and res.totals["n"] == 22
    for r in res:                                                        # (the mean of b equal terms: within the summation bound)
        assert abs(r["mrr"] - 2.0 / m) <= LOOP_BATCH * 2.0 ** -52 * (2.0 / m) and r["hits@1"] == 0.0 and r["hits@10"] == 0.0
    # a destination outside the range is not among the candidates: nothing is skipped for it, m = 2 + N_c
    toy, rp, dec = _toy_modules(LOOP_SEED)
    with torch.no_grad():
        dec.fc2.weight.zero_()
    dec.fused_scores = fused
    hi = 20
    res = evaluate_link_ranking_all(rp, toy["src"], toy["dst"], toy["t"], LOOP_BATCH, dec, candidate_range=(1, hi))
    inside = (toy["dst"] >= 1) & (toy["dst"] < hi)
    assert inside.any() and not inside.all()
    for k, r in enumerate(res):
        ms = 2.0 + (hi - 1) - inside[k * LOOP_BATCH:(k + 1) * LOOP_BATCH]
        want = float(np.mean(2.0 / ms))
        assert abs(r["mrr"] - want) <= LOOP_BATCH * 2.0 ** -52 * want, (k, r["mrr"], want)
    rp.check_device_errors()


def test_loop_on_both_routes_and_recommend_links(monkeypatch):
    _need_gpu()
    from tpnet_amd import LinkRankingMeter
    from tpnet_amd import score_fanout as sf
    from tpnet_amd.callers import LinkPredictor_v1, evaluate_link_ranking_all, evaluate_with_restore, recommend_links
    monkeypatch.setattr(LinkPredictor_v1, "SCORE_ALL_FUSED", False)          # the routes are set here, whatever the measured default
    from tpnet_amd.metrics import MAX_RANK_COLUMNS, link_ranking_metrics_host
    lo, hi = 1, N                                                        # the default range: id 0 is the padding row
    # ---- the straight-line restatement: expanded pairs through decoder.forward, the host rule, update after scoring
    toy, rp_ref, dec_ref = _toy_modules(LOOP_SEED)
    E = len(toy["src"])
    want = []
    with torch.no_grad():
        for b0 in range(0, E, LOOP_BATCH):
            s = slice(b0, min(b0 + LOOP_BATCH, E))
            src, dst, t = toy["src"][s], toy["dst"][s], toy["t"][s]
            b = len(src)
            ids = np.concatenate([dst[:, None], np.tile(np.arange(lo, hi), (b, 1))], axis=1)
            es, ed = np.repeat(src, ids.shape[1]), ids.reshape(-1)
            zeros = torch.zeros((len(es), 4), device=DEV)
            x = dec_ref(es, ed, zeros, zeros).view(b, ids.shape[1]).cpu().numpy()
            skip = np.where((dst >= lo) & (dst < hi), dst - lo, -1)
            want.append(link_ranking_metrics_host(x, skip_valid(b, hi - lo, skip)))
            rp_ref.update(src, dst, t)
    assert len(want) == 3 and len({w["m_sum"] for w in want}) > 1
    # ---- the composition route
    _, rp, dec = _toy_modules(LOOP_SEED)
    meter = LinkRankingMeter(8, DEV)
    n0 = sf.calls["score"]
    res = evaluate_link_ranking_all(rp, toy["src"], toy["dst"], toy["t"], LOOP_BATCH, dec, meter=meter)
    assert sf.calls["score"] == n0 and len(res) == 3
    recs = meter.records()
    for k, w in enumerate(want):
        assert_record(_record(recs[k]), w, f"composition, batch {k}")
    for a, b in zip(_layers(rp), _layers(rp_ref)):                       # the state after the loop: plain updates, bit for bit
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert float(rp.now_time) == float(rp_ref.now_time) == toy["t"][-1]
    # ---- the kernel route: every record is the host rule on the logits that call itself returned
    _, rp, dec = _toy_modules(LOOP_SEED)
    dec.fused_scores = True
    kept = []
    inner = dec.forward_one_to_all

    def keeping(*a, **kw):
        kept.append(inner(*a, **kw))
        return kept[-1]

    dec.forward_one_to_all = keeping
    meter = LinkRankingMeter(8, DEV)
    res_k = evaluate_link_ranking_all(rp, _dev(toy["src"]), _dev(toy["dst"]), _dev(toy["t"], torch.float64), LOOP_BATCH, dec, meter=meter)
    del dec.forward_one_to_all
    assert sf.calls["score"] == n0 + 3 and len(kept) == 3 and len(res_k) == 3
    recs = meter.records()
    for k, b0 in enumerate(range(0, E, LOOP_BATCH)):
        dst = toy["dst"][b0:b0 + LOOP_BATCH]
        skip = np.where((dst >= lo) & (dst < hi), dst - lo, -1)
        x = kept[k].cpu().numpy()
        assert x.shape == (len(dst), 1 + hi - lo)
        assert_record(_record(recs[k]), link_ranking_metrics_host(x, skip_valid(len(dst), hi - lo, skip)), f"kernel, batch {k}")
    for a, b in zip(_layers(rp), _layers(rp_ref)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # ---- composes with evaluate_with_restore; recommend_links = topk of the same logits
    before = [p.detach().clone() for p in rp.random_projections]
    res2 = evaluate_with_restore(rp, lambda: evaluate_link_ranking_all(rp, toy["src"], toy["dst"], toy["t"], LOOP_BATCH, dec))
    assert len(res2) == 3
    for a, b in zip(before, rp.random_projections):
        assert torch.equal(a, b.detach())
    q = _dev(toy["src"][:5])
    with torch.no_grad():
        logits = dec.forward_one_to_all(q, lo, hi)
    ids, vals = recommend_links(dec, q, 4, (lo, hi))
    top = torch.topk(logits, 4, dim=1)
    assert ids.shape == (5, 4) and ids.dtype == torch.int64 and torch.equal(vals, top.values) and torch.equal(ids, top.indices + lo)
    with pytest.raises(ValueError):
        recommend_links(dec, q, hi - lo + 1, (lo, hi))
    with pytest.raises(ValueError):
        evaluate_link_ranking_all(rp, toy["src"], toy["dst"], toy["t"], LOOP_BATCH, dec, candidate_range=(0, MAX_RANK_COLUMNS))
    rp.check_device_errors()
    assert FLAG_EMPTY == 4
