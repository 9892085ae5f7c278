"""Filtered, streaming all-node ranking on the GPU: the counts formed in the scoring kernel (tpnet_score_rank_range), the per-query
filter lists (tpnet_neg_filter_lists), the record from counts (tpnet_lp_ranking_counts) and the loop on them.

  counts     equal, exactly, the integer rule on tpnet_score_one_to_many's logits (range mode, lead = the positive); pos_logit is its
             column 0 bit for bit; guarded buffers, two calls; shapes around the tile (32 columns), the unit (KC = 4 columns for one
             row) and the workgroup (GPB units)
  answer     fc2.weight = 0: every logit ties
  errors     ids out of range: that row's NaN flag, one report, the other rows untouched
  lists      filter_lists_device against filter_lists_host on the filter fixture
  record     add_counts against link_ranking_counts_host; add / add_skip unchanged
  loop       evaluate_link_ranking_all(filter=, streaming=) against a straight-line restatement, on the kernel route and on L = 2
  large      a range beyond the 2^20 columns of one record

Fixtures: test_score_fanout's (N = 64 nodes, widths 64 .. 260) and test_rank_streaming_host's filter fixture."""
import numpy as np
import pytest
import torch

from test_decoder_f32 import _guarded, _intact
from test_gpu_parity import DEV, _layers, _module, _need_gpu
from test_link_ranking import _cell, _dev, _record
from test_link_ranking_host import FLAG_EMPTY, FLAG_NAN, assert_record
from test_rank_streaming_host import (FIL_E, FIL_Q, FLAG_OVERFLOW, all_filtered_case, counts_case, counts_of, fil_logits_of,
                                      filter_fixture, filter_sets)
from test_readout_phases import LAM, N, NP
from test_score_fanout import GPB, WIDTHS, _call, _decoder

pytestmark = pytest.mark.gpu

RANGES = [(0, 1), (0, 31), (0, 32), (0, 33), (3, 61), (0, 64)]


def _rank_call(dec, src, pos, rng):
    """tpnet_score_rank_range itself, into guarded buffers -> (counts [B, 4] int32, pos_logit [B], the buffers)."""
    from tpnet_amd import _lib
    from tpnet_amd import score_fanout as sf
    rp = dec.random_projections
    rp._ensure_engine()
    prep = sf._mlp_prepared(rp)
    assert prep is not None
    lib = _lib.load()
    B, Cn = int(src.numel()), rng[1] - rng[0]
    need = lib.tpnet_score_rank_scratch_bytes(B, Cn)
    assert need >= 16 and need % 16 == 0
    cbuf, cview = _guarded(shape=(B, 4))
    pbuf, p = _guarded(shape=(B,))
    sbuf, scratch = _guarded(shape=(need // 4,))
    fc1, fc2 = dec.fc1, dec.fc2
    rc = lib.tpnet_score_rank_range(
        rp._st_ref(), src.data_ptr(), pos.data_ptr(), rng[0], B, Cn, rp._now_host, float(rp.time_decay_weight),
        _lib.FLAG_NOT_SCALE if rp.not_scale else 0, prep.ref, fc1.weight.data_ptr(), fc1.in_features, fc1.in_features - 64,
        fc1.bias.data_ptr(), fc2.weight.data_ptr(), fc2.bias.data_ptr(), fc1.out_features, scratch.data_ptr(), need, p.data_ptr(),
        cview.data_ptr(), rp._stream())
    assert rc == 0, rc
    return cview.view(torch.int32), p, [cbuf, pbuf, sbuf]


# ----------------------------------------------------------------------------------------------------------------------- counts

@pytest.mark.parametrize("d", WIDTHS)
def test_counts_are_the_logits_counts_exactly(d):
    _need_gpu()
    rp, f = _cell(d, 3)
    dec = _decoder(d)
    rng = np.random.RandomState(23 + d)
    n_in = n_out = 0
    for B in (1, GPB[d] - 1, GPB[d] + 1):
        for lo, hi in RANGES:
            src = _dev(f["u"][rng.randint(0, NP, B)])
            pos_h = rng.randint(0, N, B).astype(np.int64)
            pos_h[0] = lo + (hi - lo) // 2                               # inside ...
            if B > 1 and hi < N:
                pos_h[1] = hi                                            # ... and just outside the range
            pos = _dev(pos_h)
            counts, p, bufs = _rank_call(dec, src, pos, (lo, hi))
            x = _call(dec, src, rng=(lo, hi), lead=pos, want_gram=False)[0]
            assert _intact(*bufs), (B, lo, hi)
            assert torch.equal(p, x[:, 0]), (B, lo, hi)
            want = counts_of(x.cpu().numpy(), lo, pos_h)
            got = counts.cpu().numpy()
            assert np.array_equal(got, want), (B, lo, hi, got[:4], want[:4])
            inside = (pos_h >= lo) & (pos_h < hi)
            assert np.array_equal(got[:, 2], (hi - lo) - inside) and (got[:, 3] == 0).all()
            n_in, n_out = n_in + int(inside.sum()), n_out + int((~inside).sum())
            counts2, p2, _ = _rank_call(dec, src, pos, (lo, hi))
            assert torch.equal(counts2, counts) and torch.equal(p2, p)
    assert n_in > 0 and n_out > 0
    rp.check_device_errors()


def test_rows_of_one_unit_write_their_counts_themselves():
    """Many rows: anchored_chunk gives KC = C, a row is one unit, its record goes straight into counts (no third launch)."""
    _need_gpu()
    from tpnet_amd import _lib
    rp, f = _cell(128, 3)
    dec = _decoder(128)
    B, lo, hi = 9000, 2, 9                                               # 9000 x 7 / 8192 > 7: KC = C
    assert _lib.load().tpnet_score_rank_scratch_bytes(B, hi - lo) == 16
    rng = np.random.RandomState(4)
    src, pos_h = _dev(f["u"][rng.randint(0, NP, B)]), rng.randint(0, 12, B).astype(np.int64)
    counts, p, bufs = _rank_call(dec, src, _dev(pos_h), (lo, hi))
    x = _call(dec, src, rng=(lo, hi), lead=_dev(pos_h), want_gram=False)[0]
    assert _intact(*bufs) and torch.equal(p, x[:, 0])
    assert np.array_equal(counts.cpu().numpy(), counts_of(x.cpu().numpy(), lo, pos_h))
    rp.check_device_errors()


def _zero_fc2_decoder(rp, seed=3):
    from tpnet_amd.callers import LinkPredictor_v1
    torch.manual_seed(seed)
    dec = LinkPredictor_v1(4, 4, 8, 1, rp, not_encode=True).to(DEV)
    with torch.no_grad():
        dec.fc2.weight.zero_()
    for p in dec.parameters():
        p.requires_grad_(False)
    return dec


@pytest.mark.parametrize("d", [64, 260])
def test_known_answer_with_a_zero_second_layer(d):
    """fc2.weight = 0: every logit is fc2.bias, so g = 0 and e = nv = C - [pos in range]."""
    _need_gpu()
    from tpnet_amd import score_fanout as sf
    rp, f = _cell(d, 3)
    dec = _zero_fc2_decoder(rp)
    assert sf.serves(dec)
    src = _dev(f["u"])
    pos_h = np.arange(NP, dtype=np.int64) % N
    n0 = sf.calls["rank"]
    for lo, hi in [(0, 33), (3, 20), (5, 6)]:
        counts, p = sf.rank_range(dec, src, _dev(pos_h), (lo, hi))
        c = counts.cpu().numpy()
        inside = (pos_h >= lo) & (pos_h < hi)
        assert inside.any() and not inside.all()
        assert (c[:, 0] == 0).all() and np.array_equal(c[:, 1], (hi - lo) - inside) and np.array_equal(c[:, 2], c[:, 1])
        assert (c[:, 3] == 0).all() and torch.equal(p, dec.fc2.bias.expand(NP))
    assert sf.calls["rank"] == n0 + 3
    with pytest.raises(ValueError):
        sf.rank_range(dec, src, _dev(pos_h), (5, 5))
    rp.check_device_errors()


# ----------------------------------------------------------------------------------------------------------------------- errors

@pytest.mark.parametrize("d", [64, 256])
def test_out_of_range_ids_flag_their_row_and_report_once(d):
    _need_gpu()
    rp, f = _cell(d, 3)
    dec = _decoder(d)
    u, v = _dev(f["u"]), _dev(f["v"])
    rp.check_device_errors()
    clean_c, clean_p, _ = _rank_call(dec, u, v, (0, N))
    clean_c, clean_p = clean_c.cpu().numpy(), clean_p.cpu().numpy().view(np.uint32)
    assert (clean_c[:, 3] == 0).all()

    def reported_once():
        with pytest.raises(IndexError):
            rp.check_device_errors()
        rp.check_device_errors()

    for what, row, bad in (("src", 11, N), ("pos", 2, N + 5), ("pos", 5, -1)):
        uu, vv = u.clone(), v.clone()
        (uu if what == "src" else vv)[row] = bad
        c, p, bufs = _rank_call(dec, uu, vv, (0, N))
        c, p = c.cpu().numpy(), p.cpu().numpy()
        keep = np.arange(NP) != row
        assert _intact(*bufs)
        assert c[row, 3] == FLAG_NAN and np.isnan(p[row]), (what, c[row])
        assert np.array_equal(c[keep], clean_c[keep]) and np.array_equal(p[keep].view(np.uint32), clean_p[keep]), what
        reported_once()


# ------------------------------------------------------------------------------------------------------------------------ lists

def _fixture_sampler():
    from tpnet_amd import GpuNegativeEdgeSampler
    fx = filter_fixture()
    return fx, GpuNegativeEdgeSampler(fx["src"], fx["dst"], fx["t"], negative_sample_strategy="random", seed=7, device=DEV)


def test_filter_lists_device_equals_the_host_rule():
    _need_gpu()
    from tpnet_amd.negative_sampler import filter_lists_host
    fx, sampler = _fixture_sampler()
    q = fx["q"]
    bs, bd, bt = _dev(fx["src"][q]), _dev(fx["dst"][q]), _dev(fx["t"][q], torch.float64)
    calls0 = sampler._calls
    for mode in ("same_time", "known"):
        cap = sampler.filter_capacity(mode)
        groups = {}
        for s_, d_, t_ in zip(fx["src"], fx["dst"], fx["t"]):
            groups.setdefault((s_, t_ if mode == "same_time" else 0.0), set()).add(d_)
        assert cap == max(len(g) for g in groups.values()) >= max(len(r) for r in filter_sets(fx, mode, 1, 64))
        for rng in [(1, 64), (9, 41), (9, 30)]:
            for F in (None, 1, 10) if mode == "known" else (None,):
                fil, n_fil = sampler.filter_lists_device(bs, bd, bt, mode, rng, capacity=F)
                Fh = cap if F is None else F
                want_fil, want_n = filter_lists_host(fx["src"], fx["dst"], fx["t"], fx["src"][q], fx["dst"][q], fx["t"][q], mode, rng, Fh)
                assert fil.dtype == torch.int64 and n_fil.dtype == torch.int32 and tuple(fil.shape) == (FIL_Q, Fh)
                assert np.array_equal(fil.cpu().numpy(), want_fil) and np.array_equal(n_fil.cpu().numpy(), want_n), (mode, rng, F)
                if F is None:
                    assert (want_n <= Fh).all()                          # the default capacity cannot overflow
                elif F == 1:
                    assert (want_n > F).all()
    assert sampler._calls == calls0
    with pytest.raises(ValueError):
        sampler.filter_lists_device(bs, bd, bt, "seen", (1, 64))
    with pytest.raises(TypeError):
        sampler.filter_lists_device(bs, bd, bt.float(), "known", (1, 64))


# ----------------------------------------------------------------------------------------------------------------------- record

def _big_counts_case():
    rng = np.random.RandomState(9)
    B, C, F, lo = 1000, 100, 8, 1
    x = np.round(rng.randn(B, 1 + C) * 4).astype(np.float32) / 4         # a grid of quarters: ties with the positive are common
    pos = rng.randint(0, C + 5, B).astype(np.int64)
    fil = np.full((B, F), -1, dtype=np.int64)
    n_fil = rng.randint(0, F + 1, B).astype(np.int32)
    for i in range(B):
        ids = np.setdiff1d(np.arange(lo, lo + C), [pos[i]])
        fil[i, :n_fil[i]] = np.sort(rng.choice(ids, n_fil[i], replace=False))
    return dict(x=x, lo=lo, pos=pos, fil=fil, n_fil=n_fil, F=F)


@pytest.mark.parametrize("name", ["B50_C40", "all_filtered", "B1000_C100"])
def test_record_from_counts_equals_the_host_rule(name):
    _need_gpu()
    from tpnet_amd import LinkRankingMeter
    from tpnet_amd.metrics import link_ranking_counts_host, link_ranking_metrics_host
    case = {"B50_C40": counts_case, "all_filtered": all_filtered_case, "B1000_C100": _big_counts_case}[name]()
    x, lo, pos = case["x"], case["lo"], case["pos"]
    counts, fl = counts_of(x, lo, pos), fil_logits_of(case)
    dc, dp = _dev(counts, torch.int32), _dev(x[:, 0].copy(), torch.float32)
    dfl, dfi, dnf = _dev(fl, torch.float32), _dev(case["fil"]), _dev(case["n_fil"], torch.int32)
    meter = LinkRankingMeter(8, DEV)
    for _ in range(2):
        meter.add_counts(dc, dp, dfl, dfi, dnf)
    meter.add_counts(dc, dp)
    C = x.shape[1] - 1
    skip = np.where((pos >= lo) & (pos < lo + C), pos - lo, -1).astype(np.int64)
    meter.add_skip(_dev(x, torch.float32), _dev(skip))
    meter.add(_dev(x, torch.float32))
    rec = meter.records()
    assert np.array_equal(rec[0], rec[1])                                # two appends: the same bits
    want = link_ranking_counts_host(counts, x[:, 0], fl, case["fil"], case["n_fil"])
    assert_record(_record(rec[0]), want, name)
    if name == "B50_C40":
        assert want["flags"] == FLAG_NAN | FLAG_OVERFLOW
    elif name == "all_filtered":
        assert want["flags"] == FLAG_EMPTY
    else:
        assert want["flags"] == 0 and want["n"] == 1000 and want["n_valid_candidates"] < int(counts[:, 2].sum())
    # no filter: the record add_skip writes from the logits, bit for bit; add and add_skip are what they were
    own = (lo + np.arange(C))[None, :] != pos[:, None]
    assert_record(_record(rec[3]), link_ranking_metrics_host(x, own), name + " add_skip")
    assert np.array_equal(rec[2], rec[3])
    assert_record(_record(rec[4]), link_ranking_metrics_host(x, None), name + " add")
    with pytest.raises(ValueError):
        meter.add_counts(dc, dp, dfl)
    with pytest.raises(TypeError):
        meter.add_counts(dc.long(), dp)


# ------------------------------------------------------------------------------------------------------------------------- loop
LOOP_BATCH = 8                                                           # the 24 queries: three batches


def _loop_modules(L, zero_fc2=False):
    """A module of N = 64 nodes (d = 64) warmed with the fixture's first 160 edges, a not_encode decoder on it; weights drawn as
    test_link_ranking._toy_modules draws them."""
    from tpnet_amd.callers import LinkPredictor_v1
    fx = filter_fixture()
    rng = np.random.RandomState(77)
    P0 = (rng.uniform(-1.0, 1.0, (N, 64)) / 8.0).astype(np.float32)
    rp = _module(N, 64, L, LAM, 0.0, P0=P0)
    rp.FANOUT_PAIRS_FROM = 0
    gen = torch.Generator().manual_seed(900 + L)
    dec = LinkPredictor_v1(4, 4, 8, 1, rp, not_encode=True)
    with torch.no_grad():
        for m in list(rp.mlp) + [dec.fc1, dec.fc2]:
            for p in m.parameters():
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * 4.0 / np.sqrt(m.in_features))
        if zero_fc2:
            dec.fc2.weight.zero_()
    dec = dec.to(DEV)
    for p in dec.parameters():
        p.requires_grad_(False)
    warm = FIL_E - FIL_Q
    for a in range(0, warm, 40):
        rp.update(fx["src"][a:min(a + 40, warm)], fx["dst"][a:min(a + 40, warm)], fx["t"][a:min(a + 40, warm)])
    return fx, rp, dec


def _restated(L, filt, lo, hi):
    """decoder.forward on the expanded pairs [dst | lo .. hi - 1], the host rule with the mask (own destination and the filter set
    dropped), update after scoring -> (the per-batch records, the module)."""
    from tpnet_amd.metrics import link_ranking_metrics_host
    fx, rp, dec = _loop_modules(L)
    sets = filter_sets(fx, filt, lo, hi) if filt else [[] for _ in range(FIL_Q)]
    q0 = FIL_E - FIL_Q
    want = []
    with torch.no_grad():
        for b0 in range(q0, FIL_E, LOOP_BATCH):
            s = slice(b0, b0 + LOOP_BATCH)
            src, dst, t = fx["src"][s], fx["dst"][s], fx["t"][s]
            b = len(src)
            ids = np.concatenate([dst[:, None], np.tile(np.arange(lo, hi), (b, 1))], axis=1)
            es, ed = np.repeat(src, ids.shape[1]), ids.reshape(-1)
            zeros = torch.zeros((len(es), 4), device=DEV)
            x = dec(es, ed, zeros, zeros).view(b, ids.shape[1]).cpu().numpy()
            mask = np.arange(lo, hi)[None, :] != dst[:, None]
            for i in range(b):
                mask[i, np.asarray(sets[b0 - q0 + i], dtype=np.int64) - lo] = False
            want.append(link_ranking_metrics_host(x, mask))
            rp.update(src, dst, t)
    return want, rp


@pytest.mark.parametrize("L", [3, 2])
@pytest.mark.parametrize("rng", [(1, 64), (9, 30)])
@pytest.mark.parametrize("filt", [None, "same_time", "known"])
def test_loop_against_a_straight_line_restatement(L, rng, filt):
    _need_gpu()
    from tpnet_amd import LinkRankingMeter
    from tpnet_amd import score_fanout as sf
    from tpnet_amd.callers import evaluate_link_ranking_all
    lo, hi = rng
    want, rp_ref = _restated(L, filt, lo, hi)
    assert len(want) == 3 and all(w["n"] == LOOP_BATCH and w["flags"] == 0 for w in want)
    fx, rp, dec = _loop_modules(L)
    _, sampler = _fixture_sampler()
    assert sf.serves(dec) is (L == 3)
    q = fx["q"]
    meter = LinkRankingMeter(4, DEV)
    n_rank, n_score = sf.calls["rank"], sf.calls["score"]
    res = evaluate_link_ranking_all(rp, fx["src"][q], fx["dst"][q], fx["t"][q], LOOP_BATCH, dec, candidate_range=rng, meter=meter,
                                    filter=filt, negative_sampler=sampler, streaming=True)
    assert len(res) == 3
    assert sf.calls["rank"] == n_rank + (3 if L == 3 else 0)
    assert sf.calls["score"] == n_score + (3 if (L == 3 and filt) else 0)          # one list-mode call per batch for the filter lists
    recs = meter.records()
    for k, w in enumerate(want):
        assert_record(_record(recs[k]), w, f"L={L} {filt} {rng}, batch {k}")
    for a, b in zip(_layers(rp), _layers(rp_ref)):                       # the state after the loop: plain updates, bit for bit
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert float(rp.now_time) == float(rp_ref.now_time) == fx["t"][-1]
    rp.check_device_errors()


def test_loop_known_answer_defaults_and_refusals():
    _need_gpu()
    from tpnet_amd import score_fanout as sf
    from tpnet_amd.callers import evaluate_link_ranking_all
    fx = filter_fixture()
    q = fx["q"]
    lo, hi = 9, 30
    inside = (fx["dst"][q] >= lo) & (fx["dst"][q] < hi)
    m_sums = {}
    for filt in (None, "same_time", "known"):
        _, rp, dec = _loop_modules(3, zero_fc2=True)
        _, sampler = _fixture_sampler()
        n_fil = np.array([len(r) for r in filter_sets(fx, filt, lo, hi)]) if filt else np.zeros(FIL_Q, dtype=np.int64)
        res = evaluate_link_ranking_all(rp, fx["src"][q], fx["dst"][q], fx["t"][q], LOOP_BATCH, dec, candidate_range=(lo, hi),
                                        filter=filt, negative_sampler=sampler, streaming=True)
        m = 2 + (hi - lo) - inside - n_fil                               # every logit ties: m = 2 + nv - n_fil
        assert res.flags == [0, 0, 0] and res.totals["n"] == FIL_Q
        for k, r in enumerate(res):
            want = float(np.mean(2.0 / m[k * LOOP_BATCH:(k + 1) * LOOP_BATCH]))
            assert abs(r["mrr"] - want) <= LOOP_BATCH * 2.0 ** -52 * want, (filt, k, r["mrr"], want)
        m_sums[filt] = int(m.sum())
    assert len(set(m_sums.values())) == 3                                # the filters change the ranks
    # ---- the defaults are the parent's loop: forward_one_to_all + add_skip, no rank call
    _, rp, dec = _loop_modules(3)
    _, rp2, dec2 = _loop_modules(3)
    n_rank = sf.calls["rank"]
    res_default = evaluate_link_ranking_all(rp, fx["src"][q], fx["dst"][q], fx["t"][q], LOOP_BATCH, dec, candidate_range=(lo, hi))
    assert sf.calls["rank"] == n_rank
    res_stream = evaluate_link_ranking_all(rp2, fx["src"][q], fx["dst"][q], fx["t"][q], LOOP_BATCH, dec2, candidate_range=(lo, hi),
                                           streaming=True)
    assert sf.calls["rank"] == n_rank + 3
    assert list(res_default) == list(res_stream) and res_default.flags == res_stream.flags       # the same logits, the same records
    with pytest.raises(ValueError):
        evaluate_link_ranking_all(rp, fx["src"][q], fx["dst"][q], fx["t"][q], LOOP_BATCH, dec, candidate_range=(lo, hi), filter="known")
    with pytest.raises(ValueError):
        evaluate_link_ranking_all(rp, fx["src"][q], fx["dst"][q], fx["t"][q], LOOP_BATCH, dec, candidate_range=(lo, hi), filter="all",
                                  negative_sampler=_fixture_sampler()[1])
    rp.check_device_errors()


def test_composition_slices_rows_and_columns():
    """A state the kernel does not serve, pairs_per_call below one row: the slices' counts and gathered filter logits are those of the
    whole matrix."""
    _need_gpu()
    fx, rp, dec = _loop_modules(2)
    _, sampler = _fixture_sampler()
    q = fx["q"]
    src, dst, t = _dev(fx["src"][q]), _dev(fx["dst"][q]), _dev(fx["t"][q], torch.float64)
    lo, hi = 1, 64
    fil, n_fil = sampler.filter_lists_device(src, dst, t, "known", (lo, hi))
    with torch.no_grad():
        x = dec.forward_one_to_all(src, lo, hi, lead_node_ids=dst)
    want = counts_of(x.cpu().numpy(), lo, fx["dst"][q])
    for per in (1 << 18, 5 * 64, 17):
        counts, p, fl = dec.rank_one_to_all(src, dst, lo, hi, filter_ids=fil, pairs_per_call=per)
        assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy()[:, :3], want[:, :3]), per
        if per == 1 << 18:                                               # one slice: the same call, the same bits
            assert torch.equal(p, x[:, 0])
            look = fil >= 0
            assert torch.equal(fl[look], x[:, 1:].gather(1, (fil - lo).clamp(min=0))[look])
    with pytest.raises(ValueError):
        dec.rank_one_to_all(src, dst, 5, 5)


# ------------------------------------------------------------------------------------------------------------------------ large

def test_a_range_beyond_the_columns_of_one_record():
    """N = 2^20 + 8 nodes: one forward_one_to_all call still fits (3 rows), its record does not; the streaming path has neither bound."""
    _need_gpu()
    from tpnet_amd import score_fanout as sf
    from tpnet_amd.callers import LinkPredictor_v1, evaluate_link_ranking_all
    from tpnet_amd.metrics import MAX_RANK_COLUMNS
    big = (1 << 20) + 8
    rp = _module(big, 64, 3, LAM, 0.0)
    rng = np.random.RandomState(31)
    e_src, e_dst = rng.randint(1, big, 64).astype(np.int64), rng.randint(1, big, 64).astype(np.int64)
    rp.update(e_src, e_dst, np.sort(rng.uniform(1.0, 1e5, 64)))
    torch.manual_seed(5)
    dec = LinkPredictor_v1(4, 4, 8, 1, rp, not_encode=True).to(DEV)
    for p in dec.parameters():
        p.requires_grad_(False)
    assert sf.serves(dec)
    src_h, pos_h = e_src[:3].copy(), np.array([e_dst[0], big - 1, 0], dtype=np.int64)      # inside, the last id, outside (1, big)
    src, pos = _dev(src_h), _dev(pos_h)
    lo, hi = 1, big
    assert 1 + (hi - lo) > MAX_RANK_COLUMNS
    n0 = sf.calls["rank"]
    counts, p, fl = dec.rank_one_to_all(src, pos, lo, hi)
    assert sf.calls["rank"] == n0 + 1 and fl is None
    with torch.no_grad():
        x = dec.forward_one_to_all(src, lo, hi, lead_node_ids=pos)
    assert torch.equal(p, x[:, 0])
    want = counts_of(x.cpu().numpy(), lo, pos_h)
    assert np.array_equal(counts.cpu().numpy(), want) and list(want[:, 2]) == [hi - lo - 1, hi - lo - 1, hi - lo]
    t = np.array([2e5, 2e5 + 1, 2e5 + 2])
    with pytest.raises(ValueError):
        evaluate_link_ranking_all(rp, src_h, pos_h, t, 3, dec)
    res = evaluate_link_ranking_all(rp, src_h, pos_h, t, 3, dec, streaming=True)
    assert len(res) == 1 and res.flags == [0] and res.totals["n"] == 3
    m = 2 + 2 * want[:, 0].astype(np.int64) + want[:, 1]
    assert abs(res[0]["mrr"] - float(np.mean(2.0 / m))) <= 3 * 2.0 ** -52 * float(np.mean(2.0 / m))
    rp.check_device_errors()
