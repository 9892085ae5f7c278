"""Streaming top-k over all nodes on the GPU: the k best ids per query formed in the scoring kernel (tpnet_score_topk_range) and what
stands on it (`score_fanout.topk_range`, `LinkPredictor_v1.topk_one_to_all`, `recommend_links(streaming=, exclude=, exclude_self=)`).

  exact      ids, logits and info equal, exactly, the rule (`topk_host`) on tpnet_score_one_to_many's logits of the same range:
             guarded buffers, two calls; shapes around the tile (32 columns), the unit (KC = 4 columns for one row: K below, at and
             above it, K above C) and the workgroup (GPB units); with and without a skip id and exclusion lists
  paths      rows of one unit (one launch, no scratch) and rows of four units with K below and above KC (the replace-min path)
  answer     fc2.weight = 0: every logit ties, the ids are the smallest admitted ones
  admission  lists from the sampler's table (held to filter_lists_host first), skip = the source, overflow, a row left empty
  errors     a source out of range: that row's NaN flag, one report, the other rows untouched
  recommend  the defaults unchanged; streaming equal in value; exclude = 'known' against a straight-line restatement; the slice route
             on an L = 2 module against the rule
  large      one query over a range beyond 2^20 ids

Every comparison is exact (floats by equality, NaN matched to NaN): promise (1) of tpnet_score_one_to_many.
Fixtures: test_score_fanout's (N = 64 nodes, widths 64 .. 260), test_rank_streaming's modules and test_rank_streaming_host's filter
fixture."""
import numpy as np
import pytest
import torch

from test_decoder_f32 import _guarded, _intact
from test_gpu_parity import DEV, _module, _need_gpu
from test_link_ranking import _cell, _dev
from test_rank_streaming import RANGES, _fixture_sampler, _loop_modules, _zero_fc2_decoder
from test_rank_streaming_host import FIL_Q, filter_fixture
from test_readout_phases import LAM, N, NP
from test_score_fanout import GPB, WIDTHS, _call, _decoder
from test_score_topk_host import FLAG_NAN, FLAG_OVERFLOW, brute_topk, same_floats

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 5, 33, 128)


def _topk_call(dec, src, rng, K, skip=None, excl=None, n_excl=None):
    """tpnet_score_topk_range itself, into guarded buffers -> (ids [B, K] int64, logits [B, K], info [B, 2] int32, the buffers)."""
    from tpnet_amd import _lib
    from tpnet_amd import score_fanout as sf
    rp = dec.random_projections
    rp._ensure_engine()
    prep = sf._mlp_prepared(rp)
    assert prep is not None
    lib = _lib.load()
    B, Cn = int(src.numel()), rng[1] - rng[0]
    need = lib.tpnet_score_topk_scratch_bytes(B, Cn, K)
    assert need >= 16 and need % 8 == 0
    ibuf, iview = _guarded(shape=(B, 2 * K))
    lbuf, logits = _guarded(shape=(B, K))
    nbuf, nview = _guarded(shape=(B, 2))
    sbuf, scratch = _guarded(shape=(need // 4,))
    fc1, fc2 = dec.fc1, dec.fc2
    rc = lib.tpnet_score_topk_range(
        rp._st_ref(), src.data_ptr(), None if skip is None else skip.data_ptr(), None if excl is None else excl.data_ptr(),
        None if excl is None else n_excl.data_ptr(), 0 if excl is None else int(excl.shape[1]), rng[0], B, Cn, K, rp._now_host,
        float(rp.time_decay_weight), _lib.FLAG_NOT_SCALE if rp.not_scale else 0, prep.ref, fc1.weight.data_ptr(), fc1.in_features,
        fc1.in_features - 64, fc1.bias.data_ptr(), fc2.weight.data_ptr(), fc2.bias.data_ptr(), fc1.out_features, scratch.data_ptr(),
        need, iview.data_ptr(), logits.data_ptr(), nview.data_ptr(), rp._stream())
    assert rc == 0, rc
    return iview.view(torch.int64), logits, nview.view(torch.int32), [ibuf, lbuf, nbuf, sbuf]


def _same(got, want, what):
    ids, logits, info = (a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in got[:3])
    assert np.array_equal(ids, want[0]), (what, ids[:3], want[0][:3])
    assert same_floats(logits, want[1]), (what, logits[:3], want[1][:3])
    assert np.array_equal(info, want[2]), (what, info[:6], want[2][:6])


def _random_lists(rng, B, lo, hi, F):
    """Exclusion lists as filter_lists_device lays them out: ascending, distinct ids of [lo, hi), -1 behind them."""
    excl = np.full((B, F), -1, dtype=np.int64)
    n = rng.randint(0, min(F, hi - lo) + 1, B).astype(np.int32)
    for i in range(B):
        excl[i, :n[i]] = np.sort(rng.choice(np.arange(lo, hi), n[i], replace=False))
        if n[i] == F and i % 2:
            n[i] += 2                                                    # a full row whose true list was longer: overflow
    return excl, n


# ------------------------------------------------------------------------------------------------------------------------ exact

@pytest.mark.parametrize("d", WIDTHS)
def test_topk_is_the_logits_topk_exactly(d):
    _need_gpu()
    from tpnet_amd.score_fanout import topk_host
    rp, f = _cell(d, 3)
    dec = _decoder(d)
    rng = np.random.RandomState(41 + d)
    n_short = n_over_c = 0
    for B in (1, GPB[d] - 1, GPB[d] + 1):
        for lo, hi in RANGES:
            src = _dev(f["u"][rng.randint(0, NP, B)])
            x = _call(dec, src, rng=(lo, hi), want_gram=False)[0].cpu().numpy()
            skip_h = rng.randint(lo - 1, hi + 1, B).astype(np.int64)         # mostly inside, now and then just outside
            excl_h, n_h = _random_lists(rng, B, lo, hi, 7)
            skip, excl, n_ex = _dev(skip_h), _dev(excl_h), _dev(n_h, torch.int32)
            for K in KS:
                got = _topk_call(dec, src, (lo, hi), K)
                assert _intact(*got[3]), (B, lo, hi, K)
                _same(got, topk_host(x, K, lo), (B, lo, hi, K))
                again = _topk_call(dec, src, (lo, hi), K)
                assert all(torch.equal(a, b) for a, b in zip(got[:3], again[:3])), (B, lo, hi, K)
                got = _topk_call(dec, src, (lo, hi), K, skip=skip, excl=excl, n_excl=n_ex)
                assert _intact(*got[3]), (B, lo, hi, K)
                want = topk_host(x, K, lo, skip_ids=skip_h, exclude_ids=excl_h, n_exclude=n_h)
                _same(got, want, (B, lo, hi, K, "admission"))
                n_short += int((want[2][:, 0] < K).sum())
                n_over_c += int(K > hi - lo)
    assert n_short > 0 and n_over_c > 0
    rp.check_device_errors()


@pytest.mark.parametrize("B,K,units", [(9000, 5, 1), (2100, 5, 4), (2100, 20, 4)])
def test_rows_of_one_unit_and_the_replace_min_path(B, K, units):
    """C = 64 at d = 128.  9000 rows: KC = 64, a row is one unit, the kernel writes the outputs itself (scratch 16 bytes, one
    launch).  2100 rows: KC = 17, four units per row; K = 5 fills a unit's list early and replaces its minimum from then on,
    K = 20 > KC hands on lists of 17."""
    _need_gpu()
    from tpnet_amd import _lib
    from tpnet_amd.score_fanout import topk_host
    rp, f = _cell(128, 3)
    dec = _decoder(128)
    lo, hi = 0, 64
    kc = 64 if units == 1 else 17
    assert _lib.load().tpnet_score_topk_scratch_bytes(B, hi - lo, K) == 16 + (B * units * min(K, kc) * 8 if units > 1 else 0)
    rng = np.random.RandomState(B + K)
    src = _dev(f["u"][rng.randint(0, NP, B)])
    x = _call(dec, src, rng=(lo, hi), want_gram=False)[0].cpu().numpy()
    got = _topk_call(dec, src, (lo, hi), K)
    assert _intact(*got[3])
    _same(got, topk_host(x, K, lo), (B, K))
    skip_h = rng.randint(lo, hi, B).astype(np.int64)
    excl_h, n_h = _random_lists(rng, B, lo, hi, 9)
    got = _topk_call(dec, src, (lo, hi), K, skip=_dev(skip_h), excl=_dev(excl_h), n_excl=_dev(n_h, torch.int32))
    assert _intact(*got[3])
    _same(got, topk_host(x, K, lo, skip_ids=skip_h, exclude_ids=excl_h, n_exclude=n_h), (B, K, "admission"))
    rp.check_device_errors()


# ----------------------------------------------------------------------------------------------------------------------- answer

@pytest.mark.parametrize("d", [64, 260])
def test_known_answer_with_a_zero_second_layer(d):
    """fc2.weight = 0: every logit is fc2.bias, so a row's answer is its K smallest admitted ids in ascending order."""
    _need_gpu()
    from tpnet_amd import score_fanout as sf
    rp, f = _cell(d, 3)
    dec = _zero_fc2_decoder(rp)
    assert sf.serves(dec)
    src_h = f["u"]
    src = _dev(src_h)
    bias = float(dec.fc2.bias.item())
    n0 = sf.calls["topk"]
    for lo, hi, K in [(0, 33, 5), (3, 20, 17), (5, 6, 3), (0, 64, 40)]:
        ids, logits, info = sf.topk_range(dec, src, K, (lo, hi))
        n = min(K, hi - lo)
        want = np.concatenate([np.arange(lo, lo + n), np.full(K - n, -1)])
        assert (ids.cpu().numpy() == want[None, :]).all() and (info.cpu().numpy() == [n, 0]).all()
        assert (logits.cpu().numpy()[:, :n] == np.float32(bias)).all() and np.isneginf(logits.cpu().numpy()[:, n:]).all()
        # skip = lo + (row % 3), and the two ids behind it on the row's list
        skip_h = lo + (np.arange(NP, dtype=np.int64) % 3)
        excl_h = np.stack([skip_h + 1, skip_h + 2, np.full(NP, -1)], axis=1)
        ids, logits, info = sf.topk_range(dec, src, K, (lo, hi), skip_ids=_dev(skip_h), exclude_ids=_dev(excl_h),
                                          n_exclude=_dev(np.full(NP, 2), torch.int32))
        for i in (0, 1, 2, NP - 1):
            left = [c for c in range(lo, hi) if not skip_h[i] <= c <= skip_h[i] + 2]
            w = left[:K] + [-1] * (K - min(K, len(left)))
            assert list(ids[i].cpu().numpy()) == w and list(info[i].cpu().numpy()) == [min(K, len(left)), 0], (lo, hi, K, i)
    assert sf.calls["topk"] == n0 + 8
    for bad in (dict(k=0), dict(k=129), dict(cand_range=(5, 5))):
        kw = dict(k=3, cand_range=(0, 9))
        kw.update(bad)
        with pytest.raises(ValueError):
            sf.topk_range(dec, src, **kw)
    rp.check_device_errors()


# -------------------------------------------------------------------------------------------------------------------- admission

@pytest.mark.parametrize("rng", [(1, 64), (9, 41), (9, 30)])
def test_admission_with_the_samplers_lists(rng):
    _need_gpu()
    from tpnet_amd.negative_sampler import filter_lists_host
    from tpnet_amd.score_fanout import topk_host
    lo, hi = rng
    rp, f = _cell(128, 3)
    dec = _decoder(128)
    fx, sampler = _fixture_sampler()
    q = fx["q"]
    src_h = fx["src"][q]
    none = np.full(FIL_Q, -1, dtype=np.int64)
    src, dst, t = _dev(src_h), _dev(none), _dev(np.zeros(FIL_Q), torch.float64)
    x = _call(dec, src, rng=rng, want_gram=False)[0].cpu().numpy()
    cap = sampler.filter_capacity("known")
    for F in (None, 10):
        fil, n_fil = sampler.filter_lists_device(src, dst, t, "known", rng, capacity=F)
        Fh = cap if F is None else F
        fil_h, n_h = filter_lists_host(fx["src"], fx["dst"], fx["t"], src_h, none, np.zeros(FIL_Q), "known", rng, Fh)
        assert np.array_equal(fil.cpu().numpy(), fil_h) and np.array_equal(n_fil.cpu().numpy(), n_h)      # a destination of -1 drops nothing
        known = [sorted({int(b) for a, b in zip(fx["src"], fx["dst"]) if a == s and lo <= b < hi}) for s in src_h]
        assert all(list(fil_h[i, :min(Fh, len(r))]) == r[:Fh] and n_h[i] == len(r) for i, r in enumerate(known))
        for K in (3, 10, 60):
            got = _topk_call(dec, src, rng, K, skip=src, excl=fil, n_excl=n_fil)
            assert _intact(*got[3])
            _same(got, topk_host(x, K, lo, skip_ids=src_h, exclude_ids=fil_h, n_exclude=n_h), (rng, F, K))
            ids, info = got[0].cpu().numpy(), got[2].cpu().numpy()
            over = n_h > Fh
            assert np.array_equal((info[:, 1] & FLAG_OVERFLOW) != 0, over) and over.any() == (F == 10)     # exactly the overflowing rows
            for i in range(FIL_Q):
                assert src_h[i] not in ids[i] and not set(ids[i]) & set(fil_h[i][fil_h[i] >= 0]), (rng, F, K, i)
                if not over[i]:
                    assert info[i, 0] == min(K, (hi - lo) - len(known[i]) - int(lo <= src_h[i] < hi))
    # a row whose every candidate is on its list, beside an ordinary one
    small = (9, 13)
    excl = _dev(np.array([[9, 10, 11, 12, -1], [10, -1, -1, -1, -1]], dtype=np.int64))
    got = _topk_call(dec, src[:2], small, 3, excl=excl, n_excl=_dev(np.array([4, 1]), torch.int32))
    ids, logits, info = (a.cpu().numpy() for a in got[:3])
    assert list(info[0]) == [0, 0] and (ids[0] == -1).all() and np.isneginf(logits[0]).all()
    assert list(info[1]) == [3, 0] and sorted(ids[1]) == [9, 11, 12]
    rp.check_device_errors()


# ----------------------------------------------------------------------------------------------------------------------- errors

@pytest.mark.parametrize("d", [64, 256])
def test_a_source_out_of_range_flags_its_row_and_reports_once(d):
    _need_gpu()
    rp, f = _cell(d, 3)
    dec = _decoder(d)
    u = _dev(f["u"])
    rp.check_device_errors()
    K = 6
    clean = [a.cpu().numpy() for a in _topk_call(dec, u, (0, N), K)[:3]]
    assert (clean[2] == [K, 0]).all()
    for row, bad, kw in ((11, N, {}), (2, -1, dict(skip=_dev(np.full(NP, 1))))):
        uu = u.clone()
        uu[row] = bad
        got = _topk_call(dec, uu, (0, N), K, **kw)
        ids, logits, info = (a.cpu().numpy() for a in got[:3])
        keep = np.arange(NP) != row
        assert _intact(*got[3])
        first = [c for c in range(N) if not (kw and c == 1)][:K]             # every key ties at NaN: the smallest admitted ids
        assert list(ids[row]) == first and np.isnan(logits[row]).all() and list(info[row]) == [K, FLAG_NAN], (row, ids[row], info[row])
        if not kw:
            assert np.array_equal(ids[keep], clean[0][keep]) and np.array_equal(logits[keep].view(np.uint32), clean[1][keep].view(np.uint32))
        assert (info[keep] == [K, 0]).all()
        with pytest.raises(IndexError):
            rp.check_device_errors()
        rp.check_device_errors()                                             # reported once


# -------------------------------------------------------------------------------------------------------------------- recommend

def test_recommend_links_defaults_streaming_and_known():
    _need_gpu()
    from tpnet_amd import score_fanout as sf
    from tpnet_amd.callers import recommend_links
    fx, rp, dec = _loop_modules(3)
    _, sampler = _fixture_sampler()
    assert sf.serves(dec)
    lo, hi = 1, 64
    src_h = np.array([1, 2, 3, 4, 5, 33, 2], dtype=np.int64)                   # the fixture's four sources, two without edges, a repeat
    src = _dev(src_h)
    with torch.no_grad():
        x = dec.forward_one_to_all(src, lo, hi)
    xh = x.cpu().numpy()
    for k in (1, 10, 63):
        n_topk, n_score = sf.calls["topk"], sf.calls["score"]
        ids, logits = recommend_links(dec, src_h, k, (lo, hi))
        top = torch.topk(x, k, dim=1)
        assert torch.equal(ids, top.indices + lo) and torch.equal(logits, top.values)              # the defaults: the parent's lines
        assert sf.calls["topk"] == n_topk and sf.calls["score"] == n_score + 1
        ids_s, logits_s = recommend_links(dec, src_h, k, (lo, hi), streaming=True)
        assert sf.calls["topk"] == n_topk + 1 and sf.calls["score"] == n_score + 1                 # no logit matrix
        assert ids_s.dtype == torch.int64 and logits_s.dtype == torch.float32
        assert torch.equal(logits_s, logits)
        for i in range(len(src_h)):
            if len(set(xh[i])) == xh.shape[1]:                                                     # no ties in the row
                assert torch.equal(ids_s[i], ids[i]), (k, i)
        want = brute_topk(xh, k, lo)
        assert np.array_equal(ids_s.cpu().numpy(), want[0])
        # exclude = "known" (+ the source itself) against a straight-line restatement: Python sets from the stream
        known = [sorted({int(b) for a, b in zip(fx["src"], fx["dst"]) if a == s and lo <= b < hi}) for s in src_h]
        F = max(1, max(len(r) for r in known))
        excl = np.full((len(src_h), F), -1, dtype=np.int64)
        for i, r in enumerate(known):
            excl[i, :len(r)] = r
        for self_too in (False, True):
            ids_k, logits_k = recommend_links(dec, src, k, (lo, hi), exclude="known", negative_sampler=sampler, exclude_self=self_too)
            want = brute_topk(xh, k, lo, skip=src_h if self_too else None, excl=excl)
            assert np.array_equal(ids_k.cpu().numpy(), want[0]) and same_floats(logits_k.cpu().numpy(), want[1]), (k, self_too)
        assert len(known[0]) > 0 and known[4] == [] and (want[0][0] == -1).any() == (k > 62 - len(known[0]))
    with pytest.raises(ValueError):
        recommend_links(dec, src, 3, (lo, hi), exclude="known")
    with pytest.raises(ValueError):
        recommend_links(dec, src, 3, (lo, hi), exclude="seen", negative_sampler=sampler)
    with pytest.raises(ValueError):
        recommend_links(dec, src, 64, (lo, hi), streaming=True)
    rp.check_device_errors()


def test_slice_route_on_an_unserved_module_equals_the_rule():
    """L = 2: the kernel does not serve the module; pairs_per_call forces row slices, one row per slice and column slices.  Also
    k beyond the kernel's 128 on a served module."""
    _need_gpu()
    from tpnet_amd import score_fanout as sf
    from tpnet_amd.callers import recommend_links
    from tpnet_amd.score_fanout import topk_host
    fx, rp, dec = _loop_modules(2)
    _, sampler = _fixture_sampler()
    assert not sf.serves(dec)
    q = fx["q"]
    src_h = fx["src"][q]
    src = _dev(src_h)
    lo, hi = 1, 64
    fil, n_fil = sampler.filter_lists_device(src, _dev(np.full(FIL_Q, -1)), _dev(np.zeros(FIL_Q), torch.float64), "known", (lo, hi), capacity=12)
    fil_h, n_h = fil.cpu().numpy(), n_fil.cpu().numpy()
    assert (n_h > 12).any()
    with torch.no_grad():
        x = dec.forward_one_to_all(src, lo, hi).cpu().numpy()
    n0 = sf.calls["topk"]

    def sliced(per):
        """forward_one_to_all's logits taken in the route's own slices (the torch layers' bits may depend on a call's shape)."""
        C = hi - lo
        rows, width = max(1, per // C), min(C, per)
        with torch.no_grad():
            return torch.cat([torch.cat([dec.forward_one_to_all(src[r0:r0 + rows], c0, min(c0 + width, hi), pairs_per_call=per)
                                         for c0 in range(lo, hi, width)], dim=1) for r0 in range(0, FIL_Q, rows)], dim=0).cpu().numpy()

    for per in (1 << 18, 5 * 63, 63, 17):                                    # one slice; row slices; one row a slice; column slices
        xs = x if per == 1 << 18 else sliced(per)
        assert xs.shape == x.shape
        for k in (1, 5, 63, 70, 200):
            got = dec.topk_one_to_all(src, k, lo, hi, pairs_per_call=per)
            _same(got, topk_host(xs, k, lo), (k, per))
            got = dec.topk_one_to_all(src, k, lo, hi, skip_node_ids=src, exclude_ids=fil, n_exclude=n_fil, pairs_per_call=per)
            _same(got, topk_host(xs, k, lo, skip_ids=src_h, exclude_ids=fil_h, n_exclude=n_h), (k, per, "admission"))
    ids, logits = recommend_links(dec, src_h, 5, (lo, hi), exclude="known", negative_sampler=sampler, exclude_self=True)
    full, n_full = sampler.filter_lists_device(src, _dev(np.full(FIL_Q, -1)), _dev(np.zeros(FIL_Q), torch.float64), "known", (lo, hi))
    want = topk_host(x, 5, lo, skip_ids=src_h, exclude_ids=full.cpu().numpy(), n_exclude=n_full.cpu().numpy())
    assert np.array_equal(ids.cpu().numpy(), want[0]) and same_floats(logits.cpu().numpy(), want[1])
    assert sf.calls["topk"] == n0
    # a served module, k = 200 > 128: the slices, not the kernel
    _, rp3, dec3 = _loop_modules(3)
    with torch.no_grad():
        x3 = dec3.forward_one_to_all(src, lo, hi).cpu().numpy()
    got = dec3.topk_one_to_all(src, 200, lo, hi, skip_node_ids=src)
    assert sf.calls["topk"] == n0
    _same(got, topk_host(x3, 200, lo, skip_ids=src_h), "k = 200")
    got = dec3.topk_one_to_all(src, 128, lo, hi, skip_node_ids=src)
    assert sf.calls["topk"] == n0 + 1
    _same(got, topk_host(x3, 128, lo, skip_ids=src_h), "k = 128")


# ------------------------------------------------------------------------------------------------------------------------ large

def test_one_query_over_a_range_beyond_2_to_the_20():
    """N = 2^20 + 8 nodes, one query: 8 129 units of 129 ids, whose lists the second launch selects from; the reference is
    forward_one_to_all taken in four slices."""
    _need_gpu()
    from tpnet_amd import _lib
    from tpnet_amd import score_fanout as sf
    from tpnet_amd.callers import LinkPredictor_v1, recommend_links
    from tpnet_amd.score_fanout import topk_host
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
    lo, hi = 1, big
    src_h = e_src[:1].copy()
    src = _dev(src_h)
    cuts = [lo, lo + 300000, lo + 300001, lo + 800000, hi]
    with torch.no_grad():
        x = torch.cat([dec.forward_one_to_all(src, a, b) for a, b in zip(cuts[:-1], cuts[1:])], dim=1).cpu().numpy()
    assert x.shape == (1, hi - lo) and hi - lo > 1 << 20
    for K in (10, 128):
        assert _lib.load().tpnet_score_topk_scratch_bytes(1, hi - lo, K) == 16 + 8129 * min(K, 129) * 8
        n0 = sf.calls["topk"]
        got = dec.topk_one_to_all(src, K, lo, hi)
        assert sf.calls["topk"] == n0 + 1
        want = topk_host(x, K, lo)
        _same(got, want, K)
        # the best ten ids on the exclusion list, the eleventh skipped: the answer moves down the order
        best = topk_host(x, 11 + K, lo)[0][0]
        excl = _dev(np.sort(best[:10])[None, :])
        got = dec.topk_one_to_all(src, K, lo, hi, skip_node_ids=_dev(best[10:11]), exclude_ids=excl, n_exclude=_dev(np.array([10]), torch.int32))
        assert np.array_equal(got[0].cpu().numpy()[0], best[11:]) and list(got[2].cpu().numpy()[0]) == [K, 0]
    ids, logits = recommend_links(dec, src_h, 10, (lo, hi), streaming=True)
    assert np.array_equal(ids.cpu().numpy(), topk_host(x, 10, lo)[0]) and same_floats(logits.cpu().numpy(), topk_host(x, 10, lo)[1])
    rp.check_device_errors()
