"""The one-vs-many ranking evaluation without a GPU: the host rule of the ranking record against a brute-force double loop, the
per-query candidate rule of `GpuNegativeEdgeSampler.sample_many_device` restated in Python and checked for what it promises, the
new C symbols (declared, exported, bound, argument checks) and the Python surface on a CPU module.

The record (include/tpnet_hip.h: tpnet_lp_ranking): per query over its valid candidates g = #{q > p}, e = #{q == p}, m = 2 + 2 g + e
(twice the rank); a query with a NaN among p and its valid candidates, or without a valid candidate, is not counted; mrr = mean 2 / m,
hits@k = #{m <= 2 k} / n.

The candidate rule (include/tpnet_hip.h: tpnet_neg_sample_many), for query i = (s, d, t): a destination d' is excluded when d' == d
or (s, d') occurs at time exactly t.  Historical part: the unique edges of source s in ascending destination order, visited in the
order perm_i(R, 5, j); eligible = not excluded and first seen before t; the first Qh eligible ones.  Random part: Ud visited in the
order perm_i(|Ud|, 6, j); accepted = not excluded and not a historical pick; until the row is full; -1 where they run out.  perm_i =
perm under the seed whose high word is xored with i.  `restated_rows` is that rule; tests/test_link_ranking.py holds the device to it
bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

from test_negative_sampler import Table, perm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tpnet_pair_gram_fanout", "tpnet_pair_gram_fanout_supported", "tpnet_neg_sample_many", "tpnet_lp_ranking_scratch_bytes",
               "tpnet_lp_ranking")
FLAG_NO_QUERY, FLAG_NAN, FLAG_EMPTY = 1, 2, 4


# ------------------------------------------------------------------------------------------------------ the record's host rule

def brute_force_record(logits, valid, ks):
    """The rule as a double loop over queries and candidates, in Python numbers."""
    B, C1 = logits.shape
    ms, nvalid, flags = [], 0, 0
    for i in range(B):
        p = logits[i, 0]
        g = e = nv = 0
        nan = bool(np.isnan(p))
        for c in range(C1 - 1):
            if not valid[i, c]:
                continue
            q = logits[i, 1 + c]
            nv += 1
            nan = nan or bool(np.isnan(q))
            g += int(q > p)
            e += int(q == p)
        nvalid += nv
        if nan:
            flags |= FLAG_NAN
        if nv == 0:
            flags |= FLAG_EMPTY
        if not nan and nv:
            ms.append(2 + 2 * g + e)
    n = len(ms)
    if n == 0:
        return dict(mrr=float("nan"), hits=tuple(float("nan") for _ in ks), m_sum=0, n=0, n_valid_candidates=nvalid,
                    flags=flags | FLAG_NO_QUERY)
    mrr = 0.0
    for m in ms:
        mrr += 2.0 / m
    return dict(mrr=mrr / n, hits=tuple(sum(1 for m in ms if m <= 2 * k) / n for k in ks), m_sum=sum(ms), n=n,
                n_valid_candidates=nvalid, flags=flags)


def record_cases():
    """name -> (logits [B, 1 + C] fp32, valid [B, C] bool or None, hits_at): the cases both the host rule and the device record are held to."""
    rng = np.random.RandomState(5)
    nan = np.float32(np.nan)
    cases = {}
    x = rng.randint(-3, 4, (40, 13)).astype(np.float32)                   # small integers: many ties with the positive, e odd and even
    x[0, 1:4] = x[0, 0]
    x[0, 4:] = x[0, 0] - 1                                                 # e = 3
    x[1, 1:5] = x[1, 0]
    x[1, 5:] = x[1, 0] + 1                                                 # e = 4, everything else above
    cases["ties"] = (x, None, (1, 3, 10))
    x = rng.randn(9, 8).astype(np.float32)
    v = rng.rand(9, 7) < 0.7
    v[3] = False                                                           # a row with all candidates absent
    v[0, 0] = True
    cases["absent_row"] = (x, v, (1, 3, 10))
    x = rng.randn(6, 6).astype(np.float32)
    x[2, 0] = nan                                                          # a NaN positive
    cases["nan_positive"] = (x, None, (1, 3, 10))
    x = rng.randn(7, 9).astype(np.float32)
    v = np.ones((7, 8), dtype=bool)
    x[1, 4] = nan                                                          # a NaN among the valid candidates: flagged, not counted
    x[5, 3] = nan
    v[5, 2] = False                                                        # a NaN under an absent slot: neither
    cases["nan_candidate"] = (x, v, (1, 3, 10))
    x = rng.randn(5, 7).astype(np.float32)
    v = np.ones((5, 6), dtype=bool)
    x[2, 5] = nan
    v[2, 4] = False
    cases["nan_under_absent_only"] = (x, v, (1, 3, 10))
    cases["one_candidate"] = (rng.randint(0, 2, (11, 2)).astype(np.float32), None, (1, 3, 10))        # C = 1
    cases["k_beyond_columns"] = (rng.randn(8, 4).astype(np.float32), None, (1, 5, 100))               # k > C + 1
    cases["nothing_counted"] = (np.full((3, 4), nan, dtype=np.float32), None, (1, 3, 10))
    cases["signed_zero_and_inf"] = (np.array([[0.0, -0.0, np.inf, -np.inf], [np.inf, np.inf, 1.0, 2.0]], dtype=np.float32), None, (1, 2, 3))
    return cases


def assert_record(got, want, what):
    """Integers exact, hits bit for bit, mrr within n 2^-52 relative (the float64 sums differ in order only)."""
    for k in ("m_sum", "n", "n_valid_candidates", "flags"):
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"
    assert len(got["hits"]) == len(want["hits"])
    for a, b in zip(got["hits"], want["hits"]):
        assert np.float64(a).tobytes() == np.float64(b).tobytes() or (np.isnan(a) and np.isnan(b)), f"{what}: hits {a} != {b}"
    if want["n"] == 0:
        assert np.isnan(got["mrr"]), what
    else:
        print(f"{what}: mrr {got['mrr']!r} against {want['mrr']!r}")
        assert abs(got["mrr"] - want["mrr"]) <= want["n"] * 2.0 ** -52 * abs(want["mrr"]), f"{what}: mrr {got['mrr']!r} != {want['mrr']!r}"


@pytest.mark.parametrize("name", sorted(record_cases()))
def test_host_rule_against_a_brute_force_double_loop(name):
    from tpnet_amd.metrics import link_ranking_metrics_host
    x, v, ks = record_cases()[name]
    valid = np.ones((x.shape[0], x.shape[1] - 1), dtype=bool) if v is None else v
    want = brute_force_record(x, valid, ks)
    assert_record(link_ranking_metrics_host(x, v, hits_at=ks), want, name)
    if name == "nan_under_absent_only":
        assert want["flags"] == 0 and want["n"] == 5
    if name == "nan_candidate":
        assert want["flags"] == FLAG_NAN and want["n"] == 6
    if name == "absent_row":
        assert want["flags"] == FLAG_EMPTY and want["n"] == 8
    if name == "nothing_counted":
        assert want["flags"] == FLAG_NO_QUERY | FLAG_NAN
    if name == "ties":
        assert want["n"] == 40


# ------------------------------------------------------------------------------------------------ the candidate rule, restated

class Graph:
    """Edges (src, dst, t) and their table (test_negative_sampler.Table: unique edges in key order with ascending occurrence times)."""

    def __init__(self, src, dst, t):
        self.src, self.dst, self.t = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(t, np.float64)
        self.tab = Table(self.src, self.dst, self.t)
        self.usrc, self.udst = self.tab.ukeys >> 32, self.tab.ukeys & 0xFFFFFFFF
        self.end = np.append(self.tab.start[1:], len(self.tab.times))


def _visit_orders(g, s, d, t, i, seed, call):
    """Query i's two visiting lists, whatever Q and Qh: the eligible historical destinations and the non-excluded destinations of Ud."""
    tab = g.tab
    key = seed ^ (i << 32)                                            # perm_i: the seed's high word xor i
    lo, hi = np.searchsorted(g.usrc, s, "left"), np.searchsorted(g.usrc, s, "right")
    R = int(hi - lo)
    at_t = lambda e: bool((tab.times[tab.start[e]:g.end[e]] == t).any())
    hist = []
    if R:
        for x in perm(R, 5, np.arange(R), key, call).astype(np.int64):
            e = lo + int(x)
            dd = int(g.udst[e])
            if dd != d and tab.first[e] < t and not at_t(e):
                hist.append(dd)
    same_instant = {int(g.udst[e]) for e in range(lo, hi) if at_t(e)}
    nud = len(tab.ud)
    rand = [int(tab.ud[x]) for x in perm(nud, 6, np.arange(nud), key, call).astype(np.int64)]
    return hist, [dd for dd in rand if dd != d and dd not in same_instant]


def restated_rows(g, bs, bd, bt, Q, Qh, seed, call, cache=None):
    """-> (cand [B, Q] int64, n_hist [B] int32) by the rule.  cache: a dict that keeps the visiting lists across (Q, Qh)."""
    B = len(bs)
    cand = np.full((B, Q), -1, dtype=np.int64)
    n_hist = np.zeros(B, dtype=np.int32)
    for i in range(B):
        k = (i, int(bs[i]), int(bd[i]), float(bt[i]), seed, call)
        if cache is None or k not in cache:
            lists = _visit_orders(g, int(bs[i]), int(bd[i]), float(bt[i]), i, seed, call)
            if cache is not None:
                cache[k] = lists
        else:
            lists = cache[k]
        hist = lists[0][:Qh]
        row = hist + [dd for dd in lists[1] if dd not in hist][:Q - len(hist)]
        cand[i, :len(row)] = row
        n_hist[i] = len(hist)
    return cand, n_hist


_graphs = {}


def graph(name):
    """'mixed': 25 sources x 40 destinations, 900 edges, integer stamps of ~6 edges each (same-instant positives exist);
    'hub': source 1 has R = 200 unique destinations (more than one wave step), 30 other sources; 'seven': |Ud| = 7."""
    if name not in _graphs:
        rng = np.random.RandomState({"mixed": 3, "hub": 4, "seven": 5}[name])
        if name == "mixed":
            src, dst = rng.randint(1, 26, 900), rng.randint(26, 66, 900)
            t = np.sort(rng.randint(0, 150, 900)).astype(np.float64)
        elif name == "hub":
            src = np.concatenate([np.ones(420, np.int64), rng.randint(2, 32, 300)])
            dst = np.concatenate([np.tile(np.arange(100, 300), 3)[:420], rng.randint(100, 340, 300)])
            o = rng.permutation(720)
            src, dst = src[o], dst[o]
            t = np.sort(rng.randint(0, 90, 720)).astype(np.float64)
        else:
            src, dst = rng.randint(1, 6, 120), rng.randint(10, 17, 120)
            t = np.sort(rng.randint(0, 30, 120)).astype(np.float64)
        _graphs[name] = Graph(src, dst, t)
    return _graphs[name]


def batch_of(g, B, start=None):
    """B consecutive edges of the graph as queries, late in the stream (most sources have a history by then)."""
    E = len(g.src)
    b0 = (E * 2) // 3 if start is None else start
    idx = (b0 + np.arange(B)) % E
    return g.src[idx].copy(), g.dst[idx].copy(), g.t[idx].copy()


def assert_row_promises(g, bs, bd, bt, cand, n_hist, Q, Qh, what):
    """What a row promises, from the raw edge arrays (not from the table): distinct entries, never the true destination, never a
    same-instant positive; the first n_hist are earlier edges of the source and n_hist = min(Qh, #eligible); -1 exactly when the
    admissible destinations run out."""
    ud = set(int(x) for x in np.unique(g.dst))
    for i in range(len(bs)):
        s, d, t = int(bs[i]), int(bd[i]), float(bt[i])
        mine = g.src == s
        same_instant = set(int(x) for x in g.dst[mine & (g.t == t)])
        earlier = set(int(x) for x in g.dst[mine & (g.t < t)])
        eligible = earlier - same_instant - {d}
        admissible = ud - same_instant - {d}
        row = [int(x) for x in cand[i]]
        real = [x for x in row if x >= 0]
        assert len(set(real)) == len(real), f"{what} row {i}: repeated entries"
        assert d not in real and not (set(real) & same_instant), f"{what} row {i}: an excluded destination"
        assert set(real) <= ud
        h = int(n_hist[i])
        assert h == min(Qh, len(eligible)), f"{what} row {i}: n_hist {h}, {len(eligible)} eligible, Qh {Qh}"
        assert set(row[:h]) <= eligible, f"{what} row {i}: a historical entry that is no earlier edge of the source"
        assert len(real) == min(Q, len(admissible)), f"{what} row {i}: {len(real)} entries, {len(admissible)} admissible, Q {Q}"
        assert row[len(real):] == [-1] * (Q - len(real)), f"{what} row {i}: -1 before the end"


@pytest.mark.parametrize("name,Q,Qh", [("mixed", 20, 10), ("mixed", 1, 0), ("mixed", 39, 39), ("hub", 100, 50), ("hub", 250, 250),
                                       ("seven", 10, 5), ("seven", 10, 0), ("seven", 6, 6)])
def test_restated_candidate_rule_keeps_its_promises(name, Q, Qh):
    g = graph(name)
    bs, bd, bt = batch_of(g, 40)
    cand, n_hist = restated_rows(g, bs, bd, bt, Q, Qh, seed=1234, call=0)
    assert_row_promises(g, bs, bd, bt, cand, n_hist, Q, Qh, f"{name} Q={Q} Qh={Qh}")
    if name == "seven" and Q == 10:
        assert (cand == -1).any(axis=1).all()                        # at most 6 admissible destinations: every row runs out
    if name == "hub":
        assert (bs == 1).any() and n_hist[bs == 1].max() >= min(Qh, 65)          # the hub's rows take more than one step of 64


def test_restated_row_does_not_depend_on_the_other_rows():
    g = graph("mixed")
    bs, bd, bt = batch_of(g, 30)
    cand, n_hist = restated_rows(g, bs, bd, bt, 20, 10, seed=99, call=3)
    bs2, bd2, bt2 = batch_of(g, 30, start=100)
    keep = [4, 17, 29]
    bs2[keep], bd2[keep], bt2[keep] = bs[keep], bd[keep], bt[keep]
    cand2, n_hist2 = restated_rows(g, bs2, bd2, bt2, 20, 10, seed=99, call=3)
    assert np.array_equal(cand2[keep], cand[keep]) and np.array_equal(n_hist2[keep], n_hist[keep])
    other = [i for i in range(30) if i not in keep]
    assert not np.array_equal(cand2[other], cand[other])
    # ... nor on the batch's length; it does depend on the row's index, the seed and the call
    c3, h3 = restated_rows(g, bs[:5], bd[:5], bt[:5], 20, 10, seed=99, call=3)
    assert np.array_equal(c3, cand[:5]) and np.array_equal(h3, n_hist[:5])
    c4, _ = restated_rows(g, bs[1:], bd[1:], bt[1:], 20, 10, seed=99, call=3)
    assert not np.array_equal(c4, cand[1:])
    assert not np.array_equal(restated_rows(g, bs, bd, bt, 20, 10, seed=100, call=3)[0], cand)
    assert not np.array_equal(restated_rows(g, bs, bd, bt, 20, 10, seed=99, call=4)[0], cand)


# ------------------------------------------------------------------------------------------------------------ the C boundary

def test_new_symbols_declared_exported_and_bound_with_matching_arity(hip_lib):
    from tpnet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tpnet_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/tpnet_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert getattr(hip_lib, name) is not None


def _state(d, L=3, N=64):
    from tpnet_amd import _lib
    return _lib.State(p0=8, q=8, meta=8, N=N, d=d, L=L, err=8)


def test_argument_checks_without_a_gpu(hip_lib):
    import ctypes
    # ---- fan-out readout
    for d, want in ((64, 1), (120, 1), (260, 1), (16, 0), (30, 0), (110, 0)):
        st = _state(d)
        assert hip_lib.tpnet_pair_gram_fanout_supported(ctypes.byref(st)) == want, d
    assert hip_lib.tpnet_pair_gram_fanout_supported(None) == 0
    st = _state(64)
    call = lambda **kw: hip_lib.tpnet_pair_gram_fanout(*[kw.get(k, v) for k, v in (
        ("st", ctypes.byref(st)), ("src", 16), ("cand", 16), ("n_rows", 4), ("C", 5), ("now", 0.0), ("lam", 1e-6), ("flags", 0),
        ("out", 256), ("stream", None))])
    for bad in (dict(st=None), dict(src=None), dict(cand=None), dict(out=None), dict(C=0), dict(C=-3), dict(n_rows=-1), dict(out=260),
                dict(flags=8), dict(n_rows=1 << 40)):
        assert call(**bad) == -1, bad
    assert call(n_rows=0) == 0                                       # nothing to do, nothing launched
    assert call(n_rows=0, flags=8) == -1                             # packed rows are refused whatever the size
    st16 = _state(16)
    assert call(st=ctypes.byref(st16)) == -1                         # a geometry the walk does not serve is refused, not served slowly
    # ---- per-query candidates
    many = lambda **kw: hip_lib.tpnet_neg_sample_many(*[kw.get(k, v) for k, v in (
        ("neg", 8), ("E", 10), ("bs", 8), ("bd", 8), ("bt", 8), ("B", 4), ("Q", 6), ("Qh", 3), ("seed", 0), ("call", 0), ("cand", 8),
        ("n_hist", 8), ("stream", None))])
    for bad in (dict(neg=None), dict(E=0), dict(E=1 << 30), dict(bs=None), dict(bd=None), dict(bt=None), dict(cand=None), dict(n_hist=None),
                dict(B=-1), dict(B=1 << 31), dict(Q=0), dict(Q=1 << 16), dict(Qh=-1), dict(Qh=7)):
        assert many(**bad) == -1, bad
    assert many(B=0, bs=None, bd=None, bt=None, cand=None, n_hist=None) == 0
    # ---- ranking record
    assert hip_lib.tpnet_lp_ranking_scratch_bytes(1000, 101) >= 3 * 4 * 1000
    for B, C1 in ((-1, 5), (1 << 31, 5), (10, 0), (10, -2), (10, (1 << 20) + 1)):
        assert hip_lib.tpnet_lp_ranking_scratch_bytes(B, C1) == 0, (B, C1)
    rank = lambda **kw: hip_lib.tpnet_lp_ranking(*[kw.get(k, v) for k, v in (
        ("logits", 8), ("B", 4), ("C1", 5), ("cand", None), ("k1", 1), ("k2", 3), ("k3", 10), ("scratch", 8), ("bytes", 1 << 20),
        ("record", 64), ("stream", None))])
    for bad in (dict(logits=None), dict(B=-1), dict(C1=0), dict(k1=0), dict(k2=-1), dict(k3=0), dict(scratch=None), dict(scratch=12),
                dict(record=None), dict(record=68)):
        assert rank(**bad) == -1, bad
    assert rank(bytes=16) == -2                                      # scratch too small: refused before any launch


# ------------------------------------------------------------------------------------------------ the Python surface on a CPU module

def _cpu_module(L=3, d=64):
    from tpnet_amd import RandomProjectionModule
    return RandomProjectionModule(node_num=50, edge_num=1000, dim_factor=10, num_layer=L, time_decay_weight=1e-6, device="cpu",
                                  use_matrix=False, beginning_time=np.float64(0.0), not_scale=False, enforce_dim=d)


def test_python_surface_on_a_cpu_module():
    from tpnet_amd import LinkRankingMeter, TPNetHipError
    from tpnet_amd.callers import LinkPredictor_v1
    rp = _cpu_module()
    src, cand = np.array([1, 2, 3]), np.arange(12).reshape(3, 4)
    with pytest.raises(TPNetHipError):
        rp.pair_gram_one_to_many(src, cand)
    with pytest.raises(TPNetHipError):
        rp.get_pair_wise_feature_one_to_many(src, cand)
    with pytest.raises(TPNetHipError):
        rp.pair_gram_one_to_many(torch.from_numpy(src), torch.from_numpy(cand))
    with pytest.raises(TPNetHipError):
        LinkRankingMeter(4, "cpu")
    dec = LinkPredictor_v1(16, 16, 32, 1, rp, not_encode=False)
    with pytest.raises(ValueError, match="not_encode"):
        dec.forward_one_to_many(src, cand)
    with pytest.raises(ValueError):
        dec.forward_one_to_many(src, cand.reshape(-1), torch.zeros(12, 16), torch.zeros(12, 16))        # cand must be [B, C]
    # a decoder without a pairwise-feature module needs no GPU: forward_one_to_many is forward on the expanded pairs
    plain = LinkPredictor_v1(16, 16, 32, 1, None, not_encode=False)
    es, ed = torch.randn(12, 16), torch.randn(12, 16)
    got = plain.forward_one_to_many(src, cand, es, ed)
    assert got.shape == (3, 4)
    assert torch.equal(got.reshape(-1, 1), plain(np.repeat(src, 4), cand.reshape(-1), es, ed))
