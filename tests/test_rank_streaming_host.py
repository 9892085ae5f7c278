"""Filtered, streaming all-node ranking: the host rules (no GPU).

  filter_lists_host          tpnet_neg_filter_lists' rule in numpy, against Python sets on the filter fixture
  link_ranking_counts_host   tpnet_lp_ranking_counts' rule in numpy, against link_ranking_metrics_host on the full logit matrix with
                             a mask that drops the query's own destination and its filter ids

The filter fixture (shared with tests/test_rank_streaming.py): 184 edges of 4 sources and 32 destinations, eight edges per instant;
the sampler is built on all of them and the queries are the last 24, so a query's own edge and its instant's other positives are in
the table.  Its facts are asserted, so a changed fixture cannot make the tests vacuous."""
import numpy as np
import pytest

from test_link_ranking_host import FLAG_EMPTY, FLAG_NAN, assert_record

FLAG_OVERFLOW = 8
FIL_E, FIL_Q = 184, 24
RANGES = [(1, 64), (9, 41), (9, 30)]


def filter_fixture():
    """-> dict(src, dst, t: the stream of 184 edges; q: the slice of the 24 queries)."""
    rng = np.random.RandomState(2024)
    E = FIL_E
    src = rng.randint(1, 5, E).astype(np.int64)
    dst = rng.randint(9, 41, E).astype(np.int64)
    t = 100.0 * (1 + np.arange(E) // 8)
    src[E - 3], dst[E - 3] = src[E - 5], dst[E - 5]                      # a positive repeated inside one instant
    return dict(src=src, dst=dst, t=t, q=slice(E - FIL_Q, E))


def filter_sets(fx, mode, lo, hi):
    """The rule as Python sets: per query the sorted list of excluded destinations."""
    src, dst, t = fx["src"], fx["dst"], fx["t"]
    out = []
    for i in range(FIL_E - FIL_Q, FIL_E):
        seen = {int(dst[j]) for j in range(FIL_E) if src[j] == src[i] and (mode == "known" or t[j] == t[i])}
        out.append(sorted(d for d in seen if d != dst[i] and lo <= d < hi))
    return out


def test_the_fixture_is_what_the_tests_need():
    fx = filter_fixture()
    q = fx["q"]
    facts = {("same_time", (1, 64)): (20, 0, 2), ("same_time", (9, 30)): (16, 0, 2), ("known", (1, 64)): (24, 18, 27),
             ("known", (9, 30)): (24, 10, 18)}
    for (mode, (lo, hi)), (nonempty, shortest, longest) in facts.items():
        lens = [len(r) for r in filter_sets(fx, mode, lo, hi)]
        assert (sum(n > 0 for n in lens), min(lens), max(lens)) == (nonempty, shortest, longest), (mode, lo, hi, lens)
    d = fx["dst"][q]
    assert int(((d < 9) | (d >= 30)).sum()) == 10                       # destinations outside (9, 30)
    trip = list(zip(fx["src"][q], d, fx["t"][q]))
    assert sum(trip.count(x) > 1 for x in trip) == 2                     # a positive repeated inside one instant: two queries


@pytest.mark.parametrize("mode", ["same_time", "known"])
@pytest.mark.parametrize("rng", RANGES)
def test_filter_lists_host_against_sets(mode, rng):
    from tpnet_amd.negative_sampler import filter_lists_host
    fx = filter_fixture()
    q = fx["q"]
    want = filter_sets(fx, mode, *rng)
    F = max(1, max(len(r) for r in want))
    fil, n_fil = filter_lists_host(fx["src"], fx["dst"], fx["t"], fx["src"][q], fx["dst"][q], fx["t"][q], mode, rng, F)
    assert fil.shape == (FIL_Q, F) and fil.dtype == np.int64 and n_fil.dtype == np.int32
    for i, r in enumerate(want):
        assert n_fil[i] == len(r) and list(fil[i, :len(r)]) == r and (fil[i, len(r):] == -1).all(), (i, r, fil[i])


@pytest.mark.parametrize("F", [1, 10])
def test_filter_lists_host_overflow_keeps_the_true_count_and_the_smallest(F):
    from tpnet_amd.negative_sampler import filter_lists_host
    fx = filter_fixture()
    q = fx["q"]
    want = filter_sets(fx, "known", 1, 64)
    fil, n_fil = filter_lists_host(fx["src"], fx["dst"], fx["t"], fx["src"][q], fx["dst"][q], fx["t"][q], "known", (1, 64), F)
    assert fil.shape == (FIL_Q, F) and (n_fil > F).all()
    for i, r in enumerate(want):
        assert n_fil[i] == len(r) and list(fil[i]) == r[:F]
    with pytest.raises(ValueError):
        filter_lists_host(fx["src"], fx["dst"], fx["t"], fx["src"][q], fx["dst"][q], fx["t"][q], "seen", (1, 64), F)


# ------------------------------------------------------------------------------------------------------------------ the record

def counts_of(x, lo, pos):
    """The integer rule on logits [B, 1 + C] whose column 1 + c is id lo + c: (g, e, nv, flags) per row, column pos - lo skipped."""
    x = np.asarray(x, dtype=np.float32)
    B, C = x.shape[0], x.shape[1] - 1
    on = (lo + np.arange(C))[None, :] != np.asarray(pos)[:, None]
    p, q = x[:, :1], x[:, 1:]
    with np.errstate(invalid="ignore"):
        g, e = ((q > p) & on).sum(axis=1), ((q == p) & on).sum(axis=1)
    nan = np.isnan(p[:, 0]) | (np.isnan(q) & on).any(axis=1)
    return np.stack([g, e, on.sum(axis=1), 2 * nan], axis=1).astype(np.int32)


def counts_case(B=50, C=40, F=6, seed=5):
    """Logits on a grid of quarters (ties are common) over the ids lo .. lo + C - 1, a positive per row (some outside the range), a
    filter list per row; row 3 has a NaN candidate, row 4 a NaN under a filtered id (a NaN filter logit), row 7 overflows (the row
    whose every candidate is filtered is all_filtered_case's).  -> dict(x, lo, pos, fil, n_fil, F, mask [B, C])."""
    rng = np.random.RandomState(seed)
    lo = 5
    x = np.round(rng.randn(B, 1 + C) * 4).astype(np.float32) / 4
    pos = rng.randint(lo - 3, lo + C + 3, B).astype(np.int64)
    fil = np.full((B, F), -1, dtype=np.int64)
    n_fil = np.zeros(B, dtype=np.int32)
    mask = (lo + np.arange(C))[None, :] != pos[:, None]
    for i in range(B):
        ids = np.setdiff1d(np.arange(lo, lo + C), [pos[i]])
        n = rng.randint(1 if i == 4 else 0, F + 1)
        pick = np.sort(rng.choice(ids, n, replace=False))
        fil[i, :n], n_fil[i] = pick, n
        mask[i, pick - lo] = False
    x[3, 1 + int(np.flatnonzero(mask[3])[0])] = np.nan
    x[4, 1 + int(fil[4, 0] - lo)] = np.nan
    n_fil[7] = F + 2                                                     # two more than the row holds: its mask is unknown
    return dict(x=x, lo=lo, pos=pos, fil=fil, n_fil=n_fil, F=F, mask=mask)


def all_filtered_case():
    """One query whose every candidate is on its filter list (C = F = 4), beside an ordinary one."""
    x = np.array([[1.0, 3.0, 0.0, 1.0, 2.0], [1.0, 3.0, 0.0, 1.0, 2.0]], dtype=np.float32)
    return dict(x=x, lo=10, pos=np.array([50, 50]), fil=np.array([[10, 11, 12, 13], [11, -1, -1, -1]]), n_fil=np.array([4, 1], dtype=np.int32),
                F=4, mask=np.array([[False] * 4, [True, False, True, True]]))


def fil_logits_of(case):
    """The filter ids' logits, read from the matrix (0 under a -1)."""
    x, fil, lo = case["x"], case["fil"], case["lo"]
    col = np.where(fil >= 0, fil - lo + 1, 0)
    return np.where(fil >= 0, np.take_along_axis(x, col, axis=1), np.float32(0)).astype(np.float32)


def want_of(case, ks=(1, 3, 10)):
    """link_ranking_metrics_host on the full matrix with the mask; rows it cannot express (NaN filter logit, overflow) are taken out
    of the counted queries by hand: their m leaves m_sum and n."""
    from tpnet_amd.metrics import link_ranking_metrics_host
    x, mask, n_fil, F = case["x"], case["mask"], case["n_fil"], case["F"]
    over = n_fil > F
    nan_f = np.array([np.isnan(fl[:min(n, F)][ids[:min(n, F)] >= 0]).any()
                      for fl, ids, n in zip(fil_logits_of(case), case["fil"], n_fil)])
    keep = ~(over | nan_f)
    xx = x.copy()
    xx[~keep, 0] = np.nan                                                # not counted, whatever else the row holds
    want = link_ranking_metrics_host(xx, mask, hits_at=ks)
    want["flags"] = (want["flags"] & ~FLAG_NAN) | (FLAG_OVERFLOW if over.any() else 0)
    with np.errstate(invalid="ignore"):
        real_nan = nan_f | np.isnan(x[:, 0]) | (np.isnan(x[:, 1:]) & mask).any(axis=1)
    want["flags"] |= FLAG_NAN if real_nan.any() else 0
    want["n_valid_candidates"] = int(np.maximum(counts_of(x, case["lo"], case["pos"])[:, 2] - np.maximum(n_fil, 0), 0).sum())
    return want


@pytest.mark.parametrize("name", ["B50_C40", "all_filtered"])
def test_counts_rule_against_the_mask_rule(name):
    from tpnet_amd.metrics import link_ranking_counts_host, link_ranking_metrics_host
    case = counts_case() if name == "B50_C40" else all_filtered_case()
    counts = counts_of(case["x"], case["lo"], case["pos"])
    got = link_ranking_counts_host(counts, case["x"][:, 0], fil_logits_of(case), case["fil"], case["n_fil"])
    want = want_of(case)
    assert_record(got, want, name)
    if name == "B50_C40":
        assert got["flags"] == FLAG_NAN | FLAG_OVERFLOW and 0 < got["n"] == 50 - 3       # rows 3, 4 and 7 are not counted
    else:
        assert got["flags"] == FLAG_EMPTY and got["n"] == 1 and got["m_sum"] == 2 + 2 * 2 + 1      # 3.0 and 2.0 above, 1.0 ties
    # no filter: the skip rule alone
    plain = link_ranking_counts_host(counts, case["x"][:, 0])
    own = (case["lo"] + np.arange(case["x"].shape[1] - 1))[None, :] != case["pos"][:, None]
    assert_record(plain, link_ranking_metrics_host(case["x"], own), name + " unfiltered")
