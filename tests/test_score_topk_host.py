"""Streaming top-k over all nodes, without a GPU: the rule (`score_fanout.topk_host`) against a brute-force sort on crafted rows and
against torch.topk, the slice route's torch keys against the rule, the checks of `topk_one_to_all` / `recommend_links` that come
before any computation, the scratch arithmetic of tpnet_score_topk_scratch_bytes and the argument checks of tpnet_score_topk_range.  Shared with tests/test_score_topk.py:
`brute_topk`, `same_floats`, `crafted_rows`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_score_fanout_host import _mlp, _state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_NAN, FLAG_OVERFLOW = 2, 8
NEW_SYMBOLS = ("tpnet_score_topk_scratch_bytes", "tpnet_score_topk_range")


def same_floats(a, b):
    """Equality of floats with NaN matched to NaN (and -0.0 == +0.0, as == has it)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _order_key(q, c):
    """The rule as a Python tuple, larger = better: (NaN first, then the float, with -0.0 == +0.0), then the SMALLER id."""
    q = float(q)
    return (1, 0.0, -c) if q != q else (0, q, -c)


def brute_topk(x, k, lo, skip=None, excl=None, n_excl=None):
    """The rule by a Python sort per row -> (ids, logits, info), as topk_host returns them."""
    x = np.asarray(x, dtype=np.float32)
    B, C = x.shape
    ids = np.full((B, k), -1, dtype=np.int64)
    out = np.full((B, k), -np.inf, dtype=np.float32)
    info = np.zeros((B, 2), dtype=np.int32)
    for i in range(B):
        drop = set()
        if skip is not None:
            drop.add(int(skip[i]))
        if excl is not None:
            F = excl.shape[1]
            n = int(n_excl[i]) if n_excl is not None else int((excl[i] >= 0).sum())
            drop |= {int(e) for e in excl[i, :min(n, F)] if e >= 0}
            if n > F:
                info[i, 1] |= FLAG_OVERFLOW
        adm = [c for c in range(C) if lo + c not in drop]
        adm.sort(key=lambda c: _order_key(x[i, c], c), reverse=True)
        if any(np.isnan(x[i, c]) for c in adm):
            info[i, 1] |= FLAG_NAN
        info[i, 0] = min(k, len(adm))
        for j, c in enumerate(adm[:k]):
            ids[i, j] = lo + c
            out[i, j] = x[i, c] + np.float32(0.0)
    return ids, out, info


def crafted_rows():
    """Rows of 12 candidates (ids 5 .. 16) that meet every clause of the rule."""
    inf, nan = np.inf, np.nan
    x = np.array([
        [1.0, 2.0, 2.0, -1.0, 2.0, 0.5, 0.5, -1.0, 3.0, 3.0, 0.25, -7.0],                 # ties at several levels
        [0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 1e-45, -1e-45, 0.0, -2.0, -0.0, 0.5],            # -0.0 against +0.0, denormals either side
        [-inf, inf, 0.0, nan, -inf, inf, 3.0, nan, -3.0, 1e38, -1e38, 0.0],                # the infinities and NaN
        [nan] * 12,                                                                        # every key ties at NaN
        [-inf] * 12,
        [4.0, 3.5, 3.0, 2.5, 2.0, 1.5, 1.0, 0.5, 0.0, -0.5, -1.0, -1.5],                   # no ties, no NaN
    ], dtype=np.float32)
    return x, 5


def _assert_same(got, want, what):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int32, what
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert same_floats(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(got[2], want[2]), (what, got[2], want[2])


@pytest.mark.parametrize("k", [1, 3, 11, 12, 13, 20])
def test_rule_against_a_brute_force_sort(k):
    from tpnet_amd.score_fanout import topk_host
    x, lo = crafted_rows()
    B, C = x.shape
    _assert_same(topk_host(x, k, lo), brute_topk(x, k, lo), "plain")
    # skip: inside the range (the best id of row 0, a NaN of row 2), at its two ends, outside either side
    skip = np.array([13, 5, 8, 16, 4, 17], dtype=np.int64)
    _assert_same(topk_host(x, k, lo, skip_ids=skip), brute_topk(x, k, lo, skip=skip), "skip")
    # lists: empty, short, one that leaves k or fewer candidates, every candidate, overflow (n > F: the rest is NOT left out)
    F = 12
    excl = np.full((B, F), -1, dtype=np.int64)
    n_ex = np.zeros(B, dtype=np.int32)
    for i, ids in enumerate([[], [6, 7, 9], [6, 8, 12], list(range(5, 17)), [5, 6, 7, 8, 9, 10, 11, 12, 13], [5, 16]]):
        excl[i, :len(ids)], n_ex[i] = ids, len(ids)
    _assert_same(topk_host(x, k, lo, exclude_ids=excl, n_exclude=n_ex), brute_topk(x, k, lo, excl=excl, n_excl=n_ex), "lists")
    _assert_same(topk_host(x, k, lo, exclude_ids=excl), brute_topk(x, k, lo, excl=excl, n_excl=n_ex), "lists, counted")
    got = topk_host(x, k, lo, skip_ids=skip, exclude_ids=excl, n_exclude=n_ex)
    _assert_same(got, brute_topk(x, k, lo, skip=skip, excl=excl, n_excl=n_ex), "skip and lists")
    assert got[2][3, 0] == 0 and (got[0][3] == -1).all() and np.isneginf(got[1][3]).all()          # nothing left: all empty
    assert got[2][4, 0] == min(k, 3) and (got[2][:, 1] & FLAG_OVERFLOW == 0).all()
    short, n_true = excl[:, :2].copy(), n_ex.copy()                                               # capacity 2: rows 1 .. 4 overflow
    got = topk_host(x, k, lo, exclude_ids=short, n_exclude=n_true)
    _assert_same(got, brute_topk(x, k, lo, excl=short, n_excl=n_true), "overflow")
    assert list(got[2][:, 1] & FLAG_OVERFLOW) == [0, 8, 8, 8, 8, 0]


def test_rule_facts_on_the_crafted_rows():
    from tpnet_amd.score_fanout import topk_host
    x, lo = crafted_rows()
    ids, out, info = topk_host(x, 5, lo)
    assert list(ids[0]) == [13, 14, 6, 7, 9] and list(out[0]) == [3.0, 3.0, 2.0, 2.0, 2.0]        # id ascending inside a tie
    assert list(ids[1][:2]) == [7, 16] and list(ids[1][2:5]) == [11, 5, 6]                       # 1.0, 0.5, 1e-45, then the zeros by id
    assert not np.signbit(out[1][3:5]).any()                                                     # -0.0 comes back as +0.0
    assert list(ids[2]) == [8, 12, 6, 10, 14] and np.isnan(out[2][:2]).all() and np.isposinf(out[2][2:4]).all()
    assert list(ids[3]) == [5, 6, 7, 8, 9] and np.isnan(out[3]).all()                            # all NaN: the smallest ids
    assert list(info[:, 1]) == [0, 0, FLAG_NAN, FLAG_NAN, 0, 0] and (info[:, 0] == 5).all()
    with pytest.raises(ValueError):
        topk_host(x, 0, lo)


def test_values_agree_with_torch_topk_where_nothing_ties():
    from tpnet_amd.score_fanout import topk_host
    rng = np.random.RandomState(3)
    x = rng.permutation(np.arange(-300, 300, dtype=np.float32) / 7).reshape(6, 100)               # distinct floats
    for k in (1, 7, 100):
        ids, out, info = topk_host(x, k, 9)
        top = torch.topk(torch.from_numpy(x), k, dim=1)
        assert np.array_equal(ids, top.indices.numpy() + 9) and np.array_equal(out, top.values.numpy())
        assert (info[:, 0] == k).all() and (info[:, 1] == 0).all()


def test_torch_keys_are_the_rule():
    """The signed keys of the slice route: the same order and the same decoded words as the host rule, on every special value."""
    from tpnet_amd import score_fanout as sf
    x, lo = crafted_rows()
    col = np.arange(x.shape[1], dtype=np.int64)
    kh = sf._keys_host(x, col[None, :])
    kt = sf.topk_keys_torch(torch.from_numpy(x), torch.from_numpy(col).unsqueeze(0)).numpy()
    assert np.array_equal((kt.astype(np.int64).view(np.uint64) + np.uint64(1 << 63)), kh)         # key - 2^63, wrapped
    srt = torch.sort(torch.from_numpy(kt), dim=1, descending=True).values
    ids, out = sf.topk_decode_torch(srt, lo)
    want = brute_topk(x, x.shape[1], lo)
    assert np.array_equal(ids.numpy(), want[0]) and same_floats(out.numpy(), want[1])
    e_ids, e_out = sf.topk_decode_torch(torch.full((1, 2), sf._EMPTY_KEY, dtype=torch.int64), lo)
    assert (e_ids == -1).all() and torch.isneginf(e_out).all()


# ------------------------------------------------------------------------------------------------------------------ the surface
# (a CPU module computes nothing -- RandomProjectionModule has no CPU fallback -- so the slice route of topk_one_to_all is held to
# the rule in tests/test_score_topk.py, on an L = 2 module; here: the checks that come before any computation)

def test_surface_checks_on_a_cpu_module():
    from tpnet_amd import RandomProjectionModule
    from tpnet_amd.callers import LinkPredictor_v1, recommend_links
    rp = RandomProjectionModule(node_num=40, edge_num=200, dim_factor=10, num_layer=3, time_decay_weight=1e-6, device="cpu",
                                use_matrix=False, beginning_time=np.float64(0.0), not_scale=False, enforce_dim=64)
    dec = LinkPredictor_v1(4, 4, 8, 1, rp, not_encode=True)
    src = np.array([3, 7, 12], dtype=np.int64)
    te, tn = torch.full((3, 4), -1, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    for bad in (dict(k=0), dict(first_id=5, end_id=5), dict(skip_node_ids=src[:2]), dict(exclude_ids=te), dict(n_exclude=tn)):
        kw = dict(k=3, first_id=1, end_id=40)
        kw.update(bad)
        with pytest.raises(ValueError):
            dec.topk_one_to_all(src, **kw)
    for bad in (dict(exclude_ids=te.int(), n_exclude=tn), dict(exclude_ids=te, n_exclude=tn.long()), dict(exclude_ids=te[:2], n_exclude=tn),
                dict(exclude_ids=te, n_exclude=tn[:2]), dict(exclude_ids=te.numpy(), n_exclude=tn)):
        with pytest.raises(TypeError):
            dec.topk_one_to_all(src, 3, 1, 40, **bad)
    with pytest.raises(ValueError):
        LinkPredictor_v1(4, 4, 8, 1, rp, not_encode=False).topk_one_to_all(src, 3, 1, 40)
    with pytest.raises(ValueError):
        recommend_links(dec, src, 4, (1, 40), exclude="known")                                    # no sampler
    with pytest.raises(ValueError):
        recommend_links(dec, src, 4, (1, 40), exclude="same_time", negative_sampler=object())
    for kw in (dict(), dict(streaming=True), dict(exclude_self=True)):
        with pytest.raises(ValueError):
            recommend_links(dec, src, 40, (1, 40), **kw)                                          # k beyond the candidates
        with pytest.raises(ValueError):
            recommend_links(dec, src, 0, (1, 40), **kw)


# ------------------------------------------------------------------------------------------------------------------- the C ABI

def test_new_symbols_declared_exported_and_bound_with_matching_arity(hip_lib):
    from tpnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "tpnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/tpnet_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert getattr(hip_lib, name) is not None
    assert "tpnet_score_topk_range" in header[:header.index("#define TPNET_MAX_LAYERS")]           # the list of additions to ABI 7


def _chunk(n_rows, C):
    """anchored_chunk's cut: at least about 8192 units in the launch, at least 4 ids each, KC = C on long lists of rows."""
    return int(min(C, max(4, (C * n_rows + 8191) // 8192)))


def test_scratch_bytes_arithmetic(hip_lib):
    f = hip_lib.tpnet_score_topk_scratch_bytes
    for n_rows, C, K in [(1, 64, 5), (1, 64, 1), (17, 33, 128), (9000, 64, 5), (2100, 64, 5), (2100, 64, 20), (200, 9227, 10),
                         (200, 9227, 100), (1, (1 << 20) + 7, 128), (1, 3, 128), (1, 4, 2), (0, 10, 3), (5, (1 << 31) - 1, 128)]:
        kc = _chunk(n_rows, C)
        nch = -(-C // kc)
        want = 16 + (n_rows * nch * min(K, kc) * 8 if nch > 1 else 0)
        assert f(n_rows, C, K) == want, (n_rows, C, K, kc, nch)
        assert n_rows * nch <= 8192 + n_rows and want <= 16 + (8192 + n_rows) * K * 8                # whatever the range
    assert f(9000, 64, 5) == 16 and f(2100, 64, 20) == 16 + 2100 * 4 * 17 * 8
    for bad in [(-1, 10, 3), (1 << 31, 10, 3), (4, 0, 3), (4, -2, 3), (4, 10, 0), (4, 10, 129), (4, 10, -1)]:
        assert f(*bad) == 0, bad


def test_bad_arguments_are_rejected_without_a_gpu(hip_lib):
    st, mlp = _state(128, N=64), _mlp()
    call = lambda **kw: hip_lib.tpnet_score_topk_range(*[kw.get(k, v) for k, v in (
        ("st", ctypes.byref(st)), ("src", 16), ("skip", None), ("excl", None), ("n_excl", None), ("F", 0), ("cand_lo", 0), ("n_rows", 4),
        ("C", 5), ("K", 3), ("now", 0.0), ("lam", 1e-6), ("flags", 0), ("mlp", ctypes.byref(mlp)), ("wd", 256), ("ldw", 408),
        ("off", 344), ("bd", 16), ("wd2", 16), ("bd2", 16), ("H", 172), ("scratch", 256), ("bytes", 1 << 20), ("ids", 256),
        ("logits", 256), ("info", 256), ("stream", None))])
    wide, two = _state(516), _state(128, L=2)
    for bad in (dict(st=None), dict(src=None), dict(ids=None), dict(logits=None), dict(info=None), dict(scratch=None), dict(mlp=None),
                dict(wd=None), dict(bd=None), dict(wd2=None), dict(bd2=None), dict(C=0), dict(C=-3), dict(n_rows=-1),
                dict(n_rows=1 << 31), dict(K=0), dict(K=-1), dict(K=129), dict(flags=8), dict(scratch=264), dict(ids=260),
                dict(logits=258), dict(info=258), dict(skip=260), dict(wd=260), dict(bd=18), dict(H=0), dict(H=257), dict(off=342),
                dict(ldw=406), dict(st=ctypes.byref(wide)), dict(st=ctypes.byref(two)), dict(cand_lo=-1), dict(cand_lo=60),
                dict(excl=256), dict(excl=256, n_excl=16, F=0), dict(excl=256, n_excl=16, F=-2), dict(excl=260, n_excl=16, F=4),
                dict(excl=256, n_excl=18, F=4)):
        assert call(**bad) == -1, bad                                    # (nothing is launched: there is no GPU here)
        if "n_rows" not in bad:
            assert call(n_rows=0, **bad) == -1, bad                      # ... and an empty call does not excuse them
    assert call(n_rows=0) == 0 and call(n_rows=0, K=128, C=2) == 0 and call(n_rows=0, skip=16, excl=256, n_excl=16, F=4) == 0
    assert call(bytes=8) == -2                                           # a short scratch (checked before anything is launched)
    assert call(C=64, n_rows=1, K=4, bytes=16 + 16 * 4 * 8 - 1) == -2
