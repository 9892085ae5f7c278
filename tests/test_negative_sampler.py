"""The device negative edge sampler (tpnet_amd/negative_sampler.py `GpuNegativeEdgeSampler`, csrc/negsampler.hip) against a numpy
restatement of its rule and against fixture G13 (tests/golden/make_golden_negatives.py: the reference's own NegativeEdgeSampler
with 'historical' and 'inductive' on a toy graph).

The rule (include/tpnet_hip.h): an edge of the sampler's data is a candidate iff first_time <= t0 and it has no occurrence in
[t0, t1] ('inductive': and first_time > last_observed_time); C = the candidates in ascending key order (src << 32 | dst), M = |C|.
size <= M: out[i] = C[perm(M, tag 0, i)].  Else F = size - M pairs of (unique src) x (unique dst) that are not pairs of the batch come
first -- trial slots j < min(D, F + B) hold perm(D, tag 1, j); the first F valid ones, or, when only P < F exist, F draws
valid[(word(2, i, 0) P) >> 32] -- and all of C follows.  word(tag, a, b) = word 0 of Philox4x32-10, counter (a, b, tag, call), key =
the seed; perm = a six-round alternating Feistel network on the bitlength(n - 1) bits of a slot, walked back into [0, n).  Everything is compared bit for bit."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_sampler_strategies import philox4x32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 6


# ------------------------------------------------------------------------------------------------ the numpy restatement

def word(seed, call, tag, a, b):
    """word(tag, a, b) for arrays a (and scalar or array b): uint64 values < 2^32."""
    a = np.asarray(a, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    b = np.broadcast_to(np.asarray(b, dtype=np.uint64), a.shape)
    ctr = np.stack([a, b, np.full_like(a, tag), np.full_like(a, call)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return philox4x32(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,)))[..., 0].astype(np.uint64)


def perm(n, tag, idx, seed, call):
    """Slots idx of the keyed permutation of [0, n)."""
    x = np.array(idx, dtype=np.uint64)
    if n <= 1:
        return np.zeros_like(x)
    bits = int(n - 1).bit_length()
    a, b = bits // 2, bits - bits // 2
    mask_l, mask_r, sh = np.uint64((1 << a) - 1), np.uint64((1 << b) - 1), np.uint64(b)
    todo = np.ones(len(x), dtype=bool)
    while todo.any():
        L, R = x[todo] >> sh, x[todo] & mask_r
        for r in range(0, ROUNDS, 2):
            L = L ^ (word(seed, call, tag, R, r) & mask_l)
            R = R ^ (word(seed, call, tag, L, r + 1) & mask_r)
        y = (L << sh) | R
        x[todo] = y
        todo[todo] = y >= np.uint64(n)
    return x


class Table:
    """The unique edges in ascending key order with their ascending occurrence times, and the sorted unique ids."""

    def __init__(self, src, dst, t, last_observed_time=None):
        src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        t = np.zeros(len(src)) if t is None else np.asarray(t, dtype=np.float64)
        keys = (src << 32) | dst
        order = np.lexsort((t, keys))
        self.times = t[order]
        self.ukeys, self.start = np.unique(keys[order], return_index=True)
        self.first = self.times[self.start]
        self.observed = self.first <= last_observed_time if last_observed_time is not None else np.zeros(len(self.ukeys), dtype=bool)
        self.us, self.ud = np.unique(src), np.unique(dst)

    def candidates(self, strategy, t0, t1):
        inside = np.add.reduceat(((self.times >= t0) & (self.times <= t1)).astype(np.int64), self.start)
        ok = (self.first <= t0) & (inside == 0)
        if strategy == "inductive":
            ok &= ~self.observed
        return self.ukeys[ok]

    def sample(self, strategy, size, bs, bd, t0, t1, seed, call):
        """-> (src, dst, info); info: M, F, P (valid pairs seen), D, trials, replaced."""
        if strategy == "random":
            i = np.arange(size)
            si = (word(seed, call, 3, i, 0) * np.uint64(len(self.us))) >> np.uint64(32)
            di = (word(seed, call, 4, i, 0) * np.uint64(len(self.ud))) >> np.uint64(32)
            return self.us[si.astype(np.int64)], self.ud[di.astype(np.int64)], {}
        cand = self.candidates(strategy, t0, t1)
        M = len(cand)
        if size <= M:
            keys = cand[perm(M, 0, np.arange(size), seed, call).astype(np.int64)]
            return keys >> 32, keys & 0xFFFFFFFF, dict(M=M, F=0)
        F, nd = size - M, len(self.ud)
        D = len(self.us) * nd
        trials = min(D, F + len(bs))
        x = perm(D, 1, np.arange(trials), seed, call).astype(np.int64)
        tk = (self.us[x // nd] << 32) | self.ud[x % nd]
        bs, bd = np.asarray(bs, dtype=np.int64), np.asarray(bd, dtype=np.int64)
        inr = (bs >= 0) & (bs < 2 ** 31) & (bd >= 0) & (bd < 2 ** 31)
        valid = tk[~np.isin(tk, (bs[inr] << 32) | bd[inr])]
        P = len(valid)
        info = dict(M=M, F=F, P=P, D=D, trials=trials, replaced=P < F)
        if P >= F:
            head = valid[:F]
        elif P == 0:
            return (np.concatenate([np.full(F, -1, dtype=np.int64), cand >> 32]),
                    np.concatenate([np.full(F, -1, dtype=np.int64), cand & 0xFFFFFFFF]), info)
        else:
            head = valid[((word(seed, call, 2, np.arange(F), 0) * np.uint64(P)) >> np.uint64(32)).astype(np.int64)]
        keys = np.concatenate([head, cand])
        return keys >> 32, keys & 0xFFFFFFFF, info


def bound(p, T):
    """|frequency - p| allowed over T draws: the convention of test_sampler_strategies.test_distribution_against_the_reference."""
    return 5.0 * np.sqrt(p * (1 - p) / T) + 1.0 / T


_cache = {}


def g13(golden_dir):
    if "g13" not in _cache:
        _cache["g13"] = dict(np.load(os.path.join(golden_dir, "g13_negatives.npz")))
    return _cache["g13"]


def graph_with(U, seed=7):
    """E = U + max(3, U / 2) edges over exactly U distinct pairs (every pair at least once, the rest repeats), integer stamps with
    about eight edges each: (src, dst, t)."""
    if ("u", U) not in _cache:
        rng = np.random.RandomState(seed + U)
        ns = max(1, int(np.ceil(np.sqrt(U))))
        nd = (U + ns - 1) // ns
        pairs = rng.permutation(ns * nd)[:U]
        pick = rng.permutation(np.concatenate([pairs, pairs[rng.randint(0, U, max(3, U // 2))]]))
        t = np.sort(rng.randint(0, max(4, len(pick) // 8), len(pick))).astype(np.float64)
        _cache[("u", U)] = ((pick // nd + 1).astype(np.int64), (pick % nd + ns + 1).astype(np.int64), t)
    return _cache[("u", U)]


def grid_graph():
    """30 sources x 40 destinations, 3 000 edges, integer stamps: a domain of 1 200 pairs that batches of ~1 000 edges cover a lot of."""
    if "grid" not in _cache:
        rng = np.random.RandomState(23)
        _cache["grid"] = (rng.randint(1, 31, 3000).astype(np.int64), rng.randint(31, 71, 3000).astype(np.int64),
                          np.sort(rng.randint(0, 300, 3000)).astype(np.float64))
    return _cache["grid"]


# ---------------------------------------------------------------------------------------------------------------- CPU tier

def test_restated_candidates_equal_the_reference(golden_dir):
    g = g13(golden_dir)
    tabs = {}
    kinds = set()
    for c in range(len(g["call_size"])):
        lot = None if np.isnan(g["call_lot"][c]) else float(g["call_lot"][c])
        tab = tabs.setdefault(lot, Table(g["src"], g["dst"], g["t"], lot))
        strategy = "historical" if g["call_strategy"][c] == 1 else "inductive"
        want = g["cand_keys"][g["cand_off"][c]:g["cand_off"][c + 1]]
        got = tab.candidates(strategy, g["call_t0"][c], g["call_t1"][c])
        assert np.array_equal(got, want), f"call {c}"
        kinds.add("empty" if len(want) == 0 else "fill" if len(want) < g["call_size"][c] else "draw")
        # |possible - batch| as the restated fill counts it: the whole domain minus the batch's distinct pairs
        b = slice(g["call_b0"][c], g["call_b1"][c])
        assert len(tab.us) * len(tab.ud) - len(set(zip(g["src"][b], g["dst"][b]))) == g["call_possible"][c]
    assert kinds == {"empty", "fill", "draw"} and g["call_replace"].sum() >= 1
    # the toy graph has what the boundaries need: an edge stamped exactly t0 / t1 of a batch, one that is history and recurs inside
    t, keys = g["t"], (g["src"] << 32) | g["dst"]
    starts = range(25, 300, 25)
    assert any(t[b - 1] == t[b] for b in starts) and any(t[b + 24] == t[b + 25] for b in starts if b + 25 < 300)
    assert any(np.intersect1d(keys[t < t[b]], keys[(t >= t[b]) & (t <= t[b + 24])]).size for b in starts)


def test_the_reference_meets_the_distribution_bound(golden_dir):
    g = g13(golden_dir)
    T = int(g["T"])
    p = g["dist_call"][2] / len(g["dist_keys"])
    assert np.all(np.abs(g["dist_counts"] / T - p) <= bound(p, T))
    p = g["fill_call"][3] / len(g["fill_keys"])
    assert np.all(np.abs(g["fill_counts"] / T - p) <= bound(p, T))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 65537])
def test_restated_permutation_is_a_bijection(n):
    for call, tag in ((0, 0), (7, 1)):
        assert np.array_equal(np.sort(perm(n, tag, np.arange(n), 99, call)), np.arange(n, dtype=np.uint64))


def _inclusion(golden_dir, sample):
    """Inclusion frequencies of the fixture's two cases over calls 0..T-1 of seed 5; sample(strategy, size, b0, b1, call) -> keys."""
    g = g13(golden_dir)
    T = int(g["T"])
    out = []
    for which, keys in (("dist", g["dist_keys"]), ("fill", g["fill_keys"])):
        b0, b1, size = (int(x) for x in g[which + "_call"][:3])
        head = size if which == "dist" else int(g["fill_call"][3])
        cnt = np.zeros(len(keys), dtype=np.int64)
        for k in sample(b0, b1, size, T):
            assert len(np.unique(k[:head])) == head
            cnt[np.searchsorted(keys, k[:head])] += 1
        out.append((cnt / T, head / len(keys), T))
    return out


def test_restated_rule_meets_the_distribution_bound(golden_dir):
    g = g13(golden_dir)
    tab = Table(g["src"], g["dst"], g["t"])

    def sample(b0, b1, size, T):
        for call in range(T):
            s, d, _ = tab.sample("historical", size, g["src"][b0:b1], g["dst"][b0:b1], g["t"][b0], g["t"][b1 - 1], 5, call)
            yield (s << 32) | d
    for f, p, T in _inclusion(golden_dir, sample):
        assert np.all(np.abs(f - p) <= bound(p, T)), np.abs(f - p).max() / bound(p, T)


def test_new_symbols_declared_and_bound_with_matching_arity():
    from tpnet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tpnet_hip.h")).read(), flags=re.S)
    for name in ("tpnet_neg_bytes", "tpnet_neg_build", "tpnet_neg_uniques", "tpnet_neg_scratch_bytes", "tpnet_neg_sample",
                 "tpnet_neg_check"):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/tpnet_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name


def test_size_and_argument_checks_without_a_gpu(hip_lib):
    import ctypes
    assert hip_lib.tpnet_neg_bytes(300) >= 300 * 45 and hip_lib.tpnet_neg_bytes(0) == 0 and hip_lib.tpnet_neg_bytes(-4) == 0
    assert hip_lib.tpnet_neg_bytes(1 << 30) == 0
    assert hip_lib.tpnet_neg_scratch_bytes(300, 25, 25) >= 300 * 5 + 25 * 8
    assert hip_lib.tpnet_neg_scratch_bytes(300, 25, 2000) >= 300 * 5 + 25 * 8 + 2 * 2000 * 8   # + the batch's keys, twice
    assert hip_lib.tpnet_neg_scratch_bytes(300, -1, 5) == 0 and hip_lib.tpnet_neg_scratch_bytes(0, 5, 5) == 0
    assert hip_lib.tpnet_neg_scratch_bytes(300, 5, -1) == 0
    counts = (ctypes.c_int64 * 3)()
    assert hip_lib.tpnet_neg_build(None, 1 << 20, 8, 8, 8, 10, 0.0, 0, counts, None) == -1
    assert hip_lib.tpnet_neg_build(8, 1 << 20, None, 8, 8, 10, 0.0, 0, counts, None) == -1
    assert hip_lib.tpnet_neg_build(8, 1 << 20, 8, 8, 8, 0, 0.0, 0, counts, None) == -1
    assert hip_lib.tpnet_neg_build(8, 1 << 20, 8, 8, 8, 10, 0.0, 0, None, None) == -1
    assert hip_lib.tpnet_neg_build(8, 16, 8, 8, 8, 10, 0.0, 0, counts, None) == -2          # buffer too small
    assert hip_lib.tpnet_neg_uniques(None, 10, 1, 1, 8, 8, None) == -1 and hip_lib.tpnet_neg_uniques(8, 10, 11, 1, 8, 8, None) == -1
    ok = lambda **kw: hip_lib.tpnet_neg_sample(*[kw.get(k, v) for k, v in (
        ("neg", 8), ("E", 10), ("strategy", 1), ("size", 4), ("bs", 8), ("bd", 8), ("B", 4), ("t0", 0.0), ("t1", 1.0), ("seed", 0),
        ("call", 0), ("scratch", 8), ("scratch_bytes", 0), ("out_src", 8), ("out_dst", 8), ("stream", None))])
    for bad in (dict(neg=None), dict(E=0), dict(strategy=3), dict(strategy=-1), dict(size=-1), dict(size=1 << 31), dict(B=-2),
                dict(out_src=None), dict(out_dst=None), dict(bs=None), dict(bd=None), dict(scratch=None)):
        assert ok(**bad) == -1, bad
    assert ok() == -2                                              # scratch too small: refused before any launch
    assert ok(size=0, out_src=None, out_dst=None) == 0             # size == 0: no-op
    assert hip_lib.tpnet_neg_check(None, None) == -1


def test_python_surface_without_a_gpu():
    from tpnet_amd import GpuNegativeEdgeSampler, TPNetHipError
    from tpnet_amd.callers import link_prediction_batch, run_evaluation
    src, dst, t = np.array([1, 2]), np.array([3, 4]), np.array([0.0, 1.0])
    with pytest.raises(ValueError, match="Not implemented error for negative_sample_strategy nearest!"):
        GpuNegativeEdgeSampler(src, dst, t, negative_sample_strategy="nearest", seed=0)
    with pytest.raises(TPNetHipError):
        GpuNegativeEdgeSampler(src, dst, t, negative_sample_strategy="historical", seed=0, device="cpu")
    sig = inspect.signature(GpuNegativeEdgeSampler.__init__)
    assert list(sig.parameters)[1:] == ["src_node_ids", "dst_node_ids", "interact_times", "last_observed_time",
                                        "negative_sample_strategy", "seed", "device"]
    assert sig.parameters["negative_sample_strategy"].default == "random" and sig.parameters["seed"].default is None
    assert list(inspect.signature(GpuNegativeEdgeSampler.sample).parameters)[1:] == [
        "size", "batch_src_node_ids", "batch_dst_node_ids", "current_batch_start_time", "current_batch_end_time"]
    # link_prediction_batch: the new keyword is last and defaults to None, the path of every existing caller
    p = inspect.signature(link_prediction_batch).parameters
    assert list(p)[-1] == "neg_src" and p["neg_src"].default is None and list(p)[:7] == ["rp", "neighbor_sampler", "src", "dst", "neg_dst",
                                                                                        "t", "num_neighbors"]
    assert list(inspect.signature(run_evaluation).parameters) == ["rp", "neighbor_sampler", "negative_sampler", "src", "dst", "t",
                                                                  "batch_size", "num_neighbors", "encoder", "decoder", "on_batch"]


# ---------------------------------------------------------------------------------------------------------------- GPU tier

def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")


def _dev(x, dt=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0", dt)


def _sampler(src, dst, t, strategy="historical", lot=None, seed=1234):
    from tpnet_amd import GpuNegativeEdgeSampler
    return GpuNegativeEdgeSampler(src, dst, t, last_observed_time=lot, negative_sample_strategy=strategy, seed=seed, device="cuda:0")


def _check_call(smp, tab, size, bs, bd, t0, t1, seed=1234):
    """One sample_device call against the restatement, bit for bit; -> the restatement's info.  A fill that found no valid pair must
    leave the error word set: check() raises once, then the word is clear."""
    from tpnet_amd import TPNetHipError
    call = smp._calls
    s, d = smp.sample_device(size, _dev(bs), _dev(bd), t0, t1)
    ws, wd, info = tab.sample(smp.negative_sample_strategy, size, bs, bd, t0, t1, seed, call)
    assert s.dtype == torch.int64 and d.dtype == torch.int64 and s.shape == (size,) and d.shape == (size,)
    what = f"size={size} t0={t0} t1={t1} B={len(bs)} call={call} {info}"
    assert np.array_equal(s.cpu().numpy(), ws), "src differs: " + what
    assert np.array_equal(d.cpu().numpy(), wd), "dst differs: " + what
    if info.get("F") and info["P"] == 0:
        with pytest.raises(TPNetHipError):
            smp.check()
    smp.check()
    return info


def _sizes(M):
    return sorted({0, 1, max(M - 1, 1), max(M, 1), M + 1, M + 37, max(M // 3, 1)})


@pytest.mark.gpu
@pytest.mark.parametrize("strategy,lot", [("historical", None), ("inductive", -5.0), ("inductive", 20.0), ("inductive", 33.0),
                                          ("inductive", 1000.0)])
def test_toy_graph_bit_for_bit(golden_dir, strategy, lot):
    """Every batch of the fixture's graph -- the first (t0 = earliest: M = 0), batches whose ends are tied stamps, one behind the
    last stamp -- with sizes around M (M - 1, M, M + 1, M / 3, M + 37, 1, 0); inductive with last_observed_time before, inside and
    after the history."""
    _need_gpu()
    g = g13(golden_dir)
    src, dst, t = g["src"], g["dst"], g["t"]
    tab, smp = Table(src, dst, t, lot), _sampler(src, dst, t, strategy, lot)
    assert smp.earliest_time == t.min() and smp.last_observed_time == lot and smp.num_unique_edges == len(tab.ukeys)
    assert np.array_equal(smp.unique_src_node_ids, tab.us) and np.array_equal(smp.unique_dst_node_ids, tab.ud)
    seen = set()
    windows = [(b0, min(b0 + 25, 300), t[b0], t[min(b0 + 25, 300) - 1]) for b0 in range(0, 300, 25)]
    windows += [(150, 175, t[150] + 0.5, t[150] + 0.25), (0, 25, 1.0e6, 2.0e6), (0, 0, t[200], t[210])]
    for b0, b1, t0, t1 in windows:
        M = len(tab.candidates(strategy, t0, t1))
        for size in _sizes(M):
            _check_call(smp, tab, size, src[b0:b1], dst[b0:b1], t0, t1)
            seen.add("M=0" if M == 0 else "fill" if size > M else "draw")
    assert seen == ({"M=0"} if lot == 1000.0 else {"M=0", "fill", "draw"})


@pytest.mark.gpu
@pytest.mark.parametrize("U", [1, 255, 256, 257, 769, 70001])
def test_every_level_of_the_scan_bit_for_bit(U):
    """Tables of 1, 255, 256, 257 (one tile, its edges), 769 (four tiles) and 70 001 unique edges (274 tile sums: the second level
    runs twice with a carry); windows at the earliest stamp, in the middle and behind the end; sizes around M."""
    _need_gpu()
    src, dst, t = graph_with(U)
    tab = Table(src, dst, t, float(np.median(t)))
    assert len(tab.ukeys) == U
    E = len(src)
    for strategy in ("historical", "inductive"):
        smp = _sampler(src, dst, t, strategy, float(np.median(t)) if strategy == "inductive" else None)
        assert smp.num_unique_edges == U
        assert np.array_equal(smp.unique_src_node_ids, tab.us) and np.array_equal(smp.unique_dst_node_ids, tab.ud)
        for b0 in (0, E // 2, E - min(E, 200)):
            b1 = min(b0 + 200, E)
            windows = [(t[b0], t[b1 - 1])] + ([(t[-1] + 1.0, t[-1] + 2.0)] if b0 else [])
            for t0, t1 in windows:
                M = len(tab.candidates(strategy, t0, t1))
                for size in ([1, 200, max(M - 1, 1), M + 1] if U > 1000 else _sizes(M)):
                    _check_call(smp, tab, size, src[b0:b1], dst[b0:b1], t0, t1)


@pytest.mark.gpu
def test_fill_branches_bit_for_bit():
    """A domain of 2 x 3 = 6 pairs: F + B beyond D (the whole domain enumerated) with P >= F (distinct) and P < F (replacement), and
    a batch that holds every pair (P = 0): -1 in the fill, the error word set, sample() raises, tpnet_neg_check clears the word."""
    _need_gpu()
    from tpnet_amd import TPNetHipError
    src = np.array([1, 1, 2, 2, 1, 2, 1], dtype=np.int64)
    dst = np.array([5, 6, 5, 7, 7, 6, 5], dtype=np.int64)
    t = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    tab, smp = Table(src, dst, t), _sampler(src, dst, t)
    full_s, full_d = np.repeat([1, 2], 3).astype(np.int64), np.tile([5, 6, 7], 2).astype(np.int64)
    kinds = set()
    for t0, t1, bs, bd, size in ((3.5, 3.6, src[4:6], dst[4:6], 8),        # M = 4: the edges stamped 0..3 ((1, 5) recurs only at 6)
                                 (3.5, 3.6, src[4:6], dst[4:6], 9), (3.5, 3.6, src[4:6], dst[4:6], 12),
                                 (0.0, 0.0, src[:1], dst[:1], 5), (0.0, 0.0, src[:1], dst[:1], 6), (0.0, 0.5, full_s[:5], full_d[:5], 4),
                                 (0.0, 0.0, full_s, full_d, 3), (3.5, 3.6, full_s, full_d, 6),
                                 (0.0, 0.0, np.array([1, -1, 2 ** 31]), np.array([2 ** 40, 5, 6]), 6)):
        info = _check_call(smp, tab, size, np.asarray(bs, dtype=np.int64), np.asarray(bd, dtype=np.int64), t0, t1)
        assert info["F"] > 0 and info["trials"] == info["D"] == 6
        kinds.add("P=0" if info["P"] == 0 else "replaced" if info["replaced"] else "distinct")
    assert kinds == {"P=0", "replaced", "distinct"}
    with pytest.raises(TPNetHipError):
        smp.sample(3, full_s, full_d, 0.0, 0.0)
    smp.check()                                                    # sample() has cleared the word
    s, d = smp.sample(3, src[:1], dst[:1], 0.0, 0.0)
    assert s.dtype == np.int64 and len(s) == 3 and (s > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [200, 1024, 1025, 2000])
def test_batch_lookup_on_either_side_of_its_threshold(B):
    """Batches of up to 1 024 pairs are looked up in the LDS table, larger ones in their sorted keys: a 30 x 40 domain of which the
    batch covers hundreds of pairs, an early window (few candidates), so that most trial slots meet the lookup and many are refused."""
    _need_gpu()
    src, dst, t = grid_graph()
    tab, smp = Table(src, dst, t), _sampler(src, dst, t)
    for b0, size in ((60, B), (60, 1150), (900, 1190)):
        info = _check_call(smp, tab, size, src[b0:b0 + B], dst[b0:b0 + B], t[b0], t[b0 + B - 1])
        assert info["F"] > 0 and info["trials"] - info["P"] >= 20, info      # (trial slots that met a pair of the batch)


@pytest.mark.gpu
def test_ids_next_to_the_largest_served():
    _need_gpu()
    top = 2 ** 31 - 1
    rng = np.random.RandomState(3)
    src = np.array([top, top - 1, 0, 5])[rng.randint(0, 4, 60)].astype(np.int64)
    dst = np.array([top, top - 2, 1, 0])[rng.randint(0, 4, 60)].astype(np.int64)
    t = np.sort(rng.randint(0, 20, 60)).astype(np.float64)
    tab, smp = Table(src, dst, t), _sampler(src, dst, t)
    assert np.array_equal(smp.unique_src_node_ids, tab.us) and np.array_equal(smp.unique_dst_node_ids, tab.ud)
    for size in (3, 12, 30):
        _check_call(smp, tab, size, src[40:50], dst[40:50], t[40], t[49])
    src[7] = 2 ** 31
    with pytest.raises(IndexError):
        _sampler(src, dst, t)
    src[7] = -1
    with pytest.raises(IndexError):
        _sampler(src, dst, t)


@pytest.mark.gpu
def test_contract_against_the_reference_on_every_recorded_call(golden_dir):
    """sample() with the reference's signature: size <= |C|: `size` distinct elements of the reference's C; else all of C behind a
    head in possible - batch that is duplicate-free exactly when the reference drew without replacement."""
    _need_gpu()
    g = g13(golden_dir)
    src, dst, t = g["src"], g["dst"], g["t"]
    smps = {}
    us, ud = np.unique(src), np.unique(dst)
    for c in range(len(g["call_size"])):
        lot = None if np.isnan(g["call_lot"][c]) else float(g["call_lot"][c])
        strategy = "historical" if g["call_strategy"][c] == 1 else "inductive"
        smp = smps.setdefault((strategy, lot), _sampler(src, dst, t, strategy, lot, seed=0))
        b, size = slice(g["call_b0"][c], g["call_b1"][c]), int(g["call_size"][c])
        C = g["cand_keys"][g["cand_off"][c]:g["cand_off"][c + 1]]
        s, d = smp.sample(size, src[b], dst[b], g["call_t0"][c], g["call_t1"][c])
        assert isinstance(s, np.ndarray) and s.dtype == np.int64 and d.dtype == np.int64 and len(s) == len(d) == size
        assert size == g["out_off"][c + 1] - g["out_off"][c]
        k = (s << 32) | d
        if size <= len(C):
            assert np.isin(k, C).all() and len(np.unique(k)) == size, f"call {c}"
        else:
            F = size - len(C)
            assert np.array_equal(np.sort(k[F:]), C), f"call {c}"
            head = k[:F]
            assert np.isin(s[:F], us).all() and np.isin(d[:F], ud).all() and not np.isin(head, (src[b] << 32) | dst[b]).any(), f"call {c}"
            assert (len(np.unique(head)) == F) == (not g["call_replace"][c]), f"call {c}"


@pytest.mark.gpu
def test_distribution_against_the_reference(golden_dir):
    """The fixture's two cases over calls 0..511 of one seed: every candidate's inclusion frequency within 5 sigma + 1/T of
    size / |C|, every possible non-batch edge's within the same of F / |possible - batch| in the fill's head."""
    _need_gpu()
    g = g13(golden_dir)
    src, dst, t = g["src"], g["dst"], g["t"]
    smp = _sampler(src, dst, t, seed=5)

    def sample(b0, b1, size, T):
        smp.reset_random_state()
        bs, bd = _dev(src[b0:b1]), _dev(dst[b0:b1])
        outs = [smp.sample_device(size, bs, bd, t[b0], t[b1 - 1]) for _ in range(T)]
        k = (torch.stack([o[0] for o in outs]) << 32) | torch.stack([o[1] for o in outs])
        return k.cpu().numpy()
    worst = 0.0
    for f, p, T in _inclusion(golden_dir, sample):
        worst = max(worst, float(np.abs(f - p).max() / bound(p, T)))
        assert np.all(np.abs(f - p) <= bound(p, T)), np.abs(f - p).max() / bound(p, T)
    print("largest |freq - p| / bound:", worst)


@pytest.mark.gpu
def test_determinism(golden_dir):
    _need_gpu()
    g = g13(golden_dir)
    src, dst, t = g["src"], g["dst"], g["t"]
    bs, bd = _dev(src[200:225]), _dev(dst[200:225])
    a, b = (_sampler(src, dst, t, seed=77) for _ in range(2))
    run = lambda s, sizes=(25, 25, 90): [torch.stack(s.sample_device(n, bs, bd, t[200], t[224])) for n in sizes]
    ra, rb = run(a), run(b)
    assert all(torch.equal(x, y) for x, y in zip(ra, rb)), "the same (seed, call index) must give identical arrays"
    assert not torch.equal(ra[0], ra[1]), "consecutive calls must differ"
    a.reset_random_state()
    assert all(torch.equal(x, y) for x, y in zip(run(a), ra)), "reset_random_state() must replay call 0"
    a.reset_random_state()
    other = run(a, (3, 0, 90))                                     # a call's output does not depend on the sizes of earlier calls
    assert torch.equal(other[2], ra[2]) and other[1].shape == (2, 0)
    assert not torch.equal(run(_sampler(src, dst, t, seed=78))[0], ra[0]), "two seeds must differ"
    u = _sampler(src, dst, t, seed=None)
    with pytest.raises(AssertionError):
        u.sample(5, src[:5], dst[:5], 1.0, 2.0)
    with pytest.raises(AssertionError):
        a.sample(5)


@pytest.mark.gpu
def test_random_strategy(golden_dir):
    """Values from the unique arrays, bit for bit against the restatement (whatever the size), marginal frequencies over 4 096 draws
    within 5 sigma + 1/n; interact_times may be absent, as in the reference's training sampler."""
    _need_gpu()
    g = g13(golden_dir)
    src, dst = g["src"], g["dst"]
    tab = Table(src, dst, None)
    smp = _sampler(src, dst, None, "random", seed=9)
    assert smp.earliest_time is None and smp.negative_sample_strategy == "random" and smp.seed == 9
    for call, size in enumerate((1, 0, 255, 257, 4096)):
        s, d = smp.sample(size)
        ws, wd, _ = tab.sample("random", size, None, None, 0.0, 0.0, 9, call)
        assert s.dtype == np.int64 and np.array_equal(s, ws) and np.array_equal(d, wd), size
    for got, uniq in ((s, tab.us), (d, tab.ud)):
        assert np.isin(got, uniq).all()
        p = 1.0 / len(uniq)
        f = np.array([(got == x).mean() for x in uniq])
        assert np.all(np.abs(f - p) <= bound(p, 4096))
    np.random.seed(5)
    u1 = _sampler(src, dst, None, "random", seed=None)
    np.random.seed(5)
    u2 = _sampler(src, dst, None, "random", seed=None)
    assert u1.seed is None and np.array_equal(u1.sample(40)[1], u2.sample(40)[1])


def _module(N, d=32):
    import tpnet_amd
    torch.manual_seed(11)
    return tpnet_amd.RandomProjectionModule(node_num=N, edge_num=300, dim_factor=10, num_layer=3, time_decay_weight=1e-3, device="cuda:0",
                                            use_matrix=False, beginning_time=np.float64(0.0), not_scale=False, enforce_dim=d).to("cuda:0")


@pytest.mark.gpu
def test_run_evaluation_with_the_device_samplers(golden_dir):
    """'historical' negatives through run_evaluation on the toy graph: every batch's negatives satisfy the contract, the negative
    readout is get_pair_wise_feature(neg_src, neg_dst) on the state before the batch's update, and the state afterwards equals a
    plain update loop's."""
    _need_gpu()
    import tpnet_amd
    from tpnet_amd.callers import run_evaluation
    g = g13(golden_dir)
    src, dst, t = g["src"], g["dst"], g["t"]
    tab = Table(src, dst, t)
    rp, plain, probe = _module(41), _module(41), _module(41)
    assert torch.equal(rp.random_projections[0], plain.random_projections[0])
    nbr = tpnet_amd.GpuRecentNeighborSampler(src, dst, t, device="cuda:0", num_nodes=41)
    neg = _sampler(src, dst, t, seed=3)
    seen = []

    def on_batch(i, neg_src, neg_dst, res):
        b = slice(25 * i, 25 * i + 25)
        C = tab.candidates("historical", t[b][0], t[b][-1])
        k = (neg_src << 32) | neg_dst
        F = max(25 - len(C), 0)
        assert len(k) == 25 and np.isin(k[F:], C).all() and len(np.unique(k[F:])) == 25 - F
        assert not np.isin(k[:F], (src[b] << 32) | dst[b]).any() and len(np.unique(k[:F])) == F
        feats, outs = res
        assert feats[1].shape == (50, 4, 2 * rp.pair_wise_feature_dim)
        with torch.no_grad():                                      # `probe` holds the state before this batch's update
            assert torch.equal(outs[1], probe.get_pair_wise_feature(neg_src, neg_dst))
            assert torch.equal(outs[0], probe.get_pair_wise_feature(src[b], dst[b]))
        probe.update(src[b], dst[b], t[b])
        seen.append(F)
    probe.mlp.load_state_dict(rp.mlp.state_dict())
    with torch.no_grad():
        res = run_evaluation(rp, nbr, neg, src, dst, t, 25, 4, on_batch=on_batch)
    assert len(res) == 12 and seen[0] == 25 and seen[-1] == 0 and neg._calls == 12
    for b0 in range(0, 300, 25):
        plain.update(src[b0:b0 + 25], dst[b0:b0 + 25], t[b0:b0 + 25])
    for i in range(4):
        assert torch.equal(rp.random_projections[i].detach(), plain.random_projections[i].detach())
    assert float(rp.now_time) == t[-1]
    # a 'random' sampler: `size` destinations, the negative source is the batch's own -- the path of link_prediction_batch without neg_src
    rnd = _sampler(src, dst, None, "random", seed=3)
    got = []
    with torch.no_grad():
        run_evaluation(rp, nbr, rnd, src[:50], dst[:50], t[:50] + 100.0, 25, 4, on_batch=lambda i, ns, nd, r: got.append((ns, nd)))
    assert np.array_equal(got[0][0], src[:25]) and np.array_equal(got[1][0], src[25:50]) and np.isin(got[1][1], tab.ud).all()
