"""GPU tests of the narrow walk of short chains (wstep.hip: the short region of a window's chain list, WinDesc::n_wide, walked by
16-lane x 2-vector groups, four chains per wave, where rows are 17..32 vectors long).

The streams are built by hand so that every chain's length is known: N = 200, B = 32, 8 batches -- two windows of 4 batches under
schedule="windowed" -- and every node's number of contributions per window is set exactly.
  named        nodes of exactly 1, 2, 3, 4, 5, 7, 8, 9, 15, 16 and 17 contributions in window 0 (each side of the cuts at 3 and at 7
               contributions and of the medium walker's 16); the 9 are ONE run inside one batch, src side and dst side (a run that
               crosses a WIN_BLOCK boundary, a node that is src and dst in one batch); the named nodes come back in window 1 with the
               lengths reversed (chains that start from a log slot; those of window 0 start from the table); beside them ~130 nodes
               of 1 or 2 contributions: the short region spreads over several workgroups
  named_long   the same named nodes in three windows of 14 batches (42 batches), where the library cuts the short region at 7
               contributions (below 14 batches per window: at 3), beside 154 nodes of 1..7 contributions and six of 32-33
  few_short    chains of 1, 2, 3, 5 and 7 contributions beside chains of 17: 3 short chains per window with the cut at 3 that
               windows of 4 batches get, 5 with the cut at 7 (either way fewer than the 16 a workgroup takes, no multiple of 16)
  no_short     every chain of 8, 12 or 16 contributions: an empty short region
  only_short   every chain of 1, 2 or 3 contributions: nothing but the short region
Shapes: d = 128, L = 3 (rows that fill their geometry) and d = 100, L = 2 (the same geometry, rows that do not; the heavy threshold
is 16 there, so 17 contributions are a hub chain).

Each case asserts (a) features and final layers against the numpy oracle with the tolerances of tests/test_plan_records.py, and
(b) that schedule="windowed" (dense planner) and "windowed-hashed" give the bits of "windowed-sorted", whose plan has no short
region: every chain walked the old way.  The tests compare results only: they hold the narrow walk to the wide walk's bits, and
would also pass on a library that marked no short region at all -- that the region is marked and walked is seen in the kernel's
times (profiles/narrow_chains.md), not here."""
import numpy as np
import pytest

from test_plan_records import Case, _layers, _need_gpu, _times, _window_batches, check_against_oracle, oracle_run, run

pytestmark = pytest.mark.gpu

N, B = 200, 32
BATCHES = {"named_long": (42, 14)}              # (batches, batches per window: what the library picks for that many, plan.hip:
DEFAULT_BATCHES = (8, 4)                        # window_batches_for; tests/test_plan_records.py: _window_batches)
NAMED = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)    # contributions of node 10 + c in window 0 (node 19: all 9 in one batch)


def _window(rng, counts, KW, pinned=()):
    """The (src, dst) of one window of KW batches in which node n is an endpoint exactly counts[n] times (a contribution per
    endpoint: the chain of n in this window holds counts[n]).  A node's endpoints are dealt over the batches in turn; those of a
    node in `pinned` (node -> batch) all fall into that batch.  Sides and partners are random."""
    assert sum(counts.values()) == 2 * B * KW
    per_batch = [[] for _ in range(KW)]
    for n, b in pinned:
        per_batch[b] += [n] * counts[n]
    b = 0
    for n in sorted(counts):
        if n in dict(pinned):
            continue
        for _ in range(counts[n]):
            while len(per_batch[b]) >= 2 * B:
                b = (b + 1) % KW
            per_batch[b].append(n)
            b = (b + 1) % KW
    src, dst = [], []
    for ends in per_batch:
        assert len(ends) == 2 * B
        ends = rng.permutation(np.array(ends, dtype=np.int64))
        src.append(ends[:B])
        dst.append(ends[B:])
    return np.concatenate(src), np.concatenate(dst)


def _counts(name, window):
    if name in ("named", "named_long"):
        lengths = NAMED if window % 2 == 0 else NAMED[::-1]
        counts = {10 + c: n for c, n in zip(NAMED, lengths)}
        if name == "named":
            counts.update({40 + k: 1 for k in range(85)})
            counts.update({125 + k: 2 for k in range(42)})
        else:
            counts.update({40 + k: 1 + (k + window) % 7 for k in range(154)})
            counts.update({194 + k: 32 + (k == 0) for k in range(6)})
        return counts
    if name == "few_short":
        counts = {11 + k: n for k, n in enumerate((1, 2, 3, 5, 7))}
        counts.update({20 + k + window: 17 for k in range(14)})
        return counts
    if name == "no_short":
        counts = {20 + k: 8 for k in range(8)}
        counts.update({30 + k: 12 for k in range(8)})
        counts.update({40 + k + window: 16 for k in range(6)})
        return counts
    assert name == "only_short"
    counts = {10 + k + 5 * window: 1 + k % 3 for k in range(126)}
    counts.update({150 + k: 1 for k in range(4)})
    return counts


def make_stream(name, d, L):
    NB, KW = BATCHES.get(name, DEFAULT_BATCHES)
    rng = np.random.RandomState(len(name) * 1000 + d)
    parts = [_window(rng, _counts(name, w), KW, pinned=((19, 1),) if (name.startswith("named") and w == 0) else ())
             for w in range(NB // KW)]
    src = np.concatenate([p[0] for p in parts])
    dst = np.concatenate([p[1] for p in parts])
    E = len(src)
    assert _window_batches(B, NB) == KW and E == NB * B and src.min() >= 1 and max(src.max(), dst.max()) < N
    for w in range(NB // KW):                                      # the fixture is what it says: contributions per (node, window)
        s = slice(w * KW * B, (w + 1) * KW * B)
        got = np.bincount(src[s], minlength=N) + np.bincount(dst[s], minlength=N)
        want = np.zeros(N, dtype=np.int64)
        for n, k in _counts(name, w).items():
            want[n] = k
        np.testing.assert_array_equal(got, want)
    if name.startswith("named"):
        b1 = slice(B, 2 * B)
        assert (src[b1] == 19).sum() + (dst[b1] == 19).sum() == 9 and (src[b1] == 19).any() and (dst[b1] == 19).any()
    neg = rng.randint(0, N, E).astype(np.int64)
    P0 = (rng.randn(N, d) / np.sqrt(d)).astype(np.float32)
    return Case(f"{name}-d{d}", d, L, N, B, NB, src, dst, neg, _times(rng, E), P0)


_cache = {}


def stream_with_oracle(name, d, L):
    """A stream and the oracle's run of it, computed once and shared (never modified)."""
    if (name, d) not in _cache:
        c = make_stream(name, d, L)
        _cache[(name, d)] = (c,) + oracle_run(c)
    return _cache[(name, d)]


@pytest.mark.parametrize("d,L", [(128, 3), (100, 2)])
@pytest.mark.parametrize("name", ["named", "named_long", "few_short", "no_short", "only_short"])
def test_narrow_walk_gives_the_wide_walk_s_bits_and_the_oracle_s_values(name, d, L):
    _need_gpu()
    c, st_final, states = stream_with_oracle(name, d, L)
    outs = {}
    for sch in ("windowed-sorted", "windowed", "windowed-hashed"):
        rp, fp, fn = run(c, sch)
        rp.check_device_errors()
        assert rp.last_stream_schedule == "windowed"
        outs[sch] = (fp.cpu().numpy(), fn.cpu().numpy(), _layers(rp))
        check_against_oracle(c, fp, fn, outs[sch][2], states, st_final)                       # (a)
    ref = outs["windowed-sorted"]
    for sch in ("windowed", "windowed-hashed"):                                               # (b)
        np.testing.assert_array_equal(outs[sch][0], ref[0], err_msg=f"{c.name} {sch}: (src, dst) features")
        np.testing.assert_array_equal(outs[sch][1], ref[1], err_msg=f"{c.name} {sch}: (src, neg) features")
        for i in range(L):
            np.testing.assert_array_equal(outs[sch][2][i], ref[2][i], err_msg=f"{c.name} {sch}: layer {i + 1}")
