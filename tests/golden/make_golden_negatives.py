"""Generates tests/golden/g13_negatives.npz (fixture G13): the reference's own `NegativeEdgeSampler` with the 'historical' and
'inductive' strategies on a toy graph, CPU.

Runs only where the read-only reference checkout is present (TPNET_REFERENCE, default /root/reference); the fixture holds DATA
only -- the edge list and, per recorded call (strategy, t0, t1, batch slice, size, last_observed_time), the reference's candidate set
(`unique_historical_edges` / `unique_inductive_edges`, utils/utils.py:438, 478) as sorted keys src << 32 | dst, |possible_edges -
batch_edges| (:413), and the reference's outputs for a sampler of seed 0 reset before the call.  For one call with size < |C| and one
fill call: how often each candidate (each possible non-batch edge, in the fill's head) was returned over T = 512 consecutive calls of
one seeded sampler.  Ragged arrays are stored concatenated, call c at [off[c], off[c + 1]).

Graph: RandomState(13), E = 300 edges drawn from a pool of 90 distinct pairs of 15 source nodes (1..15) x 25 destination nodes
(16..40); integer stamps sorted(randint(0, 60)) -- about five edges per stamp, so batches of 25 begin and end on tied stamps and an
edge is often stamped exactly t0 or t1."""
import os
import sys

import numpy as np

REF = os.environ.get("TPNET_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from utils.utils import NegativeEdgeSampler  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
BATCH, T = 25, 512


def graph():
    rng = np.random.RandomState(13)
    pool = rng.permutation(15 * 25)[:90]
    pick = pool[rng.randint(0, 90, 300)]
    src = (pick // 25 + 1).astype(np.int64)
    dst = (pick % 25 + 16).astype(np.int64)
    t = np.sort(rng.randint(0, 60, 300)).astype(np.float64)
    return src, dst, t


def key(edges):
    return np.array(sorted((int(a) << 32) | int(b) for a, b in edges), dtype=np.int64)


def candidates(smp, strategy, t0, t1):
    hist = smp.get_unique_edges_between_start_end_time(smp.earliest_time, t0)
    cur = smp.get_unique_edges_between_start_end_time(t0, t1)
    return hist - cur if strategy == "historical" else hist - smp.observed_edges - cur


def main():
    src, dst, t = graph()
    E = len(src)
    calls = []                                                  # (strategy, b0, b1, t0, t1, size, last_observed_time)
    for b0 in range(0, E, BATCH):
        b1 = min(b0 + BATCH, E)
        for size in (b1 - b0, 3, 200):
            calls.append(("historical", b0, b1, t[b0], t[b1 - 1], size, np.nan))
    for lot in (-5.0, 20.0, 33.0, 1000.0):                       # before, inside (twice) and after the history
        for b0 in (0, 100, 200, 275):
            for size in (25, 2, 120):
                calls.append(("inductive", b0, b0 + BATCH, t[b0], t[b0 + BATCH - 1], size, lot))
    calls.append(("historical", 150, 175, t[150], t[174], 700, np.nan))          # more than the possible edges: replacement
    calls.append(("historical", 150, 175, t[150] + 0.5, t[150] + 0.25, 40, np.nan))   # an empty window between two stamps
    calls.append(("historical", 0, 25, 1.0e6, 2.0e6, 60, np.nan))                # behind the last stamp: every edge is history

    def make(strategy, lot):
        return NegativeEdgeSampler(src, dst, t, last_observed_time=None if np.isnan(lot) else lot, negative_sample_strategy=strategy,
                                   seed=0)
    samplers = {}
    c_keys, c_off, o_src, o_dst, o_off, possible, replace = [], [0], [], [], [0], [], []
    for strategy, b0, b1, t0, t1, size, lot in calls:
        smp = samplers.setdefault((strategy, lot), make(strategy, lot))
        smp.reset_random_state()
        C = candidates(smp, strategy, t0, t1)
        batch = set(zip(src[b0:b1], dst[b0:b1]))
        P = len(smp.possible_edges - batch)
        ns, nd = smp.sample(size, src[b0:b1], dst[b0:b1], t0, t1)
        assert len(ns) == size and (size > len(C) or set(zip(ns, nd)) <= C)
        c_keys.append(key(C)), c_off.append(c_off[-1] + len(C))
        o_src.append(ns), o_dst.append(nd), o_off.append(o_off[-1] + size)
        possible.append(P), replace.append(int(size > len(C) and P < size - len(C)))
    out = dict(src=src, dst=dst, t=t, call_strategy=np.array([1 if c[0] == "historical" else 2 for c in calls], dtype=np.int64),
               call_b0=np.array([c[1] for c in calls], dtype=np.int64), call_b1=np.array([c[2] for c in calls], dtype=np.int64),
               call_t0=np.array([c[3] for c in calls]), call_t1=np.array([c[4] for c in calls]),
               call_size=np.array([c[5] for c in calls], dtype=np.int64), call_lot=np.array([c[6] for c in calls]),
               call_possible=np.array(possible, dtype=np.int64), call_replace=np.array(replace, dtype=np.int64),
               cand_keys=np.concatenate(c_keys), cand_off=np.array(c_off, dtype=np.int64),
               out_src=np.concatenate(o_src).astype(np.int64), out_dst=np.concatenate(o_dst).astype(np.int64),
               out_off=np.array(o_off, dtype=np.int64), T=T)

    # inclusion counts over T consecutive calls of one seeded sampler
    b0, b1 = 200, 225
    smp = make("historical", np.nan)
    C = key(candidates(smp, "historical", t[b0], t[b1 - 1]))
    size = 7
    assert size < len(C)
    cnt = np.zeros(len(C), dtype=np.int64)
    for _ in range(T):
        ns, nd = smp.sample(size, src[b0:b1], dst[b0:b1], t[b0], t[b1 - 1])
        cnt[np.searchsorted(C, (ns << 32) | nd)] += 1
    out.update(dist_call=np.array([b0, b1, size], dtype=np.int64), dist_keys=C, dist_counts=cnt)
    b0, b1 = 25, 50                                             # few candidates yet: a fill of size - |C| possible non-batch edges
    smp = make("historical", np.nan)
    C = candidates(smp, "historical", t[b0], t[b1 - 1])
    size = len(C) + 60
    possible_keys = key(smp.possible_edges - set(zip(src[b0:b1], dst[b0:b1])))
    cnt = np.zeros(len(possible_keys), dtype=np.int64)
    for _ in range(T):
        ns, nd = smp.sample(size, src[b0:b1], dst[b0:b1], t[b0], t[b1 - 1])
        head = (ns[:60] << 32) | nd[:60]
        assert len(set(head)) == 60
        cnt[np.searchsorted(possible_keys, head)] += 1
    out.update(fill_call=np.array([b0, b1, size, 60], dtype=np.int64), fill_keys=possible_keys, fill_counts=cnt)
    np.savez_compressed(os.path.join(HERE, "g13_negatives.npz"), **out)
    print("g13_negatives.npz:", len(calls), "calls,", c_off[-1], "candidate keys,", o_off[-1], "outputs;",
          "fills:", sum(1 for c, k in zip(calls, range(len(calls))) if c[5] > c_off[k + 1] - c_off[k]), "replace:", sum(replace))


if __name__ == "__main__":
    main()
