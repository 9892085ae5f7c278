"""Generates tests/golden/g12_sampler.npz (fixture G12): the reference's own `NeighborSampler` with the
'time_interval_aware' strategy on a toy graph, CPU.

Runs only where the read-only reference checkout is present (TPNET_REFERENCE, default /root/reference); the fixture holds DATA
only -- the edge list, and per recorded (time_scaling_factor, node, query time) the `find_neighbors_before` slices (neighbour
ids, edge ids, times) and the probability vector the reference hands to `RandomState.choice`: softmax(float32(p[:n]))
(utils/utils.py:141-158, 191-198).  Ragged arrays are stored concatenated, case c at [case_off[c], case_off[c + 1]).

Graph: RandomState(5), N = 12 nodes, E = 400 edges; src = randint(1, 5) with the first 60 set to node 1 (a hub), dst =
randint(5, 12); times = the sorted union of 200 draws in [0, 50] and 200 in [5000, 5100] with t[100:104] made equal; edge ids
1..E.  Scales {0.0, 1e-2, 0.5} x nodes {1, 2, 7} x query times {10, 49, 5050, 6000, t[100]}; queries without an earlier
interaction are not recorded.  At 0.5 the early cluster underflows (exp(-2500) = 0): NaN prefixes and all-NaN prefixes.  No
entry may have s (t_j - t_last) in [-760, -700], where a denormal exp decides between NaN and 1 (asserted below)."""
import os
import sys

import numpy as np

REF = os.environ.get("TPNET_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import torch  # noqa: E402
from utils.utils import NeighborSampler  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SCALES = (0.0, 1e-2, 0.5)
NODES = (1, 2, 7)


def graph():
    rng = np.random.RandomState(5)
    N, E = 12, 400
    src = rng.randint(1, 5, E).astype(np.int64)
    src[:60] = 1
    dst = rng.randint(5, 12, E).astype(np.int64)
    t = np.sort(np.concatenate([rng.uniform(0.0, 50.0, 200), rng.uniform(5000.0, 5100.0, 200)]))
    t[100:104] = t[100]
    eid = np.arange(1, E + 1, dtype=np.int64)
    return N, src, dst, t, eid


def main():
    N, src, dst, t, eid = graph()
    assert np.all(np.diff(t) >= 0)
    adj = [[] for _ in range(N)]
    for s_, d_, e_, t_ in zip(src, dst, eid, t):                  # utils/utils.py:303-312
        adj[s_].append((d_, e_, t_))
        adj[d_].append((s_, e_, t_))
    qtimes = (10.0, 49.0, 5050.0, 6000.0, float(t[100]))
    out = dict(N=N, src=src, dst=dst, t=t, eid=eid)
    cs, cn, ct, off = [], [], [], [0]
    ids, eids, times, probs = [], [], [], []
    for s in SCALES:
        sampler = NeighborSampler(adj_list=adj, sample_neighbor_strategy="time_interval_aware", time_scaling_factor=s, seed=0)
        for lst in sampler.nodes_neighbor_times:
            if len(lst):
                z = s * (lst - lst.max())
                assert not np.any((z >= -760.0) & (z <= -700.0)), "an entry sits where a denormal exp decides"
        for node in NODES:
            for q in qtimes:
                a, b, c, p = sampler.find_neighbors_before(node_id=node, interact_time=q, return_sampled_probabilities=True)
                if len(a) == 0:
                    continue
                p = torch.softmax(torch.from_numpy(p).float(), dim=0).numpy()         # utils/utils.py:194
                cs.append(s), cn.append(node), ct.append(q), off.append(off[-1] + len(a))
                ids.append(a), eids.append(b), times.append(c), probs.append(p)
    out.update(case_scale=np.array(cs), case_node=np.array(cn, dtype=np.int64), case_time=np.array(ct),
               case_off=np.array(off, dtype=np.int64), nbr_ids=np.concatenate(ids).astype(np.int64),
               nbr_eids=np.concatenate(eids).astype(np.int64), nbr_times=np.concatenate(times).astype(np.float64),
               probs=np.concatenate(probs).astype(np.float32))
    np.savez_compressed(os.path.join(HERE, "g12_sampler.npz"), **out)
    print("g12_sampler.npz:", len(cs), "cases,", off[-1], "entries")


if __name__ == "__main__":
    main()
