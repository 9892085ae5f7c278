"""The device neighbour sampler's random strategies (tpnet_amd/sampler.py `GpuNeighborSampler`, csrc/sampler.hip
k_sampler_weights / k_sample_random) against a numpy restatement of their rule and against fixture G12
(tests/golden/make_golden_sampler.py: the reference's own NeighborSampler('time_interval_aware') on a toy graph).

The rule (include/tpnet_hip.h): cut = searchsorted-left of the query time in the node's time-sorted list, n = the prefix length; K
positions with replacement, Philox4x32-10 word r of (seed, call, row, slot); uniform position = (r * n) >> 32; weighted position =
the first j with W[j] >= (r + 0.5) 2^-32 W[n - 1], W = cumsum of exp(float32(p_j)) (0 for a NaN p_j); the row in ascending
position.  'uniform' is compared bit for bit; 'time_interval_aware' up to the rounding of W (summation order, exp)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the numpy restatement

def philox4x32(counter, key, rounds=10):
    """Philox4x32-10 on uint32 arrays: counter [..., 4], key [..., 2] -> [..., 4]."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & M32, (k[1] + np.uint64(0xBB67AE85)) & M32]
    return np.stack(c, axis=-1).astype(np.uint32)


def draws(seed, call, n, K):
    """The word of every (row, slot): uint64 [n, K] (values < 2^32)."""
    nb = (K + 3) // 4
    row = np.arange(n, dtype=np.uint64)[:, None].repeat(nb, 1)
    blk = np.arange(nb, dtype=np.uint64)[None, :].repeat(n, 0)
    ctr = np.stack([row & M32, row >> np.uint64(32), blk, np.full_like(row, call)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return philox4x32(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,))).reshape(n, nb * 4)[:, :K].astype(np.uint64)


class Csr:
    """The undirected adjacency as callers.RecentNeighborSampler lays it out (lexsort by node, time, append order)."""

    def __init__(self, src, dst, t, eid, num_nodes=None):
        from tpnet_amd.callers import RecentNeighborSampler
        h = RecentNeighborSampler(src, dst, t, eid)
        self.nbr, self.t, self.e, self.start = h._nbr, h._t, h._e, h._start
        self.num_nodes = len(self.start) - 1 if num_nodes is None else num_nodes

    def prefix(self, nid, q):
        """(row start, n) of one query; n = 0 for an id outside the graph."""
        if nid < 0 or nid >= self.num_nodes or nid + 1 >= len(self.start):
            return 0, 0
        lo, hi = int(self.start[nid]), int(self.start[nid + 1])
        return lo, int(np.searchsorted(self.t[lo:hi], q))

    def weights(self, s):
        """(w, W): exp(float32(p_j)) with 0 for NaN, and its per-node inclusive prefix sum."""
        w, W = np.zeros(len(self.t)), np.zeros(len(self.t))
        for nid in range(len(self.start) - 1):
            lo, hi = int(self.start[nid]), int(self.start[nid + 1])
            if hi > lo:
                with np.errstate(all="ignore"):
                    E = np.exp(s * (self.t[lo:hi] - self.t[hi - 1]))
                    p = E / np.cumsum(E)
                w[lo:hi] = np.where(np.isnan(p), 0.0, np.exp(p.astype(np.float32).astype(np.float64)))
                W[lo:hi] = np.cumsum(w[lo:hi])
        return w, W

    def gather(self, lo, pos, K):
        if pos is None:
            return np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K)
        j = lo + np.sort(pos).astype(np.int64)
        return self.nbr[j], self.e[j], self.t[j]

    def sample_uniform(self, nodes, times, K, seed, call):
        if len(nodes) == 0:
            return np.zeros((0, K), np.int64), np.zeros((0, K), np.int64), np.zeros((0, K))
        r = draws(seed, call, len(nodes), K)
        out = [self.gather(lo, (r[i] * np.uint64(n)) >> np.uint64(32) if n else None, K)
               for i, (lo, n) in enumerate(self.prefix(int(a), b) for a, b in zip(nodes, times))]
        return [np.stack([o[c] for o in out]).reshape(len(nodes), K) for c in range(3)]


def _g12(golden_dir):
    return np.load(os.path.join(golden_dir, "g12_sampler.npz"))


_cache = {}


def _graph(name, golden_dir):
    """'g12' = the fixture's graph; 'rand' = 300 nodes / 3 000 edges with rounded (tied) times, node 7 a hub."""
    if name not in _cache:
        if name == "g12":
            g = _g12(golden_dir)
            _cache[name] = (g["src"], g["dst"], g["t"], g["eid"], int(g["N"]))
        else:
            rng = np.random.RandomState(31)
            src, dst = rng.randint(1, 300, 3000), rng.randint(1, 300, 3000)
            src[rng.rand(3000) < 0.2] = 7
            dst[dst == src] = dst[dst == src] % 298 + 1            # no self loops: an edge id is unique within a node's list
            t = np.sort(np.round(rng.uniform(0.0, 1.0e4, 3000)))
            _cache[name] = (src.astype(np.int64), dst.astype(np.int64), t, rng.permutation(3000).astype(np.int64) + 1, 300)
    return _cache[name]


def _queries(csr, t, K, n, rng):
    """The query mix: node 0, an id >= num_nodes, a time before the node's first interaction, prefixes of length 1 and K - 1,
    the hub; the rest random."""
    deg = np.diff(csr.start)
    hub = int(np.argmax(deg))
    nodes = rng.randint(0, csr.num_nodes, n).astype(np.int64)
    times = rng.uniform(t.min() - 1.0, t.max() + 1.0, n)
    lo = int(csr.start[hub])
    special = [(0, t.max()), (csr.num_nodes, t.max()), (csr.num_nodes + 5, t[0]), (-1, t.max()), (hub, csr.t[lo]),
               (hub, np.nextafter(csr.t[lo], np.inf)), (hub, t.max() + 1.0), (hub, np.median(t))]
    if deg[hub] >= K and K > 1:
        tk = csr.t[lo + K - 1]                                     # the first entry of that time: the prefix ends before its ties
        special.append((hub, tk if np.searchsorted(csr.t[lo:lo + deg[hub]], tk) == K - 1 else np.nextafter(csr.t[lo + K - 2], np.inf)))
    for i, (a, b) in enumerate(special[:n]):
        nodes[i], times[i] = a, b
    return nodes, times


def _dev(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0", dt)


# ---------------------------------------------------------------------------------------------------------------- CPU tier

def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for c, k, want in kat:
        got = philox4x32(np.array(c, dtype=np.uint32), np.array(k, dtype=np.uint32))
        assert " ".join(f"{int(x):08x}" for x in got) == want
    r = draws(1234, 0, 3, 6)                                       # slot k of row i: word k & 3 of counter (i, 0, k >> 2, call)
    assert r[2, 5] == philox4x32(np.array([2, 0, 1, 0], dtype=np.uint32), np.array([1234, 0], dtype=np.uint32))[1]


def test_new_symbols_declared_and_bound_with_matching_arity():
    from tpnet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tpnet_hip.h")).read(), flags=re.S)
    for name in ("tpnet_sampler_weights_bytes", "tpnet_sampler_build_weights", "tpnet_sample_random"):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/tpnet_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name


def test_size_and_argument_checks_without_a_gpu(hip_lib):
    assert hip_lib.tpnet_sampler_weights_bytes(400) >= 2 * 400 * 8
    assert hip_lib.tpnet_sampler_build_weights(None, 10, 5, 0.0, None, 0, None) == -1
    for K in (0, 257, -3):
        assert hip_lib.tpnet_sample_random(8, None, 10, 5, 8, 8, 4, K, 0, 0, 8, None, None, None) == -1
    assert hip_lib.tpnet_sample_random(8, None, 10, 5, None, None, 0, 20, 0, 0, None, None, None, None) == 0      # n == 0: no-op


def test_weight_rule_reproduces_the_reference_probabilities(golden_dir):
    """P(j) ~ exp(float32(p_j)) over the non-NaN entries of the prefix, uniform over an all-NaN prefix: the recorded
    softmax(float32(p[:n])) vectors to 1.5e-7 of their largest entry, and the recorded slices are the CSR's prefixes."""
    g = _g12(golden_dir)
    csr = Csr(g["src"], g["dst"], g["t"], g["eid"])
    off = g["case_off"]
    seen = set()
    for s in np.unique(g["case_scale"]):
        w, W = csr.weights(float(s))
        for c in np.flatnonzero(g["case_scale"] == s):
            lo, n = csr.prefix(int(g["case_node"][c]), float(g["case_time"][c]))
            sl = slice(off[c], off[c + 1])
            assert n == off[c + 1] - off[c]
            assert np.array_equal(csr.nbr[lo:lo + n], g["nbr_ids"][sl]) and np.array_equal(csr.e[lo:lo + n], g["nbr_eids"][sl])
            assert np.array_equal(csr.t[lo:lo + n], g["nbr_times"][sl])
            p = w[lo:lo + n] / W[lo + n - 1] if W[lo + n - 1] > 0 else np.full(n, 1.0 / n)
            ref = g["probs"][sl].astype(np.float64)
            assert np.abs(p - ref).max() <= 1.5e-7 * ref.max()
            seen.add("all-nan" if W[lo + n - 1] == 0 else "nan-zone" if w[lo] == 0 else "plain")
    assert seen == {"all-nan", "nan-zone", "plain"}


# ---------------------------------------------------------------------------------------------------------------- GPU tier

def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")


def _sampler(graph, golden_dir, strategy="uniform", scale=0.0, seed=1234, shift=0.0):
    from tpnet_amd import GpuNeighborSampler
    src, dst, t, eid, N = _graph(graph, golden_dir)
    return GpuNeighborSampler(src, dst, t + shift, eid, device="cuda:0", num_nodes=N, sample_neighbor_strategy=strategy,
                              time_scaling_factor=scale, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0.0, 1.7e9, -2.0e4])
@pytest.mark.parametrize("graph", ["g12", "rand"])
def test_uniform_bit_for_bit(golden_dir, graph, shift):
    """All three outputs equal the numpy restatement, for every K that changes the rows-per-workgroup geometry (1, 3, 20, 33, 128,
    256: 256, 85, 12, 7, 2, 1 rows) and n in {0, 1, 300}, with the clock at zero, at Unix-epoch scale and below zero; the call
    index advances with every call; with_edges=False returns the same ids."""
    _need_gpu()
    src, dst, t, eid, N = _graph(graph, golden_dir)
    t = t + shift
    csr = Csr(src, dst, t, eid, N)
    smp = _sampler(graph, golden_dir, shift=shift)
    rng = np.random.RandomState(3)
    call = 0
    for K in (1, 3, 20, 33, 128, 256):
        for n in (0, 1, 300):
            nodes, times = _queries(csr, t, K, n, rng)
            if n == 1:
                nodes[0], times[0] = int(np.argmax(np.diff(csr.start))), t.max() + 1.0
            got = smp.sample_device(_dev(nodes, torch.int64), _dev(times, torch.float64), K)
            want = csr.sample_uniform(nodes, times, K, 1234, call)
            for a, b, what in zip(got, want, ("ids", "edge ids", "times")):
                assert a.shape == (n, K) and np.array_equal(a.cpu().numpy(), b), f"{what} differ at K={K} n={n} call={call}"
            ids2, e2, t2 = smp.sample_device(_dev(nodes, torch.int64), _dev(times, torch.float64), K, with_edges=False)
            assert e2 is None and t2 is None
            assert np.array_equal(ids2.cpu().numpy(), csr.sample_uniform(nodes, times, K, 1234, call + 1)[0])
            call += 2
    h = smp.get_historical_neighbors(nodes, times, 20)              # the reference's signature: numpy in, numpy out
    assert all(isinstance(x, np.ndarray) for x in h) and np.array_equal(h[1], csr.sample_uniform(nodes, times, 20, 1234, call)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("graph,scale", [("g12", 0.0), ("g12", 1e-2), ("g12", 0.5), ("rand", 0.0), ("rand", 1e-2), ("rand", 5e-2)])
def test_time_interval_aware_draws_are_valid(golden_dir, graph, scale):
    """With W recomputed in numpy: the row's positions (recovered from the edge ids, unique per node list here) in ascending order
    are those of the row's sorted x = (r + 0.5) 2^-32 W[n-1], each with W[j-1] (1 - eps) <= x <= W[j] (1 + eps), eps = (n + 4) 2^-52
    (summation order and exp rounding); the triples are the CSR's entries; a zero-weight entry is returned only from an all-NaN
    prefix, which is drawn by the uniform formula.  The scales keep s (t_j - t_last) out of [-760, -700], where a denormal exp
    decides between NaN and 1 (the random graph spans 1e4: down to -500; the fixture graph at 0.5 jumps from -50 to -2500)."""
    _need_gpu()
    src, dst, t, eid, N = _graph(graph, golden_dir)
    assert np.all(src != dst)
    csr = Csr(src, dst, t, eid, N)
    w, W = csr.weights(scale)
    smp = _sampler(graph, golden_dir, "time_interval_aware", scale)
    rng = np.random.RandomState(4)
    kinds = set()
    for call, K in enumerate((1, 20, 33, 128, 256)):
        nodes, times = _queries(csr, t, K, 200, rng)
        ids, eids, ts = [x.cpu().numpy() for x in smp.sample_device(_dev(nodes, torch.int64), _dev(times, torch.float64), K)]
        r = draws(1234, call, len(nodes), K)
        for i in range(len(nodes)):
            lo, n = csr.prefix(int(nodes[i]), times[i])
            if n == 0:
                assert not ids[i].any() and not eids[i].any() and not ts[i].any()
                continue
            where = {int(e): j for j, e in enumerate(csr.e[lo:lo + n])}
            pos = np.array([where[int(e)] for e in eids[i]])
            assert np.all(np.diff(pos) >= 0), "row not in ascending position"
            assert np.array_equal(ids[i], csr.nbr[lo + pos]) and np.array_equal(ts[i], csr.t[lo + pos])
            wt = W[lo + n - 1]
            if wt == 0:
                kinds.add("all-nan")
                assert np.array_equal(pos, np.sort((r[i] * np.uint64(n)) >> np.uint64(32)).astype(np.int64))
                continue
            kinds.add("nan-zone" if w[lo] == 0 else "plain")
            x = np.sort((r[i].astype(np.float64) + 0.5) * 2.0 ** -32 * wt)
            eps = (n + 4) * 2.0 ** -52
            below = np.where(pos > 0, W[lo + np.maximum(pos, 1) - 1], 0.0)
            assert np.all(below * (1 - eps) <= x) and np.all(x <= W[lo + pos] * (1 + eps)), f"row {i} K={K}"
            assert np.all(w[lo + pos] > 0), "a zero-weight entry was returned"
    # (the fixture graph at 0.5: the early cluster underflows, so a prefix is all NaN or begins with the NaN zone)
    assert kinds == ({"all-nan", "nan-zone"} if (graph, scale) == ("g12", 0.5) else {"plain"})


def _frequencies(smp, node, q, eids_of_prefix):
    smp.reset_random_state()
    nodes, times = np.full(128, node, dtype=np.int64), np.full(128, q)
    _, eids, _ = smp.sample_device(_dev(nodes, torch.int64), _dev(times, torch.float64), 32)
    where = {int(e): j for j, e in enumerate(eids_of_prefix)}
    pos = np.array([where[int(e)] for e in eids.cpu().numpy().reshape(-1)])
    return np.bincount(pos, minlength=len(eids_of_prefix)) / 4096.0


@pytest.mark.gpu
def test_distribution_against_the_reference(golden_dir):
    """Per recorded (scale, node, time): 128 identical rows x K = 32 = 4 096 draws (seed 1234, call 0); every position's frequency
    within 5 sigma + 1/M of the reference's probability.  'uniform': the same bound against 1/n."""
    _need_gpu()
    g = _g12(golden_dir)
    off, M = g["case_off"], 4096
    smps = {float(s): _sampler("g12", golden_dir, "time_interval_aware", float(s)) for s in np.unique(g["case_scale"])}
    uni = _sampler("g12", golden_dir)
    worst = 0.0
    for c in range(len(off) - 1):
        sl = slice(off[c], off[c + 1])
        p = g["probs"][sl].astype(np.float64)
        for smp, ref in ((smps[float(g["case_scale"][c])], p), (uni, np.full(len(p), 1.0 / len(p)))):
            if smp is uni and g["case_scale"][c] != 0.0:
                continue
            f = _frequencies(smp, int(g["case_node"][c]), float(g["case_time"][c]), g["nbr_eids"][sl])
            bound = 5.0 * np.sqrt(ref * (1 - ref) / M) + 1.0 / M
            worst = max(worst, float((np.abs(f - ref) / bound).max()))
            assert np.all(np.abs(f - ref) <= bound), f"case {c}: {np.abs(f - ref).max()} against {bound.min()}"
    print("largest |freq - p| / bound:", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", ["uniform", "time_interval_aware"])
def test_determinism(golden_dir, strategy):
    _need_gpu()
    src, dst, t, eid, N = _graph("rand", golden_dir)
    csr = Csr(src, dst, t, eid, N)
    rng = np.random.RandomState(8)
    nodes, times = _queries(csr, t, 20, 120, rng)
    nd, td = _dev(nodes, torch.int64), _dev(times, torch.float64)
    a, b = (_sampler("rand", golden_dir, strategy, 1e-3, seed=77) for _ in range(2))
    run = lambda s: [torch.stack([x.double() for x in s.sample_device(nd, td, 20)]) for _ in range(3)]
    ra, rb = run(a), run(b)
    assert all(torch.equal(x, y) for x, y in zip(ra, rb)), "the same (seed, call index) must give identical arrays"
    assert not torch.equal(ra[0], ra[1]) and not torch.equal(ra[1], ra[2]), "consecutive calls must differ"
    a.reset_random_state()
    assert all(torch.equal(x, y) for x, y in zip(run(a), ra)), "reset_random_state() must replay the sequence"
    c = _sampler("rand", golden_dir, strategy, 1e-3, seed=78)
    assert not torch.equal(run(c)[0], ra[0]), "two seeds must differ"
    # a query's draws do not change when rows are appended after it (nor with the launch geometry that comes with them)
    a.reset_random_state()
    more = a.sample_device(torch.cat([nd, nd.flip(0)]), torch.cat([td, td.flip(0)]), 20)
    assert torch.equal(torch.stack([x.double() for x in more])[:, :120], ra[0])
    # unseeded: a key from numpy's global generator, the attribute stays None
    np.random.seed(5)
    u1 = _sampler("rand", golden_dir, strategy, 1e-3, seed=None)
    np.random.seed(5)
    u2 = _sampler("rand", golden_dir, strategy, 1e-3, seed=None)
    assert u1.seed is None and u1.sample_neighbor_strategy == strategy and u1.time_scaling_factor == 1e-3
    assert torch.equal(u1.sample_device(nd, td, 20)[0], u2.sample_device(nd, td, 20)[0])


@pytest.mark.gpu
def test_recent_strategy_is_the_parent(golden_dir):
    _need_gpu()
    from tpnet_amd.sampler import GpuRecentNeighborSampler
    src, dst, t, eid, N = _graph("rand", golden_dir)
    csr = Csr(src, dst, t, eid, N)
    nodes, times = _queries(csr, t, 20, 100, np.random.RandomState(9))
    nd, td = _dev(nodes, torch.int64), _dev(times, torch.float64)
    want = GpuRecentNeighborSampler(src, dst, t, eid, device="cuda:0", num_nodes=N).sample_device(nd, td, 20)
    got = _sampler("rand", golden_dir, "recent").sample_device(nd, td, 20)
    assert all(torch.equal(x, y) for x, y in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [0, 257])
def test_unserved_widths_are_refused(golden_dir, K):
    """Argument checks of tpnet_sample_random: nothing is launched."""
    _need_gpu()
    from tpnet_amd import TPNetHipError
    smp = _sampler("g12", golden_dir)
    with pytest.raises(TPNetHipError):
        smp.sample_device(_dev(np.array([1, 2]), torch.int64), _dev(np.array([10.0, 20.0]), torch.float64), K)
    with pytest.raises(ValueError):
        _sampler("g12", golden_dir, "newest")


# ------------------------------------------------------------------------------------------------------------------ wiring

class _HostStub:
    """A host sampler that answers with recorded arrays (what the encoder sees from the reference's NeighborSampler)."""
    sample_neighbor_strategy, seed = "uniform", 0

    def __init__(self, answers):
        self.answers = list(answers)

    def reset_random_state(self):
        pass

    def get_historical_neighbors(self, node_ids, node_interact_times, num_neighbors=20):
        return self.answers.pop(0)


def _wiring(golden_dir, d=64):
    import tpnet_amd
    g = np.load(os.path.join(golden_dir, "g11_encoder.npz"))
    torch.manual_seed(21)
    rp = tpnet_amd.RandomProjectionModule(node_num=int(g["N"]), edge_num=int(g["E"]), dim_factor=10, num_layer=3, time_decay_weight=1e-4,
                                          device="cuda:0", use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                          enforce_dim=d).to("cuda:0")
    smp = tpnet_amd.GpuNeighborSampler(g["src"], g["dst"], g["t"], g["eid"], device="cuda:0", num_nodes=int(g["N"]),
                                       sample_neighbor_strategy="uniform", seed=3)
    model = tpnet_amd.TPNet(node_raw_features=g["node_raw"], edge_raw_features=g["edge_raw"], neighbor_sampler=smp, time_feat_dim=8,
                            dropout=0.1, random_projections=rp, num_layers=2, num_neighbors=6, device="cuda:0").to("cuda:0").eval()
    rp.update(g["src"][:200], g["dst"][:200], g["t"][:200])
    batches = [slice(200 + 25 * b, 225 + 25 * b) for b in range(3)]
    return g, rp, smp, model, batches


@pytest.mark.gpu
def test_tpnet_with_a_uniform_device_sampler(golden_dir):
    """The encoder keeps the batch on the device with the new sampler: the embeddings equal those of the same model fed by a host
    stub that returns the device sampler's arrays of that call; after set_neighbor_sampler two passes over three batches agree."""
    _need_gpu()
    g, rp, smp, model, batches = _wiring(golden_dir)
    src, dst, t = g["src"], g["dst"], g["t"]

    def one_pass():
        model.set_neighbor_sampler(smp)
        with torch.no_grad():
            return [torch.cat(model.compute_src_dst_node_temporal_embeddings(src[s], dst[s], t[s])) for s in batches]
    first, second = one_pass(), one_pass()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert not torch.equal(first[0], first[1])
    smp.reset_random_state()
    answers = [smp.get_historical_neighbors(np.concatenate([src[s], dst[s]]), np.tile(t[s], 2), 6) for s in batches]
    model.set_neighbor_sampler(_HostStub(answers))
    with torch.no_grad():
        for s, want in zip(batches, first):
            got = torch.cat(model.compute_src_dst_node_temporal_embeddings(src[s], dst[s], t[s]))
            assert torch.equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True])
def test_encoder_pair_features_draws_from_the_sampler(golden_dir, host):
    """rp.encoder_pair_features with a uniform sampler: the neighbours of sample_device at that call index and the features of
    get_pair_wise_feature_anchored on them -- not the 'recent' window read from the sampler's CSR."""
    _need_gpu()
    from tpnet_amd.sampler import GpuRecentNeighborSampler
    g, rp, smp, model, batches = _wiring(golden_dir)
    s = batches[1]
    src, dst, t = g["src"][s], g["dst"][s], g["t"][s]
    sd, dd, td = _dev(src, torch.int64), _dev(dst, torch.int64), _dev(t, torch.float64)
    smp.reset_random_state()
    smp.sample_device(sd, td, 6)                                   # call 0 goes by: the readout below is call 1
    with torch.no_grad():
        feats, neigh = rp.encoder_pair_features(smp, *((src, dst, t) if host else (sd, dd, td)), 6)
    smp.reset_random_state()
    smp.sample_device(sd, td, 6)
    want_neigh, _, _ = smp.sample_device(torch.cat([sd, dd]), td.repeat(2), 6, with_edges=False)
    assert torch.equal(neigh, want_neigh)
    with torch.no_grad():
        want = rp.get_pair_wise_feature_anchored(want_neigh, sd.repeat(2), dd.repeat(2))
    assert feats.shape == (4 * 25 * 6, rp.pair_wise_feature_dim) and torch.equal(feats, want)
    recent = GpuRecentNeighborSampler(g["src"], g["dst"], g["t"], g["eid"], device="cuda:0", num_nodes=int(g["N"]))
    assert not torch.equal(neigh, recent.sample_device(torch.cat([sd, dd]), td.repeat(2), 6, with_edges=False)[0])


@pytest.mark.gpu
def test_link_prediction_batch_runs_with_it(golden_dir):
    _need_gpu()
    from tpnet_amd.callers import link_prediction_batch
    g, rp, smp, model, batches = _wiring(golden_dir)
    s = batches[0]
    neg = np.random.RandomState(1).randint(1, int(g["N"]), 25).astype(np.int64)
    smp.reset_random_state()
    feats, outs = link_prediction_batch(rp, smp, g["src"][s], g["dst"][s], neg, g["t"][s], 6)
    assert feats[0].shape == (50, 6, 2 * rp.pair_wise_feature_dim) and feats[1].shape == feats[0].shape
    assert all(torch.isfinite(f).all() for f in feats) and len(outs) == 2
    assert smp._calls == 2                                         # one call of the random sequence per (src, other) readout
