"""GPU tests of the windowed plan's per-contribution record (tpnet_common.h: WRec -- one 32-byte record per sorted contribution,
written once by each planner, read by the chain walkers and the write-back of wstep.hip).

Every reader of the record, at the smallest shape at which it can go wrong:
  hub          a chain of 1 600 contributions (200 blocks of 8) per 8-batch window: chain_heavy walks it in TWO segments of <= 152 blocks
  mixed        chain_light and chain_medium (nodes repeated 20-60 times per window), a window count that does not divide, one bad
               edge id and one bad negative
  geometries   the other row geometries (lanes per row / per column part, column parts): d = 64, 16, 256
The three planners (dense, hashed, sorted) must agree bit for bit, and each is held against the numpy oracle with the tolerances
of tests/test_gpu_parity.py.  Replay keeps the records and forms only the negatives' references again; no reader may depend on a
byte no writer wrote (the record's spare word, records of positions that hold no contribution)."""
import numpy as np
import pytest
import torch

from oracle import tpnet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAM = 2e-6
SCHEDULES = ("windowed", "windowed-hashed", "windowed-sorted")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: run on the MI355X box (python -m pytest -m gpu)")


def _module(N, d, L, t0, P0):
    from tpnet_amd import RandomProjectionModule
    rp = RandomProjectionModule(node_num=N, edge_num=1000, dim_factor=10, num_layer=L, time_decay_weight=LAM, device=DEV,
                                use_matrix=False, beginning_time=np.float64(t0), not_scale=False, enforce_dim=d)
    rp.random_projections[0].data = torch.from_numpy(np.ascontiguousarray(P0))
    return rp.to(DEV)


def _layers(rp):
    return np.stack([rp.random_projections[i].detach().cpu().numpy() for i in range(1, rp.num_layer + 1)])


# ---- the oracle comparison: copied from tests/test_gpu_parity.py ----------------------------------------------------------------
def _assert_state(got, want, rtol, what=""):
    """tests/test_gpu_parity.py::_assert_state: rtol from the caller (2e-4 below), atol 1e-6 * max|P[i]|."""
    for i in range(want.shape[0]):
        scale = max(1e-30, float(np.abs(want[i]).max()))
        np.testing.assert_allclose(got[i], want[i], rtol=rtol, atol=1e-6 * scale, err_msg=f"{what} layer {i + 1}")


def _gram_bound(P, u, v, L, rel):
    """tests/test_gpu_parity.py::_gram_bound."""
    R = np.stack([P[i][u] for i in range(L + 1)] + [P[i][v] for i in range(L + 1)], axis=1).astype(np.float64)
    nrm = np.linalg.norm(R, axis=2)
    return (rel * nrm[:, :, None] * nrm[:, None, :]).reshape(len(u), -1) + 1e-30


def _assert_features(got, st, u, v, what=""):
    """tests/test_gpu_parity.py::_assert_features: rtol 1e-4, atol 1e-5 + 1e-6 * ||R_a|| * ||R_b|| / (1 + relu(G))."""
    raw = O.pair_gram(st, u, v, not_scale=True)
    want = O.pair_gram(st, u, v)
    atol = 1e-5 + _gram_bound(st.P, u, v, st.L, 1e-6) / (1.0 + np.maximum(raw, 0))
    bad = np.abs(got - want) > 1e-4 * np.abs(want) + atol
    assert not bad.any(), f"{what}: {int(bad.sum())} features off, worst |delta| {np.abs(got - want)[bad].max():.3e}"


# ---- the streams ------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, d, L, N, B, nb, src, dst, neg, t, P0, bad_edge=None, bad_neg=None):
        self.name, self.d, self.L, self.N, self.B, self.nb = name, d, L, N, B, nb
        self.src, self.dst, self.neg, self.t, self.P0 = src, dst, neg, t, P0
        self.bad_edge, self.bad_neg = bad_edge, bad_neg
        self.E = len(src)

    def dev(self, neg=None):
        f = lambda x: torch.from_numpy(x).to(DEV)
        return f(self.src), f(self.dst), f(self.neg if neg is None else neg), f(self.t)

    def ok_rows(self):
        """rows whose (src, dst) / (src, neg) features are defined: not those of an edge with a bad id / of a bad negative"""
        pos = np.ones(self.E, dtype=bool)
        if self.bad_edge is not None:
            pos[self.bad_edge] = False
        neg = pos.copy()
        if self.bad_neg is not None:
            neg[self.bad_neg] = False
        return pos, neg


def _window_batches(B, nb):
    """Batches per window the library picks for a stream of nb batches of B edges (plan.hip: wplan_window_batches, window_batches_for).
    Only used to scale how often the cases repeat a node: no assertion depends on it."""
    kmax = min(64, 24576 // B)
    k = 2
    while k < kmax and k * k < 5 * nb:
        k += 1
    nw = (nb + k - 1) // k
    return (nb + nw - 1) // nw


def _times(rng, E):
    return np.sort(rng.uniform(1.0e6, 1.0e6 + 4.0e5, E))


def make_case(name):
    if name == "hub":
        d, L, N, B, nb = 128, 3, 300, 200, 16
        rng = np.random.RandomState(11)
        E = nb * B - B // 3                                       # a short last batch
        src = rng.randint(2, N, E).astype(np.int64)
        dst = np.ones(E, dtype=np.int64)                          # every edge's dst is node 1: 1 600 contributions per 8-batch window
        neg = rng.randint(0, N, E).astype(np.int64)
        return Case(name, d, L, N, B, nb, src, dst, neg, _times(rng, E), (rng.randn(N, d) / np.sqrt(d)).astype(np.float32))
    shapes = {"mixed": (128, 3, 400, 64, 50), "d64": (64, 2, 3000, 200, 20), "d16": (16, 4, 300, 100, 24),
              "d256": (256, 3, 500, 500, 13)}
    d, L, N, B, nb = shapes[name]
    rng = np.random.RandomState(d + B + nb)
    E = nb * B - B // 3
    src = rng.randint(1, N, E).astype(np.int64)
    dst = rng.randint(1, N, E).astype(np.int64)
    # a few nodes repeated 20-60 times per window: the medium walker's lengths (16 .. 128 contributions), beside light chains of every
    # length; the geometry cases also hold one node of ~200 per window (a workgroup per column part walks it)
    per_window = _window_batches(B, nb) * B
    repeated = [(3, 25), (5, 40), (9, 55)] + ([] if name == "mixed" else [(12, 200)])
    for node, count in repeated:
        src[rng.rand(E) < count * 2 / 3 / per_window] = node
        dst[rng.rand(E) < count / 3 / per_window] = node
    dst[::17] = src[::17]                                         # self pairs
    neg = rng.randint(0, N, E).astype(np.int64)                   # includes the padding row 0
    bad_edge = bad_neg = None
    if name == "mixed":
        src[5] = N + 3                                            # a bad edge and a bad negative: skipped and counted
        neg[7] = -2
        bad_edge, bad_neg = 5, 7
    return Case(name, d, L, N, B, nb, src, dst, neg, _times(rng, E), (rng.randn(N, d) / np.sqrt(d)).astype(np.float32), bad_edge, bad_neg)


def oracle_run(c, neg=None, src=None):
    """The oracle's loop over the batches: readout, readout, update.  An edge with a bad id takes no part in the update (the kernels
    give it weight 0) and its rows, like the row of a bad negative, are not defined: zeros here, excluded by the callers."""
    src = c.src if src is None else src
    neg = c.neg if neg is None else neg
    st = O.OracleState(c.P0, c.L, LAM, c.t[0])
    okp, okn = c.ok_rows()
    states = []
    for b in range(0, c.E, c.B):
        s = np.arange(b, min(b + c.B, c.E))
        states.append((s, [p.copy() for p in st.P]))
        m = s[okp[s]]
        assert m[-1] == s[-1]                                      # (the batch's clock is its last edge's: that edge must be a good one)
        O.update(st, src[m], c.dst[m], c.t[s][okp[s]])
    return st, states


def check_against_oracle(c, fp, fn, layers, states, st_final, src=None, neg=None):
    src = c.src if src is None else src
    neg = c.neg if neg is None else neg
    okp, okn = c.ok_rows()
    fp = fp.cpu().numpy()
    fn = fn.cpu().numpy()
    view = O.OracleState(c.P0, c.L, LAM, c.t[0])
    for s, P in states:
        view.P = P
        sp, sn = s[okp[s]], s[okn[s]]
        _assert_features(fp[sp], view, src[sp], c.dst[sp], f"{c.name} pos batch {s[0] // c.B}")
        _assert_features(fn[sn], view, src[sn], neg[sn], f"{c.name} neg batch {s[0] // c.B}")
    _assert_state(layers, np.stack(st_final.P[1:]), 2e-4, f"{c.name} state")   # (2e-4: test_gpu_parity.py's windowed-schedule comparisons)


_cache = {}


def case_with_oracle(name):
    """A case and the oracle's run of it, computed once and shared (never modified)."""
    if name not in _cache:
        c = make_case(name)
        _cache[name] = (c,) + oracle_run(c)
    return _cache[name]


def run(c, schedule, streams=None, **kw):
    rp = _module(c.N, c.d, c.L, c.t[0], c.P0)
    ds, dd, dn, dt = streams or c.dev()
    fp, fn = rp.run_stream(ds, dd, dn, dt, c.B, schedule=schedule, **kw)
    return rp, fp, fn


def assert_same_bits(c, a, b, what):
    okp, okn = (torch.from_numpy(m).to(DEV) for m in c.ok_rows())
    assert torch.equal(a[0][okp], b[0][okp]), f"{what}: (src, dst) features differ"
    assert torch.equal(a[1][okn], b[1][okn]), f"{what}: (src, neg) features differ"
    np.testing.assert_array_equal(a[2], b[2], err_msg=f"{what}: state differs")


# ---- the tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hub", "mixed", "d64", "d16", "d256"])
def test_three_planners_write_the_same_records(name):
    """Features and state bit for bit between the dense, the hashed and the sorted planner, and each against the oracle."""
    _need_gpu()
    c, st_final, states = case_with_oracle(name)
    outs = {}
    for sch in SCHEDULES:
        rp, fp, fn = run(c, sch)
        outs[sch] = (fp, fn, _layers(rp))
        if c.bad_edge is not None:
            with pytest.raises(IndexError):
                rp.check_device_errors()
        else:
            rp.check_device_errors()
    for sch in SCHEDULES[1:]:
        assert_same_bits(c, outs[sch], outs[SCHEDULES[0]], f"{name}: {sch} against {SCHEDULES[0]}")
    for sch in SCHEDULES:
        check_against_oracle(c, outs[sch][0], outs[sch][1], outs[sch][2], states, st_final)


def test_replay_keeps_the_records_and_a_changed_stream_rebuilds_them():
    """Run, reset, run again with the same stream tensors and fresh negatives: the replayed plan's records are the first run's, and the
    results are a cold run's bit for bit.  After an in-place write to src the plan is built anew for the changed stream."""
    _need_gpu()
    c, _, _ = case_with_oracle("mixed")
    rng = np.random.RandomState(5)
    neg2 = rng.randint(0, c.N, c.E).astype(np.int64)
    neg2[c.bad_neg] = -2
    ds, dd, dn, dt = c.dev()
    dn2 = torch.from_numpy(neg2).to(DEV)

    def epoch(rp, negs, **kw):
        rp.reset_random_projections()
        rp.random_projections[0].data.copy_(torch.from_numpy(c.P0))
        fp, fn = rp.run_stream(ds, dd, negs, dt, c.B, schedule="windowed", **kw)
        return fp.clone(), fn.clone(), _layers(rp), rp.last_stream_replayed

    cold = _module(c.N, c.d, c.L, c.t[0], c.P0)
    c1 = epoch(cold, dn, replay=False)
    c2 = epoch(cold, dn2, replay=False)
    rp = _module(c.N, c.d, c.L, c.t[0], c.P0)
    e1 = epoch(rp, dn)
    e2 = epoch(rp, dn2)
    assert not c1[3] and not c2[3] and not e1[3] and e2[3]
    assert_same_bits(c, e1, c1, "first epoch against a cold run")
    assert_same_bits(c, e2, c2, "replayed epoch against a cold run")
    # an in-place write to src: another partner for one contribution, another target for the other one of that edge
    k = 3 * c.B + 1
    assert c.src[k] != 9
    ds[k] = 9
    src3 = c.src.copy()
    src3[k] = 9
    e3 = epoch(rp, dn2)
    assert not e3[3]
    c3 = epoch(cold, dn2, replay=False)
    assert_same_bits(c, e3, c3, "changed stream against a cold run")
    assert not torch.equal(e3[0], e2[0])                           # (the change is seen in the results)
    st3, states3 = oracle_run(c, neg=neg2, src=src3)
    check_against_oracle(c, e3[0], e3[1], e3[2], states3, st3, src=src3, neg=neg2)
    with pytest.raises(IndexError):
        rp.check_device_errors()
    with pytest.raises(IndexError):
        cold.check_device_errors()


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_no_reader_depends_on_bytes_no_writer_wrote(schedule):
    """The same stream on a workspace filled with 0xFF bytes and on a zeroed one: identical results (the record's spare word and the
    records of positions that hold no contribution are never read for their contents)."""
    _need_gpu()
    c, _, _ = case_with_oracle("mixed")
    outs = []
    for fill in (0xFF, 0x00):
        rp = _module(c.N, c.d, c.L, c.t[0], c.P0)
        rp.reserve_stream(c.E, c.B)
        ws = rp._eng["ws"]                                         # the module's stream workspace (a uint8 tensor)
        ws.fill_(fill)
        ds, dd, dn, dt = c.dev()
        fp, fn = rp.run_stream(ds, dd, dn, dt, c.B, schedule=schedule, replay=False)
        assert rp._eng["ws"] is ws                                 # (the run used the workspace that was filled)
        outs.append((fp, fn, _layers(rp)))
        with pytest.raises(IndexError):
            rp.check_device_errors()
    assert_same_bits(c, outs[0], outs[1], f"{schedule}: 0xFF-filled against zeroed workspace")
