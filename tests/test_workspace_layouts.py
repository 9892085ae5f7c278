"""Caller-owned buffers of the C ABI at exactly the size their *_bytes export names, at a base that is not 256-byte aligned, between
guard bytes: nothing outside the buffer is written, the results are those of a generous aligned buffer bit for bit, and one byte
less is refused before anything is launched.  The sizes used are E = 1, 255, 256, 257 -- the edges of the n / 256 + 2 tile-sum array
-- and tables of 2 and 300 nodes."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, _need_gpu, _random_stream

GUARD = 0xA5
ES = (1, 255, 256, 257)
NODES = (2, 300)
ERR_WORKSPACE = -2


class _Guarded:
    """8 + nbytes + 4096 bytes of 0xA5; the buffer under test is the nbytes at base + 8."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.t = torch.full((8 + self.nbytes + 4096,), GUARD, dtype=torch.uint8, device=DEV)
        self.ptr = self.t.data_ptr() + 8
        assert self.ptr % 256 == 8, "precondition: the allocator hands out 256-byte aligned blocks"

    def intact(self):
        return bool((self.t[:8] == GUARD).all()) and bool((self.t[8 + self.nbytes:] == GUARD).all())

    def untouched(self):
        return bool((self.t == GUARD).all())


class _Generous:
    """A 256-byte aligned buffer of twice the size and a page."""

    def __init__(self, nbytes):
        self.nbytes = 2 * int(nbytes) + 4096
        self.t = torch.zeros(self.nbytes + 256, dtype=torch.uint8, device=DEV)
        self.ptr = (self.t.data_ptr() + 255) // 256 * 256


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _edges(E, n_nodes, seed=3):
    rng = np.random.RandomState(seed + 7 * E + n_nodes)
    src = torch.from_numpy(rng.randint(0, n_nodes, E).astype(np.int64)).to(DEV)
    dst = torch.from_numpy(rng.randint(0, n_nodes, E).astype(np.int64)).to(DEV)
    t = torch.from_numpy(np.sort(rng.randint(0, 50, E).astype(np.float64))).to(DEV)       # non-decreasing, with ties
    return rng, src, dst, t


def _both(nbytes, run):
    """run(ptr, nbytes) -> tensors, on the guarded exact buffer and on the generous one: guards intact, results equal bit for bit."""
    g = _Guarded(nbytes)
    got = run(g.ptr, g.nbytes)
    torch.cuda.synchronize()
    assert g.intact(), "a write outside the buffer"
    w = _Generous(nbytes)
    want = run(w.ptr, w.nbytes)
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"result {i} differs from the run on a generous buffer"


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes", NODES)
@pytest.mark.parametrize("E", ES)
def test_sampler_buffer_of_exactly_its_size(hip_lib, E, n_nodes):
    _need_gpu()
    rng, src, dst, t = _edges(E, n_nodes)
    eids = torch.arange(E, dtype=torch.int64, device=DEV)
    n, K = 40, 3
    nodes = torch.from_numpy(rng.randint(0, n_nodes, n).astype(np.int64)).to(DEV)
    times = torch.from_numpy(rng.randint(0, 60, n).astype(np.float64)).to(DEV)

    def run(ptr, nbytes):
        assert hip_lib.tpnet_sampler_build(ptr, nbytes, src.data_ptr(), dst.data_ptr(), t.data_ptr(), eids.data_ptr(), E, n_nodes,
                                           _stream()) == 0
        out = (torch.full((n * K,), -9, dtype=torch.int64, device=DEV), torch.full((n * K,), -9, dtype=torch.int64, device=DEV),
               torch.full((n * K,), -9.0, dtype=torch.float64, device=DEV))
        assert hip_lib.tpnet_sample_recent(ptr, E, n_nodes, nodes.data_ptr(), times.data_ptr(), n, K, out[0].data_ptr(),
                                           out[1].data_ptr(), out[2].data_ptr(), _stream()) == 0
        return out
    _both(hip_lib.tpnet_sampler_bytes(E, n_nodes), run)


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes", NODES)
@pytest.mark.parametrize("E", ES)
def test_negative_sampler_table_and_scratch_of_exactly_their_sizes(hip_lib, E, n_nodes):
    _need_gpu()
    rng, src, dst, t = _edges(E, n_nodes)
    batches = {B: (torch.from_numpy(rng.randint(0, n_nodes, B).astype(np.int64)).to(DEV),
                   torch.from_numpy(rng.randint(0, n_nodes, B).astype(np.int64)).to(DEV)) for B in (5, 1025)}
    calls = [(1, 5), (2, 5), (1, 1025)]                       # (strategy: historical / inductive, size = B); 1025: the batch is sorted
    scratches = []

    def run(ptr, nbytes):
        counts = (C.c_int64 * 3)()
        assert hip_lib.tpnet_neg_build(ptr, nbytes, src.data_ptr(), dst.data_ptr(), t.data_ptr(), E, 20.0, 1, counts, _stream()) == 0
        out = [torch.tensor(list(counts), dtype=torch.int64, device=DEV)]
        exact = not scratches                                   # the first run (the guarded table) also guards its scratch
        for i, (strategy, B) in enumerate(calls):
            sb = hip_lib.tpnet_neg_scratch_bytes(E, B, B)
            s = _Guarded(sb) if exact else _Generous(sb)
            scratches.append(s)
            o = (torch.full((B,), -9, dtype=torch.int64, device=DEV), torch.full((B,), -9, dtype=torch.int64, device=DEV))
            bs, bd = batches[B]
            assert hip_lib.tpnet_neg_sample(ptr, E, strategy, B, bs.data_ptr(), bd.data_ptr(), B, 25.0, 49.0, 1234567, i, s.ptr,
                                            s.nbytes, o[0].data_ptr(), o[1].data_ptr(), _stream()) == 0
            out += [o[0], o[1], torch.tensor([hip_lib.tpnet_neg_check(ptr, _stream())], device=DEV)]
        return out
    _both(hip_lib.tpnet_neg_bytes(E), run)
    for s in scratches[:len(calls)]:
        assert s.intact(), "a write outside the scratch buffer"


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes", NODES)
@pytest.mark.parametrize("E", ES)
def test_edgebank_table_of_exactly_its_size(hip_lib, E, n_nodes):
    _need_gpu()
    rng, src, dst, t = _edges(E, n_nodes)
    Q = 30
    qs = torch.from_numpy(rng.randint(0, n_nodes, Q).astype(np.int64)).to(DEV)
    qd = torch.from_numpy(rng.randint(0, n_nodes, Q).astype(np.int64)).to(DEV)
    scratches = []

    def run(ptr, nbytes):
        counts = (C.c_int64 * 1)()
        assert hip_lib.tpnet_edgebank_build(ptr, nbytes, src.data_ptr(), dst.data_ptr(), t.data_ptr(), E, counts, _stream()) == 0
        sb = hip_lib.tpnet_edgebank_scratch_bytes(E)
        s = _Generous(sb) if scratches else _Guarded(sb)
        scratches.append(s)
        out = torch.full((Q,), -9.0, dtype=torch.float32, device=DEV)
        window = torch.full((2,), -9.0, dtype=torch.float64, device=DEV)
        # TIME_WINDOW with REPEAT_INTERVAL: the one mode that uses the scratch
        assert hip_lib.tpnet_edgebank_predict(ptr, E, 1, 1, 0.15, E, qs.data_ptr(), qd.data_ptr(), Q, out.data_ptr(), None, None, 0, None,
                                              s.ptr, s.nbytes, window.data_ptr(), _stream()) == 0
        return [torch.tensor([counts[0]], device=DEV), out, window]
    _both(hip_lib.tpnet_edgebank_bytes(E), run)
    assert scratches[0].intact(), "a write outside the scratch buffer"


@pytest.mark.gpu
def test_metrics_scratch_of_exactly_its_size(hip_lib):
    _need_gpu()
    P = N = 257
    rng = np.random.RandomState(5)
    pl, nl = (torch.from_numpy(rng.randn(n).astype(np.float32)).to(DEV) for n in (P, N))
    ps, ns = torch.sigmoid(pl), torch.sigmoid(nl)

    def run(ptr, nbytes):
        record = torch.full((8,), -1, dtype=torch.int64, device=DEV)
        assert hip_lib.tpnet_lp_metrics(ps.data_ptr(), P, ns.data_ptr(), N, pl.data_ptr(), nl.data_ptr(), ptr, nbytes, record.data_ptr(),
                                        _stream()) == 0
        return [record]
    _both(hip_lib.tpnet_lp_metrics_scratch_bytes(P, N), run)


@pytest.mark.gpu
def test_one_byte_short_is_refused_before_any_launch(hip_lib):
    """(tpnet_edgebank_predict's scratch: tests/test_edge_bank.py::test_device_refusals_launch_nothing)"""
    _need_gpu()
    E, n_nodes, B = 257, 300, 1025
    rng, src, dst, t = _edges(E, n_nodes)
    a = (src.data_ptr(), dst.data_ptr(), t.data_ptr())
    bs = torch.from_numpy(rng.randint(0, n_nodes, B).astype(np.int64)).to(DEV)
    out = torch.full((2 * B,), -9, dtype=torch.int64, device=DEV)
    c3, c1 = (C.c_int64 * 3)(), (C.c_int64 * 1)()
    scores = torch.rand(E, device=DEV)
    record = torch.full((8,), -1, dtype=torch.int64, device=DEV)
    neg = _Generous(hip_lib.tpnet_neg_bytes(E))
    assert hip_lib.tpnet_neg_build(neg.ptr, neg.nbytes, *a, E, 20.0, 1, c3, _stream()) == 0
    short = [
        (hip_lib.tpnet_sampler_bytes(E, n_nodes), lambda p, n: hip_lib.tpnet_sampler_build(p, n, *a, None, E, n_nodes, _stream())),
        (hip_lib.tpnet_neg_bytes(E), lambda p, n: hip_lib.tpnet_neg_build(p, n, *a, E, 20.0, 1, c3, _stream())),
        (hip_lib.tpnet_neg_scratch_bytes(E, B, B), lambda p, n: hip_lib.tpnet_neg_sample(
            neg.ptr, E, 1, B, bs.data_ptr(), bs.data_ptr(), B, 25.0, 49.0, 1, 0, p, n, out.data_ptr(), out.data_ptr() + 8 * B, _stream())),
        (hip_lib.tpnet_edgebank_bytes(E), lambda p, n: hip_lib.tpnet_edgebank_build(p, n, *a, E, c1, _stream())),
        (hip_lib.tpnet_lp_metrics_scratch_bytes(E, E), lambda p, n: hip_lib.tpnet_lp_metrics(
            scores.data_ptr(), E, scores.data_ptr(), E, None, None, p, n, record.data_ptr(), _stream())),
    ]
    for nbytes, call in short:
        assert nbytes > 0
        g = _Guarded(nbytes)
        assert call(g.ptr, nbytes - 1) == ERR_WORKSPACE
        torch.cuda.synchronize()
        assert g.untouched(), "a refused call wrote to its buffer"
    assert (out == -9).all() and (record == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("planner", ["sorted", "hashed", "default"])
def test_stream_workspace_of_exactly_its_size(hip_lib, planner):
    """tpnet_run_stream over 40 batches in a workspace of exactly tpnet_stream_workspace_bytes at a misaligned base: the features and
    the table are those of the run in a generous workspace, bit for bit, and the guards stay."""
    from tpnet_amd import _lib
    _need_gpu()
    N, d, L, B, nb, lam, t0 = 300, 16, 3, 64, 40, 1e-6, 1.0e6
    E, row = B * nb, (2 * L + 2) ** 2
    flags = {"sorted": _lib.FLAG_SCHED_WINDOWED | _lib.FLAG_PLAN_SORTED, "hashed": _lib.FLAG_SCHED_WINDOWED | _lib.FLAG_PLAN_HASHED,
             "default": 0}[planner]
    src, dst, neg, t = (torch.from_numpy(x).to(DEV) for x in _random_stream(np.random.RandomState(5), N, E, 4.0e5))
    P0 = torch.from_numpy(np.random.RandomState(6).randn(N, d).astype(np.float32)).to(DEV)

    def run(ptr, nbytes):
        keep = dict(p0=P0.clone(), q=torch.zeros(2, N, L, d, device=DEV), meta=torch.zeros(N * 32, dtype=torch.uint8, device=DEV),
                    err=torch.zeros(4, dtype=torch.int32, device=DEV), pos=torch.zeros(E, row, device=DEV),
                    neg=torch.zeros(E, row, device=DEV))
        st = _lib.State(p0=keep["p0"].data_ptr(), q=keep["q"].data_ptr(), meta=keep["meta"].data_ptr(), N=N, d=d, L=L,
                        err=keep["err"].data_ptr())
        _lib.check(hip_lib.tpnet_state_init(C.byref(st), t0, _stream()), "state_init")
        _lib.check(hip_lib.tpnet_run_stream(C.byref(st), src.data_ptr(), dst.data_ptr(), neg.data_ptr(), t.data_ptr(), E, B, t0, lam, 1,
                                            flags, keep["pos"].data_ptr(), keep["neg"].data_ptr(), ptr, nbytes, None, _stream()),
                   "run_stream")
        _lib.check(hip_lib.tpnet_check_errors(C.byref(st), _stream()), "check_errors")
        return [keep[k] for k in ("pos", "neg", "q", "meta")]
    _both(hip_lib.tpnet_stream_workspace_bytes(N, d, L, E, B), run)
