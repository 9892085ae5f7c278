"""GPU tests of the opt-in padded engine rows (RandomProjectionModule.padded_rows, run with -m gpu): a module whose width is no
multiple of 4 floats keeps its engine table at the next multiple, pad columns +0.0, and shows the caller the reference's [N, dim].

The main test needs no tolerance: a padded module of width d and an unpadded "twin" of width engine_dim whose P[0] is the padded
module's with zero columns behind it run the same kernels on the same bits, so every output is torch.equal.  The comparisons with the
numpy oracle take the bounds of tests/test_gpu_parity.py (its header and helpers), no others:
  state P[i]      rtol 1e-4, atol 1e-6 * max|P[i]|
  log(relu(G)+1)  rtol 1e-4, atol 1e-5 + the Gram-bound term of _assert_features
"""
import copy
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from oracle import tpnet_oracle as O
from test_gpu_parity import DEV, _assert_features, _assert_state, _layers, _need_gpu

pytestmark = pytest.mark.gpu

N, B, NB, HUB = 48, 24, 12, 7
E = (NB - 1) * B + 13                       # 12 batches, a ragged last one
LAM, T0 = 1e-6, 5.0


def _stream(seed=0, n_edges=E):
    """Edges over nodes 1..N-1 with one hub node at one end of more than a third of them, increasing times, and one negative each."""
    rng = np.random.RandomState(seed)
    src = rng.randint(1, N, n_edges).astype(np.int64)
    dst = rng.randint(1, N, n_edges).astype(np.int64)
    hub = rng.random_sample(n_edges) < 0.42
    side = rng.random_sample(n_edges) < 0.5
    src[hub & side] = HUB
    dst[hub & ~side] = HUB
    assert ((src == HUB) | (dst == HUB)).mean() > 1 / 3
    t = (T0 + np.sort(rng.uniform(0.0, 2e5, n_edges))).astype(np.float64)
    neg = rng.randint(1, N, n_edges).astype(np.int64)
    return src, dst, t, neg


def _mk(d, L, padded=False, P0=None, exact=False, mlp_from=None):
    from tpnet_amd import RandomProjectionModule
    rp = RandomProjectionModule(node_num=N, edge_num=1000, dim_factor=10, num_layer=L, time_decay_weight=LAM, device=DEV,
                                use_matrix=False, beginning_time=np.float64(T0), not_scale=False, enforce_dim=d, exact=exact)
    rp.padded_rows = padded
    if P0 is not None:
        rp.random_projections[0].data = P0.clone()
    if mlp_from is not None:
        rp.mlp.load_state_dict(mlp_from.mlp.state_dict())
    return rp.to(DEV)


def _wide(x, ed):
    """[..., d] -> [..., ed] with zero columns behind."""
    out = torch.zeros(x.shape[:-1] + (ed,), dtype=x.dtype, device=x.device)
    out[..., :x.shape[-1]] = x
    return out


def _twins(d, L, exact=False):
    """(A, Bt, ed): A of width d with the switch set, Bt of width engine_dim without, P[0] = A's with zero columns behind, same mlp."""
    A = _mk(d, L, padded=True, exact=exact)
    ed = A.engine_dim
    assert ed == (d + 3) // 4 * 4 and ed != d
    Bt = _mk(ed, L, P0=_wide(A.random_projections[0].detach().cpu(), ed), exact=exact, mlp_from=A)
    assert Bt.engine_dim == ed and Bt.padded_rows is False
    return A, Bt, ed


def _same_layers(A, Bt, d, what):
    for i in range(1, A.num_layer + 1):
        a, b = A.random_projections[i].detach(), Bt.random_projections[i].detach()
        assert tuple(a.shape) == (N, d), what
        assert torch.equal(a, b[:, :d]), f"{what}: layer {i}"
        assert not b[:, d:].any() and not torch.signbit(b[:, d:]).any(), f"{what}: pad columns of layer {i}"


# ---------------------------------------------------------------------------------------------------------
# 1. twin, bit for bit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,L,exact", [(6, 1, False), (37, 3, False), (38, 4, False), (75, 3, False), (110, 3, False), (110, 2, False),
                                       (130, 3, False), (150, 3, False), (110, 3, True)])
def test_twin_bit_for_bit(d, L, exact):
    _need_gpu()
    src, dst, t, neg = _stream(1)
    A, Bt, ed = _twins(d, L, exact)
    dev = lambda x: torch.from_numpy(x).to(DEV)
    sl = lambda b0, b1: slice(b0 * B, min(b1 * B, E))
    rng = np.random.RandomState(2)
    for b in range(2):                                                    # host-array batches
        s = sl(b, b + 1)
        for rp in (A, Bt):
            rp.update(src[s], dst[s], t[s])
    s = sl(2, 3)                                                          # a device-array one
    for rp in (A, Bt):
        rp.update(dev(src[s]), dev(dst[s]), t[s])
    _same_layers(A, Bt, d, "after updates")
    for n in (10, 600):                                                   # readouts, short and longer lists
        u, v = rng.randint(0, N, n).astype(np.int64), rng.randint(0, N, n).astype(np.int64)
        assert torch.equal(A.get_pair_wise_feature(u, v), Bt.get_pair_wise_feature(u, v)), f"get_pair_wise_feature n={n}"
        with torch.no_grad():
            assert torch.equal(A.get_pair_wise_feature(u, v), Bt.get_pair_wise_feature(u, v)), f"get_pair_wise_feature (no grad) n={n}"
        assert torch.equal(A.pair_gram(u, v), Bt.pair_gram(u, v)), f"pair_gram n={n}"
        assert torch.equal(A.pair_gram(dev(u), dev(v)), Bt.pair_gram(dev(u), dev(v))), f"pair_gram (device ids) n={n}"
    ids = rng.randint(0, N, 17).astype(np.int64)
    ra, rb = A.get_random_projections(ids), Bt.get_random_projections(ids)
    assert len(ra) == len(rb) == L + 1
    for i, (x, y) in enumerate(zip(ra, rb)):
        assert tuple(x.shape) == (17, d) and torch.equal(x, y[:, :d]) and not y[:, d:].any(), f"get_random_projections layer {i}"
    assert A.anchored_call_served(8, 5) == Bt.anchored_call_served(8, 5)
    if Bt.anchored_call_served(8, 5):
        nb_ids = dev(rng.randint(0, N, (8, 5)).astype(np.int64))
        a1, a2 = rng.randint(1, N, 8).astype(np.int64), rng.randint(1, N, 8).astype(np.int64)
        with torch.no_grad():
            assert torch.equal(A.get_pair_wise_feature_anchored(nb_ids, a1, a2), Bt.get_pair_wise_feature_anchored(nb_ids, a1, a2))
    # streams: per batch with negatives, windowed without; a backup between them
    s = sl(3, 7)
    got = [rp.run_stream(dev(src[s]), dev(dst[s]), dev(neg[s]), dev(t[s]), B, schedule="batch") for rp in (A, Bt)]
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), "run_stream batch"
    assert A.last_stream_schedule == Bt.last_stream_schedule == "batch"
    _same_layers(A, Bt, d, "after the per-batch stream")
    bk = [rp.backup_random_projections() for rp in (A, Bt)]
    assert all(tuple(x.shape) == (N, d) for x in bk[0][1])
    s = sl(7, 12)
    got = [rp.run_stream(dev(src[s]), dev(dst[s]), None, dev(t[s]), B, schedule="windowed") for rp in (A, Bt)]
    assert torch.equal(got[0][0], got[1][0]) and got[0][1] is None and got[1][1] is None, "run_stream windowed"
    assert A.last_stream_schedule == Bt.last_stream_schedule == ("batch" if exact else "windowed")
    _same_layers(A, Bt, d, "after the windowed stream")
    # reload, then the other two combinations
    for rp, saved in zip((A, Bt), bk):
        rp.reload_random_projections(saved)
    _same_layers(A, Bt, d, "after reload")
    got = [rp.run_stream(dev(src[s]), dev(dst[s]), dev(neg[s]), dev(t[s]), B, schedule="windowed") for rp in (A, Bt)]
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), "run_stream windowed with negatives"
    s2 = slice(0, 2 * B)
    got = [rp.run_stream(dev(src[s2]), dev(dst[s2]), None, dev(t[s2] + 3e5), B, schedule="batch") for rp in (A, Bt)]
    assert torch.equal(got[0][0], got[1][0]), "run_stream batch without negatives"
    _same_layers(A, Bt, d, "at the end")
    assert float(A.now_time) == float(Bt.now_time)
    A.check_device_errors()
    Bt.check_device_errors()


# ---------------------------------------------------------------------------------------------------------
# 2. against the oracle
# ---------------------------------------------------------------------------------------------------------
def _oracle_walk(P0, L, src, dst, t, neg, runs):
    """One pass of the oracle over the stream; `runs`: {name: (feat_pos [E, F], feat_neg [E, F] or None)} checked batch by batch on
    the pre-batch state.  Returns the final oracle state."""
    st = O.OracleState(P0, L, LAM, T0)
    for b0 in range(0, len(src), B):
        s = slice(b0, min(b0 + B, len(src)))
        for name, (fp, fn) in runs.items():
            _assert_features(fp[s], st, src[s], dst[s], f"{name} pos batch {b0 // B}")
            if fn is not None:
                _assert_features(fn[s], st, src[s], neg[s], f"{name} neg batch {b0 // B}")
        O.update(st, src[s], dst[s], t[s])
    return st


@pytest.mark.parametrize("d", [110, 75])
def test_against_the_oracle(d):
    _need_gpu()
    L = 3
    src, dst, t, neg = _stream(3)
    A = _mk(d, L, padded=True)
    P0 = A.random_projections[0].detach().cpu().numpy().copy()
    dev = lambda x: torch.from_numpy(x).to(DEV)
    fp, fn = A.run_stream(dev(src), dev(dst), dev(neg), dev(t), B, schedule="windowed")
    assert A.last_stream_schedule == "windowed"
    layers_stream = _layers(A)
    A.reset_random_projections()
    A.random_projections[0].data.copy_(torch.from_numpy(P0))
    lp, ln = [], []
    for b0 in range(0, E, B):
        s = slice(b0, min(b0 + B, E))
        lp.append(A.pair_gram(src[s], dst[s]))
        ln.append(A.pair_gram(src[s], neg[s]))
        A.update(src[s], dst[s], t[s])
    layers_loop = _layers(A)
    st = _oracle_walk(P0, L, src, dst, t, neg, {"windowed stream": (fp.cpu().numpy(), fn.cpu().numpy()),
                                                "per-call loop": (torch.cat(lp).cpu().numpy(), torch.cat(ln).cpu().numpy())})
    want = np.stack(st.P[1:])
    assert layers_stream.shape == (L, N, d)
    _assert_state(layers_stream, want, 1e-4, "windowed stream")
    _assert_state(layers_loop, want, 1e-4, "per-call loop")
    assert float(A.now_time) == float(st.now_time)


# ---------------------------------------------------------------------------------------------------------
# 3. schedule
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [110, 130, 150])
def test_auto_schedule_takes_the_windowed_pipeline_only_with_the_switch(d):
    _need_gpu()
    from tpnet_amd import _lib
    L, b, nb = 3, 8, 28
    src, dst, t, _ = _stream(4, nb * b)
    dev = lambda x: torch.from_numpy(x).to(DEV)
    lib = _lib.load()
    for padded, want in ((True, "windowed"), (False, "batch")):
        rp = _mk(d, L, padded=padded)
        assert rp.last_stream_schedule is None
        rp.run_stream(dev(src), dev(dst), None, dev(t), b, schedule="auto")
        assert rp.last_stream_schedule == want
        ws = rp._eng["ws"].numel()
        assert rp.engine_dim == ((d + 3) // 4 * 4 if padded else d)
        assert (lib.tpnet_stream_schedule(N, rp.engine_dim, L, nb * b, b, 0, ws) == 1) == (want == "windowed")
        assert lib.tpnet_stream_schedule(N, d, L, nb * b, b, 0, ws) == 0


# ---------------------------------------------------------------------------------------------------------
# 4. surface
# ---------------------------------------------------------------------------------------------------------
def test_surface_checkpoints_and_copies():
    _need_gpu()
    d, L = 110, 3
    src, dst, t, _ = _stream(5)
    A = _mk(d, L, padded=True)
    P0 = A.random_projections[0].detach().cpu()
    U = _mk(d, L, P0=P0)
    upd = lambda rp, b: rp.update(src[b * B:(b + 1) * B], dst[b * B:(b + 1) * B], t[b * B:(b + 1) * B])
    for b in range(3):
        upd(A, b)
        upd(U, b)
    sa, su = A.state_dict(), U.state_dict()
    assert list(sa.keys()) == list(su.keys())
    assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in su.values()]
    assert tuple(sa["random_projections.1"].shape) == (N, d)
    # padded -> unpadded -> padded, with further updates at each stop, against the oracle
    U2 = _mk(d, L)
    U2.load_state_dict(copy.deepcopy(sa))
    for b in range(3, 6):
        upd(U2, b)
    A2 = _mk(d, L, padded=True)
    A2.load_state_dict(copy.deepcopy(U2.state_dict()))
    for b in range(6, 9):
        upd(A2, b)
    st = O.OracleState(P0.numpy(), L, LAM, T0)
    for b in range(9):
        O.update(st, src[b * B:(b + 1) * B], dst[b * B:(b + 1) * B], t[b * B:(b + 1) * B])
    _assert_state(_layers(A2), np.stack(st.P[1:]), 1e-4, "padded -> unpadded -> padded")
    assert float(A2.now_time) == float(st.now_time)
    u, v = src[:40], dst[40:80]
    _assert_features(A2.pair_gram(u, v).cpu().numpy(), st, u, v, "after the round trip")
    # copies keep the state
    before = [A2.random_projections[i].detach().clone() for i in range(L + 1)]
    saved = (torch.tensor(float(t[9 * B - 1]), dtype=torch.float64, device=DEV), before[1:])
    A2.reload_random_projections(saved)                                   # (every copy below starts from an import of these layers)
    upd(A2, 9)
    after9 = [A2.random_projections[i].detach().clone() for i in range(L + 1)]
    A2.reload_random_projections(saved)
    for name, c in (("deepcopy", copy.deepcopy(A2)), ("pickle", pickle.loads(pickle.dumps(A2))), ("cpu/cuda", A2.cpu().cuda())):
        assert c.padded_rows is True and c.engine_dim == 112
        for i in range(L + 1):
            assert tuple(c.random_projections[i].shape) == (N, d)
            assert torch.equal(c.random_projections[i].detach().to(DEV), before[i]), f"{name}: layer {i}"
        upd(c, 9)                                                         # (and go on from it as the original does)
        for i in range(L + 1):
            assert torch.equal(c.random_projections[i].detach().to(DEV), after9[i]), f"{name}: layer {i} after an update"


# ---------------------------------------------------------------------------------------------------------
# 5. the wide copy of P[0] follows P[0]
# ---------------------------------------------------------------------------------------------------------
def test_wide_copy_of_p0_is_rebuilt_when_p0_changes():
    _need_gpu()
    d, L = 110, 3
    src, dst, t, _ = _stream(6)
    A, Bt, ed = _twins(d, L)
    rng = np.random.RandomState(7)
    u, v = rng.randint(0, N, 50).astype(np.int64), rng.randint(0, N, 50).astype(np.int64)
    upd = lambda b: [rp.update(src[b * B:(b + 1) * B], dst[b * B:(b + 1) * B], t[b * B:(b + 1) * B]) for rp in (A, Bt)]
    same = lambda what: (A.get_pair_wise_feature(u, v), Bt.get_pair_wise_feature(u, v))
    upd(0)
    x, y = same("start")
    assert torch.equal(x, y)
    # a write through .data of entry 0: neither pointer nor version counter shows it
    X = torch.randn(N, d, device=DEV) / 10
    A.random_projections[0].data.copy_(X)
    Bt.random_projections[0].data[:, :d].copy_(X)
    x2, y2 = same("injected")
    assert torch.equal(x2, y2) and not torch.equal(x2, x), "after .data.copy_"
    upd(1)
    # reset, then such an injection (what callers.run_epoch's after_reset hook does)
    X2 = torch.randn(N, d, device=DEV) / 10
    A.reset_random_projections()
    Bt.reset_random_projections()
    A.random_projections[0].data.copy_(X2)
    Bt.random_projections[0].data.copy_(_wide(X2, ed))
    x3, y3 = same("reset + injected")
    assert torch.equal(x3, y3), "after reset + injection"
    upd(0)
    x4, y4 = same("reset + injected + update")
    assert torch.equal(x4, y4) and not torch.equal(x4, x3)
    # a reset alone redraws P[0]: the kernels must read the new draw
    A.reset_random_projections()
    Bt.random_projections[0].data.copy_(_wide(A._plist()[0].detach(), ed))       # (_plist: entry 0 is NOT handed out here)
    Bt.reload_random_projections((torch.tensor(T0, dtype=torch.float64, device=DEV), [torch.zeros(N, ed, device=DEV) for _ in range(L)]))
    x5, y5 = same("reset")
    assert torch.equal(x5, y5), "after reset"
    # load_state_dict
    Cm = _mk(d, L)
    for b in range(2):
        Cm.update(src[b * B:(b + 1) * B], dst[b * B:(b + 1) * B], t[b * B:(b + 1) * B])
    sd = Cm.state_dict()
    A.load_state_dict(copy.deepcopy(sd))
    Bt.load_state_dict({k: (_wide(val, ed) if k.startswith("random_projections.") else val.clone()) for k, val in sd.items()})
    x6, y6 = same("load_state_dict")
    assert torch.equal(x6, y6) and not torch.equal(x6, x5), "after load_state_dict"
    _same_layers(A, Bt, d, "after load_state_dict")


# ---------------------------------------------------------------------------------------------------------
# 6. toggling on a live instance
# ---------------------------------------------------------------------------------------------------------
def test_toggle_mid_stream_loses_nothing():
    _need_gpu()
    d, L = 110, 3
    src, dst, t, neg = _stream(8)
    rp = _mk(d, L)
    P0 = rp.random_projections[0].detach().cpu().numpy().copy()
    st = O.OracleState(P0, L, LAM, T0)
    dev = lambda x: torch.from_numpy(x).to(DEV)
    s4 = slice(0, 4 * B)
    call = rp.prepare_stream(dev(src[s4]), dev(dst[s4]), None, dev(t[s4]), B)
    b = 0
    for padded in (False, True, False):
        rp.padded_rows = padded
        assert rp.engine_dim == (112 if padded else 110)
        for _ in range(3):
            s = slice(b * B, (b + 1) * B)
            _assert_features(rp.pair_gram(src[s], neg[s]).cpu().numpy(), st, src[s], neg[s], f"batch {b}, padded {padded}")
            rp.update(src[s], dst[s], t[s])
            O.update(st, src[s], dst[s], t[s])
            b += 1
        assert rp._eng["d"] == rp.engine_dim
    _assert_state(_layers(rp), np.stack(st.P[1:]), 1e-4, "off, on, off")
    assert float(rp.now_time) == float(st.now_time)
    with pytest.raises(RuntimeError, match="prepare it again"):
        call()
    rp.padded_rows = False                                                # (no change of width: nothing is dropped)
    eng = rp._eng
    rp.update(src[:B], dst[:B], t[:B] + 3e5)
    assert rp._eng is eng


# ---------------------------------------------------------------------------------------------------------
# 7. the C entry points
# ---------------------------------------------------------------------------------------------------------
SENT = float(np.float32(-12345.5))


def _raw_state(n, d, L, lib):
    from tpnet_amd import _lib
    q = torch.full((lib.tpnet_q_bytes(n, d, L) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    meta = torch.zeros(lib.tpnet_meta_bytes(n), dtype=torch.uint8, device=DEV)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    p0 = torch.zeros((n, d), dtype=torch.float32, device=DEV)
    st = _lib.State(p0=p0.data_ptr(), q=q.data_ptr(), meta=meta.data_ptr(), N=n, d=d, L=L, err=err.data_ptr())
    return st, (q, meta, err, p0)


@pytest.mark.parametrize("n,ld,d", [(5, 6, 8), (5, 7, 8), (3, 110, 112)])
@pytest.mark.parametrize("guard", [2, 1])          # narrow rows that start 8-byte aligned / only 4-byte aligned
def test_import_then_export_returns_the_input_bits(hip_lib, n, ld, d, guard):
    _need_gpu()
    from tpnet_amd import _lib
    L = 2
    st, keep = _raw_state(n, d, L, hip_lib)
    q = keep[0]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.RandomState(n * 1000 + ld)
    src_bufs, layers = [], []
    for i in range(L):
        x = rng.standard_normal((n, ld)).astype(np.float32)
        x[0, 0], x[n - 1, ld - 1] = -0.0, np.float32(1e-40)               # a negative zero, a denormal
        buf = torch.full((guard + n * ld + 8,), SENT, dtype=torch.float32, device=DEV)
        buf[guard: guard + n * ld] = torch.from_numpy(x.reshape(-1)).to(DEV)
        assert buf.data_ptr() % 16 == 0
        src_bufs.append(buf)
        layers.append(x)
    ptrs = (C.c_void_p * L)(*[b.data_ptr() + 4 * guard for b in src_bufs])
    _lib.check(hip_lib.tpnet_import_layers_ld(C.byref(st), ptrs, ld, 3.0, stream), "import_layers_ld")
    qv = q.view(2, n, L, d)
    for i in range(L):
        assert np.array_equal(qv[0, :, i, :ld].cpu().numpy().view(np.uint32), layers[i].view(np.uint32)), "copy 0 holds the input bits"
    assert not qv[:, :, :, ld:].cpu().numpy().view(np.uint32).any(), "pad columns of both copies are +0.0"
    assert torch.isnan(qv[1, :, :, :ld]).all(), "copy 1 is written in its pad columns only"
    meta = keep[1].cpu().numpy().view(np.dtype([("ver", "<u4"), ("pad0", "<u4"), ("tref", "<f8", 2), ("pad1", "<u8")]))
    assert (meta["ver"] == 0).all() and (meta["tref"] == 3.0).all()
    outs = [torch.full((guard + n * ld + 8,), SENT, dtype=torch.float32, device=DEV) for _ in range(L)]
    optrs = (C.c_void_p * L)(*[o.data_ptr() + 4 * guard for o in outs])
    _lib.check(hip_lib.tpnet_export_layers_ld(C.byref(st), optrs, ld, 3.0, 0.25, stream), "export_layers_ld")
    for i in range(L):
        o = outs[i].cpu().numpy()
        assert np.array_equal(o[guard: guard + n * ld].view(np.uint32), layers[i].reshape(-1).view(np.uint32)), "export returns the bits"
        assert (o[:guard] == np.float32(SENT)).all() and (o[guard + n * ld:] == np.float32(SENT)).all(), "nothing outside the rows"
    # the wide copy of a narrow table, and the gather with narrow output rows
    wide = torch.full((n * d + 8,), SENT, dtype=torch.float32, device=DEV)
    _lib.check(hip_lib.tpnet_pad_rows(ptrs[0], ld, wide.data_ptr(), d, n, stream), "pad_rows")
    w = wide.cpu().numpy()
    assert np.array_equal(w[:n * d].reshape(n, d)[:, :ld].view(np.uint32), layers[0].view(np.uint32))
    assert not w[:n * d].reshape(n, d)[:, ld:].view(np.uint32).any() and (w[n * d:] == np.float32(SENT)).all()
    st.p0 = wide.data_ptr()
    ids = torch.tensor([n - 1, 0, n - 1], dtype=torch.int64, device=DEV)
    out = torch.full((guard + (L + 1) * 3 * ld + 8,), SENT, dtype=torch.float32, device=DEV)
    _lib.check(hip_lib.tpnet_gather_rows_ld(C.byref(st), ids.data_ptr(), 3, 3.0, 0.25, ld, out.data_ptr() + 4 * guard, stream),
               "gather_rows_ld")
    o = out.cpu().numpy()
    got = o[guard: guard + (L + 1) * 3 * ld].reshape(L + 1, 3, ld)
    want = np.stack([layers[0][[n - 1, 0, n - 1]]] + [layers[i][[n - 1, 0, n - 1]] for i in range(L)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (o[:guard] == np.float32(SENT)).all() and (o[guard + (L + 1) * 3 * ld:] == np.float32(SENT)).all()
    _lib.check(hip_lib.tpnet_check_errors(C.byref(st), stream), "check_errors")


def test_bad_arguments_launch_nothing(hip_lib):
    """Each documented bad argument: TPNET_ERR_BAD_ARG, and the buffers a launch would have written keep their contents."""
    _need_gpu()
    n, ld, d, L = 5, 6, 8, 2
    st, keep = _raw_state(n, d, L, hip_lib)
    q = keep[0]
    lay = [torch.full((n * ld + 4,), SENT, dtype=torch.float32, device=DEV) for _ in range(L)]
    ptrs = (C.c_void_p * L)(*[x.data_ptr() for x in lay])
    null1 = (C.c_void_p * L)(lay[0].data_ptr(), None)
    ref = lambda: C.byref(st)
    imp, exp_, pad, gat = (hip_lib.tpnet_import_layers_ld, hip_lib.tpnet_export_layers_ld, hip_lib.tpnet_pad_rows,
                           hip_lib.tpnet_gather_rows_ld)
    ids = torch.zeros(2, dtype=torch.int64, device=DEV)
    out = torch.full((64,), SENT, dtype=torch.float32, device=DEV)
    calls = []
    for bad_ld in (0, d + 1, -3):
        calls += [imp(ref(), ptrs, bad_ld, 0.0, None), exp_(ref(), ptrs, bad_ld, 0.0, 0.0, None),
                  gat(ref(), ids.data_ptr(), 2, 0.0, 0.0, bad_ld, out.data_ptr(), None)]
    calls += [imp(None, ptrs, ld, 0.0, None), imp(ref(), None, ld, 0.0, None), imp(ref(), null1, ld, 0.0, None),
              exp_(None, ptrs, ld, 0.0, 0.0, None), exp_(ref(), None, ld, 0.0, 0.0, None), exp_(ref(), null1, ld, 0.0, 0.0, None),
              gat(ref(), None, 2, 0.0, 0.0, ld, out.data_ptr(), None), gat(ref(), ids.data_ptr(), 2, 0.0, 0.0, ld, None, None),
              pad(None, ld, out.data_ptr(), d, n, None), pad(lay[0].data_ptr(), ld, None, d, n, None),
              pad(lay[0].data_ptr(), 0, out.data_ptr(), d, n, None), pad(lay[0].data_ptr(), d + 1, out.data_ptr(), d, n, None),
              pad(lay[0].data_ptr(), ld, out.data_ptr() + 4, d, n, None), pad(lay[0].data_ptr(), ld, out.data_ptr(), 6, n, None)]
    st.q = q.data_ptr() + 8                                               # a wide side that is not 16-byte aligned
    calls += [imp(ref(), ptrs, ld, 0.0, None), exp_(ref(), ptrs, ld, 0.0, 0.0, None),
              gat(ref(), ids.data_ptr(), 2, 0.0, 0.0, ld, out.data_ptr(), None)]
    st.q = q.data_ptr()
    st.p0 = keep[3].data_ptr() + 4
    calls += [gat(ref(), ids.data_ptr(), 2, 0.0, 0.0, ld, out.data_ptr(), None)]
    st.p0 = keep[3].data_ptr()
    st.d = 6                                                              # wide rows that are no whole 16-byte vectors
    calls += [imp(ref(), ptrs, ld, 0.0, None), exp_(ref(), ptrs, ld, 0.0, 0.0, None)]
    assert calls == [-1] * len(calls), calls
    torch.cuda.synchronize()
    assert torch.isnan(q).all() and all((x == SENT).all() for x in lay) and (out == SENT).all()
