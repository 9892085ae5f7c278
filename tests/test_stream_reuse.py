"""Plan reuse of run_stream against the oracle (run with -m gpu on an MI355X; the last tests of the file need no GPU).

run_stream skips most of its work by replaying the plan a stream left in the workspace (tpnet_run_stream_tagged), and the row
shard keeps a stream's exchange plan and its kernels' plan across calls.  A replay is right only for the very arrays the plan was
built from.  An address and torch's version counter do not name them: a freed block goes to the next tensor of its size, whose
counter starts at 0 again.  These tests build exactly that collision -- a stream's one allocation freed and a stream of other
contents built in the same block -- and check every result against the oracle (tests/test_gpu_parity.py's tolerances) and,
where the code promises bits, against a cold module."""
import numpy as np
import pytest
import torch

from oracle import tpnet_oracle as O
from test_gpu_parity import DEV, _assert_features, _assert_state, _layers, _module, _need_gpu, _random_stream

T0 = 1.0e6                     # every stream's times lie in [T0, T0 + span] (_random_stream): one beginning time for all


def _host_stream(seed, N, E):
    """src / dst / neg / t of one stream in ONE host int64 array of 4 E (t as float64 bits), and the four arrays."""
    src, dst, neg, t = _random_stream(np.random.RandomState(seed), N, E, 4.0e5)
    host = np.concatenate([src, dst, neg, t.view(np.int64)])
    return host, (src, dst, neg, t)


class _Stream:
    """A stream in ONE device allocation (torch.from_numpy(host).to(dev): a new tensor, _version 0) and its four views."""

    def __init__(self, host, E):
        self.buf = torch.from_numpy(host).to(DEV)
        self.src, self.dst, self.neg = self.buf[:E], self.buf[E:2 * E], self.buf[2 * E:3 * E]
        self.t = self.buf[3 * E:].view(torch.float64)

    def args(self):
        return self.src, self.dst, self.neg, self.t


def _check_oracle(P0, L, lam, arrays, B, fp, fn, layers, what):
    """All batches' features (readout on the pre-batch state) and the final state against the oracle loop."""
    src, dst, neg, t = arrays
    E = len(src)
    st = O.OracleState(P0, L, lam, T0)
    for b in range(0, E, B):
        s = slice(b, min(b + B, E))
        if fp is not None:
            _assert_features(fp[s], st, src[s], dst[s], f"{what}: pos batch {b // B}")
        if fn is not None:
            _assert_features(fn[s], st, src[s], neg[s], f"{what}: neg batch {b // B}")
        O.update(st, src[s], dst[s], t[s])
    _assert_state(layers, np.stack(st.P[1:]), 1e-4, f"{what}: final state")


def _epoch(rp, P0, run):
    """train_link_prediction.py:234-253: reset the projections (P[0] set back to P0), then one stream call."""
    rp.reset_random_projections()
    rp.random_projections[0].data.copy_(torch.from_numpy(P0))
    fp, fn = run()
    return fp.clone(), fn.clone(), _layers(rp), rp.last_stream_replayed


def _cold(N, d, L, lam, P0, args, B, **kw):
    """The stream on a fresh module with replay off: the bits a plan built for it gives."""
    c = _module(N, d, L, lam, T0, P0=P0)
    fp, fn = c.run_stream(*args, B, replay=False, **kw)
    return fp.clone(), fn.clone(), _layers(c)


def _assert_bits(got, want, what):
    assert torch.equal(got[0], want[0]), f"{what}: (src, dst) features differ from a cold run"
    assert torch.equal(got[1], want[1]), f"{what}: (src, neg) features differ from a cold run"
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"{what}: state differs from a cold run")


# ---------------------------------------------------------------------------------------------------------
# A. a stream built in the block a freed stream left
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("schedule,N,d,L,B,nb,per,prepared",
                         [("windowed", 300, 64, 3, 40, 9, None, False),        # one chunk, windowed
                          ("batch", 300, 64, 3, 40, 6, None, False),           # one chunk, per batch (stream_sig alone decides)
                          ("windowed", 3000, 64, 2, 200, 150, 70, False),      # three chunks, their plans side by side
                          ("windowed", 300, 64, 3, 40, 9, None, True)])        # through prepare_stream: a new handle for B
def test_stream_in_a_recycled_block_is_not_replayed(schedule, N, d, L, B, nb, per, prepared):
    """reset, stream A, A freed, stream B (same length, other ids and times) built in A's block -- same address, _version 0 --,
    reset, stream B: B is planned afresh, gives a cold module's bits and the oracle's values, and replays from then on."""
    _need_gpu()
    lam = 2e-6
    E = nb * B - B // 3
    P0 = (np.random.RandomState(11).randn(N, d) / np.sqrt(d)).astype(np.float32)
    host_a, arr_a = _host_stream(1, N, E)
    host_b, arr_b = _host_stream(2, N, E)
    rp = _module(N, d, L, lam, T0, P0=P0)
    if per is not None:
        rp.stream_log_cap_bytes = per * B * 2 * L * d * 4

    NG = (2 * L + 2) ** 2
    outs = (torch.empty((E, NG), device=DEV), torch.empty((E, NG), device=DEV))   # (held here: dropping a handle frees its block only)

    def runner(s):
        if prepared:
            call = rp.prepare_stream(*s.args(), B, schedule=schedule, out_pos=outs[0], out_neg=outs[1])
            return call, call
        return None, lambda: rp.run_stream(*s.args(), B, schedule=schedule)

    a = _Stream(host_a, E)
    ptr = a.buf.data_ptr()
    call, run = runner(a)
    ea1 = _epoch(rp, P0, run)
    ea2 = _epoch(rp, P0, run)
    assert not ea1[3] and ea2[3], "the same live stream run again must replay its plan"
    _assert_bits(ea2, ea1, "A replayed")
    if per is not None:
        from tpnet_amd import _lib
        assert rp._eng["ws"].numel() < _lib.load().tpnet_stream_workspace_bytes(N, d, L, E, B)      # (several chunks)
    del a, call, run                                      # the last references to A's block: it goes back to the allocator ...
    b = _Stream(host_b, E)                                # ... and is the next block of its size
    assert b.buf.data_ptr() == ptr and b.buf._version == 0, "precondition: B is built in A's block"
    call, run = runner(b)
    eb1 = _epoch(rp, P0, run)
    assert not eb1[3], "a stream built in a freed stream's block replayed that stream's plan"
    _assert_bits(eb1, _cold(N, d, L, lam, P0, b.args(), B, schedule=schedule), "B")
    _check_oracle(P0, L, lam, arr_b, B, eb1[0].cpu().numpy(), eb1[1].cpu().numpy(), eb1[2], "B")
    eb2 = _epoch(rp, P0, run)
    assert eb2[3], "B run again (the same live tensors) must replay"
    _assert_bits(eb2, eb1, "B replayed")


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["windowed", "batch"])
def test_a_prepared_call_that_stays_alive_keeps_replaying(schedule):
    """examples/epoch_stream.py's loop: ONE prepared call, a new `neg` written into the tensor it holds every epoch -- replayed in
    every epoch after the first, the bits of a cold run with the same negatives, the oracle's values."""
    _need_gpu()
    N, d, L, B, lam, nb = 300, 64, 3, 40, 2e-6, 9
    E = nb * B - B // 3
    P0 = (np.random.RandomState(12).randn(N, d) / np.sqrt(d)).astype(np.float32)
    host, arr = _host_stream(3, N, E)
    s = _Stream(host, E)
    held_neg = s.neg.clone()                  # (its own allocation: a write into a view of the stream's block is a write to src / t)
    rp = _module(N, d, L, lam, T0, P0=P0)
    call = rp.prepare_stream(s.src, s.dst, held_neg, s.t, B, schedule=schedule, t_end=float(arr[3][-1]))
    negs = [arr[2]] + [np.random.RandomState(40 + k).randint(0, N, E).astype(np.int64) for k in range(2)]
    for k, neg in enumerate(negs):
        call.neg.copy_(torch.from_numpy(neg))
        e = _epoch(rp, P0, call)
        assert e[3] == (k > 0), f"epoch {k}: replayed = {e[3]}"
        _assert_bits(e, _cold(N, d, L, lam, P0, (s.src, s.dst, held_neg, s.t), B, schedule=schedule), f"epoch {k}")
        if k < 2:
            _check_oracle(P0, L, lam, (arr[0], arr[1], neg, arr[3]), B, e[0].cpu().numpy(), e[1].cpu().numpy(), e[2],
                          f"epoch {k}")


def _shard_worker(rank, world, port, cfg, q):
    """One rank of a two-rank row shard (gloo, both on cuda:0), per-batch exchange: an epoch with negatives A, A's negatives
    freed, an epoch with negatives B built in their block -- src / dst / t the same live tensors throughout."""
    import os
    import torch.distributed as dist
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        from tpnet_amd.sharded import ShardedStreamRunner
        N, d, L, E, B, lam, seed = cfg
        dev = torch.device(DEV)
        src, dst, neg_a, t = _random_stream(np.random.RandomState(seed), N, E, 4.0e5)
        neg_b = np.random.RandomState(seed + 1).randint(0, N, E).astype(np.int64)
        P0 = torch.from_numpy((np.random.RandomState(seed + 2).randn(N, d) / np.sqrt(d)).astype(np.float32))
        runner = ShardedStreamRunner.create(node_num=N, edge_num=E, dim=d, num_layer=L, time_decay_weight=lam, device=dev,
                                            beginning_time=np.float64(T0), halo_rows=3 * B, seed=rank)
        runner.exchange = "targeted"
        D = lambda x: torch.from_numpy(x).to(dev)
        ds, dd, dt = D(src), D(dst), D(t)

        def epoch(neg):
            runner.rp.reset_random_projections()
            runner.set_full_p0(P0)
            fp, fn = runner.run_stream(ds, dd, neg, dt, B)
            return fp.cpu().numpy(), fn.cpu().numpy(), runner.last_stream_windowed

        neg = D(neg_a)
        ptr = neg.data_ptr()
        ea = epoch(neg)
        del neg
        neg = D(neg_b)
        recycled = neg.data_ptr() == ptr and neg._version == 0
        eb = epoch(neg)
        layers = runner.gather_full_layers().cpu().numpy()
        q.put((rank, recycled, ea[2] or eb[2], eb[0], eb[1], layers[1:]))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_row_shard_does_not_reuse_the_exchange_plan_of_freed_negatives():
    """Two gloo ranks sharing cuda:0 on the per-batch shard (7 batches), the same src / dst / t twice and a fresh `neg` of other
    contents in the block the first one left: the second call relabels the new negatives (the exchange plan of the first holds
    the old ones) -- out_neg equals a single-GPU run and the oracle, and so do out_pos and the state."""
    _need_gpu()
    import socket
    import torch.multiprocessing as mp
    cfg = (211, 64, 3, 7 * 50 - 13, 50, 2e-6, 5)
    N, d, L, E, B, lam, seed = cfg
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, cfg, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda m: m[0])
    for p in procs:
        p.join(timeout=120)
    assert all(r[1] for r in res), "precondition: the second neg is built in the first one's block on both ranks"
    assert not any(r[2] for r in res), "the stream took the windowed shard: the per-batch shard is under test"
    src, dst, _, t = _random_stream(np.random.RandomState(seed), N, E, 4.0e5)
    neg_b = np.random.RandomState(seed + 1).randint(0, N, E).astype(np.int64)
    P0 = (np.random.RandomState(seed + 2).randn(N, d) / np.sqrt(d)).astype(np.float32)
    one = _module(N, d, L, lam, T0, P0=P0)
    D = lambda x: torch.from_numpy(x).to(DEV)
    rfp, rfn = one.run_stream(D(src), D(dst), D(neg_b), D(t), B, schedule="batch")
    for _, _, _, fp, fn, layers in res:
        # (the shard's features: the single-GPU tolerance of tests/test_sharded.py)
        assert np.abs(fn - rfn.cpu().numpy()).max() < 2e-4 and np.abs(fp - rfp.cpu().numpy()).max() < 2e-4
        _check_oracle(P0, L, lam, (src, dst, neg_b, t), B, fp, fn, layers, "row shard, negatives B")


@pytest.mark.gpu
def test_row_shard_plans_again_after_the_module_planned_in_its_workspace():
    """One rank on the per-batch shard (no exchange), then the shard's module runs a stream of its own in the same workspace
    (rp.run_stream keeps its plan there), then the shard runs its stream again from the same clock: its kernels' plan
    is built again -- the bits of the first call and the oracle's values."""
    _need_gpu()
    from tpnet_amd.sharded import ShardedStreamRunner
    N, d, L, B, lam, nb = 300, 64, 3, 40, 2e-6, 9
    E = nb * B - B // 3
    P0 = (np.random.RandomState(13).randn(N, d) / np.sqrt(d)).astype(np.float32)
    host_s, arr_s = _host_stream(4, N, E)
    host_o, _ = _host_stream(5, N, E)
    runner = ShardedStreamRunner.create(node_num=N, edge_num=E, dim=d, num_layer=L, time_decay_weight=lam, device=torch.device(DEV),
                                        beginning_time=np.float64(T0), halo_rows=3 * B, world=1, rank=0)
    runner.exchange = "targeted"
    runner.single_rank_pipeline = False            # (the per-batch shard's own plan, tpnet_plan_stream, not the module's schedules)
    rp = runner.rp
    rp.reserve_stream(E, B)                        # a workspace that serves both users as it is: nothing reallocates it
    s, o = _Stream(host_s, E), _Stream(host_o, E)

    def shard_epoch():
        rp.reset_random_projections()
        runner.set_full_p0(torch.from_numpy(P0))
        fp, fn = runner.run_stream(*s.args(), B)
        return fp.clone(), fn.clone(), _layers(rp)[:, :N]

    ws = rp._eng["ws"]
    e1 = shard_epoch()
    rp.reset_random_projections()
    rp.run_stream(*o.args(), B, schedule="windowed")
    assert rp._eng["ws"] is ws
    e2 = shard_epoch()
    assert rp._eng["ws"] is ws
    _assert_bits(e2, e1, "the shard after the module's own stream")
    _check_oracle(P0, L, lam, arr_s, B, e2[0].cpu().numpy(), e2[1].cpu().numpy(), e2[2], "row shard")


# ---------------------------------------------------------------------------------------------------------
# B. a bounded slice of tools/soak_sequence.py, against the oracle
# ---------------------------------------------------------------------------------------------------------
_SOAK = {"replayed": 0, "recreated": 0, "recreated_not_replayed": 0}


def _soak_sequence(seed, batch_replay):
    """One random sequence of module calls on one table -- stream slices whose lengths repeat (so that plans replay), restart,
    per-batch update and readout, backup and reload, an in-place touch of the stream, and "recreate": the stream's block freed
    and a stream of other contents built in it (then a restart: a new epoch) -- closed by two epochs of one slice, the second
    replayed.  The oracle's state is checked after every op and its features for every stream call.  batch_replay: every stream on
    the per-batch schedule, bit for bit against a module that plans every call (replay=False)."""
    rng = np.random.RandomState(seed)
    d, L, N = int(rng.choice([32, 64])), int(rng.choice([2, 3])), int(rng.choice([90, 400]))
    B = int(rng.choice([16, 50]))
    E = int(rng.randint(20, 40)) * B
    lam = 2e-6
    exact = batch_replay and seed % 3 == 0
    rtol = 5e-6 if exact else 1e-4
    host, arr = _host_stream(1000 + seed, N, E)
    P0 = (rng.randn(N, d) / np.sqrt(d)).astype(np.float32)
    a = _module(N, d, L, lam, T0, P0=P0, exact=exact)
    b = _module(N, d, L, lam, T0, P0=P0, exact=exact) if batch_replay else None
    mods = (a,) if b is None else (a, b)
    if not batch_replay and rng.rand() < 0.4:
        a.stream_log_cap_bytes = int(rng.randint(6, 16)) * B * 2 * L * d * 4
    st = O.OracleState(P0, L, lam, T0)
    v = dict(s=_Stream(host, E), arr=arr, pos=0, fresh=False)
    log = []

    def stream(n, sched):
        s, pos = v["s"], v["pos"]
        sl = slice(pos, pos + n)
        fp, fn = a.run_stream(s.src[sl], s.dst[sl], s.neg[sl], s.t[sl], B, schedule=sched)
        _SOAK["replayed"] += int(a.last_stream_replayed)
        log.append(f"stream[{pos}:{pos + n}] {sched}{' R' if a.last_stream_replayed else ''}")
        if v["fresh"]:
            _SOAK["recreated_not_replayed"] += int(not a.last_stream_replayed)
            assert not a.last_stream_replayed, f"seed {seed}: a recreated stream replayed the freed one's plan; ops {log}"
            v["fresh"] = False
        if b is not None:
            gp, gn = b.run_stream(s.src[sl], s.dst[sl], s.neg[sl], s.t[sl], B, schedule="batch", replay=False)
            assert torch.equal(fp, gp) and torch.equal(fn, gn), f"seed {seed}: features differ from a run without replay; ops {log}"
        fp, fn = fp.cpu().numpy(), fn.cpu().numpy()
        src, dst, neg, t = (x[sl] for x in v["arr"])
        for c in range(0, n, B):
            cs = slice(c, min(c + B, n))
            _assert_features(fp[cs], st, src[cs], dst[cs], f"seed {seed} {log[-1]} pos batch {c // B}")
            _assert_features(fn[cs], st, src[cs], neg[cs], f"seed {seed} {log[-1]} neg batch {c // B}")
            O.update(st, src[cs], dst[cs], t[cs])
        v["pos"] = pos + n

    def restart():
        for m in mods:
            m.reset_random_projections()
            m.random_projections[0].data.copy_(torch.from_numpy(P0))
        st.reset(P0)
        v["pos"] = 0

    def check():
        _assert_state(_layers(a), np.stack(st.P[1:]), rtol, f"seed {seed} after {log}")
        assert float(a.now_time.item()) == float(st.now_time)
        if b is not None:
            np.testing.assert_array_equal(_layers(a), _layers(b), err_msg=f"seed {seed}: state differs from a run without replay")

    saved, lengths = None, {}
    for _ in range(int(rng.randint(8, 16))):
        op = str(rng.choice(["stream", "stream", "stream", "restart", "restart", "update", "readout", "backup", "reload", "touch",
                             "recreate"]))
        pos = v["pos"]
        if op == "stream" and pos < E:
            n = max(1, min(E - pos, int(rng.randint(1, 30)) * B - int(rng.randint(0, B)) * int(rng.rand() < 0.3)))
            sched = "batch" if batch_replay else str(rng.choice(["auto", "windowed"]))
            if pos in lengths and rng.rand() < 0.85:
                n, sched = lengths[pos]                 # the slice an earlier epoch ran from here: a candidate for a replayed plan
            lengths[pos] = (n, sched)
            stream(n, sched)
        elif op in ("restart", "recreate"):
            if op == "recreate":
                ptr = v["s"].buf.data_ptr()
                host, v["arr"] = _host_stream(int(rng.randint(1 << 30)), N, E)
                del v["s"]
                v["s"] = _Stream(host, E)
                _SOAK["recreated"] += 1
                v["fresh"] = v["s"].buf.data_ptr() == ptr     # (a stream in the freed block: its first call must plan again)
            restart()
            saved = None
            log.append(op)
        elif op == "update" and pos + B <= E:
            sl = slice(pos, pos + B)
            for m in mods:
                m.update(v["arr"][0][sl], v["arr"][1][sl], v["arr"][3][sl])
            O.update(st, v["arr"][0][sl], v["arr"][1][sl], v["arr"][3][sl])
            v["pos"] = pos + B
            log.append("update")
        elif op == "readout":
            u, w = rng.randint(0, N, 300).astype(np.int64), rng.randint(0, N, 300).astype(np.int64)
            _assert_features(a.pair_gram(u, w).cpu().numpy(), st, u, w, f"seed {seed} readout")
            log.append("readout")
        elif op == "backup":
            saved = ([m.backup_random_projections() for m in mods], st.backup(), pos)
            log.append("backup")
        elif op == "reload" and saved is not None:
            for m, k in zip(mods, saved[0]):
                m.reload_random_projections(k)
            st.reload(saved[1])
            v["pos"] = saved[2]
            log.append("reload")
        elif op == "touch":
            k = int(rng.randint(0, E))
            v["s"].dst[k] = v["s"].dst[k]                # (an in-place write: torch bumps the version counter, the plan is not replayed)
            log.append("touch")
        else:
            continue
        check()
    # two epochs of one slice from a reset table on the per-batch schedule (one chunk): the second replays the first one's plan
    n = min(E, 8 * B - B // 2)
    for k in range(2):
        restart()
        stream(n, "batch")
        check()
        assert a.last_stream_replayed == (k == 1), f"seed {seed}: epoch {k} of the closing slice: replayed = {a.last_stream_replayed}"
    for m in mods:
        m.check_device_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(12))
def test_soak_sequence_against_the_oracle(seed):
    _need_gpu()
    _soak_sequence(seed, batch_replay=False)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(100, 104))
def test_soak_sequence_batch_replay_bit_for_bit(seed):
    _need_gpu()
    _soak_sequence(seed, batch_replay=True)


@pytest.mark.gpu
def test_soak_sequences_reached_what_they_claim():
    """The soak slices above replayed plans, and a stream recreated in a freed block was planned again (they run first: file
    order; run alone, this test runs the twelve sequences itself)."""
    _need_gpu()
    if _SOAK["recreated"] == 0:
        for seed in range(12):
            _soak_sequence(seed, batch_replay=False)
    assert _SOAK["replayed"] >= 1, _SOAK
    assert _SOAK["recreated_not_replayed"] >= 1, _SOAK

# ---------------------------------------------------------------------------------------------------------
# the reuse decisions on the host (no GPU): a recycled address is made exactly with one numpy array -- a tensor over it freed, a
# new one built over the same memory (same data_ptr, _version 0)
# ---------------------------------------------------------------------------------------------------------
def test_held_tensors_are_told_apart_from_a_recycled_address():
    from tpnet_amd.random_projection import _Held, _owners
    host = np.arange(12, dtype=np.int64)
    buf = torch.from_numpy(host)
    a, b = buf[:6], buf[6:]
    held = _Held(_owners(a, b, None))
    assert held.same(_owners(a, b, None))
    assert held.same(_owners(buf[:6], buf[6:], None))           # new views of the same live base: the same memory
    assert not held.same(_owners(a, b, a)) and not held.same(_owners(a, b.clone(), None))
    # (views of one base have one owner: which view sits where is the addresses' part of the key, _stream_sig / stream_sig)
    ptr = buf.data_ptr()
    del buf, a, b                                              # the owner is gone ...
    buf = torch.from_numpy(host)                               # ... and a new tensor has its address and version counter
    assert buf.data_ptr() == ptr and buf._version == 0
    assert not held.same(_owners(buf[:6], buf[6:], None))
    assert _Held(_owners(buf)).gen != held.gen


def test_row_shard_exchange_plan_is_made_again_for_negatives_in_a_recycled_block():
    """ShardedStreamRunner._exchange_plan on the host (rank 0 of two, torch plan): the same live tensors reuse the plan, a fresh
    `neg` of other contents over the memory of a freed one does not -- its relabelled negatives are the new ones."""
    from tpnet_amd.sharded import ShardedStreamRunner
    N, E, B = 97, 300, 40
    src, dst, neg_a, t = _random_stream(np.random.RandomState(3), N, E, 4.0e5)
    neg_b = np.random.RandomState(4).randint(0, N, E).astype(np.int64)

    class _Stub:                                   # stands in for the local module (no GPU in this tier)
        node_num = (N + 1) // 2 + 3 * B
        dropped = 0

        def _drop_plan(self):
            self.dropped += 1

    run = ShardedStreamRunner(_Stub(), N, 3 * B, world=2, rank=0)
    ts, tt = torch.from_numpy(src), torch.from_numpy(dst)
    tm = torch.from_numpy(t)
    host = neg_a.copy()
    neg = torch.from_numpy(host)
    R1, h1 = run._exchange_plan(ts, tt, neg, tm, B)
    R2, h2 = run._exchange_plan(ts, tt, neg, tm, B)
    assert R2 is R1 and h2 is h1 and run.rp.dropped == 1
    sig, ptr = run._stream_sig(ts, tt, neg, tm, E, B), neg.data_ptr()
    del neg
    host[:] = neg_b
    neg = torch.from_numpy(host)
    assert run._stream_sig(ts, tt, neg, tm, E, B) == sig and neg.data_ptr() == ptr    # what the address-only key saw
    R3, h3 = run._exchange_plan(ts, tt, neg, tm, B)
    assert R3 is not R1 and h3.gen != h1.gen and run.rp.dropped == 2
    want = run.relabel_targeted(ts, tt, torch.from_numpy(neg_b.copy()), B)
    assert torch.equal(R3["neg"], want["neg"]) and not torch.equal(R3["neg"], R1["neg"])
