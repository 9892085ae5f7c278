#!/usr/bin/env python3
"""TEST DRIVER (run in a process of its own by tests/test_sharded.py::test_windowed_shard_*): G row shards of one table in ONE
process on one GPU on the WINDOWED pipeline (csrc/wshard.hip).  Transports: "copy" = pack launches, plain copies between the
shards' buffers, unpack launches (the runner's phase methods wshard_begin / wshard_step / wshard_place_* one by one);
"loopback" = every shard a host thread with its own stream, tpnet_wshard_run with a communicator of the in-process RCCL
stand-in (tests/loopback/librccl_loopback.so).  Checks: the shards' features and tables equal the SINGLE-GPU run on the windowed schedule BIT FOR BIT (a log
slot travels as it is; the table starts from a reset, so the chunk's halo rows need no decay), and the two transports equal each
other.  Prints 'WSHARD OK ...' or raises."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import tpnet_amd                                           # noqa: E402
from tpnet_amd import _lib                                 # noqa: E402
from tpnet_amd.sharded import PH_LAUNCH, PH_PACK, PH_UNPACK, ShardedStreamRunner          # noqa: E402


def stream_of(seed, N, E, hubs=True):
    rng = np.random.RandomState(seed)
    src = rng.randint(1, N, E).astype(np.int64)
    dst = rng.randint(1, N, E).astype(np.int64)
    if hubs:
        src[rng.rand(E) < 0.15] = 3                        # hubs: long chains, rows every window sends both ways
        dst[rng.rand(E) < 0.10] = 4
        dst[rng.rand(E) < 0.05] = 3
    neg = rng.randint(0, N, E).astype(np.int64)
    t = np.sort(rng.uniform(0.0, 4.0e5, E))
    return src, dst, neg, t


def make_shards(G, N, d, L, E, B, lam, t0, P0, dev, halo):
    out = []
    for r in range(G):
        run = ShardedStreamRunner.create(node_num=N, edge_num=E, dim=d, num_layer=L, time_decay_weight=lam, device=dev,
                                         beginning_time=np.float64(t0), halo_rows=halo, seed=r, world=G, rank=r)
        run.set_full_p0(P0)
        out.append(run)
    return out


def full_layers(runs, N, L, d):
    dev = runs[0].rp._dev()
    G = len(runs)
    full = torch.empty((L + 1, N, d), dtype=torch.float32, device=dev)
    for r, run in enumerate(runs):
        rows = torch.stack(run.rp.get_random_projections(torch.arange(run.n_cap, dtype=torch.int64, device=dev)))
        n_own = (N - r + G - 1) // G
        full[:, r::G] = rows[:, :n_own]
    return full


def run_copy(runs, D, B, lib):
    """All shards in one thread on the runner's own phases, the rows moved by plain copies between the shards' buffers."""
    G = len(runs)
    ds, dd, dn, dt = D
    plans = [runs[r].plan_windowed(ds, dd, dn, dt, B) for r in range(G)]
    assert all(p is not None for p in plans), "the windowed shard declined"
    E, NG = plans[0]["E"], runs[0].rp.pair_wise_feature_dim
    outs = [(torch.zeros((E, NG), device=ds.device), torch.zeros((E, NG), device=ds.device)) for _ in range(G)]
    for r in range(G):
        runs[r].wshard_begin(plans[r])
    for r in range(G):                                     # shard r's halo rows <- every owner's packed rows
        assert all(int(plans[r]["chunk_cnt"][o]) == int(plans[o]["chunk_cnt"][o]) for o in range(G))
        runs[r].wshard_place_halo(plans[r], [(p["bufs"]["send_p0"], p["bufs"]["send_q"]) for p in plans])
    moved = 0
    sent = [(p["bufs"]["sendbuf"],) for p in plans]
    for j in range(plans[0]["nsteps"]):
        for r in range(G):
            runs[r].wshard_step(plans[r], j, PH_LAUNCH | PH_PACK, *outs[r])
        cnts = [p["send_cnt"][j] for p in plans]
        for r in range(G):
            assert plans[r]["recv_cnt"][j].tolist() == [int(c[r]) for c in cnts], (j, r)
            moved += runs[r].wshard_place_step(plans[r], sent, cnts)
        for r in range(G):
            runs[r].wshard_step(plans[r], j, PH_UNPACK, *outs[r])
    for r in range(G):
        runs[r].wshard_finish(plans[r])
        lib.tpnet_wshard_destroy(plans[r]["handle"])
        runs[r].rp._advanced(float(dt[-1].item()))
    torch.cuda.synchronize()
    return outs, moved, plans[0]["nsteps"]


def run_loopback(runs, D, B, lib, so):
    G = len(runs)
    ds, dd, dn, dt = D
    idbuf = (C.c_ubyte * 128)()
    assert lib.tpnet_rccl_unique_id(so, idbuf) == 0
    comms = []
    for r in range(G):
        h = C.c_void_p()
        assert lib.tpnet_rccl_comm_create(so, idbuf, G, r, C.byref(h)) == 0
        comms.append(h)
    dev = ds.device
    streams = [torch.cuda.Stream(dev) for _ in range(G)]
    torch.cuda.synchronize()
    res, failed = [None] * G, []

    def rank_thread(r):
        try:
            with torch.cuda.stream(streams[r]):
                res[r] = runs[r].run_stream_windowed(ds, dd, dn, dt, B, merge_outputs=False, comm=comms[r])
        except Exception as ex:            # noqa: BLE001
            failed.append((r, repr(ex)))
    ths = [threading.Thread(target=rank_thread, args=(r,)) for r in range(G)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=180)
    assert not failed and not any(th.is_alive() for th in ths), failed
    torch.cuda.synchronize()
    for r in range(G):
        assert res[r] is not None, "the windowed shard declined"
        assert lib.tpnet_rccl_comm_destroy(comms[r]) == 0
    return res


def main():
    cfgs = [(2, 211, 128, 3, 2000, 100, 2e-6), (3, 150, 64, 2, 1333, 50, 1e-6), (2, 3000, 128, 3, 1500, 60, 2e-6),
            (4, 400, 256, 3, 1700, 100, 1e-6), (2, 9228, 128, 3, 20 * 2000, 2000, 1e-6)]
    if os.environ.get("TPNET_WSHARD_ONE"):
        cfgs = cfgs[:1]
    if os.environ.get("TPNET_WSHARD_RANDOM"):              # "cases,seed": random shapes instead (a development soak, not the test)
        ncase, seed = (int(x) for x in os.environ["TPNET_WSHARD_RANDOM"].split(","))
        rg = np.random.RandomState(seed)
        cfgs = []
        while len(cfgs) < ncase:
            G = int(rg.choice([2, 2, 3, 4, 5, 8]))
            B = int(rg.choice([8, 37, 100, 257, 1000]))
            nbr = int(rg.randint(4, 40))
            N = int(rg.choice([60, 211, 1000, 5000]))
            d = int(rg.choice([32, 64, 128, 256, 120]))
            L = int(rg.choice([1, 2, 3, 3, 4]))
            if (N // G + N) * 12 > B * L * d * 4:          # (the dense planner must reach the shard's table: else the call is declined)
                continue
            cfgs.append((G, N, d, L, max(4 * B, nbr * B - int(rg.randint(0, B))), B, float(rg.choice([1e-6, 2e-6, 1e-7]))))
        print("random shapes:", cfgs, flush=True)
    lib = _lib.load()
    so = os.path.join(HERE, "librccl_loopback.so").encode()
    dev = torch.device("cuda:0")
    Dv = lambda x: torch.from_numpy(x).to(dev)
    summary = []
    for ci, (G, N, d, L, E, B, lam) in enumerate(cfgs):
        src, dst, neg, t = stream_of(11 + ci, N, E)
        P0 = torch.from_numpy((np.random.RandomState(77).randn(N, d) / np.sqrt(d)).astype(np.float32))
        D = tuple(Dv(x) for x in (src, dst, neg, t))
        halo = N                                               # (every remote node of the chunk gets a halo row)
        # ---- the single-GPU run on the windowed schedule
        ref = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=E, dim_factor=10, num_layer=L, time_decay_weight=lam,
                                               device="cuda:0", use_matrix=False, beginning_time=np.float64(t[0]),
                                               not_scale=False, enforce_dim=d)
        ref.random_projections[0].data = P0.clone()
        ref = ref.to(dev)
        rfp, rfn = ref.run_stream(*D, B, schedule="windowed")
        rl = torch.stack([ref.random_projections[i].detach() for i in range(0, L + 1)])
        # ---- (A) plain copies
        runs = make_shards(G, N, d, L, E, B, lam, t[0], P0, dev, halo)
        outs, moved, nsteps = run_copy(runs, D, B, lib)
        fpA = sum(o[0] for o in outs)
        fnA = sum(o[1] for o in outs)
        layA = full_layers(runs, N, L, d)
        for r in range(G):
            runs[r].rp.check_device_errors()
        bad_f = int((fpA != rfp).sum()) + int((fnA != rfn).sum())
        bad_s = int((layA != rl).sum())
        assert bad_f == 0 and bad_s == 0, (f"config {ci}: {bad_f} feature values and {bad_s} table values differ from the single-GPU run "
                                           f"(max {float((fpA - rfp).abs().max()):.3e} / {float((layA - rl).abs().max()):.3e})")
        # ---- (B) the RCCL stand-in, one thread per shard, tpnet_wshard_run
        runs_b = make_shards(G, N, d, L, E, B, lam, t[0], P0, dev, halo)
        res = run_loopback(runs_b, D, B, lib, so)
        fpB = sum(o[0] for o in res)
        fnB = sum(o[1] for o in res)
        layB = full_layers(runs_b, N, L, d)
        assert torch.equal(fpB, rfp) and torch.equal(fnB, rfn) and torch.equal(layB, rl), f"config {ci}: the loopback transport differs"
        assert float(runs_b[0].rp.now_time.item()) == float(t[-1])
        # ---- (C) no negatives at all (run_stream(src, dst, None, t): the pointer the kernels get is null -- round 4's fault on the
        # single-GPU pipeline lived exactly there): the (src, dst) features and the tables as the single-GPU run without negatives
        if ci < 3 and not os.environ.get("TPNET_WSHARD_RANDOM"):
            ref2 = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=E, dim_factor=10, num_layer=L, time_decay_weight=lam,
                                                    device="cuda:0", use_matrix=False, beginning_time=np.float64(t[0]),
                                                    not_scale=False, enforce_dim=d)
            ref2.random_projections[0].data = P0.clone()
            ref2 = ref2.to(dev)
            r2p, r2n = ref2.run_stream(D[0], D[1], None, D[3], B, schedule="windowed")
            assert r2n is None and torch.equal(r2p, rfp)
            runs_c = make_shards(G, N, d, L, E, B, lam, t[0], P0, dev, halo)
            res_c = run_loopback(runs_c, (D[0], D[1], None, D[3]), B, lib, so)
            assert all(o[1] is None for o in res_c)
            assert torch.equal(sum(o[0] for o in res_c), rfp) and torch.equal(full_layers(runs_c, N, L, d), rl), \
                f"config {ci}: the shards without negatives differ"
            for r in range(G):
                runs_c[r].rp.check_device_errors()
        summary.append((G, N, d, L, (E + B - 1) // B, nsteps, moved))
    print("WSHARD OK " + "; ".join(f"G={g} N={n} d={d} L={l} batches={nb}: {ns} launches per shard, {mv} rows moved"
                                   for g, n, d, l, nb, ns, mv in summary))


if __name__ == "__main__":
    main()
