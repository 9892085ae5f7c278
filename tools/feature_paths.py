#!/usr/bin/env python3
"""Developer tool: a census of the module's routes.  One call per case through PUBLIC methods only, seeded inputs, every result
saved with np.save under the directory given as the first argument (default: feature_paths_out); a case that raises saves the
exception's type and text instead.  Two trees compute the same thing by the same kernels if their directories compare equal
file by file (`cmp`): the paths differ in summation order, so equal bytes pin the route.  With rocprofv3 --kernel-trace --stats
around it, the kernel names and call counts close the gap.

    python tools/feature_paths.py OUT_DIR              # everything (the readout section first: 374 of the files)
    python tools/feature_paths.py OUT_DIR readout      # only the readout kernels' matrix (readout_cases)
    python tools/feature_paths.py OUT_DIR anchored     # only the anchored readout's routes, opt-ins included (anchored_cases)
    python tools/feature_paths.py OUT_DIR mlp          # only self.mlp's six C entries, partials included (mlp_cases; not in "everything")
    python tools/feature_paths.py OUT_DIR sizes        # only the size exports of the C ABI over a grid -> OUT_DIR/sizes.json (sizes_cases;
                                                       # not in "everything"; needs no GPU -- without one rocPRIM's size queries answer 0)
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tpnet_amd
from tpnet_amd.matrix_memory import MatrixMemory
from tpnet_amd.sampler import GpuRecentNeighborSampler

OUT = sys.argv[1] if len(sys.argv) > 1 else "feature_paths_out"
ONLY = sys.argv[2:]
os.makedirs(OUT, exist_ok=True)
DEV = "cuda:0"
N = 5000
SAVED = []


def save(name, val):
    if isinstance(val, torch.Tensor):
        val = val.detach().cpu().numpy()
    if isinstance(val, (tuple, list)):
        for i, v in enumerate(val):
            save(f"{name}.{i}", v)
        return
    np.save(os.path.join(OUT, name + ".npy"), np.asarray(val))
    SAVED.append(name)


def case(name, fn):
    try:
        val = fn()
    except Exception as e:                              # the cases that must raise: type and text are the result
        val = np.array([type(e).__name__, str(e)])
    torch.cuda.synchronize()
    save(name, val)


def make(d, L=3, n_nodes=N, seed=0, batches=3, **kw):
    """A module with a few batches of history (so that layers 1..L are not zero)."""
    torch.manual_seed(seed)
    args = dict(node_num=n_nodes, edge_num=40000, dim_factor=10, num_layer=L, time_decay_weight=1e-6, device=DEV, use_matrix=False,
                beginning_time=np.float64(0.0), not_scale=False, enforce_dim=d)
    args.update(kw)
    rp = tpnet_amd.RandomProjectionModule(**args).to(DEV)
    rng = np.random.RandomState(seed + 1)
    t0 = 0.0
    for _ in range(batches):
        t = np.sort(rng.uniform(t0, t0 + 1e5, 300))
        rp.update(rng.randint(0, n_nodes, 300), rng.randint(0, n_nodes, 300), t)
        t0 = t[-1]
    return rp


def with_grads(rp, fn):
    """fn() with gradients recorded: (out, the four weight gradients of self.mlp after out.sum().backward())."""
    rp.mlp.zero_grad(set_to_none=True)
    out = fn()
    out.sum().backward()
    return [out] + [p.grad for p in rp.mlp.parameters()]


def ids(rng, n, n_nodes=N):
    return rng.randint(0, n_nodes, n).astype(np.int64)


def encoder_call(rng, rows, K, n_nodes=N, repeated=True):
    """The reference encoder's arrays: src = tile(neighbours, 2), dst = concat(repeat(a1, K), repeat(a2, K))."""
    neigh = ids(rng, rows * K, n_nodes)
    if repeated:
        v = np.concatenate([np.repeat(ids(rng, rows, n_nodes), K), np.repeat(ids(rng, rows, n_nodes), K)])
    else:
        v = ids(rng, 2 * rows * K, n_nodes)
    return np.tile(neigh, 2), v


def dev(x, dt=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dt)


def param_grads(mods, fn):
    """fn() with gradients recorded: [out] + the gradients of every Parameter of `mods` after out.sum().backward()."""
    for m in mods:
        m.zero_grad(set_to_none=True)
    out = fn()
    out.sum().backward()
    return [out] + [p.grad for m in mods for p in m.parameters() if p.grad is not None]


def embedding_stage(rng, widths, hidden_out, n_nodes=300, K=20):
    """A TPNetEmbedding of the given widths (hidden_out = (H, Dout): its projection_layer replaced, no mixers) and one call's
    arrays with pad rows and repeated ids."""
    import types
    Dn, Dt, De, F = widths
    Nn, Ne = 500, 3000
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    te = tpnet_amd.TimeEncoder(time_dim=Dt)
    emb = tpnet_amd.TPNetEmbedding(node_raw_features=f32(rng.normal(0, 1, (Nn, Dn))), edge_raw_features=f32(rng.normal(0, 1, (Ne, De))),
                                   neighbor_sampler=None, time_encoder=te, node_feat_dim=Dn, edge_feat_dim=De, time_feat_dim=Dt,
                                   num_layers=2, num_neighbors=K, dropout=0.1,
                                   random_projections=types.SimpleNamespace(pair_wise_feature_dim=F)).to(DEV)
    if hidden_out is not None:
        emb.projection_layer = nn.Sequential(nn.Linear(Dn + Dt + De + 2 * F, hidden_out[0]), nn.ReLU(),
                                             nn.Linear(hidden_out[0], hidden_out[1])).to(DEV)
        emb.mlp_mixers = nn.ModuleList()
    emb.eval()
    neigh, eids = rng.randint(1, Nn, (n_nodes, K)).astype(np.int64), rng.randint(1, Ne, (n_nodes, K)).astype(np.int64)
    tq = rng.uniform(1e5, 2e6, n_nodes)
    tn = tq[:, None] - rng.uniform(0, 1e5, (n_nodes, K))
    pad = rng.rand(n_nodes, K) < 0.2
    neigh[pad], eids[pad], tn[pad] = 0, 0, 0.0
    neigh[:, K // 2] = neigh[:, 0]
    return emb, (dev(neigh), dev(eids), dev(tn, torch.float64), dev(tq, torch.float64), f32(rng.normal(0, 1, (2 * n_nodes * K, F))))


def dense_cases(rng):
    """The dense-layer routes by their public names: fused_mlp.fused_mlp, LinkPredictor_v1.fused, fused_feature.mlp_f32 on both
    sides of its kernel switch with mlp_backward both ways, TPNetEmbedding with fused_input on and off."""
    from tpnet_amd import fused_feature as ff, fused_mlp as fm
    from tpnet_amd.callers import LinkPredictor_v1
    torch.manual_seed(11)
    mlp = nn.Sequential(nn.Linear(64, 256), nn.ReLU(), nn.Linear(256, 64)).to(DEV)
    rows = lambda n, w=64: torch.from_numpy(rng.uniform(0, 12, (n, w)).astype(np.float32)).to(DEV)   # log(1 + G) features: 0 .. ~12
    x1k = rows(1000)
    with torch.no_grad():
        case("fused_mlp_fn", lambda: fm.fused_mlp(mlp, x1k))
    case("fused_mlp_fn_grad", lambda: param_grads([mlp], lambda: fm.fused_mlp(mlp, x1k)))
    for n in (33, 8225):
        xn = rows(n)
        with torch.no_grad():
            case(f"mlp_f32_n{n}", lambda: ff.mlp_f32(mlp, xn))
    x5k = rows(5000)
    for mode in ("mfma", "torch"):
        mlp.mlp_backward = mode
        case(f"mlp_f32_n5000_grad_{mode}", lambda: param_grads([mlp], lambda: ff.mlp_f32(mlp, x5k)))
    del mlp.mlp_backward
    xg = rows(700).requires_grad_(True)
    case("mlp_f32_input_grad", lambda: param_grads([mlp], lambda: ff.mlp_f32(mlp, xg)) + [xg.grad])
    # ---- the decoder ------------------------------------------------------------------------------------------------------
    rp = make(128, seed=6)
    dec = LinkPredictor_v1(172, 172, 172, 1, rp, False).to(DEV)
    dec.fused = True
    a, b = ids(rng, 1000), ids(rng, 1000)
    se = torch.from_numpy(rng.normal(0, 1, (1000, 172)).astype(np.float32)).to(DEV)
    de = torch.from_numpy(rng.normal(0, 1, (1000, 172)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        case("decoder_fused", lambda: dec(a, b, se, de))
    seg, deg = se.clone().requires_grad_(True), de.clone().requires_grad_(True)
    case("decoder_fused_grad", lambda: param_grads([dec.fc1, dec.fc2, rp.mlp], lambda: dec(a, b, seg, deg)) + [seg.grad, deg.grad])
    # ---- the encoder module: fixture G11 end to end, then the input stage's two kernel variants --------------------------
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g11_encoder.npz"))
    for fused in (False, True):
        rp11 = tpnet_amd.RandomProjectionModule(node_num=int(g["N"]), edge_num=int(g["E"]), dim_factor=10, num_layer=int(g["L"]),
                                                time_decay_weight=float(g["lam"]), device=DEV, use_matrix=False,
                                                beginning_time=np.float64(0.0), not_scale=False, enforce_dim=int(g["d"]))
        sampler = GpuRecentNeighborSampler(g["src"], g["dst"], g["t"], g["eid"], device=DEV, num_nodes=int(g["N"]))
        model = tpnet_amd.TPNet(node_raw_features=g["node_raw"], edge_raw_features=g["edge_raw"], neighbor_sampler=sampler,
                                time_feat_dim=int(g["Dt"]), dropout=0.1, random_projections=rp11, num_layers=int(g["mixers"]),
                                num_neighbors=int(g["K"]), device=DEV)
        model.load_state_dict({str(k): torch.from_numpy(g[f"sd_{int(s)}"]) for k, s in zip(g["sd_keys"], g["sd_slot"])})
        model = model.to(DEV).eval()
        model.embedding_module.fused_input = fused
        for bb in range(4):
            sl = slice(50 * bb, 50 * bb + 50)
            rp11.update(g["src"][sl], g["dst"][sl], g["t"][sl])
        sl = slice(200, 200 + int(g["B"]))
        with torch.no_grad():
            case(f"g11_embeddings_fused_input_{int(fused)}",
                 lambda: model.compute_src_dst_node_temporal_embeddings(g["src"][sl], g["dst"][sl], g["t"][sl]))
    for tag, widths, hidden_out in (("narrow", (172, 100, 172, 64), None), ("wide", (256, 100, 172, 64), (320, 224))):
        emb, arrays = embedding_stage(rng, widths, hidden_out)
        for fused in (False, True):
            emb.fused_input = fused
            with torch.no_grad():
                case(f"embedding_{tag}_fused_input_{int(fused)}", lambda: emb.embed_from_features(*arrays))


def mlp_cases():
    """The six C entries of self.mlp on rows that exist (csrc/mlp_x3.hip, mlp_rows.hip, mlp_bwd.hip, mlp_rows_bwd.hip) on seeded
    real-valued data: the forwards around their kernel switch and past one tile per wave, the backwards with every partial of a
    2-partial and a 256-partial launch."""
    from tpnet_amd import _dense, _lib, fused_feature as ff, fused_mlp as fm
    lib = _lib.load()
    rng = np.random.RandomState(31)
    rows = lambda n, w, lo=0.0, hi=12.0: torch.from_numpy(rng.uniform(lo, hi, (n, w)).astype(np.float32)).to(DEV)
    stream = lambda: _dense.stream_ptr(torch.device(DEV))
    for F, ns in ((64, (33, 8191, 8193, 65569)), (16, (1, 31, 32, 33, 1000, 4099, 140001)), (36, (1, 31, 32, 33, 1000, 4099, 140001))):
        torch.manual_seed(F)
        mlp = nn.Sequential(nn.Linear(F, 4 * F), nn.ReLU(), nn.Linear(4 * F, F)).to(DEV)
        prep = ff.prepared(mlp, F)
        fwd = lib.tpnet_mlp64_f32 if F == 64 else lib.tpnet_mlp_rows_f32
        for n in ns:
            x, y = rows(n, F), torch.empty((n, F), device=DEV)
            case(f"mlp_fwd_F{F}_n{n}", lambda: (fwd(x.data_ptr(), n, prep.ref, y.data_ptr(), stream()), y))
        bwds = [("f32", lambda *a: (lib.tpnet_mlp64_bwd_f32 if F == 64 else lib.tpnet_mlp_rows_bwd_f32)(*a[:3], prep.ref, *a[3:]))]
        if F == 64:
            p16 = fm._prepared(mlp)
            bwds.append(("bf16", lambda *a: lib.tpnet_mlp64_bwd_bf16(*a[:3], p16[0].data_ptr(), p16[1].data_ptr(), p16[4].data_ptr(), *a[3:])))
        pf = 2 * 4 * F * F + 4 * F
        for n in (33, 1000, 9000, 80000):
            x, gy = rows(n, F, 0.0, 9.0), rows(n, F, -1.0, 1.0)
            for tag, call in bwds:
                for parts in (2, 256):
                    part = torch.zeros((parts, pf), device=DEV)
                    case(f"mlp_bwd_{tag}_F{F}_n{n}_p{parts}",
                         lambda: (call(x.data_ptr(), gy.data_ptr(), n, part.data_ptr(), parts, stream()), part))


def readout_cases():
    """The readout kernels by geometry and store path (csrc/readout.hpp): the three standalone readouts at eight row widths x L = 1..4,
    and run_stream's readouts on both schedules and in exact mode."""
    rng = np.random.RandomState(21)
    n_nodes, n, K = 64, 37, 5
    with torch.no_grad():
        for d in (12, 16, 32, 64, 100, 256, 260, 30):
            for L in (1, 2, 3, 4):
                rp = make(d, L=L, n_nodes=n_nodes, seed=d + L, batches=L + 1)
                u, v, v2 = (dev(ids(rng, n, n_nodes)) for _ in range(3))
                neigh = dev(ids(rng, n * K, n_nodes).reshape(n, K))
                tag = f"readout_d{d}_L{L}"
                case(f"{tag}_default", lambda: rp.pair_gram(u, v))
                case(f"{tag}_raw", lambda: rp.pair_gram(u, v, raw=True))
                case(f"{tag}_packed", lambda: rp.pair_gram(u, v, packed=True))
                rp.not_scale = True
                case(f"{tag}_not_scale", lambda: rp.pair_gram(u, v))
                rp.not_scale = False
                case(f"{tag}_shared", lambda: rp.pair_gram_shared(u, v, v2))
                case(f"{tag}_anchored", lambda: rp.pair_gram_anchored(neigh, u, v, matrix_cores=False))   # (d outside 36..512: the error text)
        streams = [(d, 64, 20, 500) for d in (16, 64, 128, 256)] + [(64, 2600, 3, 6000)]      # (B = 2600: the edge-fused step)
        for d, B, nb, nn_ in streams:
            E = B * nb
            src, dst, neg = (dev(ids(rng, E, nn_)) for _ in range(3))
            t = dev(np.sort(rng.uniform(1.0, 2.0e5, E)), torch.float64)
            for mode in ("batch", "windowed", "exact"):
                for packed in (False, True):
                    rp = make(d, n_nodes=nn_, seed=d, batches=0, exact=(mode == "exact"))
                    sched = None if mode == "exact" else mode
                    case(f"stream_d{d}_B{B}_{mode}_packed{int(packed)}",
                         lambda: list(rp.run_stream(src, dst, neg, t, B, packed=packed, schedule=sched)) + list(rp.backup_random_projections()[1]))


def anchored_cases():
    """The anchored readout's routes (csrc/encoder.hip: anchored_route) through every public door: `rows8_readout` on 8-byte rows,
    `layers_readout` at num_layer 1, 2, 4, the ends of the matrix-core and walk width ranges, and the widths that are refused (their
    exception texts are the result).  Three rows with K = 3, 4, 5; the host tile / repeat pattern just above 8192 pairs."""
    rng = np.random.RandomState(41)
    n_nodes, E = 300, 4000
    es, ed, et = ids(rng, E, n_nodes), ids(rng, E, n_nodes), np.sort(rng.uniform(0, 2e5, E))
    sampler = GpuRecentNeighborSampler(es, ed, et, device=DEV, num_nodes=n_nodes)
    s, o, tq = es[-3:], ed[-3:], et[-3:] + 1.0
    mods = [(f"rows8_d{d}", d, 3, "rows8_readout") for d in (110, 38)]
    mods += [(f"layers_d{d}_L{L}", d, L, "layers_readout") for L in (1, 2, 4) for d in (64, 140)]
    mods += [(f"plain_d{d}", d, 3, None) for d in (36, 160, 164, 512, 110, 34, 516)]
    for tag, d, L, switch in mods:
        rp = make(d, L=L, n_nodes=n_nodes, seed=d + L)
        if switch:
            setattr(rp, switch, True)
        for K in (3, 4, 5):
            neigh, a1, a2 = ids(rng, 3 * K, n_nodes).reshape(3, K), ids(rng, 3, n_nodes), ids(rng, 3, n_nodes)
            name = f"anchored_{tag}_K{K}"
            with torch.no_grad():
                case(f"{name}_gram", lambda: rp.pair_gram_anchored(neigh, a1, a2))
                case(f"{name}_gram_no_mfma", lambda: rp.pair_gram_anchored(dev(neigh), a1, a2, matrix_cores=False))
                case(f"{name}_feature", lambda: rp.get_pair_wise_feature_anchored(dev(neigh), dev(a1), dev(a2)))
                case(f"{name}_encoder_host", lambda: rp.encoder_pair_features(sampler, s, o, tq, K))
                case(f"{name}_encoder_device", lambda: rp.encoder_pair_features(sampler, dev(s), dev(o), dev(tq, torch.float64), K))
                if K > 3:
                    u, v = encoder_call(rng, 4100 // K + 1, K, n_nodes)
                    case(f"{name}_pattern", lambda: rp.get_pair_wise_feature(u, v))


def sizes_cases():
    """Every export that sizes a caller-owned buffer, and tpnet_stream_schedule (which decides on such sizes), over a grid of shapes
    around the tile, batch-size and chunk thresholds: {export: [[arguments..., result], ...]} in sizes.json.  Sizes decide how a
    stream is cut into chunks, so two builds lay buffers out alike only if their files are EQUAL."""
    import json
    from tpnet_amd import _lib
    lib = _lib.load()
    EB = (1, 255, 256, 257, 1000, 4096, 4097, 100000, 5000000)      # edges / list lengths
    BATCH = (200, 1000, 1024, 1025, 4096, 4097)
    DS, LS, GS, NS = (16, 64, 128, 172, 512), (1, 2, 3, 4), (1, 2, 8), (2, 300, 5000, 100000)
    out = {}

    def grid(name, *axes):
        fn, rows = getattr(lib, name), []

        def walk(prefix, rest):
            if not rest:
                rows.append(list(prefix) + [int(fn(*prefix))])
                return
            for x in rest[0]:
                walk(prefix + (x,), rest[1:])
        walk((), axes)
        out.setdefault(name, []).extend(rows)

    grid("tpnet_sampler_bytes", EB, NS)
    for name in ("tpnet_sampler_weights_bytes", "tpnet_neg_bytes", "tpnet_edgebank_bytes", "tpnet_edgebank_scratch_bytes"):
        grid(name, (0,) + EB)
    grid("tpnet_neg_scratch_bytes", EB, (0, 5) + BATCH, (0, 5) + BATCH)
    grid("tpnet_lp_metrics_scratch_bytes", (0,) + EB, (0,) + EB)
    grid("tpnet_xplan_large_bytes", EB, BATCH, GS)
    grid("tpnet_workspace_bytes", EB, (1,) + BATCH)
    for G in GS:
        for n_owned in (1, 150, 2500):
            grid("tpnet_wshard_workspace_bytes", (n_owned + 1, 2 * n_owned + 7), DS, LS, EB, BATCH, (G,), (n_owned,))
    grid("tpnet_stream_workspace_bytes", NS, DS, LS, EB, BATCH)
    flags = (0, _lib.FLAG_SCHED_WINDOWED, _lib.FLAG_SCHED_BATCH, _lib.FLAG_PLAN_SORTED, _lib.FLAG_PLAN_HASHED)
    for N in NS:
        for d in DS:
            for L in LS:
                for E in EB:
                    for B in BATCH:
                        unit = 2 * L * d * 4 * B                    # version-log bytes of one batch: a cap cuts chunks at whole batches
                        nb = (E + B - 1) // B
                        caps = sorted({0, 1} | {k * unit + o for k in (3, 4, 5, nb - 1, nb, nb + 1) if k > 0 for o in (-1, 0, 1)})
                        grid("tpnet_stream_workspace_bytes_capped", (N,), (d,), (L,), (E,), (B,), caps)
                        # either side of every size the schedule can turn on: the whole stream's workspace, a capped one's, the
                        # per-batch plan's
                        turn = {int(lib.tpnet_stream_workspace_bytes(N, d, L, E, B)), int(lib.tpnet_workspace_bytes(E, B)),
                                int(lib.tpnet_stream_workspace_bytes_capped(N, d, L, E, B, 4 * unit)),
                                int(lib.tpnet_stream_workspace_bytes_capped(N, d, L, E, B, max(nb // 2, 1) * unit))}
                        ws = sorted({0} | {w + o for w in turn for o in (-1, 0, 1) if w + o >= 0} | {w // 2 for w in turn})
                        grid("tpnet_stream_schedule", (N,), (d,), (L,), (E,), (B,), flags, ws)
    with open(os.path.join(OUT, "sizes.json"), "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
    SAVED.append("sizes")


def main():
    if ONLY:
        for name in ONLY:
            {"readout": readout_cases, "anchored": anchored_cases, "mlp": mlp_cases, "sizes": sizes_cases}[name]()
        print(f"{len(SAVED)} files in {OUT}")
        return
    readout_cases()
    anchored_cases()
    rng = np.random.RandomState(7)
    # ---- the decoder's calls from host arrays -----------------------------------------------------------------------------
    rp128 = make(128)
    for n in (200, 1000):
        u, v = ids(rng, n), ids(rng, n)
        with torch.no_grad():
            case(f"decoder_n{n}_nograd", lambda: rp128.get_pair_wise_feature(u, v))
        case(f"decoder_n{n}_grad", lambda: with_grads(rp128, lambda: rp128.get_pair_wise_feature(u, v)))
    # ---- around the staging ring's and the one-launch kernel's limits (16 386 = the ring's 16 384 pairs + 2) ---------------
    rp172 = make(172)
    for rp, d in ((rp128, 128), (rp172, 172)):
        for n in (8192, 8194, 16384, 16386):
            half = ids(rng, n // 2)
            v = ids(rng, n)
            w = ids(rng, n)
            with torch.no_grad():
                case(f"d{d}_n{n}_tiled", lambda: rp.get_pair_wise_feature(np.tile(half, 2), v))
                case(f"d{d}_n{n}_plain", lambda: rp.get_pair_wise_feature(w, v))
    # ---- the encoder's tile / repeat call, 80 000 pairs --------------------------------------------------------------------
    K = 20
    u, v = encoder_call(rng, 2000, K)
    mods = {128: rp128, 172: rp172}
    for d in (64, 128, 140, 172, 256, 512):
        rp = mods.get(d) or make(d)
        mods[d] = rp
        with torch.no_grad():
            case(f"encoder_d{d}_nograd", lambda: rp.get_pair_wise_feature(u, v))
        case(f"encoder_d{d}_grad", lambda: with_grads(rp, lambda: rp.get_pair_wise_feature(u, v)))
    rp_l2 = make(172, L=2)
    with torch.no_grad():
        case("encoder_d172_L2_nograd", lambda: rp_l2.get_pair_wise_feature(u, v))
    case("encoder_d172_L2_grad", lambda: with_grads(rp_l2, lambda: rp_l2.get_pair_wise_feature(u, v)))
    u2, v2 = encoder_call(rng, 2000, K, repeated=False)
    w2 = ids(rng, 80000)
    with torch.no_grad():
        case("tiled_not_repeated_d172", lambda: rp172.get_pair_wise_feature(u2, v2))
        case("not_tiled_d172", lambda: rp172.get_pair_wise_feature(w2, v2))
        case("not_tiled_d128", lambda: rp128.get_pair_wise_feature(w2, v2))
    case("not_tiled_d172_grad", lambda: with_grads(rp172, lambda: rp172.get_pair_wise_feature(w2, v2)))
    # ---- kinds of ids -----------------------------------------------------------------------------------------------------
    a, b = ids(rng, 500), ids(rng, 500)
    with torch.no_grad():
        case("src_device", lambda: rp128.get_pair_wise_feature(dev(a), dev(b)))
        case("src_device_dst_host", lambda: rp128.get_pair_wise_feature(dev(a), b))
        case("dst_device", lambda: rp128.get_pair_wise_feature(a, dev(b)))
        case("dst_device_d172_tiled", lambda: rp172.get_pair_wise_feature(np.tile(a, 2), dev(np.tile(b, 2))))
        case("ids_int32", lambda: rp128.get_pair_wise_feature(a.astype(np.int32), b.astype(np.int32)))
        case("ids_list", lambda: rp128.get_pair_wise_feature(a.tolist(), b.tolist()))
        case("ids_strided", lambda: rp128.get_pair_wise_feature(np.tile(a, 2)[::2], np.tile(b, 2)[::2]))
        case("ids_negative", lambda: rp128.get_pair_wise_feature(a - N, b))
        case("ids_negative_long", lambda: rp128.get_pair_wise_feature(np.tile(a - N, 40), np.tile(b, 40)))
        case("ids_negative_pair_gram", lambda: rp128.pair_gram(a - N, b - N))
        case("ids_out_of_range", lambda: rp128.get_pair_wise_feature(np.where(a == a[3], N, a), b))
        case("ids_below_minus_n", lambda: rp128.get_pair_wise_feature(np.where(a == a[3], -N - 1, a), b))
        case("ids_2d", lambda: rp128.get_pair_wise_feature(a.reshape(2, -1), b.reshape(2, -1)))
        case("ids_length_mismatch", lambda: rp128.get_pair_wise_feature(a, b[:-1]))
        case("ids_empty", lambda: rp128.get_pair_wise_feature(a[:0], b[:0]))
    # ---- self.mlp variants ------------------------------------------------------------------------------------------------
    for d in (128, 256):
        rp = make(d, seed=3)
        rp.fused_mlp = True
        with torch.no_grad():
            case(f"fused_mlp_d{d}_short", lambda: rp.get_pair_wise_feature(a, b))
            case(f"fused_mlp_d{d}_encoder", lambda: rp.get_pair_wise_feature(u, v))
        case(f"fused_mlp_d{d}_short_grad", lambda: with_grads(rp, lambda: rp.get_pair_wise_feature(a, b)))
    rp_id = make(128, seed=4)
    rp_id.mlp = nn.Identity()
    with torch.no_grad():
        case("mlp_identity_short", lambda: rp_id.get_pair_wise_feature(a, b))
        case("mlp_identity_encoder", lambda: rp_id.get_pair_wise_feature(u, v))
    rp_m = make(0, n_nodes=64, use_matrix=True, enforce_dim=-1)
    am, bm = ids(rng, 100, 64), ids(rng, 100, 64)
    with torch.no_grad():
        case("use_matrix", lambda: rp_m.get_pair_wise_feature(am, bm))
        case("use_matrix_rows", lambda: rp_m.get_random_projections(am))
    # ---- the readouts before self.mlp -------------------------------------------------------------------------------------
    big_a, big_b = ids(rng, 20000), ids(rng, 20000)
    neigh = ids(rng, 50 * K).reshape(50, K)
    a1, a2 = ids(rng, 50), ids(rng, 50)
    with torch.no_grad():
        for tag, kw in (("plain", {}), ("raw", dict(raw=True)), ("packed", dict(packed=True))):
            case(f"pair_gram_{tag}", lambda: rp128.pair_gram(a, b, **kw))
            case(f"pair_gram_{tag}_long", lambda: rp128.pair_gram(big_a, big_b, **kw))
        case("pair_gram_device", lambda: rp128.pair_gram(dev(a), dev(b)))
        case("pair_gram_shared", lambda: rp172.pair_gram_shared(a, b, ids(np.random.RandomState(9), 500)))
        case("feature_shared", lambda: rp172.get_pair_wise_feature_shared(a, b, ids(np.random.RandomState(9), 500)))
        case("pair_gram_anchored", lambda: rp128.pair_gram_anchored(neigh, a1, a2))
        case("pair_gram_anchored_no_mfma", lambda: rp128.pair_gram_anchored(neigh, a1, a2, matrix_cores=False))
        case("pair_gram_anchored_d172", lambda: rp172.pair_gram_anchored(dev(neigh), a1, a2))
        case("feature_anchored_device", lambda: rp128.get_pair_wise_feature_anchored(dev(neigh), dev(a1), dev(a2)))
        case("feature_anchored_device_d172", lambda: rp172.get_pair_wise_feature_anchored(dev(neigh), a1, a2))
        case("feature_anchored_host", lambda: rp128.get_pair_wise_feature_anchored(neigh, a1, a2))
    case("feature_anchored_device_grad",
         lambda: with_grads(rp128, lambda: rp128.get_pair_wise_feature_anchored(dev(neigh), dev(a1), dev(a2))))
    # ---- the encoder's whole readout with the device-side sampler ----------------------------------------------------------
    E = 30000
    es, ed, et = ids(rng, E), ids(rng, E), np.sort(rng.uniform(0, 2e5, E))
    sampler = GpuRecentNeighborSampler(es, ed, et, device=DEV, num_nodes=N)
    for rp, d in ((rp128, 128), (rp172, 172), (rp_l2, "172_L2")):
        for B, Kq in ((200, 20), (11000, 4)):              # (11 000: above the staging ring's largest host batch)
            s, o, tq = es[-B:], ed[-B:], et[-B:] + 1.0
            with torch.no_grad():
                case(f"encoder_features_d{d}_B{B}_host", lambda: rp.encoder_pair_features(sampler, s, o, tq, Kq))
                case(f"encoder_features_d{d}_B{B}_device",
                     lambda: rp.encoder_pair_features(sampler, dev(s), dev(o), dev(tq, torch.float64), Kq))
    sB, oB, tB = es[-200:], ed[-200:], et[-200:] + 1.0
    case("encoder_features_grad", lambda: with_grads(rp128, lambda: rp128.encoder_pair_features(sampler, sB, oB, tB, 20)[0]))
    case("encoder_features_bad_length", lambda: rp128.encoder_pair_features(sampler, sB, oB[:-1], tB, 20))
    # ---- update -----------------------------------------------------------------------------------------------------------
    for exact in (False, True):
        rp = make(128, seed=5, exact=exact)
        tag = "exact" if exact else "lazy"
        t0 = 4e5
        for B in (200, 2049, 20000):                        # (one workgroup's plan / staged + chunk planner / device copies)
            tt = np.sort(rng.uniform(t0, t0 + 1e4, B))
            t0 = tt[-1]
            uu, vv = ids(rng, B), ids(rng, B)
            case(f"update_{tag}_B{B}", lambda: (rp.update(uu, vv, tt), rp.get_random_projections(a))[1])
        tt = np.sort(rng.uniform(t0, t0 + 1e4, 200))
        t0 = tt[-1]
        case(f"update_{tag}_device", lambda: (rp.update(dev(a[:200]), dev(b[:200]), tt), rp.get_random_projections(b))[1])
        case(f"update_{tag}_negative", lambda: (rp.update(a[:200] - N, b[:200].tolist(), tt + 1e4), rp.get_random_projections(b))[1])
        t0 += 1e4
        before = rp.backup_random_projections()
        bad = a[:200].copy()
        bad[17] = N
        case(f"update_{tag}_out_of_range", lambda: rp.update(bad, b[:200], tt + 2e4))
        case(f"update_{tag}_out_of_range_dst", lambda: rp.update(b[:200], bad - 2 * N - 1, tt + 2e4))
        case(f"update_{tag}_empty", lambda: rp.update(a[:0], b[:0], tt[:0]))
        case(f"update_{tag}_length_mismatch", lambda: rp.update(a[:200], b[:199], tt))
        after = rp.backup_random_projections()
        save(f"update_{tag}_state_before", [before[0]] + before[1])
        save(f"update_{tag}_state_after", [after[0]] + after[1])
        case(f"update_{tag}_rows", lambda: rp.get_random_projections(np.arange(0, N, 7)))
        case(f"update_{tag}_rows_list", lambda: rp.get_random_projections([1, 2, -3]))
        case(f"update_{tag}_now_time", lambda: rp.now_time.detach().clone())
        with torch.no_grad():
            case(f"update_{tag}_feature", lambda: rp.get_pair_wise_feature(a, b))
    dense_cases(rng)
    # ---- MatrixMemory -----------------------------------------------------------------------------------------------------
    mm = MatrixMemory(num_node=60, num_hop=2, device=DEV).to(DEV)
    for k in range(3):
        mm.update(ids(rng, 40, 60), ids(rng, 40, 60))
    case("matrix_memory_get", lambda: mm.get_memory(ids(np.random.RandomState(11), 80, 60), ids(np.random.RandomState(12), 80, 60)))
    case("matrix_memory_backup", lambda: mm.backup_memory())
    case("matrix_memory_out_of_range", lambda: mm.update(np.array([1, 60]), np.array([2, 3])))
    case("matrix_memory_after", lambda: mm.backup_memory())
    with open(os.path.join(OUT, "cases.txt"), "w") as f:
        f.write("\n".join(SAVED) + "\n")
    print(f"{len(SAVED)} files in {OUT}")


if __name__ == "__main__":
    main()
