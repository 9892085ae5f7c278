#!/usr/bin/env python3
"""Developer tool: a census of the three training stages' kernels (feature_paths.py's manner).  One forward and backward per case
through the PUBLIC functions fused_mixer.channel_train, fused_mixer.token_train and fused_input.encoder_input_train, seeded inputs
and explicit dropout keys; every output, every gradient and both weight images saved with np.save under the directory given as the
first argument.  The C ABI of two builds being equal, one tree can load either library (TPNET_DEV_LIB): the two directories compare
equal file by file (`cmp`) exactly when the kernels give the same bits.  With rocprofv3 --kernel-trace --stats around it, the
kernel names and call counts show the launches.

    python tools/training_paths.py OUT_DIR
    TPNET_DEV_LIB=/path/to/another/libtpnet_hip.so python tools/training_paths.py OTHER_DIR && diff -r OUT_DIR OTHER_DIR
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tpnet_amd
from tpnet_amd import fused_input as fi, fused_mixer as fm

OUT = sys.argv[1] if len(sys.argv) > 1 else "training_paths_out"
os.makedirs(OUT, exist_ok=True)
DEV = "cuda:0"
SAVED = []
# the shapes the three training test files list
CHANNEL = [(172, 688), (20, 80), (100, 353), (256, 1024), (4, 1)]                      # (C, Ch)
TOKEN = [(20, 172), (6, 20), (2, 4), (32, 256), (10, 100)]                             # (K, C)
INPUT = {"small": (8, 4, 12, 4, 33, 36), "real": (172, 100, 172, 64, 344, 172), "wide": (172, 100, 256, 64, 512, 256),
         "516x416x64": (172, 100, 116, 64, 416, 64)}                                   # (Dn, Dt, De, F, H, Dout)
ROWS = [(1,), (33,), (129,), (7, 20)]
PARTS = [2, 3, 5, None]                                                                # None: the module's default
RATES = [0.0, 0.1]


def save(name, val):
    if isinstance(val, (tuple, list)):
        for i, v in enumerate(val):
            save(f"{name}.{i}", v)
        return
    np.save(os.path.join(OUT, name + ".npy"), val.detach().cpu().numpy())
    SAVED.append(name)


def mixer(K, C, Ch, seed):
    torch.manual_seed(seed)
    m = tpnet_amd.MLPMixer(num_tokens=K, num_channels=C, dropout=0.1)
    m.channel_feedforward.ffn = nn.Sequential(nn.Linear(C, Ch), nn.GELU(), nn.Dropout(0.1), nn.Linear(Ch, C), nn.Dropout(0.1))
    with torch.no_grad():
        for ln in (m.token_norm, m.channel_norm):
            ln.weight.uniform_(0.5, 1.5)
            ln.bias.normal_(0, 0.3)
    return m.to(DEV)


def grads_of(mod, fn, x, gy):
    """fn(x) with gradients recorded, backward from gy: [out, gx] + the gradient of every Parameter that got one."""
    mod.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    out = fn(x)
    out.backward(gy)
    torch.cuda.synchronize()
    return [out, x.grad] + [p.grad for p in mod.parameters() if p.grad is not None]


def with_parts(module, name, parts, fn):
    default = getattr(module, name)
    if parts is not None:
        setattr(module, name, parts)
    try:
        return fn()
    finally:
        setattr(module, name, default)


def channel_cases():
    for i, (C, Ch) in enumerate(CHANNEL):
        m = mixer(4, C, Ch, seed=100 + i)
        gen = torch.Generator().manual_seed(200 + i)
        for rows in ROWS:
            x, gy = (torch.randn(rows + (C,), generator=gen).to(DEV) for _ in range(2))
            for p in RATES:
                for parts in PARTS:
                    tag = f"channel_C{C}_Ch{Ch}_rows{'x'.join(map(str, rows))}_p{p}_parts{parts}"
                    save(tag, with_parts(fm, "CHANNEL_PARTIALS", parts,
                                         lambda: grads_of(m, lambda v: fm.channel_train(m, v, p, key=0x1234567890ABCDEF + i), x, gy)))
        rec = fm.cached(m)
        save(f"channel_C{C}_Ch{Ch}_images", [rec.img, rec.bimg])


def token_cases():
    for i, (K, C) in enumerate(TOKEN):
        m = mixer(K, C, 4 * C, seed=300 + i)
        gen = torch.Generator().manual_seed(400 + i)
        for n in (1, 7, 33):
            x, gy = (torch.randn((n, K, C), generator=gen).to(DEV) for _ in range(2))
            for p in RATES:
                for parts in (2, None):
                    tag = f"token_K{K}_C{C}_n{n}_p{p}_parts{parts}"
                    save(tag, with_parts(fm, "MAX_PARTIALS", parts,
                                         lambda: grads_of(m, lambda v: fm.token_train(m, v, p, key=0x0FEDCBA987654321 + i), x, gy)))


def input_stage(dims, n_nodes, K, seed):
    """A TPNetEmbedding of the given widths (its projection_layer replaced, no mixers) and one call's arrays with pad rows and
    repeated ids."""
    Dn, Dt, De, F, H, Dout = dims
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    Nn, Ne = 500, 3000
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
    te = tpnet_amd.TimeEncoder(time_dim=Dt)
    emb = tpnet_amd.TPNetEmbedding(node_raw_features=f32(rng.normal(0, 1, (Nn, Dn))), edge_raw_features=f32(rng.normal(0, 1, (Ne, De))),
                                   neighbor_sampler=None, time_encoder=te, node_feat_dim=Dn, edge_feat_dim=De, time_feat_dim=Dt,
                                   num_layers=2, num_neighbors=K, dropout=0.1,
                                   random_projections=types.SimpleNamespace(pair_wise_feature_dim=F)).to(DEV)
    emb.projection_layer = nn.Sequential(nn.Linear(Dn + Dt + De + 2 * F, H), nn.ReLU(), nn.Linear(H, Dout)).to(DEV)
    emb.mlp_mixers = nn.ModuleList()
    with torch.no_grad():
        te.w.bias.normal_(0, 0.5)
    neigh, eids = rng.randint(1, Nn, (n_nodes, K)).astype(np.int64), rng.randint(1, Ne, (n_nodes, K)).astype(np.int64)
    tq = rng.uniform(1e5, 2e6, n_nodes)
    tn = tq[:, None] - rng.uniform(0, 1e5, (n_nodes, K))
    pad = rng.rand(n_nodes, K) < 0.2
    neigh[pad], eids[pad], tn[pad] = 0, 0, 0.0
    neigh[:, K // 2] = neigh[:, 0]
    feats = f32(rng.normal(0, 1, (2 * n_nodes * K, F)))
    gy = f32(rng.normal(0, 1, (n_nodes, K, Dout)))
    return emb, (dev(neigh, torch.int64), dev(eids, torch.int64), dev(tn, torch.float64), dev(tq, torch.float64)), feats, gy


def input_cases():
    for i, (name, dims) in enumerate(INPUT.items()):
        for rows in ROWS:
            n_nodes, K = rows if len(rows) == 2 else (rows[0], 1)
            emb, arrays, feats, gy = input_stage(dims, n_nodes, K, seed=500 + i)
            call = lambda parts: lambda f: fi.encoder_input_train(emb.projection_layer, emb.time_encoder, emb.node_raw_features,
                                                                  emb.edge_raw_features, *arrays, f, parts=parts)
            for parts in PARTS:
                save(f"input_{name}_n{n_nodes}_K{K}_parts{parts}", grads_of(emb, call(parts), feats, gy))
        rec = fi.cached(emb.projection_layer)
        save(f"input_{name}_images", [rec.img, rec.bimg])
        fi.check_errors(rec)


def main():
    channel_cases()
    token_cases()
    input_cases()
    with open(os.path.join(OUT, "cases.txt"), "w") as f:
        f.write("\n".join(SAVED) + "\n")
    print(f"{len(SAVED)} files in {OUT}")


if __name__ == "__main__":
    main()
