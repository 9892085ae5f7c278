"""Generates tests/golden/g11_encoder.npz (fixture G11): the reference's own `TPNet` encoder on a toy graph, CPU.

Runs only where the read-only reference checkout is present (TPNET_REFERENCE, default /root/reference); the fixture holds
DATA only -- the full state dict (sd_keys[i] -> array sd_<sd_slot[i]>), the edge list and raw features, and per call the
sampler's arrays, the relative encodings, the projection_layer output (forward hook) and the embeddings; plus one train()-mode
call with dropout 0 and three gradients.

Configuration: N = 40 nodes, E = 300 edges, K = 6 neighbours; node / edge / time widths 20 / 12 / 8 (segment starts 20, 28, 40: an
8-float operand piece straddles a segment); d = 16, L = 3 (F = 64); two mixer layers.  Four 50-edge `rp.update` calls, then
call 0 = (src, dst) of edges 200..224, an update with those edges, call 1 = (src, neg) of edges 225..249.  The train()-mode call
repeats call 1 (same state, same arrays) with every Dropout at p = 0."""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("TPNET_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from models.TPNet import RandomProjectionModule, TPNet  # noqa: E402
from utils.utils import NeighborSampler  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    rng = np.random.RandomState(11)
    torch.manual_seed(11)
    N, E, K, B = 40, 300, 6, 25
    Dn, De, Dt, d, L, mixers = 20, 12, 8, 16, 3, 2
    lam = 1e-4
    src = rng.randint(1, N, E).astype(np.int64)
    dst = rng.randint(1, N, E).astype(np.int64)
    t = np.sort(np.round(rng.uniform(0.0, 2.0e4, E)))            # rounded: repeated timestamps occur
    eid = np.arange(1, E + 1, dtype=np.int64)
    node_raw = rng.normal(0, 1, (N, Dn)).astype(np.float32)
    node_raw[0] = 0
    edge_raw = rng.normal(0, 1, (E + 1, De)).astype(np.float32)
    edge_raw[0] = 0
    adj = [[] for _ in range(N)]
    for s_, d_, e_, t_ in zip(src, dst, eid, t):                  # utils/utils.py:303-312
        adj[s_].append((d_, e_, t_))
        adj[d_].append((s_, e_, t_))
    sampler = NeighborSampler(adj_list=adj, sample_neighbor_strategy="recent", seed=0)
    rp = RandomProjectionModule(node_num=N, edge_num=E, dim_factor=10, num_layer=L, time_decay_weight=lam, device="cpu",
                                use_matrix=False, beginning_time=np.float64(0.0), not_scale=False, enforce_dim=d)
    model = TPNet(node_raw_features=node_raw, edge_raw_features=edge_raw, neighbor_sampler=sampler, time_feat_dim=Dt, dropout=0.1,
                  random_projections=rp, num_layers=mixers, num_neighbors=K, device="cpu")
    with torch.no_grad():                                         # non-trivial time encoder bias and LayerNorm parameters
        model.time_encoder.w.bias.normal_(0, 0.5)
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0, 0.2)
    out = dict(N=N, E=E, K=K, B=B, Dn=Dn, De=De, Dt=Dt, d=d, L=L, mixers=mixers, lam=lam, src=src, dst=dst, t=t, eid=eid,
               node_raw=node_raw, edge_raw=edge_raw)
    sd = model.state_dict()
    out["sd_keys"] = np.array(list(sd.keys()))
    out["sd_dtypes"] = np.array([str(v.dtype) + str(tuple(v.shape)) for v in sd.values()])
    slot = {}                                                      # the shared modules' tensors appear under two prefixes: stored once
    out["sd_slot"] = np.array([slot.setdefault(v.data_ptr(), len(slot)) for v in sd.values()])
    for v in sd.values():
        out[f"sd_{slot[v.data_ptr()]}"] = v.detach().clone().numpy()

    rec = {}
    emb = model.embedding_module
    emb.projection_layer.register_forward_hook(lambda m, a, o: rec.__setitem__("proj", o.detach().clone().numpy()))
    orig_sample = sampler.get_historical_neighbors

    def sample(node_ids, node_interact_times, num_neighbors=20):
        r = orig_sample(node_ids=node_ids, node_interact_times=node_interact_times, num_neighbors=num_neighbors)
        rec["neigh"], rec["eids"], rec["tn"] = [np.array(x) for x in r]
        return r
    sampler.get_historical_neighbors = sample
    orig_feat = rp.get_pair_wise_feature

    def feat(src_node_ids, dst_node_ids):
        f = orig_feat(src_node_ids=src_node_ids, dst_node_ids=dst_node_ids)
        rec["feat"] = f.detach().clone().numpy()
        return f
    rp.get_pair_wise_feature = feat

    model.eval()
    for b in range(4):
        s = slice(50 * b, 50 * b + 50)
        rp.update(src[s], dst[s], t[s])
    neg = rng.randint(1, N, B).astype(np.int64)
    out["neg"] = neg
    calls = [(slice(200, 200 + B), dst[200:200 + B]), (slice(200 + B, 200 + 2 * B), neg)]
    for c, (s, other) in enumerate(calls):
        with torch.no_grad():
            es, ed = model.compute_src_dst_node_temporal_embeddings(src[s], other, t[s])
        out[f"c{c}_src"], out[f"c{c}_other"], out[f"c{c}_t"] = src[s], other, t[s]
        out[f"c{c}_neigh"], out[f"c{c}_eids"], out[f"c{c}_tn"] = rec["neigh"], rec["eids"], rec["tn"]
        out[f"c{c}_feat"], out[f"c{c}_proj"] = rec["feat"], rec["proj"]
        out[f"c{c}_emb_src"], out[f"c{c}_emb_dst"] = es.numpy(), ed.numpy()
        if c == 0:
            rp.update(src[s], dst[s], t[s])
    # the train()-mode call: call 1 again (no update since), dropout 0, gradients of embeddings.sum()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.train()
    s, other = calls[1]
    es, ed = model.compute_src_dst_node_temporal_embeddings(src[s], other, t[s])
    assert np.array_equal(rec["neigh"], out["c1_neigh"]) and np.array_equal(rec["feat"], out["c1_feat"])
    (es.sum() + ed.sum()).backward()
    out["train_emb_src"], out["train_emb_dst"] = es.detach().numpy(), ed.detach().numpy()
    out["grad_proj0_w"] = emb.projection_layer[0].weight.grad.numpy()
    out["grad_time_w"] = model.time_encoder.w.weight.grad.numpy()
    out["grad_rpmlp0_w"] = rp.mlp[0].weight.grad.numpy()
    path = os.path.join(HERE, "g11_encoder.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
