"""The encoder module (tpnet_amd/encoder.py) and its one-launch input stage (tpnet_amd/fused_input.py, csrc/encoder_input.hip)
against fixture G11 (tests/golden/make_golden_encoder.py: the reference's own TPNet on a toy graph) and against the module's torch
layers at the reference's real widths 172 / 100 / 172 / 64."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = (172, 100, 172, 64)            # node, time, edge feature widths and F of the reference's datasets (utils/DataLoader.py:112-125)


def _g11(golden_dir):
    return np.load(os.path.join(golden_dir, "g11_encoder.npz"))


def _state_dict(g):
    return {str(k): torch.from_numpy(g[f"sd_{int(s)}"]) for k, s in zip(g["sd_keys"], g["sd_slot"])}


def _model(g, device, sampler=None, dropout=0.1):
    """tpnet_amd.TPNet in G11's configuration with the fixture's state dict loaded."""
    import tpnet_amd
    rp = tpnet_amd.RandomProjectionModule(node_num=int(g["N"]), edge_num=int(g["E"]), dim_factor=10, num_layer=int(g["L"]),
                                          time_decay_weight=float(g["lam"]), device=device, use_matrix=False,
                                          beginning_time=np.float64(0.0), not_scale=False, enforce_dim=int(g["d"]))
    model = tpnet_amd.TPNet(node_raw_features=g["node_raw"], edge_raw_features=g["edge_raw"], neighbor_sampler=sampler,
                            time_feat_dim=int(g["Dt"]), dropout=dropout, random_projections=rp, num_layers=int(g["mixers"]),
                            num_neighbors=int(g["K"]), device=device)
    model.load_state_dict(_state_dict(g))
    return model.to(device), rp


def _scaled_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


# ---------------------------------------------------------------------------------------------------------------- CPU tier

def test_state_dict_matches_reference(golden_dir):
    """Keys (the shared random_projections and time_encoder under two prefixes each), order, dtypes and shapes."""
    g = _g11(golden_dir)
    import tpnet_amd
    rp = tpnet_amd.RandomProjectionModule(node_num=int(g["N"]), edge_num=int(g["E"]), dim_factor=10, num_layer=int(g["L"]),
                                          time_decay_weight=float(g["lam"]), device="cpu", use_matrix=False,
                                          beginning_time=np.float64(0.0), not_scale=False, enforce_dim=int(g["d"]))
    model = tpnet_amd.TPNet(node_raw_features=g["node_raw"], edge_raw_features=g["edge_raw"], neighbor_sampler=None,
                            time_feat_dim=int(g["Dt"]), dropout=0.1, random_projections=rp, num_layers=int(g["mixers"]),
                            num_neighbors=int(g["K"]), device="cpu")
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert [str(v.dtype) + str(tuple(v.shape)) for v in sd.values()] == [str(x) for x in g["sd_dtypes"]]
    assert "time_encoder.w.weight" in sd and "embedding_module.time_encoder.w.weight" in sd
    assert "random_projections.mlp.0.weight" in sd and "embedding_module.random_projections.mlp.0.weight" in sd
    assert model.embedding_module.time_encoder is model.time_encoder and model.embedding_module.random_projections is rp
    w0 = 1 / 10 ** np.linspace(0, 9, int(g["Dt"]), dtype=np.float32)
    assert np.array_equal(sd["time_encoder.w.weight"].numpy().reshape(-1), w0) and not sd["time_encoder.w.bias"].any()
    model.load_state_dict(_state_dict(g))
    for name in ("compute_src_dst_node_temporal_embeddings", "set_neighbor_sampler"):
        assert callable(getattr(model, name))
    assert callable(model.embedding_module.compute_node_temporal_embeddings)
    # without relative encodings (random_projections=None): the torch layers on the three raw segments
    plain = tpnet_amd.TPNet(node_raw_features=g["node_raw"], edge_raw_features=g["edge_raw"], neighbor_sampler=None, time_feat_dim=8,
                            dropout=0.0, random_projections=None, num_layers=1, num_neighbors=int(g["K"]), device="cpu")
    assert plain.embedding_module.projection_layer[0].in_features == 20 + 8 + 12
    e = plain.embedding_module.embed_from_features(g["c0_neigh"], g["c0_eids"], g["c0_tn"], np.tile(g["c0_t"], 2), None)
    assert tuple(e.shape) == (2 * int(g["B"]), 20)


def test_embed_from_features_reproduces_reference_on_cpu(golden_dir):
    """The tail behind the readout on the recorded sampler arrays and relative encodings: projection_layer output, embeddings, and
    (train mode, dropout 0) the two dense gradients.  Same torch ops in the same order: rtol 1e-5, atol 1e-6."""
    g = _g11(golden_dir)
    model, _ = _model(g, "cpu")
    emb = model.embedding_module
    rec = {}
    emb.projection_layer.register_forward_hook(lambda m, a, o: rec.__setitem__("proj", o.detach().numpy().copy()))
    model.eval()
    B = int(g["B"])
    for c in (0, 1):
        with torch.no_grad():
            e = emb.embed_from_features(g[f"c{c}_neigh"], g[f"c{c}_eids"], g[f"c{c}_tn"], np.tile(g[f"c{c}_t"], 2),
                                        torch.from_numpy(g[f"c{c}_feat"]))
        np.testing.assert_allclose(rec["proj"], g[f"c{c}_proj"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(e[:B].numpy(), g[f"c{c}_emb_src"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(e[B:].numpy(), g[f"c{c}_emb_dst"], rtol=1e-5, atol=1e-6)
    model, _ = _model(g, "cpu", dropout=0.0)
    model.train()
    e = model.embedding_module.embed_from_features(g["c1_neigh"], g["c1_eids"], g["c1_tn"], np.tile(g["c1_t"], 2),
                                                   torch.from_numpy(g["c1_feat"]))
    np.testing.assert_allclose(e[:B].detach().numpy(), g["train_emb_src"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(e[B:].detach().numpy(), g["train_emb_dst"], rtol=1e-5, atol=1e-6)
    e.sum().backward()
    np.testing.assert_allclose(model.embedding_module.projection_layer[0].weight.grad.numpy(), g["grad_proj0_w"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(model.time_encoder.w.weight.grad.numpy(), g["grad_time_w"], rtol=1e-5, atol=1e-6)


def test_input_stage_answers_by_host_arithmetic(hip_lib):
    """supported / image_bytes make no GPU call; null pointers and nonsense sizes return -1 (TPNET_ERR_BAD_ARG)."""
    L = hip_lib
    assert L.tpnet_encoder_input_supported(172, 100, 172, 64, 344, 172) == 1
    assert L.tpnet_encoder_input_supported(20, 8, 12, 64, 40, 20) == 1
    for F in (16, 36, 64, 100):
        assert L.tpnet_encoder_input_supported(172, 100, 172, F, 344, 172) == 1
    assert L.tpnet_encoder_input_supported(172, 100, 172, 64, 512, 256) == 1
    assert L.tpnet_encoder_input_supported(172, 100, 172, 64, 513, 172) == 0        # H > 512
    assert L.tpnet_encoder_input_supported(172, 100, 172, 64, 344, 260) == 0        # Dout > 256
    assert L.tpnet_encoder_input_supported(400, 100, 400, 64, 344, 172) == 0        # Din > 1024
    assert L.tpnet_encoder_input_supported(170, 100, 172, 64, 344, 172) == 0        # a width that is no multiple of 4
    assert L.tpnet_encoder_input_supported(172, 100, 172, 0, 344, 172) == 0         # no relative encodings: the torch layers
    # chunks of 16-byte operand elements -- KS k-steps of W1, then one chunk per hidden slice of W2 -- and the padded biases.  Up to
    # H = 352 and Dout = 192: one pass of 11 slices, 6 output tiles, chunks of 1 536 elements whatever H and Dout are; beyond: passes
    # of 8 slices, 8 tiles, chunks of 2 048
    assert L.tpnet_encoder_input_image_bytes(172, 100, 172, 64, 344, 172) == (36 + 11) * 1536 * 16 + (11 + 6) * 32 * 4
    assert L.tpnet_encoder_input_image_bytes(20, 8, 12, 64, 40, 20) == (11 + 11) * 1536 * 16 + (11 + 6) * 32 * 4
    assert L.tpnet_encoder_input_image_bytes(172, 100, 172, 64, 512, 256) == 2 * (36 + 8) * 2048 * 16 + (16 + 8) * 32 * 4
    assert L.tpnet_encoder_input_image_bytes(172, 100, 172, 64, 513, 172) == 0
    dims = (ctypes.c_int32 * 6)(172, 100, 172, 64, 344, 172)
    bad = (ctypes.c_int32 * 6)(172, 100, 172, 64, 344, 171)
    assert L.tpnet_encoder_input_prepare(None, None, None, None, dims, None, None) == -1
    assert L.tpnet_encoder_input_prepare(16, 16, 16, 16, None, 16, None) == -1
    assert L.tpnet_encoder_input_prepare(16, 16, 16, 16, bad, 16, None) == -1
    assert L.tpnet_encoder_input_prepare(16, 16, 16, 16, dims, 24, None) == -1       # image not 16-byte aligned
    args = [16, 10, 16, 10, 16, 16, 16, 16, 16, 16, 16, 5, 20, dims, 16, 16, 16, None]
    for i in (0, 2, 4, 5, 6, 7, 8, 9, 10, 13, 14, 15, 16):                           # every pointer null in turn
        a = list(args)
        a[i] = None
        assert L.tpnet_encoder_input(*a) == -1
    for i, v in ((1, 0), (3, -2), (11, -1), (12, 0), (13, bad), (11, 1 << 40)):      # sizes
        a = list(args)
        a[i] = v
        assert L.tpnet_encoder_input(*a) == -1
    a = list(args)
    a[0] = 24                                                                        # node_raw not 16-byte aligned
    assert L.tpnet_encoder_input(*a) == -1
    assert L.tpnet_encoder_input_check(None, None) == -1


def test_encoder_module_never_imports_the_test_side():
    for f in ("encoder.py", "fused_input.py", os.path.join("csrc", "encoder_input.hip")):
        assert "oracle" not in open(os.path.join(ROOT, "tpnet_amd", f)).read(), f


def test_fused_input_declines_what_it_does_not_serve():
    """CPU weights, another layer structure, no relative encodings: prepared() answers None and the torch layers serve."""
    from tpnet_amd import fused_input as fi
    mk = lambda a, b, c: torch.nn.Sequential(torch.nn.Linear(a, b), torch.nn.ReLU(), torch.nn.Linear(b, c))
    assert fi.dims_of(mk(168, 40, 20), 20, 8, 12, 64) == (20, 8, 12, 64, 40, 20)
    assert fi.dims_of(mk(160, 40, 20), 20, 8, 12, 64) is None
    assert fi.dims_of(torch.nn.Identity(), 20, 8, 12, 64) is None
    assert fi.prepared(torch.nn.Identity(), 20, 8, 12, 64) is None
    assert not fi.supported(mk(40, 40, 20), 20, 8, 12, 0)


# ---------------------------------------------------------------------------------------------------------------- GPU tier

def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")


def _samplers(g, kind):
    if kind == "host":
        from tpnet_amd.callers import RecentNeighborSampler
        return RecentNeighborSampler(g["src"], g["dst"], g["t"], g["eid"])
    from tpnet_amd.sampler import GpuRecentNeighborSampler
    return GpuRecentNeighborSampler(g["src"], g["dst"], g["t"], g["eid"], device="cuda:0", num_nodes=int(g["N"]))


def _replay(g, model, rp, upto, grad=False):
    """G11's call sequence on the GPU module: four 50-edge updates, call 0, an update, call 1.  Yields (c, src emb, dst emb)."""
    src, dst, t, B = g["src"], g["dst"], g["t"], int(g["B"])
    for b in range(4):
        s = slice(50 * b, 50 * b + 50)
        rp.update(src[s], dst[s], t[s])
    out = []
    for c in range(upto + 1):
        s = slice(200 + c * B, 200 + (c + 1) * B)
        other = dst[s] if c == 0 else g["neg"]
        if grad and c == upto:
            es, ed = model.compute_src_dst_node_temporal_embeddings(src[s], other, t[s])
        else:
            with torch.no_grad():
                es, ed = model.compute_src_dst_node_temporal_embeddings(src[s], other, t[s])
        out.append((es, ed))
        if c == 0:
            rp.update(src[s], dst[s], t[s])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["host", "device"])
def test_g11_end_to_end_torch_layers(golden_dir, kind):
    """Sampler -> readout -> tail with fused_input off, both sampler kinds: the embeddings of both calls (eval) and of the train-mode
    call (dropout 0) at the decoder fixture's tolerance (rtol 1e-4, atol 1e-5).  The gradients: next test."""
    _need_gpu()
    g = _g11(golden_dir)
    from tpnet_amd import fused_input as fi
    model, rp = _model(g, "cuda:0", _samplers(g, kind))
    model.embedding_module.fused_input = False
    model.eval()
    before = fi.calls["forward"]
    outs = _replay(g, model, rp, 1)
    assert fi.calls["forward"] == before
    for c, (es, ed) in enumerate(outs):
        print(f"G11 torch layers, {kind} sampler, call {c}: scaled err", _scaled_err(es.cpu().numpy(), g[f"c{c}_emb_src"]),
              _scaled_err(ed.cpu().numpy(), g[f"c{c}_emb_dst"]))
        np.testing.assert_allclose(es.cpu().numpy(), g[f"c{c}_emb_src"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(ed.cpu().numpy(), g[f"c{c}_emb_dst"], rtol=1e-4, atol=1e-5)
    model, rp = _model(g, "cuda:0", _samplers(g, kind), dropout=0.0)
    model.embedding_module.fused_input = False
    model.train()
    es, ed = _replay(g, model, rp, 1, grad=True)[1]
    np.testing.assert_allclose(es.detach().cpu().numpy(), g["train_emb_src"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(ed.detach().cpu().numpy(), g["train_emb_dst"], rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["host", "device"])
def test_g11_end_to_end_gradients(golden_dir, kind):
    """The train-mode call of G11 (dropout 0, fused_input off): gradients of embeddings.sum() with respect to
    projection_layer.0.weight, time_encoder.w.weight and random_projections.mlp.0.weight against the reference's, element by
    element at the decoder fixture's tolerance (rtol 1e-4, atol 1e-5).  G11's rows of 16 floats are not served by the anchored
    readout, so the encoder takes the general pair readout and self.mlp as the stock torch layers, forward and backward in true
    fp32.  Measured on an MI355X: no element beyond the tolerance, largest differences 1.6e-5 / 1.7e-5 / 9.1e-6 at gradient
    scales 37.1 / 37.2 / 10.1."""
    _need_gpu()
    g = _g11(golden_dir)
    model, rp = _model(g, "cuda:0", _samplers(g, kind), dropout=0.0)
    model.embedding_module.fused_input = False
    model.train()
    es, ed = _replay(g, model, rp, 1, grad=True)[1]
    (es.sum() + ed.sum()).backward()
    grads = (("grad_proj0_w", model.embedding_module.projection_layer[0].weight), ("grad_time_w", model.time_encoder.w.weight),
             ("grad_rpmlp0_w", rp.mlp[0].weight))
    for name, p in grads:
        got, want = p.grad.cpu().numpy(), g[name]
        beyond = int((np.abs(got - want) > 1e-5 + 1e-4 * np.abs(want)).sum())
        print(f"G11 {name}, {kind} sampler: scaled err {_scaled_err(got, want):.3e}, {beyond} of {want.size} elements beyond the "
              f"tolerance, largest difference {float(np.abs(got - want).max()):.3e}, scale {float(np.abs(want).max()):.3f}")
    for name, p in grads:
        np.testing.assert_allclose(p.grad.cpu().numpy(), g[name], rtol=1e-4, atol=1e-5, err_msg=name)


def _fixture_stage(g, c, dev="cuda:0"):
    """(embedding module, the recorded arrays of call c on the device)"""
    model, _ = _model(g, dev)
    model.eval()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    arrays = (to(g[f"c{c}_neigh"]), to(g[f"c{c}_eids"]), to(g[f"c{c}_tn"]), to(np.tile(g[f"c{c}_t"], 2)), to(g[f"c{c}_feat"]))
    return model.embedding_module, arrays


def _kernel_out(emb, arrays):
    from tpnet_amd import fused_input as fi
    prep = fi.prepared(emb.projection_layer, emb.node_feat_dim, emb.time_feat_dim, emb.edge_feat_dim, emb.random_feature_dim // 2)
    assert prep is not None
    neigh, eids, tn, tq, feat = arrays
    w = emb.time_encoder.w
    return fi.encoder_input(prep, emb.node_raw_features, emb.edge_raw_features, neigh, eids, tn, tq, w.weight, w.bias, feat)


@pytest.mark.gpu
def test_kernel_matches_recorded_projection_output(golden_dir):
    """The kernel at its own output against the reference's projection_layer output (forward hook) on the recorded arrays: the
    project's fp32-class bound err <= 2e-5 * max(1, max|want|).  A repeated call is bitwise equal."""
    _need_gpu()
    g = _g11(golden_dir)
    for c in (0, 1):
        emb, arrays = _fixture_stage(g, c)
        got = _kernel_out(emb, arrays)
        again = _kernel_out(emb, arrays)
        assert torch.equal(got, again)
        want = g[f"c{c}_proj"]
        err = _scaled_err(got.cpu().numpy(), want)
        print(f"kernel vs recorded projection output, call {c}: scaled err {err:.3e}")
        assert got.shape == want.shape and err <= 2e-5
        emb.check_device_errors()


def _real_stage(n_nodes, K, seed, dev="cuda:0", widths=REAL, hidden_out=None, t_offset=0.0):
    """A TPNetEmbedding at 172 / 100 / 172 / 64 (or `widths`) and one call's arrays: pad rows (id 0, edge 0, time 0), repeated ids,
    query times equal to neighbour times.  hidden_out = (H, Dout): a projection_layer of those widths instead of the module's
    2 Dn / Dn, and no mixers behind it (their width is Dn).  t_offset != 0: the query times moved up by it, the deltas log-uniform
    in [0.5, 1e5] with exact 1 (and, as always, 0) among them; pad rows keep time 0."""
    import tpnet_amd
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    Dn, Dt, De, F = widths
    Nn, Ne = 500, 3000
    node_raw = torch.from_numpy(rng.normal(0, 1, (Nn, Dn)).astype(np.float32)).to(dev)
    edge_raw = torch.from_numpy(rng.normal(0, 1, (Ne, De)).astype(np.float32)).to(dev)
    rp_dims = types.SimpleNamespace(pair_wise_feature_dim=F)
    te = tpnet_amd.TimeEncoder(time_dim=Dt)
    emb = tpnet_amd.TPNetEmbedding(node_raw_features=node_raw, edge_raw_features=edge_raw, neighbor_sampler=None, time_encoder=te,
                                   node_feat_dim=Dn, edge_feat_dim=De, time_feat_dim=Dt, num_layers=2, num_neighbors=K, dropout=0.1,
                                   random_projections=rp_dims).to(dev)
    if hidden_out is not None:
        H, Dout = hidden_out
        emb.projection_layer = torch.nn.Sequential(torch.nn.Linear(Dn + Dt + De + 2 * F, H), torch.nn.ReLU(),
                                                   torch.nn.Linear(H, Dout)).to(dev)
        emb.mlp_mixers = torch.nn.ModuleList()
    with torch.no_grad():
        te.w.bias.normal_(0, 0.5)
    emb.eval()
    neigh = rng.randint(1, Nn, (n_nodes, K)).astype(np.int64)
    eids = rng.randint(1, Ne, (n_nodes, K)).astype(np.int64)
    tq = rng.uniform(1e5, 2e6, n_nodes)
    tn = tq[:, None] - rng.uniform(0, 1e5, (n_nodes, K))
    if t_offset:
        tq = tq + t_offset
        delta = np.exp(rng.uniform(np.log(0.5), np.log(1e5), (n_nodes, K)))
        delta[rng.rand(n_nodes, K) < 0.1] = 1.0
        delta[0, K - 1] = 1.0
        tn = tq[:, None] - delta
    pad = rng.rand(n_nodes, K) < 0.2
    neigh[pad], eids[pad], tn[pad] = 0, 0, 0.0
    same = rng.rand(n_nodes, K) < 0.1
    tn[same] = np.broadcast_to(tq[:, None], tn.shape)[same]                 # delta 0: log(1) = 0
    if t_offset:
        tn[0, 0], tn[0, K - 1] = tq[0], tq[0] - 1.0                         # (whatever the draws: one delta 0, one delta 1, ...
        neigh[0, 1], eids[0, 1], tn[0, 1] = 0, 0, 0.0                       #  ... one pad row)
    neigh[:, K // 2] = neigh[:, 0]                                          # repeated ids
    if n_nodes > 1:
        neigh[1], eids[1] = neigh[0], eids[0]
    feat = rng.normal(0, 1, (2 * n_nodes * K, F)).astype(np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return emb, (to(neigh), to(eids), to(tn), to(tq), to(feat))


def _torch_stage(emb, arrays):
    """The module's torch layers up to projection_layer's output (hook), the path embed_from_features takes with fused_input off."""
    rec = {}
    h = emb.projection_layer.register_forward_hook(lambda m, a, o: rec.__setitem__("proj", o.detach()))
    old = emb.fused_input
    emb.fused_input = False
    try:
        with torch.no_grad():
            e = emb.embed_from_features(*arrays)
    finally:
        emb.fused_input = old
        h.remove()
    return rec["proj"], e


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 10, 20])
@pytest.mark.parametrize("n_nodes", [1, 7, 2000])
def test_kernel_matches_torch_layers_at_real_widths(n_nodes, K):
    """172 / 100 / 172 / 64 -> 344 -> 172 against the module's own torch layers: err <= 2e-5 * max(1, max|want|)
    (tests/test_fused_feature.py's fp32-class bound; the three-product scheme simulated at these widths gives 6.9e-6)."""
    _need_gpu()
    emb, arrays = _real_stage(n_nodes, K, seed=100 * n_nodes + K)
    want, _ = _torch_stage(emb, arrays)
    got = _kernel_out(emb, arrays)
    err = _scaled_err(got.cpu().numpy(), want.cpu().numpy())
    print(f"kernel vs torch layers, n_nodes {n_nodes} K {K}: scaled err {err:.3e}, max|want| {float(want.abs().max()):.3f}")
    assert got.shape == want.shape == (n_nodes, K, REAL[0])
    assert err <= 2e-5
    assert torch.equal(got, _kernel_out(emb, arrays))
    emb.check_device_errors()


# Shapes of the kernel's second instantiation (H > 352 or Dout > 192: passes of 8 hidden slices, 8 output tiles): the module's own
# 2 Dn / Dn at Dn = 256 (two full passes), 10 hidden slices with 7 output tiles (a second pass of 2 slices), 13 slices with 2 tiles
WIDE = {"512x256": ((256, 100, 172, 64), None), "320x224": ((256, 100, 172, 64), (320, 224)), "416x64": ((172, 100, 172, 36), (416, 64))}


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes", [7, 300])
@pytest.mark.parametrize("shape", sorted(WIDE))
def test_wide_kernel_matches_torch_layers(shape, n_nodes):
    """The second instantiation against the torch layers, same fp32-class bound: err <= 2e-5 * max(1, max|want|); repeated call
    bitwise equal; no error word set."""
    _need_gpu()
    widths, hidden_out = WIDE[shape]
    emb, arrays = _real_stage(n_nodes, 20, seed=7 * n_nodes, widths=widths, hidden_out=hidden_out)
    from tpnet_amd import _lib
    l1, l2 = emb.projection_layer[0], emb.projection_layer[2]
    assert l1.out_features > 352 or l2.out_features > 192
    assert _lib.load().tpnet_encoder_input_supported(*widths, l1.out_features, l2.out_features) == 1
    want, _ = _torch_stage(emb, arrays)
    got = _kernel_out(emb, arrays)
    err = _scaled_err(got.cpu().numpy(), want.cpu().numpy())
    print(f"wide kernel {shape} vs torch layers, n_nodes {n_nodes}: scaled err {err:.3e}, max|want| {float(want.abs().max()):.3f}")
    assert got.shape == want.shape == (n_nodes, 20, l2.out_features)
    assert err <= 2e-5
    assert torch.equal(got, _kernel_out(emb, arrays))
    emb.check_device_errors()


@pytest.mark.gpu
def test_wide_kernel_reports_bad_ids_and_reads_row_zero():
    _need_gpu()
    emb, (neigh, eids, tn, tq, feat) = _real_stage(50, 20, seed=9, widths=WIDE["512x256"][0])
    bad, zero = eids.clone(), eids.clone()
    bad[3, 2], zero[3, 2] = emb.edge_raw_features.shape[0], 0
    nbad, nzero = neigh.clone(), neigh.clone()
    nbad[40, 19], nzero[40, 19] = -1, 0
    got = _kernel_out(emb, (nbad, bad, tn, tq, feat))
    with pytest.raises(IndexError):
        emb.check_device_errors()
    want = _kernel_out(emb, (nzero, zero, tn, tq, feat))
    emb.check_device_errors()
    assert torch.equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["fixture", "real"] + sorted(WIDE))
def test_kernel_is_exact_on_small_integers(golden_dir, shape):
    """Small-integer features and weights (an asymmetric W), tw = tb = 0 so that the time segment is 1: every product and every
    partial sum is an integer below 2^24, so the output equals the integer result bit for bit -- a wrong lane map or segment offset
    cannot hide behind a tolerance (the style of tests/test_fused_mlp.py's exactness case)."""
    _need_gpu()
    if shape == "fixture":
        g = _g11(golden_dir)
        emb, arrays = _fixture_stage(g, 0)
        neigh, eids, tn, tq, feat = arrays
    elif shape == "real":
        emb, (neigh, eids, tn, tq, feat) = _real_stage(37, 20, seed=5)
    else:
        emb, (neigh, eids, tn, tq, feat) = _real_stage(37, 20, seed=5, widths=WIDE[shape][0], hidden_out=WIDE[shape][1])
    gen = torch.Generator().manual_seed(3)
    ints = lambda shp, lo, hi: torch.randint(lo, hi + 1, shp, generator=gen).float()
    dev = neigh.device
    emb.node_raw_features = ints(tuple(emb.node_raw_features.shape), -3, 3).to(dev)
    emb.edge_raw_features = ints(tuple(emb.edge_raw_features.shape), -3, 3).to(dev)
    feat = ints(tuple(feat.shape), -3, 3).to(dev)
    l1, l2 = emb.projection_layer[0], emb.projection_layer[2]
    with torch.no_grad():
        l1.weight.copy_(ints(tuple(l1.weight.shape), -2, 2))
        l1.bias.copy_(ints(tuple(l1.bias.shape), -5, 5))
        l2.weight.copy_(ints(tuple(l2.weight.shape), -2, 2))
        l2.bias.copy_(ints(tuple(l2.bias.shape), -5, 5))
        emb.time_encoder.w.weight.zero_()
        emb.time_encoder.w.bias.zero_()
    arrays = (neigh, eids, tn, tq, feat)
    got = _kernel_out(emb, arrays).cpu()
    n, K = neigh.shape
    x = torch.cat([emb.node_raw_features[neigh], torch.ones(n, K, emb.time_feat_dim, device=dev), emb.edge_raw_features[eids],
                   torch.cat([feat[:n * K], feat[n * K:]], dim=1).reshape(n, K, -1)], dim=2).double().cpu()
    hid = torch.relu(x @ l1.weight.detach().double().cpu().t() + l1.bias.detach().double().cpu())
    want = hid @ l2.weight.detach().double().cpu().t() + l2.bias.detach().double().cpu()
    assert float(hid.abs().max()) < 2 ** 24 and float(want.abs().max()) < 2 ** 24
    assert torch.equal(got, want.float())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("d", [36, 64])
def test_anchored_readout_branch_end_to_end(golden_dir, monkeypatch, kind, d):
    """Row widths the anchored readout serves (every real dataset's): compute_src_dst_node_temporal_embeddings goes sampler ->
    rp.get_pair_wise_feature_anchored(neigh, tile(src, 2), tile(dst, 2)) -> tail.  G11's graph and raw features with projections of
    d floats, both sampler kinds, fused_input off and on, against an independent route: the host sampler's arrays, the 4BK index
    pattern written out (callers.encoder_pair_indices), the general pair readout (rp.pair_gram) with rp.mlp as the stock torch
    layers, and the torch tail.  Bounds: the relative encodings within the project's fp32-class bound 2e-5 * max(1, max|want|)
    (the anchored call's dense layers are that class; the general readout + torch layers are plain fp32); the embeddings within
    1e-4 * max(1, max|want|), the ceiling the issue derives for an fp32-class perturbation in front of these mixers (simulated:
    1.2e-5) -- a swapped anchor, a wrong tile or row order moves both by 1e-1 and more."""
    _need_gpu()
    import tpnet_amd
    from tpnet_amd import fused_input as fi
    from tpnet_amd.callers import RecentNeighborSampler, encoder_pair_indices
    g = _g11(golden_dir)
    torch.manual_seed(1000 + d)
    rp = tpnet_amd.RandomProjectionModule(node_num=int(g["N"]), edge_num=int(g["E"]), dim_factor=10, num_layer=3,
                                          time_decay_weight=float(g["lam"]), device="cuda:0", use_matrix=False,
                                          beginning_time=np.float64(0.0), not_scale=False, enforce_dim=d)
    K = int(g["K"])
    model = tpnet_amd.TPNet(node_raw_features=g["node_raw"], edge_raw_features=g["edge_raw"], neighbor_sampler=_samplers(g, kind),
                            time_feat_dim=int(g["Dt"]), dropout=0.1, random_projections=rp, num_layers=2, num_neighbors=K,
                            device="cuda:0").to("cuda:0")
    model.eval()
    emb = model.embedding_module
    src, dst, t, B = g["src"], g["dst"], g["t"], int(g["B"])
    for b in range(4):
        s = slice(50 * b, 50 * b + 50)
        rp.update(src[s], dst[s], t[s])
    seen = []
    orig = type(rp).get_pair_wise_feature_anchored

    def spy(self, neighbor_ids, first_anchor_ids, second_anchor_ids):
        seen.append(orig(self, neighbor_ids, first_anchor_ids, second_anchor_ids))
        return seen[-1]
    monkeypatch.setattr(type(rp), "get_pair_wise_feature_anchored", spy)
    host = RecentNeighborSampler(src, dst, t, g["eid"])
    s = slice(200, 200 + B)
    for other in (dst[s], g["neg"]):
        neigh, eids, tn = host.get_historical_neighbors(np.concatenate([src[s], other]), np.tile(t[s], 2), K)
        u, v = encoder_pair_indices(neigh, src[s], other)
        with torch.no_grad():
            want_feat = rp.mlp(rp.pair_gram(u, v))
            emb.fused_input = False
            want = emb.embed_from_features(neigh, eids, tn, np.tile(t[s], 2), want_feat).cpu().numpy()
        for fused in (False, True):
            emb.fused_input = fused
            n_seen, n_fused = len(seen), fi.calls["forward"]
            with torch.no_grad():
                es, ed = model.compute_src_dst_node_temporal_embeddings(src[s], other, t[s])
            assert len(seen) == n_seen + 1 and fi.calls["forward"] == n_fused + int(fused)
            ferr = _scaled_err(seen[-1].cpu().numpy(), want_feat.cpu().numpy())
            eerr = _scaled_err(torch.cat([es, ed]).cpu().numpy(), want)
            print(f"anchored branch, d {d}, {kind} sampler, fused_input {fused}: encodings {ferr:.3e}, embeddings {eerr:.3e} of scale")
            assert tuple(seen[-1].shape) == tuple(want_feat.shape) and ferr <= 2e-5
            assert eerr <= 1e-4
    model.check_device_errors()


# Worst scaled deviation of the embeddings of G11's two calls with the kernel on, measured on an MI355X: 7.971e-6 (the mixers'
# LayerNorms amplify the projection's rounding, so the kernel's own bound above is not reused).  The bound is 3x that value -- the
# kernel is deterministic, the margin covers compiler and machine differences -- and may not exceed 1e-4: a one-product bf16
# projection moves these embeddings by 5.4e-3 of scale, the three-product one by 1.2e-5 in simulation.
G11_FUSED_MEASURED = 7.971e-6
G11_FUSED_BOUND = 3 * G11_FUSED_MEASURED


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["host", "device"])
def test_g11_end_to_end_with_the_kernel(golden_dir, kind):
    """Under no_grad the fused input stage serves both calls (call counter on the binding); embeddings against the fixture."""
    _need_gpu()
    assert G11_FUSED_BOUND <= 1e-4
    g = _g11(golden_dir)
    from tpnet_amd import fused_input as fi
    model, rp = _model(g, "cuda:0", _samplers(g, kind))
    model.embedding_module.fused_input = True
    model.eval()
    before = fi.calls["forward"]
    outs = _replay(g, model, rp, 1)
    assert fi.calls["forward"] == before + 2
    worst = 0.0
    for c, (es, ed) in enumerate(outs):
        worst = max(worst, _scaled_err(es.cpu().numpy(), g[f"c{c}_emb_src"]), _scaled_err(ed.cpu().numpy(), g[f"c{c}_emb_dst"]))
    print(f"G11 with the kernel, {kind} sampler: worst scaled err {worst:.3e} (bound {G11_FUSED_BOUND:.3e})")
    assert worst <= G11_FUSED_BOUND
    model.embedding_module.check_device_errors()


@pytest.mark.gpu
def test_grad_mode_takes_the_torch_layers_and_updates_are_seen(golden_dir):
    """With gradients recorded the fused path is not taken (call counter, not timing); after an optimiser step the next no_grad
    call runs on the new weights (one more prepare launch) and a call without a change re-uses the image."""
    _need_gpu()
    g = _g11(golden_dir)
    from tpnet_amd import fused_input as fi
    emb, arrays = _fixture_stage(g, 1)
    emb.fused_input = True
    with torch.no_grad():
        first = emb.embed_from_features(*arrays)
    f0, p0 = fi.calls["forward"], fi.calls["prepare"]
    with torch.no_grad():
        emb.embed_from_features(*arrays)
    with torch.inference_mode():
        emb.embed_from_features(*arrays)
    assert fi.calls["forward"] == f0 + 2 and fi.calls["prepare"] == p0
    emb.train()
    opt = torch.optim.SGD(emb.projection_layer.parameters(), lr=0.05)
    e = emb.embed_from_features(*arrays)                                   # grad enabled: the torch layers
    assert fi.calls["forward"] == f0 + 2 and e.requires_grad
    e.sum().backward()
    assert emb.projection_layer[0].weight.grad is not None and emb.time_encoder.w.weight.grad is not None
    opt.step()
    emb.eval()
    with torch.no_grad():
        after = emb.embed_from_features(*arrays)
    assert fi.calls["forward"] == f0 + 3 and fi.calls["prepare"] == p0 + 1
    assert not torch.equal(after, first)
    want, _ = _torch_stage(emb, arrays)
    got = _kernel_out(emb, arrays)
    assert fi.calls["prepare"] == p0 + 1
    err = _scaled_err(got.cpu().numpy(), want.cpu().numpy())
    print(f"kernel vs torch layers after an optimiser step: scaled err {err:.3e}")
    assert err <= 2e-5


@pytest.mark.gpu
def test_out_of_range_edge_id_is_reported_and_reads_row_zero(golden_dir):
    """An edge id beyond edge_raw: the launch itself raises nothing, the row reads row 0 (bitwise the output of edge id 0), and the
    check call raises IndexError once."""
    _need_gpu()
    g = _g11(golden_dir)
    emb, (neigh, eids, tn, tq, feat) = _fixture_stage(g, 0)
    emb.check_device_errors()
    bad = eids.clone()
    bad[3, 2] = emb.edge_raw_features.shape[0] + 1000
    bad[5, 0] = -7
    zero = eids.clone()
    zero[3, 2] = 0
    zero[5, 0] = 0
    got = _kernel_out(emb, (neigh, bad, tn, tq, feat))
    with pytest.raises(IndexError):
        emb.check_device_errors()
    emb.check_device_errors()                                              # the word was cleared
    want = _kernel_out(emb, (neigh, zero, tn, tq, feat))
    emb.check_device_errors()
    assert torch.equal(got, want)
    nbad = neigh.clone()
    nbad[0, 0] = emb.node_raw_features.shape[0]
    _kernel_out(emb, (nbad, eids, tn, tq, feat))
    with pytest.raises(IndexError):
        emb.check_device_errors()
