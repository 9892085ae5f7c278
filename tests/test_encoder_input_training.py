"""The encoder's input stage in a training step (tpnet_amd/fused_input.py: encoder_input_train, csrc/encoder_input_train.hip,
TPNetEmbedding.fused_input_training): the forward's bits against encoder_input's, the recorded ReLU decisions and the backward
against float64 evaluations of the expressions at the top of the kernel file, torch autograd bit for bit on small integers.
gy and every output of a direct call are views into larger buffers whose remainder is NaN (a sentinel for the bits)."""
import numpy as np
import pytest
import torch

from test_encoder_module import _g11, _model, _need_gpu, _real_stage, _scaled_err
from test_fused_mixer import _stage

DEV = "cuda:0"
# (Dn, Dt, De, F, H, Dout): the smallest served; a second hidden slice of one unit with two output tiles; the reference's datasets;
# the wide instantiation at its widest (two full passes of 8 slices, 8 output tiles) and at 516 -> 416 -> 64 (13 slices, 2 tiles)
DIMS = {"tiny": (4, 4, 4, 4, 1, 4), "small": (8, 4, 12, 4, 33, 36), "real": (172, 100, 172, 64, 344, 172),
        "wide": (172, 100, 256, 64, 512, 256), "516x416x64": (172, 100, 116, 64, 416, 64)}
# (n_nodes, K, partials offered): one row; across the 32-row tile; across the 128-row workgroup; 5 tiles in 2 (3 + 2), 3 (2 + 2 + 1:
# 4 offered) and 5 parts; 10 tiles in 2, 4 (3 + 3 + 3 + 1) and 5 parts
ROWS = [(1, 1, 32), (33, 1, 32), (129, 1, 32), (7, 20, 2), (7, 20, 4), (7, 20, 5), (15, 20, 2), (15, 20, 4), (15, 20, 5)]
NAMES = ("gw1", "gb1", "gw2", "gb2", "gtw", "gtb")
PAD = 64                                         # floats of NaN on either side of a view (keeps 16-byte alignment)
SENTINEL = 0x5A5A5A5A
# test_g11_end_to_end_gradients: 3 x the worst scaled difference of a Parameter's gradient between the switch on and off measured on an
# MI355X (7.816e-6, projection_layer.0.weight; profiles/encoder_input_training.md); the file's neighbours allow 1e-4
G11_WORST = 7.816e-6
G11_BOUND = 3 * G11_WORST


# ---------------------------------------------------------------------------------------------------------------- CPU tier

def test_sizes_are_host_arithmetic(hip_lib):
    L = hip_lib
    real, tiny = DIMS["real"], DIMS["tiny"]
    assert L.tpnet_encoder_input_bwd_partial_floats(*real) == 344 * 572 + 344 + 172 * 344 + 172 + 2 * 100 == 256652
    assert L.tpnet_encoder_input_bwd_partial_floats(*tiny) == 20 + 1 + 4 + 4 + 8
    # 32-row tiles of 2 pad(H) + pad(Din) + pad(Dout) + pad(Dt) + 1 floats per row
    assert L.tpnet_encoder_input_bwd_workspace_bytes(33, *real) == 2 * 32 * (2 * 352 + 576 + 192 + 128 + 1) * 4
    assert L.tpnet_encoder_input_bwd_workspace_bytes(1, *tiny) == 32 * (2 * 32 + 32 + 32 + 32 + 1) * 4
    assert L.tpnet_encoder_input_bwd_workspace_bytes(0, *real) == 0 and L.tpnet_encoder_input_bwd_workspace_bytes(-1, *real) == 0
    assert L.tpnet_encoder_input_bwd_workspace_bytes((1 << 31) + 1, *real) == 0
    # 3 passes of 36 k-steps + 4 slices, chunks of 8 output tiles (Dt + 2 F = 228 > 192), then b1 padded to 3 x 128 floats
    assert L.tpnet_encoder_input_bwd_image_bytes(*real) == 3 * (36 + 4) * 2048 * 16 + 3 * 128 * 4
    # one pass of 2 k-steps + 4 slices, chunks of 6 output tiles
    assert L.tpnet_encoder_input_bwd_image_bytes(*tiny) == (2 + 4) * 1536 * 16 + 128 * 4
    for name in DIMS:
        assert L.tpnet_encoder_input_supported(*DIMS[name]) == 1 and L.tpnet_encoder_input_bwd_image_bytes(*DIMS[name]) % 16 == 0
    # unserved: the forward's limits, and Dt + 2 F > 256 (which the forward serves)
    assert L.tpnet_encoder_input_supported(172, 132, 172, 64, 344, 172) == 1
    for d in ((172, 132, 172, 64, 344, 172), (172, 100, 172, 80, 344, 172), (170, 100, 172, 64, 344, 172), (172, 100, 172, 64, 0, 172),
              (172, 100, 172, 64, 513, 172), (172, 100, 172, 64, 344, 260), (0, 4, 4, 4, 1, 4), (600, 100, 300, 64, 344, 172)):
        assert L.tpnet_encoder_input_bwd_partial_floats(*d) == 0, d
        assert L.tpnet_encoder_input_bwd_image_bytes(*d) == 0 and L.tpnet_encoder_input_bwd_workspace_bytes(100, *d) == 0, d


def test_bad_arguments_return_without_a_gpu(hip_lib):
    """Null pointers, misaligned arrays, unserved dims, n_partial < 1, gfeat == feat or gy: -1 (TPNET_ERR_BAD_ARG), nothing launched;
    no rows: 0."""
    import ctypes
    L = hip_lib
    real = (ctypes.c_int32 * 6)(*DIMS["real"])
    unserved = (ctypes.c_int32 * 6)(172, 132, 172, 64, 344, 172)                         # (the forward serves it, the backward not)
    odd = (ctypes.c_int32 * 6)(170, 100, 172, 64, 344, 172)
    #      node Nn  edge Ne  neigh eid tn   tq   tw   tb   feat n  K   dims  img  out  bits err  stream
    fwd = [16, 10, 32, 10, 48, 64, 80, 96, 112, 128, 144, 5, 20, real, 160, 176, 192, 208, None]
    for i in (0, 2, 4, 5, 6, 7, 8, 9, 10, 13, 14, 15, 16, 17):                           # every pointer null in turn
        a = list(fwd)
        a[i] = None
        assert L.tpnet_encoder_input_train(*a) == -1, i
    for i, v in ((0, 20), (2, 40), (8, 116), (9, 132), (10, 148), (14, 168), (15, 180), (16, 194), (1, 0), (3, 0), (11, -1), (12, 0),
                 (11, 1 << 40), (13, odd)):
        a = list(fwd)
        a[i] = v
        assert L.tpnet_encoder_input_train(*a) == -1, (i, v)
    #      node Nn  edge Ne  neigh eid tn   tq   tw   tb   feat bits gy   n  K   dims  bimg ws   gfeat tg part np err  stream
    bwd = [16, 10, 32, 10, 48, 64, 80, 96, 112, 128, 144, 160, 176, 5, 20, real, 192, 208, 224, 1, 240, 4, 256, None]
    for i in (0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 17, 20, 22):                   # (gfeat, 18, may be null)
        a = list(bwd)
        a[i] = None
        assert L.tpnet_encoder_input_bwd(*a) == -1, i
    for i, v in ((0, 20), (2, 40), (8, 116), (9, 132), (10, 148), (11, 162), (12, 180), (16, 200), (17, 216), (18, 228), (20, 242),
                 (18, 144), (18, 176), (21, 0), (21, -3), (1, 0), (3, 0), (13, -1), (14, 0), (13, 1 << 40), (15, odd), (15, unserved)):
        a = list(bwd)
        a[i] = v
        assert L.tpnet_encoder_input_bwd(*a) == -1, (i, v)
    for a in ((None, 16, 32, real, 48, None), (16, None, 32, real, 48, None), (16, 32, None, real, 48, None), (16, 32, 48, None, 64, None),
              (16, 32, 48, real, None, None), (16, 32, 48, real, 40, None), (16, 32, 48, odd, 64, None), (16, 32, 48, unserved, 64, None)):
        assert L.tpnet_encoder_input_bwd_prepare(*a) == -1, a
    fwd[11], bwd[13] = 0, 0                                                              # nothing to do, nothing launched
    assert L.tpnet_encoder_input_train(*fwd) == 0 and L.tpnet_encoder_input_bwd(*bwd) == 0
    bwd[18] = None
    assert L.tpnet_encoder_input_bwd(*bwd) == 0


def _grads_of(emb, arrays):
    emb.zero_grad(set_to_none=True)
    emb.embed_from_features(*arrays).sum().backward()
    return {k: p.grad.clone() for k, p in emb.named_parameters() if p.grad is not None}


def test_switch_defaults_to_off_and_a_cpu_model_ignores_it(golden_dir):
    import tpnet_amd
    from tpnet_amd import fused_input as fi
    assert tpnet_amd.TPNetEmbedding.fused_input_training is False
    assert "train_forward" in fi.calls and "backward" in fi.calls
    g = _g11(golden_dir)
    model, _ = _model(g, "cpu", dropout=0.0)
    model.train()
    emb = model.embedding_module
    args = (g["c0_neigh"], g["c0_eids"], g["c0_tn"], np.tile(g["c0_t"], 2), torch.from_numpy(g["c0_feat"]))
    before = dict(fi.calls)
    off = emb.embed_from_features(*args)
    goff = _grads_of(emb, args)
    emb.fused_input_training = True
    on = emb.embed_from_features(*args)
    gon = _grads_of(emb, args)
    assert on.requires_grad and torch.equal(on, off) and fi.calls == before
    assert set(gon) == set(goff) and len(goff) > 0 and all(torch.equal(gon[k], goff[k]) for k in goff)


# ---------------------------------------------------------------------------------------------------------------- references

def _normal_stage(name, n_nodes, K, seed):
    """_real_stage at DIMS[name] with standard-normal projection weights (the time encoder keeps its own: the reference's
    frequencies, a normal bias)."""
    Dn, Dt, De, F, H, Dout = DIMS[name]
    emb, arrays = _real_stage(n_nodes, K, seed=seed, widths=(Dn, Dt, De, F), hidden_out=(H, Dout))
    gen = torch.Generator().manual_seed(7000 + seed)
    with torch.no_grad():
        for p in emb.projection_layer.parameters():
            p.copy_(torch.randn(p.shape, generator=gen))
    return emb, arrays


def _proj(emb):
    l1, l2 = emb.projection_layer[0], emb.projection_layer[2]
    return l1.weight, l1.bias, l2.weight, l2.bias


def _params(emb):
    return _proj(emb) + (emb.time_encoder.w.weight, emb.time_encoder.w.bias)


def _rows64(emb, arrays):
    """The rows in float64 on the host: x [n K, Din], the magnitude xm of the terms x is made of, lt, sin and cos of the time
    arguments and the magnitude argm of the arguments' own terms.  lt is the reference's float32 value (TPNet.py:299-301)."""
    neigh, eids, tn, tq, feat = (a.detach().cpu() for a in arrays)
    D = lambda t: t.detach().double().cpu()
    n, K = neigh.shape
    lt = torch.log((tq[:, None] - tn).float() + 1.0).reshape(-1).double()
    tw, tb = D(emb.time_encoder.w.weight).reshape(-1), D(emb.time_encoder.w.bias)
    arg = lt[:, None] * tw + tb
    argm = (lt[:, None] * tw).abs() + tb.abs()
    nr, er, f = D(emb.node_raw_features)[neigh.reshape(-1)], D(emb.edge_raw_features)[eids.reshape(-1)], D(feat)
    f1, f2 = f[:n * K], f[n * K:]
    s, c = torch.sin(arg), torch.cos(arg)
    x = torch.cat([nr, c, er, f1, f2], 1)
    # a time column is cos(arg) of an argument rounded in float: its terms are |cos| and |sin| (|tw lt| + |tb|)
    xm = torch.cat([nr.abs(), c.abs() + s.abs() * argm, er.abs(), f1.abs(), f2.abs()], 1)
    return dict(x=x, xm=xm, lt=lt, sin=s, cos=c, argm=argm, n=n * K)


def _pre64(emb, R):
    """(a, am): the pre-activations W1 . x + b1 and the sum of the absolute values of their terms."""
    w1, b1 = (t.detach().double().cpu() for t in _proj(emb)[:2])
    return R["x"] @ w1.t() + b1, R["xm"] @ w1.abs().t() + b1.abs()


def _ref64(emb, R, gy, m):
    """The kernel file's expressions in float64 on the host with the decisions m [n K, H] (bool): the six parameter gradients and
    gfeat, and for each the sum of the absolute values of its terms (as test_mixer_channel_training._ref64 derives them; the time
    columns carry the term of their argument's rounding, see _rows64)."""
    w1, b1, w2, b2 = (t.detach().double().cpu() for t in _proj(emb))
    Dn, Dt, De, F = emb.node_feat_dim, emb.time_feat_dim, emb.edge_feat_dim, emb.random_feature_dim // 2
    x, xm, lt = R["x"], R["xm"], R["lt"]
    g = gy.detach().double().cpu().reshape(R["n"], -1)
    m = m.double()
    a, am = _pre64(emb, R)
    h, hm = a * m, am * m
    gh, ghm = g @ w2, g.abs() @ w2.abs()
    ga, gam = gh * m, ghm * m
    wt, wf = w1[:, Dn:Dn + Dt], w1[:, Dn + Dt + De:]
    gxt, gxtm = ga @ wt, gam @ wt.abs()
    d, dm = gxt * -R["sin"], gxtm * (R["sin"].abs() + R["cos"].abs() * R["argm"])
    gxf, gxfm = ga @ wf, gam @ wf.abs()
    grads = (ga.t() @ x, ga.sum(0), g.t() @ h, g.sum(0), (d * lt[:, None]).sum(0)[:, None], d.sum(0))
    mags = (gam.t() @ xm, gam.sum(0), g.abs().t() @ hm, g.abs().sum(0), (dm * lt.abs()[:, None]).sum(0)[:, None], dm.sum(0))
    assert all(gr.shape == t.shape for gr, t in zip(grads, _params(emb)))
    gfeat, gfeatm = torch.cat([gxf[:, :F], gxf[:, F:]], 0), torch.cat([gxfm[:, :F], gxfm[:, F:]], 0)
    return grads + (gfeat,), mags + (gfeatm,)


def _guarded(t=None, shape=None):
    """(buffer, view): the view holds `t` (or NaN, of `shape`) inside a buffer that is NaN on either side."""
    shape = tuple(t.shape) if t is not None else tuple(shape)
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * PAD,), float("nan"), device=DEV)
    view = buf[PAD:PAD + numel].view(shape)
    if t is not None:
        view.copy_(t)
    return buf, view


def _guards_intact(buf):
    if buf.dtype == torch.int32:
        return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[-PAD:]).all())


def _call_args(emb, arrays):
    neigh, eids, tn, tq, feat = arrays
    w = emb.time_encoder.w
    nr, er = emb.node_raw_features, emb.edge_raw_features
    return (nr.data_ptr(), nr.shape[0], er.data_ptr(), er.shape[0], neigh.data_ptr(), eids.data_ptr(), tn.data_ptr(), tq.data_ptr(),
            w.weight.data_ptr(), w.bias.data_ptr(), feat.data_ptr())


def _prep(emb):
    from tpnet_amd import fused_input as fi
    prep = fi.prepared(emb.projection_layer, emb.node_feat_dim, emb.time_feat_dim, emb.edge_feat_dim, emb.random_feature_dim // 2,
                       backward=True)
    assert prep is not None and prep.bimg is not None
    return prep


def _fwd_call(emb, arrays):
    """tpnet_encoder_input_train itself into guarded outputs: (out [n, K, Dout], relu_bits [n K, NW] int32)."""
    from tpnet_amd import _dense, _lib
    prep = _prep(emb)
    n, K = arrays[0].shape
    H, Dout = prep.dims[4], prep.dims[5]
    obuf, out = _guarded(shape=(n, K, Dout))
    NW = (H + 31) // 32
    bbuf = torch.full((n * K * NW + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    bits = bbuf[PAD:PAD + n * K * NW].view(n * K, NW)
    rc = _lib.load().tpnet_encoder_input_train(*_call_args(emb, arrays), n, K, prep.dims, prep.img.data_ptr(), out.data_ptr(),
                                               bits.data_ptr(), prep.err.data_ptr(), _dense.stream_ptr(out.device))
    assert rc == 0 and _guards_intact(obuf) and _guards_intact(bbuf) and bool(torch.isfinite(out).all())
    return out, bits


def _unpack(bits, H):
    """relu_bits [n, NW] int32 -> bool [n, H] on the host, and the check that the bits of the padding are 0."""
    b = bits.cpu().numpy().view(np.uint32)
    full = ((b[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(b.shape[0], -1).astype(bool)
    assert not full[:, H:].any()
    return torch.from_numpy(full[:, :H].copy())


def _bwd_call(emb, arrays, bits, gy, n_partial=32, want_gfeat=True, time_grads=True):
    """tpnet_encoder_input_bwd itself: (rc, the six summed gradients, gfeat or None); partial buffer, workspace and gfeat prefilled
    with NaN, the partials beyond rc and all guards still NaN behind the call."""
    from tpnet_amd import _dense, _lib
    lib = _lib.load()
    prep = _prep(emb)
    d = tuple(prep.dims)
    n, K = arrays[0].shape
    pf = int(lib.tpnet_encoder_input_bwd_partial_floats(*d))
    pbuf, part = _guarded(shape=(n_partial, pf))
    wbuf, ws = _guarded(shape=(int(lib.tpnet_encoder_input_bwd_workspace_bytes(n * K, *d)) // 4,))
    gbuf, gfeat = _guarded(shape=arrays[4].shape) if want_gfeat else (None, None)
    rc = lib.tpnet_encoder_input_bwd(*_call_args(emb, arrays), bits.data_ptr(), gy.data_ptr(), n, K, prep.dims, prep.bimg.data_ptr(),
                                     ws.data_ptr(), None if gfeat is None else gfeat.data_ptr(), int(time_grads), part.data_ptr(),
                                     n_partial, prep.err.data_ptr(), _dense.stream_ptr(gy.device))
    tiles = (n * K + 31) // 32
    per_part = (tiles + n_partial - 1) // n_partial
    assert 1 <= rc <= n_partial and rc == (tiles + per_part - 1) // per_part          # equal parts, none empty
    assert _guards_intact(pbuf) and _guards_intact(wbuf) and (gbuf is None or _guards_intact(gbuf))
    assert bool(torch.isnan(part[rc:]).all()) and bool(torch.isfinite(part[:rc]).all())
    assert gfeat is None or bool(torch.isfinite(gfeat).all())
    tot, out, off = part[:rc].sum(0), [], 0
    for t in _params(emb):
        out.append(tot[off:off + t.numel()].view(t.shape))
        off += t.numel()
    assert off == tot.numel()
    return rc, out, gfeat


def _check(tag, got, ref, keep=None):
    """|err| <= 4e-5 mag + 1e-6 max|want| per entry of the six gradients and gfeat (None: not compared); prints the largest
    err / bound per tensor.  keep[name]: a bool mask of the entries to compare (all without one)."""
    want, mags = ref
    worst = {}
    for name, gt, wt, mg in zip(NAMES + ("gfeat",), got, want, mags):
        if gt is None:
            continue
        err = (gt.detach().double().cpu() - wt).abs()
        bound = 4e-5 * mg + 1e-6 * float(wt.abs().max())
        # (a bound of 0 -- one row whose only unit is off -- asks for err = 0: 0 <= 0 holds, anything else does not)
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
        if keep is not None and name in keep:
            ratio = ratio[keep[name]]
        worst[name] = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{tag}: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(np.isfinite(v) and v <= 1.0 for v in worst.values()), worst


_CASES = {}


def _case(name, n_nodes, K):
    """One stage, its gy, the train forward's (out, bits) and the float64 rows, computed once per (dims, rows) and shared."""
    key = (name, n_nodes, K)
    if key not in _CASES:
        seed = 11 * n_nodes + K + len(name)
        emb, arrays = _normal_stage(name, n_nodes, K, seed)
        gen = torch.Generator().manual_seed(2000 + seed)
        gy = _guarded(torch.randn(n_nodes, K, DIMS[name][5], generator=gen).to(DEV))[1]
        out, bits = _fwd_call(emb, arrays)
        R = _rows64(emb, arrays)
        _CASES[key] = dict(emb=emb, arrays=arrays, gy=gy, out=out, bits=bits, R=R, m=_unpack(bits, DIMS[name][4]))
    return _CASES[key]


def _band(emb, R):
    """(a64, the bool mask of the units whose decision float32-class arithmetic may take either way: |a64| <= 2e-5 (sum |w1||x| + |b1|))"""
    a, am = _pre64(emb, R)
    return a, a.abs() <= 2e-5 * am


CASES = [(name, n, K, parts) for name in DIMS for n, K, parts in ROWS] + [("real", 300, 20, None)]


# ---------------------------------------------------------------------------------------------------------------- GPU tier

@pytest.mark.gpu
@pytest.mark.parametrize("name,n_nodes,K", sorted({c[:3] for c in CASES}))
def test_forward_bits_and_mask_against_float64(name, n_nodes, K):
    """out of the train forward has the bits of fused_input.encoder_input; the recorded decisions equal a64 > 0 for every unit outside
    the band |a64| <= 2e-5 (sum |w1||x| + |b1|) (the forward's fp32-class bound), the band holds at most 1 % of the units, the bits of
    padded units are 0 (_unpack) and a second launch gives the same bits."""
    _need_gpu()
    from tpnet_amd import fused_input as fi
    c = _case(name, n_nodes, K)
    emb, arrays = c["emb"], c["arrays"]
    w = emb.time_encoder.w
    with torch.no_grad():
        want = fi.encoder_input(_prep(emb), emb.node_raw_features, emb.edge_raw_features, *arrays[:4], w.weight, w.bias, arrays[4])
    assert torch.equal(c["out"], want)
    a, band = _band(emb, c["R"])
    share = float(band.double().mean())
    print(f"{name} ({n_nodes}, {K}): {int(band.sum())} of {band.numel()} units inside the band ({share:.2e})")
    assert share <= 0.01
    assert torch.equal(c["m"][~band], (a > 0)[~band])
    out2, bits2 = _fwd_call(emb, arrays)
    assert torch.equal(out2, c["out"]) and torch.equal(bits2, c["bits"])
    emb.check_device_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_nodes,K,parts", CASES)
def test_backward_against_float64(name, n_nodes, K, parts):
    """Every partial-summed tensor and gfeat against the float64 evaluation with the exported bits: |err| <= 4e-5 mag + 1e-6 max|want|.
    A second call gives equal bits in every output; without gfeat and without the time gradients the others keep their bits and
    gtw / gtb are zeros.  Guards: _bwd_call."""
    _need_gpu()
    from tpnet_amd import fused_input as fi
    c = _case(name, n_nodes, K)
    emb, arrays, gy, bits = c["emb"], c["arrays"], c["gy"], c["bits"]
    parts = fi.MAX_PARTIALS if parts is None else parts
    rc, got, gfeat = _bwd_call(emb, arrays, bits, gy, n_partial=parts)
    _check(f"{name} ({n_nodes}, {K}) in {rc} parts", got + [gfeat], _ref64(emb, c["R"], gy, c["m"]))
    rc2, again, gfeat2 = _bwd_call(emb, arrays, bits, gy, n_partial=parts)
    assert rc2 == rc and torch.equal(gfeat2, gfeat) and all(torch.equal(a, b) for a, b in zip(again, got))
    rc3, bare, none = _bwd_call(emb, arrays, bits, gy, n_partial=parts, want_gfeat=False, time_grads=False)
    assert rc3 == rc and none is None and all(torch.equal(a, b) for a, b in zip(bare[:4], got[:4]))
    assert not bool(bare[4].any()) and not bool(bare[5].any())
    emb.check_device_errors()


def _int_stage(name, n_nodes, K):
    """_real_stage at DIMS[name] with small-integer tables, relative encodings and projection weights and tw = tb = 0, so that the
    time columns are exactly 1 and every product and partial sum is an integer below 2^24."""
    Dn, Dt, De, F, H, Dout = DIMS[name]
    emb, (neigh, eids, tn, tq, feat) = _real_stage(n_nodes, K, seed=5, widths=(Dn, Dt, De, F), hidden_out=(H, Dout))
    gen = torch.Generator().manual_seed(3)
    ints = lambda shp, lo, hi: torch.randint(lo, hi + 1, tuple(shp), generator=gen).float()
    emb.node_raw_features = ints(emb.node_raw_features.shape, -3, 3).to(DEV)
    emb.edge_raw_features = ints(emb.edge_raw_features.shape, -3, 3).to(DEV)
    feat = ints(feat.shape, -3, 3).to(DEV)
    l1, l2 = emb.projection_layer[0], emb.projection_layer[2]
    with torch.no_grad():
        l1.weight.copy_(ints(l1.weight.shape, -2, 2))
        l1.bias.copy_(ints(l1.bias.shape, -5, 5))
        l2.weight.copy_(ints(l2.weight.shape, -2, 2))
        l2.bias.copy_(ints(l2.bias.shape, -5, 5))
        emb.time_encoder.w.weight.zero_()
        emb.time_encoder.w.bias.zero_()
    gy = ints((n_nodes, K, Dout), -2, 2).to(DEV)
    return emb, (neigh, eids, tn, tq, feat), gy


def _torch_grads(emb, arrays, gy):
    """torch autograd through the module's torch layers (the route with the switch off) from gy at projection_layer's output: the
    gradients of the six Parameters and of feats."""
    neigh, eids, tn, tq, feat = arrays
    feat = feat.detach().clone().requires_grad_(True)
    rec = {}
    hook = emb.projection_layer.register_forward_hook(lambda m, a, o: rec.__setitem__("proj", o))
    assert not emb.fused_input_training
    try:
        emb.zero_grad(set_to_none=True)
        emb.embed_from_features(neigh, eids, tn, tq, feat)
    finally:
        hook.remove()
    rec["proj"].backward(gy)
    return [p.grad for p in _params(emb)] + [feat.grad]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["real", "wide", "516x416x64", "small"])
def test_small_integers_bit_for_bit(name):
    """Small-integer sources, weights and gy with tw = tb = 0: every gradient has the bits of torch autograd through the torch layers,
    at both instantiations of the forward -- a wrong lane map, segment offset or mask bit cannot hide behind a tolerance."""
    _need_gpu()
    emb, arrays, gy = _int_stage(name, 7, 20)
    want = _torch_grads(emb, arrays, gy)
    out, bits = _fwd_call(emb, arrays)
    R = _rows64(emb, arrays)
    a, am = _pre64(emb, R)
    assert float(am.max()) < 2 ** 16                                                   # (two bf16 pieces hold the hidden layer exactly)
    assert torch.equal(_unpack(bits, DIMS[name][4]), a > 0)
    rc, got, gfeat = _bwd_call(emb, arrays, bits, gy, n_partial=3)
    ref, mags = _ref64(emb, R, gy, a > 0)
    assert all(float(mg.max()) < 2 ** 24 for mg in mags)
    for nm, gt, wt in zip(NAMES + ("gfeat",), got + [gfeat], want):
        assert wt is not None and torch.equal(gt, wt.view(gt.shape)), nm
    assert not bool(got[4].any()) and not bool(got[5].any())                           # sin 0 = 0: no time gradient at all


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "real"])
def test_rows_are_independent(name):
    """The first 1 / 33 / 129 rows of a 300-row call give the shorter calls' relu_bits and gfeat bits."""
    _need_gpu()
    big = _case(name, 300, 1)
    emb, (neigh, eids, tn, tq, feat), gy = big["emb"], big["arrays"], big["gy"]
    _, _, gfeat = _bwd_call(emb, big["arrays"], big["bits"], gy)
    for m in (1, 33, 129):
        arrays = (neigh[:m].contiguous(), eids[:m].contiguous(), tn[:m].contiguous(), tq[:m].contiguous(),
                  torch.cat([feat[:m], feat[300:300 + m]]).contiguous())
        out, bits = _fwd_call(emb, arrays)
        assert torch.equal(bits, big["bits"][:m]) and torch.equal(out, big["out"][:m])
        _, _, gf = _bwd_call(emb, arrays, bits, _guarded(gy[:m])[1])
        assert torch.equal(gf, torch.cat([gfeat[:m], gfeat[300:300 + m]]))


def _leaves(emb, arrays):
    neigh, eids, tn, tq, feat = arrays
    return neigh, eids, tn, tq, feat.detach().clone().requires_grad_(True)


def _train_call(emb, arrays, **kw):
    from tpnet_amd import fused_input as fi
    return fi.encoder_input_train(emb.projection_layer, emb.time_encoder, emb.node_raw_features, emb.edge_raw_features, *arrays, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "real", "wide"])
@pytest.mark.parametrize("n_nodes,K", [(1, 1), (33, 1), (7, 20)])
def test_autograd_through_encoder_input_train(name, n_nodes, K):
    """Through encoder_input_train the gradients of the six Parameters and of feats against float64 autograd through the torch
    layers' expressions (ReLU deciding on a64 > 0), within the bound for every unit outside the band: rows of gw1 / gb1 and columns
    of gw2 of a unit with a row inside the band, gfeat of such a row and -- if any unit is inside -- gtw / gtb are not compared.
    A frozen time encoder gets None and leaves the others' bits; feats without a gradient gets none."""
    _need_gpu()
    from tpnet_amd import fused_input as fi
    c = _case(name, n_nodes, K)
    emb, gy, R = c["emb"], c["gy"], c["R"]
    a, band = _band(emb, R)
    # float64 autograd through Linear -> ReLU -> Linear and cos(Linear(1, Dt)) on the host
    P = [t.detach().double().cpu().requires_grad_(True) for t in _params(emb)]
    f64 = c["arrays"][4].detach().double().cpu().requires_grad_(True)
    Dn, Dt, De = emb.node_feat_dim, emb.time_feat_dim, emb.edge_feat_dim
    nk = R["n"]
    x = torch.cat([R["x"][:, :Dn], torch.cos(R["lt"][:, None] @ P[4].t() + P[5]), R["x"][:, Dn + Dt:Dn + Dt + De], f64[:nk], f64[nk:]], 1)
    y = torch.relu(x @ P[0].t() + P[1]) @ P[2].t() + P[3]
    y.backward(gy.detach().double().cpu().reshape(nk, -1))
    want = tuple(p.grad for p in P) + (f64.grad,)
    _, mags = _ref64(emb, R, gy, a > 0)
    clean_u, clean_r, none = ~band.any(0), ~band.any(1), not bool(band.any())
    keep = {"gw1": clean_u[:, None].expand_as(want[0]), "gb1": clean_u, "gw2": clean_u[None, :].expand_as(want[2]),
            "gtw": torch.full_like(want[4], none, dtype=torch.bool), "gtb": torch.full_like(want[5], none, dtype=torch.bool),
            "gfeat": torch.cat([clean_r, clean_r])[:, None].expand_as(want[6])}
    arrays = _leaves(emb, c["arrays"])
    emb.zero_grad(set_to_none=True)
    c0 = dict(fi.calls)
    out = _train_call(emb, arrays)
    assert torch.equal(out, c["out"]) and out.requires_grad
    out.backward(gy)
    assert fi.calls["train_forward"] == c0["train_forward"] + 1 and fi.calls["backward"] == c0["backward"] + 1
    got = [p.grad.clone() for p in _params(emb)] + [arrays[4].grad.clone()]
    _check(f"autograd {name} ({n_nodes}, {K}), {int(band.sum())} units in the band", got, (want, mags), keep)
    # a frozen time encoder; feats without a gradient
    emb.zero_grad(set_to_none=True)
    for p in emb.time_encoder.parameters():
        p.requires_grad_(False)
    try:
        plain = c["arrays"]
        assert not plain[4].requires_grad
        _train_call(emb, plain).backward(gy)
        assert emb.time_encoder.w.weight.grad is None and emb.time_encoder.w.bias.grad is None
        assert all(torch.equal(p.grad, g) for p, g in zip(_proj(emb), got[:4]))
    finally:
        for p in emb.time_encoder.parameters():
            p.requires_grad_(True)


@pytest.mark.gpu
def test_feats_without_a_gradient_computes_no_gfeat(monkeypatch):
    """The backward is called with gfeat = NULL when feats needs no gradient, and with time_grads = 0 when the time encoder is frozen."""
    _need_gpu()
    from tpnet_amd import _lib
    c = _case("small", 7, 20)
    emb = c["emb"]
    lib = _lib.load()
    seen = []

    class Spy:
        def __getattr__(self, k):
            f = getattr(lib, k)
            if k != "tpnet_encoder_input_bwd":
                return f
            return lambda *a: (seen.append((a[18], a[19])), f(*a))[1]

    monkeypatch.setattr(_lib, "load", lambda: Spy())
    emb.zero_grad(set_to_none=True)
    _train_call(emb, c["arrays"]).backward(c["gy"])
    _train_call(emb, _leaves(emb, c["arrays"])).backward(c["gy"])
    for p in emb.time_encoder.parameters():
        p.requires_grad_(False)
    try:
        _train_call(emb, c["arrays"]).backward(c["gy"])
    finally:
        for p in emb.time_encoder.parameters():
            p.requires_grad_(True)
    assert [(g is None, t) for g, t in seen] == [(True, 1), (False, 1), (True, 0)]


@pytest.mark.gpu
def test_bad_ids_are_reported_after_a_backward_as_after_a_forward():
    _need_gpu()
    emb, (neigh, eids, tn, tq, feat) = _normal_stage("small", 15, 20, seed=21)
    bad, zero = eids.clone(), eids.clone()
    bad[3, 2], zero[3, 2] = emb.edge_raw_features.shape[0], 0
    nbad, nzero = neigh.clone(), neigh.clone()
    nbad[14, 19], nzero[14, 19] = -1, 0
    gy = torch.randn(15, 20, DIMS["small"][5], device=DEV)
    out = _train_call(emb, (nbad, bad, tn, tq, feat))
    with pytest.raises(IndexError):
        emb.check_device_errors()
    emb.check_device_errors()                                                           # (cleared)
    out.backward(gy)
    with pytest.raises(IndexError):
        emb.check_device_errors()
    got = [p.grad.clone() for p in _params(emb)]
    emb.zero_grad(set_to_none=True)
    want = _train_call(emb, (nzero, zero, tn, tq, feat))
    want.backward(gy)
    emb.check_device_errors()
    assert torch.equal(out, want) and all(torch.equal(a, p.grad) for a, p in zip(got, _params(emb)))


@pytest.mark.gpu
def test_no_rows_and_a_changed_part_count(monkeypatch):
    """n = 0 gives an empty output, zero gradients of the right shapes and no launch; another fused_input.MAX_PARTIALS sizes a new
    partial buffer and gives gradients within the bound."""
    _need_gpu()
    from tpnet_amd import fused_input as fi
    emb, arrays = _normal_stage("small", 0, 20, seed=4)
    arrays = _leaves(emb, arrays)
    c0 = dict(fi.calls)
    y = _train_call(emb, arrays)
    assert y.shape == (0, 20, DIMS["small"][5]) and y.requires_grad
    y.backward(torch.empty_like(y))
    assert fi.calls["train_forward"] == c0["train_forward"] and fi.calls["backward"] == c0["backward"]
    for t in _params(emb) + (arrays[4],):
        assert t.grad is not None and t.grad.shape == t.shape and not bool(t.grad.any())
    c = _case("small", 15, 20)
    emb = c["emb"]
    ref = _ref64(emb, c["R"], c["gy"], c["m"])
    for parts in (3, 64):
        monkeypatch.setattr(fi, "MAX_PARTIALS", parts)
        emb.zero_grad(set_to_none=True)
        arrays = _leaves(emb, c["arrays"])
        _train_call(emb, arrays).backward(c["gy"])
        _check(f"MAX_PARTIALS {parts}", [p.grad for p in _params(emb)] + [arrays[4].grad], ref)


@pytest.mark.gpu
def test_parameter_updates_are_seen_by_the_next_call():
    """After an optimiser step both images are rewritten once (calls["prepare"]) and the next forward and backward run on the new
    weights; an in-place change between forward and backward raises as torch does."""
    _need_gpu()
    from tpnet_amd import fused_input as fi
    emb, arrays = _normal_stage("small", 7, 20, seed=9)
    gy = torch.randn(7, 20, DIMS["small"][5], device=DEV)
    opt = torch.optim.SGD(emb.projection_layer.parameters(), lr=0.01)
    c0 = dict(fi.calls)
    first = _train_call(emb, arrays)
    assert fi.calls["prepare"] == c0["prepare"] + 1
    first.backward(gy)
    assert fi.calls["prepare"] == c0["prepare"] + 1 and fi.cached(emb.projection_layer).bimg is not None
    opt.step()
    emb.zero_grad(set_to_none=True)
    after = _train_call(emb, arrays)
    assert fi.calls["prepare"] == c0["prepare"] + 2 and not torch.equal(after, first)
    out, bits = _fwd_call(emb, arrays)
    assert fi.calls["prepare"] == c0["prepare"] + 2 and torch.equal(out, after)
    after.backward(gy)
    assert fi.calls["prepare"] == c0["prepare"] + 2
    _check("after an optimiser step", [p.grad for p in _params(emb)] + [None],
           _ref64(emb, _rows64(emb, arrays), gy, _unpack(bits, DIMS["small"][4])))
    y = _train_call(emb, arrays)
    with torch.no_grad():
        emb.projection_layer[0].weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(gy)
    fi.invalidate(emb.projection_layer)
    assert fi.cached(emb.projection_layer) is None


@pytest.mark.gpu
def test_dispatch_on_g11(golden_dir):
    """Call counters on G11's embedding module: train_forward / backward move once per call exactly when the switch is on and a
    gradient is recorded, and forward does not; under no_grad k_encoder_input serves as before; with the switch off nothing new is
    called.  The switch combines with the mixers' two."""
    _need_gpu()
    g = _g11(golden_dir)
    from tpnet_amd import fused_input as fi, fused_mixer as fm
    emb, arrays = _stage(g, 0.0)
    emb.train()
    moved = lambda c0: {k: fi.calls[k] - c0[k] for k in fi.calls if fi.calls[k] != c0[k] and k != "prepare"}
    c0 = dict(fi.calls)
    _grads_of(emb, arrays)                                                              # the default switches: torch
    assert moved(c0) == {}
    emb.fused_input_training = True
    for mixers in (False, True):
        emb.fused_token_training = emb.fused_channel_training = mixers
        c0, m0 = dict(fi.calls), dict(fm.calls)
        out = emb.embed_from_features(*arrays)
        assert out.requires_grad and moved(c0) == {"train_forward": 1}
        c1 = dict(fi.calls)
        out.sum().backward()
        assert moved(c1) == {"backward": 1}
        assert (fm.calls["channel_bwd"] - m0["channel_bwd"], fm.calls["token_bwd"] - m0["token_bwd"]) == ((2, 2) if mixers else (0, 0))
        c2 = dict(fi.calls)
        with torch.no_grad():
            emb.embed_from_features(*arrays)                                            # no gradient: k_encoder_input
        assert moved(c2) == {"forward": 1}
    emb.check_device_errors()
    emb.fused_input_training = False
    c3 = dict(fi.calls)
    _grads_of(emb, arrays)
    assert moved(c3) == {}


@pytest.mark.gpu
def test_g11_end_to_end_gradients(golden_dir):
    """G11 at dropout 0: the gradients of embeddings.sum() for all Parameters with the switch on against off (the torch layers are
    the reference), scaled as test_encoder_module._scaled_err scales: within G11_BOUND."""
    _need_gpu()
    g = _g11(golden_dir)
    emb, arrays = _stage(g, 0.0)
    emb.train()
    off = _grads_of(emb, arrays)
    emb.fused_input_training = True
    on = _grads_of(emb, arrays)
    print(f"G11: {len(off)} Parameters with a gradient")
    assert set(on) == set(off) and len(off) == 30
    worst = {k: _scaled_err(on[k].cpu().numpy(), off[k].cpu().numpy()) for k in off}
    top = max(worst, key=worst.get)
    print(f"G11 gradients, fused_input_training on against off: worst scaled difference {worst[top]:.3e} ({top})")
    assert G11_BOUND < 1e-4 and worst[top] <= G11_BOUND
