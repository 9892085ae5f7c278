"""The device optimizer step on the GPU (tpnet_amd/optimizer.py, csrc/optimizer.hip: k_optim_step).

Bits: the kernel against `optimizer_step_host`, which restates its operation order in numpy -- equal words, for every rule, over five
steps, on tensors that meet every edge of the kernel (sizes around the workgroup's chunk and the float4, a Parameter and a gradient
that start 4 bytes into their buffers, more tensors than one launch takes, two param groups, a tensor whose step count lags), with 64
guard floats either side of every buffer.
Torch: the yardstick of tests/test_optimizer_host.py with both torch optimizers on the GPU.
Version contract: `_dense.param_key` moves with a step, and the forwards that read the Parameters see the new weights.
A training epoch with the device step against one with torch's; no synchronisation; a CPU Parameter among GPU ones."""
import copy
import logging

import numpy as np
import pytest
import torch

from tpnet_amd import _dense, _lib
from tpnet_amd import optimizer as O
from test_optimizer_host import DEVICE, LR, SHAPES, TORCH, check_yardstick, gradient, scalars_of

DEV = "cuda:0"
PAD = 64
GUARD = -777.25
RULE_NAMES = ["Adam", "SGD", "RMSprop"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")


def _guarded(n, shift=0):
    """-> (buffer, view): n floats that start PAD + shift floats into a buffer of GUARD words, PAD of them behind the view too."""
    buf = torch.full((PAD + shift + n + PAD,), GUARD, dtype=torch.float32, device=DEV)
    return buf, buf[PAD + shift:PAD + shift + n]


def _intact(buf, n, shift=0):
    return bool((buf[:PAD + shift] == GUARD).all() and (buf[PAD + shift + n:] == GUARD).all())


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _edge_set():
    """[(n, shift of p, shift of g)]: the second launch gets the largest tensor and the misaligned ones."""
    chunk, cap = _lib.load().tpnet_optim_chunk(), _lib.load().tpnet_optim_max_tensors()
    head = [(chunk + 1, 0, 0), (0, 0, 0), (1, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0), (chunk - 1, 0, 0), (chunk, 0, 0)]
    tail = [(9, 0, 1), (2 * chunk + 7, 0, 0), (chunk + 5, 1, 0)]
    fill = [(2 + 3 * i, 0, 0) for i in range(cap + 4 - len(head) - len(tail))]
    cases = head + fill + tail
    assert len(cases) == cap + 4 and sum(1 for c in cases if c[0] > 0) == cap + 3
    return cases, chunk, cap


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULE_NAMES)
def test_kernel_bits_equal_the_host_restatement(rule):
    _need_gpu()
    cases, chunk, cap = _edge_set()
    rng = np.random.RandomState(21)
    half = len(cases) // 2
    hyper = [dict(lr=LR[rule], weight_decay=0.01), dict(lr=3.0 * LR[rule], weight_decay=0.0)]
    if rule == "Adam":
        hyper[0]["betas"], hyper[1]["betas"] = (0.9, 0.999), (0.8, 0.99)
    if rule == "RMSprop":
        hyper[0]["alpha"], hyper[1]["alpha"] = 0.99, 0.9
    params, bufs, host = [], [], []
    for n, sp, sg in cases:
        x = rng.standard_normal(n).astype(np.float32)
        pb, pv = _guarded(n, sp)
        gb, gv = _guarded(n, sg)
        pv.copy_(torch.from_numpy(x))
        p = torch.nn.Parameter(pv)
        assert p.data_ptr() == pv.data_ptr() and (p.data_ptr() % 16 == 0) == (sp == 0)
        params.append(p)
        bufs.append([(pb, n, sp), (gb, n, sg)])
        host.append(dict(p=x, s1=np.zeros(n, np.float32), s2=np.zeros(n, np.float32), t=0, g=gv))
    opt = DEVICE[rule]([dict(params=params[:half], **hyper[0]), dict(params=params[half:], **hyper[1])])
    if rule != "SGD":                                          # the state in guarded buffers too (as a loaded state_dict would set it)
        for p, (n, sp, sg), b in zip(params, cases, bufs):
            st = {"step": torch.tensor(0.0)}
            for name in (("exp_avg", "exp_avg_sq") if rule == "Adam" else ("square_avg",)):
                sb, sv = _guarded(n)
                sv.zero_()
                st[name] = sv.view(p.shape)
                b.append((sb, n, 0))
            opt.state[p] = st
    lagging = 3                                                # no gradient in steps 2 and 3
    for step in range(1, 6):
        for k, (p, h) in enumerate(zip(params, host)):
            if k == lagging and step in (2, 3):
                p.grad = None
                continue
            g = gradient(rng, p.shape)
            h["g"].copy_(torch.from_numpy(g))
            p.grad = h["g"]
            h["t"] += 1
            hp = hyper[0 if k < half else 1]
            c = scalars_of(rule, hp["lr"], hp["weight_decay"], h["t"], betas=hp.get("betas"), alpha=hp.get("alpha"))
            h["p"], s1, s2 = O.optimizer_step_host(rule, h["p"], g, h["s1"], h["s2"], c)
            h["s1"], h["s2"] = (s1 if s1 is not None else h["s1"]), (s2 if s2 is not None else h["s2"])
        opt.step()
        for k, (p, h) in enumerate(zip(params, host)):
            assert np.array_equal(_bits(p.detach().cpu().numpy()), _bits(h["p"])), (rule, step, k, cases[k])
            if rule != "SGD":
                names = ("exp_avg", "exp_avg_sq") if rule == "Adam" else ("square_avg",)
                for name, key in zip(names, ("s1", "s2")):
                    assert np.array_equal(_bits(opt.state[p][name].cpu().numpy()), _bits(h[key])), (rule, step, k, name)
                assert float(opt.state[p]["step"]) == h["t"]
    assert host[lagging]["t"] == 3 and host[0]["t"] == 5
    for b in bufs:
        for buf, n, shift in b:
            assert _intact(buf, n, shift)


def _gpu_yardstick(rule, wd, steps, marks, reload_at):
    """The host tier's yardstick with torch's float64 and fp32 optimizers on the GPU and the device class as the third run.  After step
    `reload_at` a fresh device optimizer over copies of torch's fp32 parameters loads torch's state_dict and goes on beside them:
    its rows are keyed (step, 'loaded')."""
    rng = np.random.RandomState(31)
    p0 = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    mk = lambda dtype: [torch.nn.Parameter(torch.from_numpy(x).to(DEV, dtype)) for x in p0]
    p64, p32, pm = mk(torch.float64), mk(torch.float32), mk(torch.float32)
    o64 = TORCH[rule](p64, lr=LR[rule], weight_decay=wd, foreach=False)
    o32 = TORCH[rule](p32, lr=LR[rule], weight_decay=wd, foreach=False)
    om = DEVICE[rule](pm, lr=LR[rule], weight_decay=wd)
    runs = [(p64, o64), (p32, o32), (pm, om)]
    pl = None
    out = {}
    for step in range(1, steps + 1):
        grads = [torch.from_numpy(gradient(rng, s)).to(DEV) for s in SHAPES]
        for params, opt in runs:
            for p, g in zip(params, grads):
                p.grad = g.to(p.dtype).clone()
            opt.step()
        for key, mine in ((step, pm), ((step, "loaded"), pl)):
            if mine is not None and step in marks:
                out[key] = []
                for p, a, b in zip(mine, p64, p32):
                    ref = a.detach().cpu().numpy()
                    out[key].append((np.abs(p.detach().cpu().numpy().astype(np.float64) - ref).max(),
                                     np.abs(b.detach().cpu().numpy().astype(np.float64) - ref).max(),
                                     float(np.spacing(np.float32(np.abs(ref).max())))))
        if step == reload_at:
            pl = [torch.nn.Parameter(p.detach().clone()) for p in p32]
            ol = DEVICE[rule](pl, lr=7.0)
            ol.load_state_dict(copy.deepcopy(o32.state_dict()))
            runs.append((pl, ol))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("rule", RULE_NAMES)
def test_against_torch_on_the_device(rule, wd):
    _need_gpu()
    res = _gpu_yardstick(rule, wd, 20, (1, 10, 11, 20), reload_at=10)
    assert (11, "loaded") in res and (20, "loaded") in res and (10, "loaded") not in res
    check_yardstick(f"gpu {rule} wd {wd}", res)


def _decoder(fused):
    from tpnet_amd.callers import LinkPredictor_v1
    torch.manual_seed(12)
    dec = LinkPredictor_v1(16, 16, 32, 1, None, False).to(DEV)
    dec.fused = fused
    rng = np.random.RandomState(13)
    src = torch.from_numpy(rng.standard_normal((30, 16)).astype(np.float32)).to(DEV)
    dst = torch.from_numpy(rng.standard_normal((30, 16)).astype(np.float32)).to(DEV)
    return dec, src, dst, np.arange(30)


def _take_a_step(dec, rule, out):
    opt = DEVICE[rule](dec.parameters(), lr=0.1)
    ps = list(dec.parameters())
    key = _dense.param_key(*ps)
    before = [p.detach().clone() for p in ps]
    out.square().mean().backward()
    opt.step()
    after = _dense.param_key(*ps)
    assert [p.data_ptr() for p in ps] == list(key[0::2]) == list(after[0::2])
    assert all(a != b for a, b in zip(key[1::2], after[1::2]))                       # every served Parameter's _version moved
    assert all(not torch.equal(p, q) for p, q in zip(ps, before))


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULE_NAMES)
def test_version_contract_f32_decoder(rule):
    """LinkPredictor_v1.fused = 'f32' after a step: the torch layers on the NEW weights, in float64 on the host, within the bound of
    tests/test_decoder_f32.py (|got - want| <= 4e-5 mag + 1e-6 max |want|, mag the expression over absolute values); not the old logits."""
    _need_gpu()
    from tpnet_amd import fused_decoder as fd
    dec, src, dst, ids = _decoder("f32")
    assert fd.serves_f32(dec.fc1, dec.fc2, src, dst, None, False)
    n0 = fd.calls["f32_train_forward"]
    old = dec(ids, ids, src, dst)
    _take_a_step(dec, rule, old)
    with torch.no_grad():
        new = dec(ids, ids, src, dst)
    assert fd.calls["f32_train_forward"] == n0 + 1 and not torch.equal(new, old)
    w1, b1 = dec.fc1.weight.detach().double().cpu().numpy(), dec.fc1.bias.detach().double().cpu().numpy()
    w2, b2 = dec.fc2.weight.detach().double().cpu().numpy(), dec.fc2.bias.detach().double().cpu().numpy()
    x = torch.cat([src, dst], dim=1).double().cpu().numpy()
    a, amag = x @ w1.T + b1, np.abs(x) @ np.abs(w1).T + np.abs(b1)
    on = a > 0
    want = (np.where(on, a, 0.0) * w2).sum(1) + b2[0]
    mag = (np.where(on, amag, 0.0) * np.abs(w2)).sum(1) + abs(b2[0])
    err = np.abs(new.double().cpu().numpy().reshape(-1) - want)
    bound = 4e-5 * mag + 1e-6 * np.abs(want).max()
    print(f"{rule}: f32 decoder after a step, err / bound <= {(err / bound).max():.4f}; moved by {(new - old).abs().max().item():.3e}")
    assert (err <= bound).all()
    assert (new - old).abs().max().item() > 2 * bound.max()                           # (the old logits are outside the bound)


@pytest.mark.gpu
def test_version_contract_cached_weight_image():
    """fused = True packs fc1 / fc2 into a bf16 image that is cached under param_key: after a step the module gives the bits of a copy
    of itself that has never packed anything, and not the logits of before the step."""
    _need_gpu()
    from tpnet_amd import fused_decoder as fd
    dec, src, dst, ids = _decoder(True)
    assert fd.supported(dec.fc1, dec.fc2, 16, 0)
    with torch.no_grad():
        old = dec(ids, ids, src, dst)
    plain = dec.fc2(dec.act(dec.fc1(torch.cat([src, dst], dim=1))))
    _take_a_step(dec, "Adam", plain)
    with torch.no_grad():
        new = dec(ids, ids, src, dst)
        fresh = copy.deepcopy(dec)(ids, ids, src, dst)
    assert torch.equal(new, fresh) and not torch.equal(new, old)


@pytest.mark.gpu
def test_training_epoch_with_the_device_step(golden_dir):
    """train_link_prediction_epoch on the toy stream of tests/test_training_loss.py, 300 edges in batches of 26, Adam(lr = 1e-3): the
    per-batch losses with create_optimizer(device_step=True) against device_step=False, within twice the distance between two torch
    runs that differ only in foreach=True / foreach=False -- that distance is what two valid fp32 orderings of the same step do to
    the losses, measured here."""
    _need_gpu()
    from tpnet_amd.callers import create_optimizer, train_link_prediction_epoch
    from test_training_loss import _toy
    src, dst, t, rp, twin, nbr, neg, enc, dec = _toy(golden_dir)
    model = torch.nn.ModuleList([enc, dec])
    start = copy.deepcopy(model.state_dict())

    def run(make):
        model.load_state_dict(start)
        neg.reset_random_state()
        torch.manual_seed(79)
        losses, _ = train_link_prediction_epoch(rp, nbr, neg, src, dst, t, 26, 4, enc, dec, make(model))
        return np.array(losses)

    stock = run(lambda m: create_optimizer(m, "Adam", 1e-3, device_step=False))
    mine = run(lambda m: create_optimizer(m, "Adam", 1e-3, device_step=True))
    each = run(lambda m: torch.optim.Adam(m.parameters(), lr=1e-3, foreach=False))
    many = run(lambda m: torch.optim.Adam(m.parameters(), lr=1e-3, foreach=True))
    assert len(stock) == 12 and not np.array_equal(stock[1:], np.full(11, stock[0]))
    yard = np.abs(each - many).max()
    diff = np.abs(mine - stock).max()
    print(f"epoch losses: device step vs torch {diff:.3e}; torch foreach=True vs foreach=False {yard:.3e}; ratio {diff / yard if yard else float('inf'):.3f}")
    assert diff <= 2.0 * yard


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULE_NAMES)
def test_step_does_not_synchronise(rule):
    """A step behind a long kernel returns while that kernel still runs: the event recorded behind the kernel is not complete before the
    step and not complete after it; torch's synchronisation check stays quiet."""
    _need_gpu()
    ps = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (5, 3000, 64)]
    opt = DEVICE[rule](ps, lr=LR[rule], weight_decay=0.01)
    for _ in range(2):                                         # (first use loads the code object; the second step is the steady state)
        for p in ps:
            p.grad = torch.ones_like(p)
        opt.step()
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda._sleep(400_000_000)                             # some tenths of a second of GPU time
    ev.record()
    early = ev.query()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    late = ev.query()
    torch.cuda.synchronize()
    assert not early and not late
    if rule != "SGD":
        assert float(opt.state[ps[0]]["step"]) == 3.0


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULE_NAMES)
def test_cpu_parameter_among_gpu_ones(rule, caplog):
    """Both kinds are updated in one step() -- the GPU ones with the kernel's bits, the CPU one with torch's -- and the log line
    comes once."""
    _need_gpu()
    rng = np.random.RandomState(41)
    xs = [rng.standard_normal(n).astype(np.float32) for n in (7, 130, 19)]
    ps = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(d)) for x, d in zip(xs, (DEV, "cpu", DEV))]
    opt = DEVICE[rule](ps, lr=LR[rule], weight_decay=0.01)
    ref_p = torch.nn.Parameter(torch.from_numpy(xs[1].copy()))
    ref = TORCH[rule]([ref_p], lr=LR[rule], weight_decay=0.01)
    host = [dict(p=x, s1=np.zeros_like(x), s2=np.zeros_like(x)) for x in xs]
    with caplog.at_level(logging.WARNING, logger="tpnet_amd.optimizer"):
        for step in range(1, 4):
            grads = [gradient(rng, x.shape) for x in xs]
            for p, g in zip(ps, grads):
                p.grad = torch.from_numpy(g.copy()).to(p.device)
            ref_p.grad = torch.from_numpy(grads[1].copy())
            opt.step()
            ref.step()
            c = scalars_of(rule, LR[rule], 0.01, step)
            for k in (0, 2):
                h = host[k]
                h["p"], s1, s2 = O.optimizer_step_host(rule, h["p"], grads[k], h["s1"], h["s2"], c)
                h["s1"], h["s2"] = (s1 if s1 is not None else h["s1"]), (s2 if s2 is not None else h["s2"])
                assert np.array_equal(_bits(ps[k].detach().cpu().numpy()), _bits(h["p"]))
            assert torch.equal(ps[1].detach(), ref_p.detach()) and not ps[1].is_cuda
    assert not np.array_equal(ps[1].detach().numpy(), xs[1])
    assert len([r for r in caplog.records if "single-tensor update" in r.getMessage()]) == 1
