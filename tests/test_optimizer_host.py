"""The device optimizer step without a GPU (tpnet_amd/optimizer.py, csrc/optimizer.hip: tpnet_optim_step): the numpy restatement of
the kernel's rule against torch, the torch-compatible surface of DeviceAdam / DeviceSGD / DeviceRMSprop on the route a CPU tensor
takes, `callers.create_optimizer`, and the C entry's refusals.

Yardstick of `optimizer_step_host`: torch.optim.{Adam, SGD, RMSprop}(foreach=False) run in float64 on the CPU from the same fp32
parameters and gradients is the reference; torch's own fp32 CPU optimizer on the same inputs measures what an fp32 ordering loses.  At
steps 1, 10 and 60, per tensor: max |restatement - f64| <= 2 max |torch fp32 - f64| + ulp(max |p|) -- two valid fp32 orderings differ
by roundings of p.  The tensors hold 1 000 elements or more: each side's distance is the maximum of a random walk of roundings over the
elements, and the maxima of two orderings are comparable only over many elements (over one element the ratio of two such walks has no
bound, and torch's may be exactly 0).  Measured ratios (restatement's distance over torch's, the worst tensor and step of each case) are printed; the
profile profiles/optimizer.md records them.

One step, derivable: from a zero state and without weight decay every quantity of a rule is a chain of products, quotients and roots
of positive numbers and exact additions of 0 -- seven roundings of 2^-24 on the way to the update u = p - p' for Adam (two in
(c5 g) g, halved by the root, the root, the quotient by c6, + eps, m = c3 g, m / den, c0 q), fewer for the others -- and one rounding
of p - u: |p_fp32 - p_f64| <= 2^-24 |p| + 8 2^-24 |u|, with the float64 side evaluated from the same fp32 scalars.  SGD with weight
decay, g and p of one sign: three roundings."""
import copy
import ctypes
import logging
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tpnet_amd import optimizer as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1000,), (33, 50), (4099,)]
TORCH = {"Adam": torch.optim.Adam, "SGD": torch.optim.SGD, "RMSprop": torch.optim.RMSprop}
DEVICE = {"Adam": O.DeviceAdam, "SGD": O.DeviceSGD, "RMSprop": O.DeviceRMSprop}
LR = {"Adam": 1e-3, "SGD": 1e-2, "RMSprop": 1e-2}


def gradient(rng, shape):
    """randn * 10^k, k uniform in [-6, 2] per call; a fifth of the entries exactly 0; every other one at least 1e-12 in magnitude (g^2
    and its product with 1 - beta2 stay normal floats)."""
    g = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-6.0, 2.0)).astype(np.float32)
    tiny = np.abs(g) < 1e-12
    g[tiny] = np.copysign(np.float32(1e-12), g[tiny])
    g[rng.random_sample(shape) < 0.2] = 0.0
    return g


def scalars_of(rule, lr, wd, step, betas=(0.9, 0.999), eps=1e-8, alpha=0.99):
    if rule == "Adam":
        return O.adam_scalars(lr, betas[0], betas[1], eps, wd, step)
    if rule == "SGD":
        return O.sgd_scalars(lr, wd)
    return O.rmsprop_scalars(lr, alpha, eps, wd)


def yardstick(rule, wd, steps, marks, device="cpu", seed=5):
    """-> {step: [(restatement's distance, torch fp32's distance, ulp(max |p|)) per tensor]} of one case; the restatement runs on the
    host from the same inputs whatever `device` the two torch optimizers run on."""
    rng = np.random.RandomState(seed)
    p0 = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    p64 = [torch.from_numpy(x).double().to(device).requires_grad_() for x in p0]
    p32 = [torch.from_numpy(x.copy()).to(device).requires_grad_() for x in p0]
    o64 = TORCH[rule](p64, lr=LR[rule], weight_decay=wd, foreach=False)
    o32 = TORCH[rule](p32, lr=LR[rule], weight_decay=wd, foreach=False)
    mine = [(x.copy(), np.zeros_like(x), np.zeros_like(x)) for x in p0]
    out = {}
    for step in range(1, steps + 1):
        grads = [gradient(rng, s) for s in SHAPES]
        for a, b, g in zip(p64, p32, grads):
            a.grad, b.grad = torch.from_numpy(g).double().to(device), torch.from_numpy(g.copy()).to(device)
        o64.step()
        o32.step()
        c = scalars_of(rule, LR[rule], wd, step)
        mine = [O.optimizer_step_host(rule, p, g, s1, s2, c) for (p, s1, s2), g in zip(mine, grads)]
        if step in marks:
            out[step] = []
            for (p, _, _), a, b in zip(mine, p64, p32):
                ref = a.detach().cpu().numpy()
                out[step].append((np.abs(p.astype(np.float64) - ref).max(), np.abs(b.detach().cpu().numpy().astype(np.float64) - ref).max(),
                                  float(np.spacing(np.float32(np.abs(ref).max())))))
    return out


def check_yardstick(tag, result):
    worst = 0.0
    for step, rows in result.items():
        for k, (mine, stock, ulp) in enumerate(rows):
            ratio = mine / stock if stock > 0 else (0.0 if mine == 0 else float("inf"))
            worst = max(worst, ratio if np.isfinite(ratio) else mine / ulp)
            print(f"{tag} step {step} tensor {k}: restatement {mine:.3e} torch fp32 {stock:.3e} ratio {ratio:.3f} ulp {ulp:.3e}")
            assert mine <= 2.0 * stock + ulp, (tag, step, k, mine, stock, ulp)
    print(f"{tag}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("rule", ["Adam", "SGD", "RMSprop"])
def test_restatement_against_torch_float64(rule, wd):
    check_yardstick(f"{rule} wd {wd}", yardstick(rule, wd, 60, (1, 10, 60)))


def _f64_step(rule, p, g, c):
    """One step from a zero state in float64, from the fp32 values of p, g and of the scalars c."""
    p, g = p.astype(np.float64), g.astype(np.float64)
    c = np.array(O._F32.unpack(O._F32.pack(*c)), dtype=np.float64)
    g = g + c[1] * p
    if rule == "Adam":
        return p - c[0] * ((c[3] * g) / (np.sqrt(c[5] * g * g) / c[6] + c[7]))
    if rule == "SGD":
        return p - c[0] * g
    return p - c[0] * (g / (np.sqrt(c[3] * g * g) + c[4]))


@pytest.mark.parametrize("rule,wd", [("Adam", 0.0), ("SGD", 0.0), ("RMSprop", 0.0), ("SGD", 0.01)])
def test_one_step_bound(rule, wd):
    rng = np.random.RandomState(11)
    worst = 0.0
    for trial in range(20):
        p = rng.standard_normal(500).astype(np.float32)
        g = gradient(rng, (500,))
        if wd:
            g = np.copysign(g, p)                                     # (no cancellation in g + wd p; zeros stay zeros)
        c = scalars_of(rule, LR[rule], wd, 1)
        got = O.optimizer_step_host(rule, p, g, np.zeros_like(p), np.zeros_like(p), c)[0]
        want = _f64_step(rule, p, g, c)
        bound = 2.0 ** -24 * np.abs(p) + 8 * 2.0 ** -24 * np.abs(want - p)
        err = np.abs(got.astype(np.float64) - want)
        worst = max(worst, (err / bound).max())
        assert (err <= bound).all()
    print(f"{rule} wd {wd}: one-step error / bound <= {worst:.3f}")


def _pair(rule, wd, seed=2):
    """Two copies of three CPU tensors, a torch optimizer on one and the device class on the other."""
    rng = np.random.RandomState(seed)
    xs = [rng.standard_normal(s).astype(np.float32) for s in SHAPES[:3]]
    a = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in xs]
    b = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in xs]
    return rng, a, b, TORCH[rule](a, lr=LR[rule], weight_decay=wd), DEVICE[rule](b, lr=LR[rule], weight_decay=wd)


def _steps(rng, n, *sides):
    for _ in range(n):
        grads = [gradient(rng, s) for s in SHAPES[:3]]
        for params, opt in sides:
            for p, g in zip(params, grads):
                p.grad = torch.from_numpy(g.copy())
            opt.step()


def _same_state(x, y):
    sx, sy = x.state_dict(), y.state_dict()
    assert [sorted(g.keys()) for g in sx["param_groups"]] == [sorted(g.keys()) for g in sy["param_groups"]]
    assert sx["state"].keys() == sy["state"].keys()
    for k in sx["state"]:
        assert sorted(sx["state"][k].keys()) == sorted(sy["state"][k].keys())
        for name, v in sx["state"][k].items():
            w = sy["state"][k][name]
            assert v.dtype == w.dtype and v.shape == w.shape and v.device == w.device and torch.equal(v, w), (k, name)


@pytest.mark.parametrize("rule", ["Adam", "SGD", "RMSprop"])
def test_state_dict_interchange_with_torch(rule):
    """On CPU tensors the classes take torch's own single-tensor update: equal bits.  A state_dict crosses in both directions in
    mid-run, and both sides go on equal: same param_groups keys, same state keys, equal tensors."""
    rng, a, b, stock, mine = _pair(rule, 0.01)
    _steps(rng, 3, (a, stock), (b, mine))
    _same_state(stock, mine)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    if rule != "SGD":
        assert sorted(mine.state[b[0]].keys()) == (["exp_avg", "exp_avg_sq", "step"] if rule == "Adam" else ["square_avg", "step"])
        assert float(mine.state[b[0]]["step"]) == 3.0 and not mine.state[b[0]]["step"].is_cuda
    else:
        assert len(mine.state) == 0
    # torch -> here, here -> torch, into fresh optimizers over copies of the parameters
    a2 = [torch.nn.Parameter(x.detach().clone()) for x in a]
    b2 = [torch.nn.Parameter(x.detach().clone()) for x in b]
    mine2, stock2 = DEVICE[rule](a2, lr=0.5), TORCH[rule](b2, lr=0.5)
    mine2.load_state_dict(copy.deepcopy(stock.state_dict()))          # (as through a file: load_state_dict itself keeps the tensors it is given)
    stock2.load_state_dict(copy.deepcopy(mine.state_dict()))
    assert mine2.param_groups[0]["lr"] == LR[rule] and stock2.param_groups[0]["weight_decay"] == 0.01
    _steps(rng, 2, (a, stock), (b, mine), (a2, mine2), (b2, stock2))
    for other in (mine, mine2, stock2):
        _same_state(stock, other)
    for params in (b, a2, b2):
        assert all(torch.equal(x, y) for x, y in zip(a, params))


def test_parameters_without_gradient_are_skipped_and_closures_run():
    rng, a, b, stock, mine = _pair("Adam", 0.0)
    for params, opt in ((a, stock), (b, mine)):
        params[0].grad = torch.ones_like(params[0])
        params[2].grad = torch.ones_like(params[2])
        calls = []
        assert opt.step(lambda: calls.append(torch.is_grad_enabled()) or 7.5) == 7.5 and calls == [True]
    assert b[1] not in mine.state and float(mine.state[b[0]]["step"]) == 1.0
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_hyperparameters_are_read_every_step():
    """An lr scheduler edits param_groups between steps."""
    rng, a, b, stock, mine = _pair("SGD", 0.0)
    for opt in (stock, mine):
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
        for _ in range(3):
            for p in opt.param_groups[0]["params"]:
                p.grad = torch.ones_like(p)
            opt.step()
            sched.step()
    assert mine.param_groups[0]["lr"] == LR["SGD"] / 8 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_unserved_options_are_refused():
    w = [torch.nn.Parameter(torch.zeros(3))]
    for cls, kw in ((O.DeviceAdam, dict(amsgrad=True)), (O.DeviceAdam, dict(maximize=True)), (O.DeviceAdam, dict(decoupled_weight_decay=True)),
                    (O.DeviceAdam, dict(capturable=True)), (O.DeviceAdam, dict(betas=(0.9, 1.0))), (O.DeviceAdam, dict(lr=-1.0)),
                    (O.DeviceSGD, dict(lr=0.1, momentum=0.9)), (O.DeviceSGD, dict(lr=0.1, nesterov=True)),
                    (O.DeviceSGD, dict(lr=0.1, maximize=True)), (O.DeviceRMSprop, dict(centered=True)),
                    (O.DeviceRMSprop, dict(momentum=0.5)), (O.DeviceRMSprop, dict(maximize=True)), (O.DeviceRMSprop, dict(eps=-1.0))):
        with pytest.raises(ValueError):
            cls(w, **kw)
    # an option that arrives later -- a loaded state_dict, an edited group -- is refused by step()
    opt = O.DeviceAdam(w)
    opt.load_state_dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], amsgrad=True).state_dict())
    w[0].grad = torch.ones(3)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()


def test_create_optimizer_names_classes_and_error():
    from tpnet_amd import create_optimizer
    model = torch.nn.Linear(3, 2)
    for name in ("Adam", "SGD", "RMSprop"):
        dev = create_optimizer(model, name, 0.01, 0.1)
        stock = create_optimizer(model=model, optimizer_name=name, learning_rate=0.01, weight_decay=0.1, device_step=False)
        assert type(dev) is DEVICE[name] and type(stock) is TORCH[name]
        assert isinstance(dev, torch.optim.Optimizer)
        assert dev.param_groups[0]["lr"] == 0.01 and dev.param_groups[0]["weight_decay"] == 0.1
        assert sorted(dev.param_groups[0].keys()) == sorted(stock.param_groups[0].keys())
        assert dev.param_groups[0]["params"] == list(model.parameters())
    assert create_optimizer(model, "Adam", 0.01).param_groups[0]["weight_decay"] == 0.0
    with pytest.raises(ValueError, match="^Wrong value for optimizer AdamW!$"):
        create_optimizer(model, "AdamW", 0.01)
    with pytest.raises(ValueError, match="^Wrong value for optimizer adam!$"):
        create_optimizer(model, "adam", 0.01, device_step=False)


@pytest.mark.parametrize("rule", ["Adam", "SGD", "RMSprop"])
def test_model_moved_after_the_optimizer_was_built(rule, caplog):
    """train_link_prediction.py:220-223 builds the optimizer, then moves the model: `Module._apply` swaps every Parameter's data.  The
    optimizer looks at the tensors in every step.  (Here the move is .double() on the CPU, so torch's update runs, and is logged once.)"""
    from tpnet_amd import create_optimizer
    torch.manual_seed(4)
    model = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.ReLU(), torch.nn.Linear(4, 1))
    twin = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.ReLU(), torch.nn.Linear(4, 1))
    twin.load_state_dict(model.state_dict())
    opts = [create_optimizer(model, rule, LR[rule], 0.01), create_optimizer(twin, rule, LR[rule], 0.01, device_step=False)]
    model.double()
    twin.double()
    x = torch.randn(8, 5, dtype=torch.float64)
    with caplog.at_level(logging.WARNING, logger="tpnet_amd.optimizer"):
        for _ in range(3):
            for m, opt in zip((model, twin), opts):
                opt.zero_grad()
                m(x).square().mean().backward()
                opt.step()
    assert all(torch.equal(a, b) for a, b in zip(model.parameters(), twin.parameters()))
    assert not torch.equal(model[0].weight, torch.nn.Linear(5, 4).weight.double())
    assert len([r for r in caplog.records if "single-tensor update" in r.getMessage()]) == 1


# ------------------------------------------------------------------------------------------------------------------- the C entry

def _table(*entries):
    from tpnet_amd import _lib
    tab = (_lib.OptimTensor * len(entries))()
    for e, kw in zip(tab, entries):
        for k, v in kw.items():
            setattr(e, k, v)
    return tab


def test_optim_step_refusals_without_a_gpu(hip_lib):
    """Every refusal is TPNET_ERR_BAD_ARG before a launch (a launch without a GPU would be TPNET_ERR_HIP); a call with nothing to
    do is TPNET_OK."""
    f = hip_lib.tpnet_optim_step
    ok = dict(p=64, g=128, s1=192, s2=256, n=5)
    assert hip_lib.tpnet_optim_max_tensors() >= 38
    assert hip_lib.tpnet_optim_chunk() > 0 and hip_lib.tpnet_optim_chunk() % 4 == 0
    assert f(0, None, 1, None) == -1                                             # a null table
    assert f(0, _table(ok), -1, None) == -1                                      # a negative count
    assert f(3, _table(ok), 1, None) == -1 and f(-1, _table(ok), 1, None) == -1  # an unknown rule
    for rule in (0, 1, 2):
        assert f(rule, _table(dict(ok, p=None)), 1, None) == -1
        assert f(rule, _table(dict(ok, g=None)), 1, None) == -1
        assert f(rule, _table(dict(ok, n=-1)), 1, None) == -1
        assert f(rule, _table(dict(ok, n=0), dict(ok, n=-1)), 2, None) == -1     # (the whole table is checked first)
        assert f(rule, _table(dict(ok, p=66)), 1, None) == -1                    # not 4-byte aligned
        assert f(rule, _table(dict(ok, n=(1 << 41) + 1)), 1, None) == -1
    assert f(0, _table(dict(ok, s1=None)), 1, None) == -1 and f(0, _table(dict(ok, s2=None)), 1, None) == -1
    assert f(2, _table(dict(ok, s1=None)), 1, None) == -1
    assert f(2, _table(dict(ok, s2=None, n=0)), 1, None) == 0                    # RMSprop has no s2, SGD no state; n == 0 is skipped
    assert f(1, _table(dict(ok, s1=None, s2=None, n=0)), 1, None) == 0
    assert f(0, None, 0, None) == 0 and f(0, _table(dict(ok, n=0), dict(ok, n=0)), 2, None) == 0
    assert hip_lib.tpnet_abi_version() == 7                                      # additive


def test_optim_tensor_layout_matches_the_header(tmp_path):
    """tpnet_optim_tensor as gcc lays it out from include/tpnet_hip.h against the ctypes mirror and the packed entry of step()."""
    from tpnet_amd import _lib
    assert ctypes.sizeof(_lib.OptimTensor) == 80 == O._ENTRY.size
    assert [getattr(_lib.OptimTensor, f).offset for f in ("p", "g", "s1", "s2", "n", "c", "flags", "reserved")] == [0, 8, 16, 24, 32, 40, 72, 76]
    assert (_lib.OPTIM_ADAM, _lib.OPTIM_SGD, _lib.OPTIM_RMSPROP) == (0, 1, 2)
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    fields = ["p", "g", "s1", "s2", "n", "c", "flags", "reserved"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tpnet_hip.h"\nint main(void) {\n'
                   + 'printf("%zu %d %d %d\\n", sizeof(tpnet_optim_tensor), TPNET_OPTIM_ADAM, TPNET_OPTIM_SGD, TPNET_OPTIM_RMSPROP);\n'
                   + "".join(f'printf("%zu\\n", offsetof(tpnet_optim_tensor, {f}));\n' for f in fields)
                   + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[:4]] == [ctypes.sizeof(_lib.OptimTensor), 0, 1, 2]
    for f, off in zip(fields, out[4:]):
        assert getattr(_lib.OptimTensor, f).offset == int(off), f
