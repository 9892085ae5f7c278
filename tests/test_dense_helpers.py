"""tpnet_amd/_dense.py: what the four fused_* modules share -- the Linear -> ReLU -> Linear predicate, the fp32 gradient
expressions, the cache of derived weight buffers and the Python side of a backward that writes partial sums.  No GPU needed."""
import copy
import gc
import weakref
from typing import NamedTuple

import pytest
import torch
import torch.nn as nn

from tpnet_amd import _dense, fused_decoder, fused_feature, fused_input, fused_mlp


def _seq(a=64, b=256, c=256, d=64, bias1=True, bias2=True, act=nn.ReLU):
    return nn.Sequential(nn.Linear(a, b, bias=bias1), act(), nn.Linear(c, d, bias=bias2))


# name -> (module, is it Linear -> ReLU -> Linear with biases and matching widths, is it the reference's 64 -> 256 -> 64)
MODULES = {
    "reference": (lambda: _seq(), True, True),
    "other_widths": (lambda: _seq(168, 40, 40, 20), True, False),
    "no_bias_first": (lambda: _seq(bias1=False), False, False),
    "no_bias_second": (lambda: _seq(bias2=False), False, False),
    "gelu": (lambda: _seq(act=nn.GELU), False, False),
    "tanh": (lambda: _seq(act=nn.Tanh), False, False),
    "two_layers": (lambda: nn.Sequential(nn.Linear(64, 256), nn.ReLU()), False, False),
    "four_layers": (lambda: nn.Sequential(nn.Linear(64, 256), nn.ReLU(), nn.Linear(256, 64), nn.ReLU()), False, False),
    "mismatched_widths": (lambda: _seq(64, 256, 128, 64), False, False),
    "transposed_widths": (lambda: _seq(256, 64, 64, 256), True, False),
    "identity": (lambda: nn.Identity(), False, False),
    "bare_linear": (lambda: nn.Linear(64, 64), False, False),
    "relu_first": (lambda: nn.Sequential(nn.ReLU(), nn.Linear(64, 256), nn.Linear(256, 64)), False, False),
}


def predicate_answers(m):
    """What the modules' public predicates say about `m` (tools compare two trees on this)."""
    return {"fused_mlp.supported": bool(fused_mlp.supported(m)),
            "fused_feature.supported(64)": bool(fused_feature.supported(m, 64)),
            "fused_feature.supported(16)": bool(fused_feature.supported(m, 16)),
            "fused_input.dims_of(20,8,12,64)": fused_input.dims_of(m, 20, 8, 12, 64),
            "fused_input.dims_of(16,16,16,8)": fused_input.dims_of(m, 16, 16, 16, 8)}


@pytest.mark.parametrize("name", sorted(MODULES))
def test_structural_predicate(name):
    make, is_lrl, is_reference = MODULES[name]
    m = make()
    ls = _dense.linear_relu_linear(m)
    if is_lrl:
        assert ls is not None and ls[0] is m[0] and ls[1] is m[2]
    else:
        assert ls is None
    # the modules' own predicates are the shared one plus their widths (fused_feature also wants f32 weights on a GPU)
    got = predicate_answers(m)
    assert got["fused_mlp.supported"] == is_reference
    assert got["fused_feature.supported(64)"] is False and got["fused_feature.supported(16)"] is False      # CPU weights
    assert got["fused_input.dims_of(20,8,12,64)"] == ((20, 8, 12, 64, 40, 20) if name == "other_widths" else None)
    assert got["fused_input.dims_of(16,16,16,8)"] == ((16, 16, 16, 8, 256, 64) if is_reference else None)
    assert fused_input.prepared(m, 20, 8, 12, 64) is None                                                   # CPU weights / structure


class _Rec(NamedTuple):
    key: tuple
    storage: tuple
    buf: torch.Tensor
    builds: int


def _serve(cache, m, log):
    ps = (m[0].weight, m[0].bias, m[2].weight, m[2].bias)
    key = _dense.param_key(*ps)
    storage = tuple(p.data_ptr() for p in ps)

    def build(previous):
        log.append(previous)
        buf = previous.buf if previous is not None else torch.empty(64, 256)
        buf.copy_(m[0].weight.detach().t())
        return _Rec(key, storage, buf, 1 + (previous.builds if previous is not None else 0))

    return _dense.cached(cache, m, key, storage, build)


def test_cache_rebuilds_on_version_bump_and_keeps_buffers():
    cache, log, m = weakref.WeakKeyDictionary(), [], _seq()
    first = _serve(cache, m, log)
    assert _serve(cache, m, log) is first and len(log) == 1                       # a hit builds nothing
    with torch.no_grad():
        m[0].weight.mul_(2.0)                                                     # a versioned in-place op: same storage
    second = _serve(cache, m, log)
    assert second is not first and second.key != first.key and len(log) == 2
    assert log[1] is first and second.buf is first.buf and second.builds == 2     # the buffer was rewritten, not replaced
    assert torch.equal(second.buf, m[0].weight.detach().t())
    with torch.no_grad():
        m[2].bias.add_(1.0)                                                       # every one of the four Parameters is in the key
    assert _serve(cache, m, log).builds == 3
    m[0].weight = nn.Parameter(m[0].weight.detach().clone())                      # new storage: the builder starts afresh
    third = _serve(cache, m, log)
    assert log[-1] is None and third.buf is not first.buf and third.builds == 1
    declined = _dense.cached(cache, _seq(), ("k",), (), lambda previous: None)    # a builder that declines caches nothing
    assert declined is None and len(cache) == 1


def test_cache_drops_its_entry_with_the_module():
    cache, log, m = weakref.WeakKeyDictionary(), [], _seq()
    _serve(cache, m, log)
    assert len(cache) == 1
    del m
    gc.collect()
    assert len(cache) == 0


def test_deepcopy_of_a_served_module_carries_no_cache():
    """fused_mlp / fused_decoder keep their derived buffers off the module: a deep copy, a state_dict and a pickle see the module
    as it was constructed."""
    mlp = _seq()
    before = set(vars(mlp))
    prep = fused_mlp._prepared(mlp)
    assert fused_mlp._prepared(mlp) is prep and prep[0].dtype == torch.bfloat16 and tuple(prep[4].shape) == (256, 64)
    with torch.no_grad():
        mlp[0].weight.add_(1.0)
    assert fused_mlp._prepared(mlp) is not prep                                   # rebuilt on a _version bump
    owner = nn.Module()
    owner.fc1, owner.fc2 = nn.Linear(2 * 8 + 16, 40), nn.Linear(40, 1)
    owner_before = set(vars(owner))
    packed = fused_decoder._prepared(owner, owner.fc1, owner.fc2, 8, 16)
    assert fused_decoder._prepared(owner, owner.fc1, owner.fc2, 8, 16) is packed and packed[4] == 2
    for m, names in ((mlp, before), (owner, owner_before)):
        assert set(vars(m)) == names and not [k for k in vars(m) if "tpnet" in k]
        c = copy.deepcopy(m)
        assert set(vars(c)) == names and list(c.state_dict()) == list(m.state_dict())
    assert copy.deepcopy(mlp) not in fused_mlp._PREPARED and copy.deepcopy(owner) not in fused_decoder._PREPARED


def test_layer_grads_match_autograd():
    """The fp32 torch expressions of the two layers' gradients against autograd, 8 rows in float64."""
    gen = torch.Generator().manual_seed(5)
    m = _seq(12, 20, 20, 6).double()
    x = torch.randn(8, 12, dtype=torch.float64, generator=gen, requires_grad=True)
    gy = torch.randn(8, 6, dtype=torch.float64, generator=gen)
    m(x).backward(gy)
    want = (m[0].weight.grad, m[0].bias.grad, m[2].weight.grad, m[2].bias.grad, x.grad)
    with torch.no_grad():
        got = _dense.layer_grads(x, gy, m[0].weight, m[0].bias, m[2].weight, input_grad=True)
        four = _dense.layer_grads(x, gy, m[0].weight, m[0].bias, m[2].weight)
    assert len(got) == 5 and len(four) == 4
    for g, w in zip(got, want):
        assert g.shape == w.shape
        torch.testing.assert_close(g, w, rtol=1e-12, atol=1e-12)
    for g, w in zip(four, got):
        assert torch.equal(g, w)


def test_split_grads_cuts_in_order_and_respects_needs():
    """One summed partial cut into per-tensor gradients: shapes of several ranks, None where not needed (the offset still moves
    past it), views of `tot` rather than copies."""
    tensors = (torch.empty(3), torch.empty(2, 5), torch.empty(()), torch.empty(4, 1, 2), torch.empty(0, 7), torch.empty(6))
    total = sum(t.numel() for t in tensors)
    tot = torch.arange(total, dtype=torch.float32)
    needs = (True, False, True, True, True, True)
    got = _dense.split_grads(tot, tensors, needs)
    assert len(got) == len(tensors) and got[1] is None
    off = 0
    for t, need, g in zip(tensors, needs, got):
        if need:
            assert g.shape == t.shape and g.dtype == tot.dtype
            assert torch.equal(g.reshape(-1), tot[off:off + t.numel()])
            assert t.numel() == 0 or g.data_ptr() == tot[off:].data_ptr()
        off += t.numel()
    assert off == total
    assert _dense.split_grads(tot, tensors, (False,) * 6) == [None] * 6
    assert _dense.split_grads(tot, (), ()) == []


def test_split_grads_without_a_total_gives_zeros():
    tensors = (torch.full((2, 3), 7.0), torch.full((4,), 7.0, dtype=torch.float64), torch.full((1, 1, 5), 7.0))
    got = _dense.split_grads(None, tensors, (True, False, True))
    assert got[1] is None
    for t, g in ((tensors[0], got[0]), (tensors[2], got[2])):
        assert g.shape == t.shape and g.dtype == t.dtype and g.device == t.device and not g.any()
    assert tensors[0].eq(7.0).all()                                               # (new tensors: the Parameters are untouched)


def test_partial_buffer_is_one_per_device_parts_and_floats():
    cpu = torch.device("cpu")
    a = _dense.partial_buffer(cpu, 5, 11)
    assert tuple(a.shape) == (5, 11) and a.dtype == torch.float32 and a.device == cpu
    assert _dense.partial_buffer(cpu, 5, 11) is a                                 # the same key: the same tensor
    b = _dense.partial_buffer(cpu, 6, 11)                                         # another part count: a new buffer of that size
    assert b is not a and tuple(b.shape) == (6, 11)
    c = _dense.partial_buffer(cpu, 5, 12)
    assert c is not a and c is not b and tuple(c.shape) == (5, 12)
    assert _dense.partial_buffer(cpu, 5, 11) is a and _dense.partial_buffer(cpu, 6, 11) is b
    assert _dense.partial_buffer(cpu, 5, 11.0) is a                               # (the C calls' sizes arrive as ctypes / int64 values)


def test_sum_partials_adds_the_written_partials_and_raises_for_none():
    part = torch.tensor([[1.0, 2.0], [10.0, 20.0], [float("nan"), float("nan")]])
    assert torch.equal(_dense.sum_partials(2, part, "t"), torch.tensor([11.0, 22.0]))      # rows >= rc are never read
    assert torch.equal(_dense.sum_partials(1, part, "t"), part[0])
    from tpnet_amd import _lib
    for rc in (0, -1):
        with pytest.raises(_lib.TPNetHipError, match="some_backward"):
            _dense.sum_partials(rc, part, "some_backward")


class _Two(NamedTuple):
    key: tuple
    storage: tuple
    bimg: object = None


def test_cached_images_builds_the_second_image_once_asked_and_keeps_it():
    cache, log = weakref.WeakKeyDictionary(), []
    owner = nn.Identity()

    def build(previous, both):
        log.append((previous, both))
        bimg = previous.bimg if previous is not None else None
        if both and bimg is None:
            bimg = object()
        return _Two(key[0], ("s",), bimg if both else None)

    key = [("k", 0)]
    serve = lambda backward: _dense.cached_images(cache, owner, key[0], ("s",), build, backward)
    first = serve(False)
    assert first.bimg is None and log == [(None, False)] and serve(False) is first and len(log) == 1
    second = serve(True)                                                          # a record an inference call made: rebuilt once
    assert second.bimg is not None and log[-1] == (None, True) and len(log) == 2
    assert serve(True) is second and serve(False) is second and len(log) == 2
    key[0] = ("k", 1)                                                             # a Parameter changed: both rewritten, also
    third = serve(False)                                                          # for an inference call
    assert log[-1] == (second, True) and third.bimg is second.bimg and len(log) == 3
    # a build that declines the second image (the backward serves fewer shapes) gives None and keeps the inference record
    cache2, owner2 = weakref.WeakKeyDictionary(), nn.Identity()
    decl = lambda previous, both: None if both else _Two(("k",), ("s",))
    rec = _dense.cached_images(cache2, owner2, ("k",), ("s",), decl, False)
    assert _dense.cached_images(cache2, owner2, ("k",), ("s",), decl, True) is None and cache2[owner2] is rec
