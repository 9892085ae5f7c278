"""tpnet_mlp_l4_* (csrc/mlp_l4.hip: self.mlp on the matrix cores for num_layer 4): what the entries answer WITHOUT a device -- the
served width, the sizes, and every argument check, which returns before any HIP call.  No compute call is made here
(tests/test_mlp_l4.py does that, -m gpu)."""
import ctypes as C

import torch

from tpnet_amd import _lib

OK, BAD_ARG = 0, -1


def test_supported_width(hip_lib):
    assert hip_lib.tpnet_mlp_l4_supported(100, 400) == 1
    for F, H in [(16, 64), (36, 144), (64, 256), (144, 576), (100, 144), (400, 100), (0, 0), (100, 401), (-100, -400)]:
        assert hip_lib.tpnet_mlp_l4_supported(F, H) == 0, (F, H)
    # the pinned entries keep their answer
    assert hip_lib.tpnet_mlp_rows_supported(100, 400) == 0


def test_sizes_are_host_arithmetic(hip_lib):
    L = hip_lib
    # 2 passes of 7 k-steps + 7 slices, chunks of 4 output tiles (1 024 elements), then b1 padded to 448 and b2 to 128 floats
    assert L.tpnet_mlp_l4_image_bytes() == 2 * (7 + 7) * 1024 * 16 + (448 + 128) * 4 == 461056
    # 4 passes of 7 k-steps + 4 slices, chunks of 6 output tiles (1 536 elements), then b1 padded to 512 floats
    assert L.tpnet_mlp_l4_bwd_image_bytes() == 4 * (7 + 4) * 1536 * 16 + 512 * 4
    assert L.tpnet_mlp_l4_image_bytes() % 16 == 0 and L.tpnet_mlp_l4_bwd_image_bytes() % 16 == 0
    assert L.tpnet_mlp_l4_bwd_partial_floats() == 400 * 100 + 400 + 100 * 400 + 100
    assert L.tpnet_mlp_l4_bwd_partial_floats() % 4 == 0
    # 32-row tiles of 2 pad(400) + 2 pad(100) floats per row
    for n, tiles in ((1, 1), (32, 1), (33, 2), (4099, 129), (80000, 2500)):
        b = L.tpnet_mlp_l4_bwd_workspace_bytes(n)
        assert b == tiles * 32 * (2 * 416 + 2 * 128) * 4 and b > 0 and b % 16 == 0, n
    assert L.tpnet_mlp_l4_bwd_workspace_bytes(0) == 0 and L.tpnet_mlp_l4_bwd_workspace_bytes(-1) == 0
    assert L.tpnet_mlp_l4_bwd_workspace_bytes((1 << 31) + 1) == 0


def test_argument_checks_return_before_any_device_call(hip_lib):
    L = hip_lib
    x, img, y, bits = 0x200000, 0x300000, 0x400000, 0x500000
    f = L.tpnet_mlp_l4_f32
    for a in ((None, 5, img, y, bits, None), (x, 5, None, y, bits, None), (x, 5, img, None, bits, None), (x, -1, img, y, bits, None),
              (x, (1 << 31) + 1, img, y, None, None)):
        assert f(*a) == BAD_ARG, a
    for off in (4, 8, 12, 1):
        assert f(x + off, 5, img, y, None, None) == BAD_ARG
        assert f(x, 5, img + off, y, None, None) == BAD_ARG
        assert f(x, 5, img, y + off, None, None) == BAD_ARG
    for off in (1, 2, 3):
        assert f(x, 5, img, y, bits + off, None) == BAD_ARG
    assert f(x, 0, img, y, bits, None) == OK and f(x, 0, img, y, None, None) == OK          # n == 0: nothing to do
    p = L.tpnet_mlp_l4_prepare
    for i in range(5):
        a = [16, 32, 48, 64, 80, None]
        a[i] = None
        assert p(*a) == BAD_ARG, i
    assert p(16, 32, 48, 64, 88, None) == BAD_ARG
    bp = L.tpnet_mlp_l4_bwd_prepare
    for i in range(4):
        a = [16, 32, 48, 64, None]
        a[i] = None
        assert bp(*a) == BAD_ARG, i
    assert bp(16, 32, 48, 72, None) == BAD_ARG
    #      x  bits gy  n  bimg ws  part np stream
    bwd = [16, 36, 48, 5, 64, 80, 100, 4, None]
    g = L.tpnet_mlp_l4_bwd_f32
    for i in (0, 1, 2, 4, 5, 6):                                                             # every pointer null in turn
        a = list(bwd)
        a[i] = None
        assert g(*a) == BAD_ARG, i
    for i, v in ((0, 20), (1, 38), (2, 52), (4, 72), (5, 88), (6, 102), (7, 0), (7, -2), (3, -1), (3, (1 << 31) + 1)):
        a = list(bwd)
        a[i] = v
        assert g(*a) == BAD_ARG, (i, v)
    bwd[3] = 0
    assert g(*bwd) == 0                                                                      # no rows: no partial, nothing launched


def test_signatures_are_bound():
    S = _lib.SIGNATURES
    assert S["tpnet_mlp_l4_supported"] == (C.c_int, [C.c_int32, C.c_int32])
    assert S["tpnet_mlp_l4_f32"][0] is C.c_int and len(S["tpnet_mlp_l4_f32"][1]) == 6
    assert S["tpnet_mlp_l4_bwd_f32"][0] is C.c_int and len(S["tpnet_mlp_l4_bwd_f32"][1]) == 9
    assert S["tpnet_mlp_l4_bwd_workspace_bytes"] == (C.c_size_t, [C.c_int64])


def test_switch_defaults_to_off_and_cpu_tensors_are_declined(monkeypatch):
    import tpnet_amd
    from tpnet_amd import fused_feature as ff
    assert tpnet_amd.RandomProjectionModule.mlp_l4 is False
    assert {"l4", "l4_bwd"} <= set(ff.calls)
    monkeypatch.setattr(ff, "MLP_L4_FROM", 0)                                                # (routed or not: a CPU tensor is never the kernel's)
    torch.manual_seed(4)
    mlp = torch.nn.Sequential(torch.nn.Linear(100, 400), torch.nn.ReLU(), torch.nn.Linear(400, 100))
    before = dict(ff.calls)
    assert ff.mlp_l4(mlp, torch.rand(40, 100)) is None and ff.calls == before
