"""tpnet_mlp_rows_supported / tpnet_mlp_rows_f32 (csrc/mlp_rows.hip: self.mlp on the matrix cores for num_layer 1 and 2): what the
two entries answer WITHOUT a device -- the table of served widths, and every argument check, which returns before any HIP call.
No compute call is made here (tests/test_mlp_rows.py does that, -m gpu)."""
import ctypes as C

import torch

from tpnet_amd import _lib

OK, BAD_ARG = 0, -1


def _mlp(F, H, base=0x10000):
    """A tpnet_mlp whose pointers are plausible VALUES only (16-byte aligned, never dereferenced by an argument check)."""
    return _lib.Mlp(w1t=base, b1=base + 0x1000, w2t=base + 0x2000, b2=base + 0x3000, F=F, H=H, w1=None, w2f=None, wimg=None)


def test_supported_widths(hip_lib):
    # the five (F, H) = ((2L+2)^2, 4F) of L = 1..4 and L = 5: L = 1 and 2 are served, L = 3 is tpnet_mlp64_f32's, L = 4 is not served
    table = {(16, 64): 1, (36, 144): 1, (64, 256): 0, (100, 400): 0, (144, 576): 0}
    for (F, H), want in table.items():
        assert hip_lib.tpnet_mlp_rows_supported(F, H) == want, (F, H)
    for F, H in [(0, 0), (-16, -64), (16, 144), (36, 64), (16, 63), (36, 145), (64, 16), (144, 36), (17, 68), (2 ** 31 - 1, 64)]:
        assert hip_lib.tpnet_mlp_rows_supported(F, H) == 0, (F, H)


def test_argument_checks_return_before_any_device_call(hip_lib):
    f = hip_lib.tpnet_mlp_rows_f32
    x, y = 0x200000, 0x300000
    for F, H in [(16, 64), (36, 144)]:
        m = _mlp(F, H)
        assert f(x, 5, None, y, None) == BAD_ARG                       # NULL mlp
        assert f(None, 5, C.byref(m), y, None) == BAD_ARG              # NULL x / y with n > 0
        assert f(x, 5, C.byref(m), None, None) == BAD_ARG
        assert f(x, -1, C.byref(m), y, None) == BAD_ARG
        for off in (4, 8, 12, 1):                                      # misaligned pointer values
            assert f(x + off, 5, C.byref(m), y, None) == BAD_ARG
            assert f(x, 5, C.byref(m), y + off, None) == BAD_ARG
        for field in ("w1t", "b1", "w2t", "b2"):                       # a weight array that is missing
            bad = _mlp(F, H)
            setattr(bad, field, None)
            assert f(x, 5, C.byref(bad), y, None) == BAD_ARG, field
        assert f(x, 0, C.byref(m), y, None) == OK                      # n == 0: nothing to do
        assert f(None, 0, C.byref(m), None, None) == OK
    for F, H in [(64, 256), (100, 400), (16, 144), (0, 0)]:            # an (F, H) that is not served
        m = _mlp(F, H)
        assert f(x, 5, C.byref(m), y, None) == BAD_ARG, (F, H)


def test_signatures_are_bound():
    assert _lib.SIGNATURES["tpnet_mlp_rows_supported"] == (C.c_int, [C.c_int32, C.c_int32])
    assert _lib.SIGNATURES["tpnet_mlp_rows_f32"][0] is C.c_int and len(_lib.SIGNATURES["tpnet_mlp_rows_f32"][1]) == 5


def test_mlp_f32_declines_cpu_tensors(monkeypatch):
    from tpnet_amd import fused_feature as ff
    assert set(ff.MLP_ROWS_FROM) == {16, 36}
    for F in (16, 36):
        monkeypatch.setitem(ff.MLP_ROWS_FROM, F, 0)                    # (routed or not: a CPU tensor is never the kernel's)
        torch.manual_seed(F)
        mlp = torch.nn.Sequential(torch.nn.Linear(F, 4 * F), torch.nn.ReLU(), torch.nn.Linear(4 * F, F))
        assert ff.mlp_f32(mlp, torch.rand(40, F)) is None
