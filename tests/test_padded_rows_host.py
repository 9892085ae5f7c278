"""CPU tests of the opt-in padded engine rows (RandomProjectionModule.padded_rows): the engine_dim rule, the four C entry points that
convert between the caller's row width and the engine's (declared, exported, bound, and refusing bad arguments before any launch),
and the Python surface that needs no kernel.  The compute side is tests/test_padded_rows.py (-m gpu)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tpnet_import_layers_ld", "tpnet_export_layers_ld", "tpnet_pad_rows", "tpnet_gather_rows_ld")


def _mk(**kw):
    from tpnet_amd import RandomProjectionModule
    args = dict(node_num=50, edge_num=120, dim_factor=10, num_layer=3, time_decay_weight=1e-6, device="cpu",
                use_matrix=False, beginning_time=np.float64(12.5), not_scale=False, enforce_dim=32)
    args.update(kw)
    return RandomProjectionModule(**args)


@pytest.mark.parametrize("use_matrix", [False, True])
def test_engine_dim_rule(use_matrix):
    """engine_dim = dim rounded up to a multiple of 4 only with the switch set, use_matrix false and dim % 4 != 0; else dim."""
    from tpnet_amd import RandomProjectionModule
    assert RandomProjectionModule.padded_rows is False
    for d in range(1, 21):
        rp = _mk(node_num=d if use_matrix else 50, enforce_dim=-1 if use_matrix else d, use_matrix=use_matrix)
        assert rp.dim == d and rp.padded_rows is False and rp.engine_dim == d
        rp.padded_rows = True
        want = d if (use_matrix or d % 4 == 0) else (d + 3) // 4 * 4
        assert rp.engine_dim == want and rp.dim == d
        assert tuple(rp.random_projections[0].shape) == (rp.node_num, d)
        rp.padded_rows = False
        assert rp.engine_dim == d
    assert RandomProjectionModule.padded_rows is False                    # (set per instance: the class keeps its default)


def test_switch_keeps_the_reference_surface_on_the_host():
    """State-dict keys and shapes, copies and pickles of a module with the switch set are those of one without; the switch itself
    travels with a copy."""
    import copy
    import pickle
    a, b = _mk(enforce_dim=110), _mk(enforce_dim=110)
    a.padded_rows = True
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    assert [tuple(v.shape) for v in sa.values()] == [tuple(v.shape) for v in sb.values()]
    for c in (copy.deepcopy(a), pickle.loads(pickle.dumps(a))):
        assert c.padded_rows is True and c.engine_dim == 112 and c.dim == 110
        assert torch.equal(c.random_projections[0], a.random_projections[0])
    b.load_state_dict(sa)
    assert torch.equal(b.random_projections[0], a.random_projections[0])
    assert a.anchored_call_served(8, 5) and not _mk(enforce_dim=110).anchored_call_served(8, 5)


def test_handing_out_entry_zero_is_noticed():
    """Entry 0 of the list handed out (it may then be written through .data): remembered for the wide copy of P[0]; the hot methods'
    own access (_plist) does not count, and layers 1..L stay lazy about it."""
    rp = _mk(enforce_dim=110)
    rp.padded_rows = True
    rp._p0_exposed = False
    rp._params_exposed = False
    rp._plist()[0]
    len(rp.random_projections)
    assert rp._p0_exposed is False
    rp.random_projections[0]
    assert rp._p0_exposed is True and rp._params_exposed is False
    rp._p0_exposed = False
    list(rp.random_projections)
    assert rp._p0_exposed is True
    rp._p0_exposed = False
    rp.state_dict()
    assert rp._p0_exposed is True


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "tpnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(tpnet_[a-z_0-9]+)\s*\(", text))


def test_new_symbols_declared_exported_and_bound(hip_lib):
    from tpnet_amd import _lib
    declared = _declared_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in declared, f"{s} not declared in include/tpnet_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _lib.SIGNATURES, f"{s} not bound"
        assert getattr(hip_lib, s).restype is ctypes.c_int
    assert hip_lib.tpnet_abi_version() == 7


def test_bad_arguments_are_refused_before_any_launch(hip_lib):
    """Null pointers, ld outside 1..d, a wide side that is not whole 16-byte vectors at a 16-byte aligned address: -1 (on a machine
    without a GPU a launch would give the HIP error -3 instead)."""
    from tpnet_amd import _lib
    ptrs = (ctypes.c_void_p * 3)(64, 64, 64)
    ok = dict(p0=64, q=64, meta=64, N=10, d=8, L=3, err=64)

    def st(**kw):
        return ctypes.byref(_lib.State(**{**ok, **kw}))
    for fn, tail in ((hip_lib.tpnet_import_layers_ld, (0.0, None)), (hip_lib.tpnet_export_layers_ld, (0.0, 0.0, None))):
        assert fn(None, ptrs, 6, *tail) == -1
        assert fn(st(), None, 6, *tail) == -1
        assert fn(st(), (ctypes.c_void_p * 3)(64, None, 64), 6, *tail) == -1          # a null layer
        assert fn(st(), ptrs, 0, *tail) == -1 and fn(st(), ptrs, 9, *tail) == -1       # ld outside 1..d
        assert fn(st(q=72), ptrs, 6, *tail) == -1                                      # q not 16-byte aligned
        assert fn(st(d=6), ptrs, 6, *tail) == -1                                       # wide rows that are no whole vectors
        assert fn(st(q=None), ptrs, 6, *tail) == -1
    pad = hip_lib.tpnet_pad_rows
    assert pad(None, 6, 64, 8, 5, None) == -1 and pad(64, 6, None, 8, 5, None) == -1
    assert pad(64, 0, 64, 8, 5, None) == -1 and pad(64, 9, 64, 8, 5, None) == -1
    assert pad(64, 6, 72, 8, 5, None) == -1 and pad(64, 6, 64, 6, 5, None) == -1 and pad(64, 6, 64, 8, -1, None) == -1
    assert pad(64, 6, 64, 8, 0, None) == 0                                             # no rows: nothing to launch
    g = hip_lib.tpnet_gather_rows_ld
    assert g(st(), None, 2, 0.0, 0.0, 6, 64, None) == -1 and g(st(), 64, 2, 0.0, 0.0, 6, None, None) == -1
    assert g(st(), 64, 2, 0.0, 0.0, 0, 64, None) == -1 and g(st(), 64, 2, 0.0, 0.0, 9, 64, None) == -1
    assert g(st(p0=68), 64, 2, 0.0, 0.0, 6, 64, None) == -1 and g(st(q=72), 64, 2, 0.0, 0.0, 6, 64, None) == -1
    assert g(st(), 64, -1, 0.0, 0.0, 6, 64, None) == -1
    assert g(st(), 64, 0, 0.0, 0.0, 6, 64, None) == 0
