"""The host-side helpers of RandomProjectionModule that every route shares: the pinned upload's packing, the id normaliser and the
engine-side initialiser.  No GPU needed: the pinned buffer and the stream are stood in for."""
import numpy as np
import pytest
import torch

from tpnet_amd import RandomProjectionModule
from tpnet_amd import random_projection as R
from tpnet_amd.matrix_memory import _bare_table

N = 10


def _mk():
    return RandomProjectionModule(node_num=N, edge_num=120, dim_factor=10, num_layer=3, time_decay_weight=1e-6, device="cpu",
                                  use_matrix=False, beginning_time=np.float64(12.5), not_scale=False, enforce_dim=8)


class _Event:
    def __init__(self):
        self.recorded = 0

    def record(self, stream):
        self.recorded += 1


def _host_upload(monkeypatch, rp):
    """_to_device with a plain host tensor for the pinned buffer and the host for the device: returns the slot it uses."""
    slot = [torch.full((64,), -7, dtype=torch.int64), _Event()]
    monkeypatch.setattr(rp, "_dev", lambda: torch.device("cpu"))
    monkeypatch.setattr(rp, "_pin_slot", lambda items: slot)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: None)
    return slot


def test_upload_packs_equal_lengths_as_rows(monkeypatch):
    """Equally long arrays (what the former _to_device took): array i is row i of a [k, n] int64 block at the head of the buffer;
    float64 arrays come back as float64 views of their bits."""
    rp = _mk()
    slot = _host_upload(monkeypatch, rp)
    u, v, t = np.array([1, 2, 3], dtype=np.int64), np.array([7, 8, 9], dtype=np.int64), np.array([0.5, 1.5, -2.25])
    du, dv, dt = rp._to_device(u, v, t)
    assert slot[1].recorded == 1
    np.testing.assert_array_equal(slot[0][:9].view(3, 3).numpy(), np.stack([u, v, t.view(np.int64)]))
    assert (slot[0][9:] == -7).all()
    assert du.dtype == dv.dtype == torch.int64 and dt.dtype == torch.float64
    np.testing.assert_array_equal(du.numpy(), u)
    np.testing.assert_array_equal(dv.numpy(), v)
    np.testing.assert_array_equal(dt.numpy(), t)


def test_upload_packs_unequal_lengths_end_to_end(monkeypatch):
    """Arrays of different lengths (what the former _to_device_multi took): end to end in argument order, one view each; an empty
    array gets an empty view."""
    rp = _mk()
    slot = _host_upload(monkeypatch, rp)
    w, a1, e, t = np.arange(6, dtype=np.int64), np.array([4, 5], dtype=np.int64), np.zeros(0, dtype=np.int64), np.array([3.0])
    dw, da, de, dt = rp._to_device(w, a1, e, t)
    np.testing.assert_array_equal(slot[0][:9].numpy(), np.concatenate([w, a1, t.view(np.int64)]))
    assert [x.numel() for x in (dw, da, de, dt)] == [6, 2, 0, 1]
    np.testing.assert_array_equal(dw.numpy(), w)
    np.testing.assert_array_equal(da.numpy(), a1)
    assert de.dtype == torch.int64 and dt.dtype == torch.float64 and dt.item() == 3.0
    # a strided view (the encoder's anchors: dst[:h:K]) is packed by value
    s = np.arange(12, dtype=np.int64)[::4]
    np.testing.assert_array_equal(rp._to_device(s, a1)[0].numpy(), [0, 4, 8])


def test_upload_leaves_tensors_alone_and_brings_mixed_ones_to_the_host(monkeypatch):
    rp = _mk()
    _host_upload(monkeypatch, rp)
    a, b = torch.tensor([1, 2]), torch.tensor([3, 4])
    out = rp._to_device(a, b)
    assert out[0] is a and out[1] is b                       # all tensors: returned as they are, nothing staged
    da, dt = rp._to_device(a, np.array([0.25, 0.75]))
    np.testing.assert_array_equal(da.numpy(), [1, 2])
    np.testing.assert_array_equal(dt.numpy(), [0.25, 0.75])


_RANGE = "x: index out of range for 10 nodes"
_DIM = "x must be one-dimensional"
# input, what the C calls that stage ids themselves get (staged=True), what an upload gets: an array's values, None, or the error
_ID_TABLE = [
    ([1, 2, 3], [1, 2, 3], [1, 2, 3]),
    (np.array([4, 5], dtype=np.int32), [4, 5], [4, 5]),
    (np.arange(10)[::3], [0, 3, 6, 9], [0, 3, 6, 9]),
    (np.arange(6).reshape(2, 3), (ValueError, _DIM), (ValueError, _DIM)),
    (np.arange(6).reshape(2, 3)[:, 0], [0, 3], [0, 3]),
    ([-1, 2], [-1, 2], [9, 2]),                              # (staged: wrapped by the C call; upload: as ATen indexing)
    ([-10, 9], [-10, 9], [0, 9]),
    ([3, 10], [3, 10], (IndexError, _RANGE)),                # (staged: left to the C call's check)
    ([-11], [-11], (IndexError, _RANGE)),
    (np.zeros(0, dtype=np.int64), [], []),
    ([], [], []),
    (torch.tensor([1, 2]), None, [1, 2]),                    # (a host tensor: no staging; uploaded like an array)
    (5, (ValueError, _DIM), [5]),
    (np.int64(-2), (ValueError, _DIM), [8]),
]


@pytest.mark.parametrize("staged", [True, False])
def test_id_normaliser_accepts_and_raises_as_before(staged):
    rp = _mk()
    for ids, want_staged, want_upload in _ID_TABLE:
        want = want_staged if staged else want_upload
        if isinstance(want, tuple):
            with pytest.raises(want[0]) as e:
                rp._ids(ids, "x", staged)
            assert str(e.value) == want[1], ids
        elif want is None:
            assert rp._ids(ids, "x", staged) is None
        else:
            got = rp._ids(ids, "x", staged)
            assert type(got) is np.ndarray and got.dtype == np.int64 and got.ndim == 1 and got.flags.c_contiguous, ids
            np.testing.assert_array_equal(got, np.asarray(want, dtype=np.int64))
    ready = np.array([0, 9, 4], dtype=np.int64)
    assert rp._ids(ready, "x", staged) is ready              # what the reference's callers pass: no copy


def test_id_normaliser_checks_staged_ids_for_the_exact_mode():
    """update() in exact mode checks the range of host ids before it enqueues the decay: the normaliser on the staged arrays."""
    rp = _mk()
    rp._ids(rp._ids([-10, 9], "x", True), "x")
    for bad in ([0, 10], [-11, 0]):
        with pytest.raises(IndexError) as e:
            rp._ids(rp._ids(bad, "x", True), "x")
        assert str(e.value) == _RANGE


def test_device_ids_are_checked_for_type_and_shape_only():
    class _Dev(torch.Tensor):                                # (stands in for a cuda tensor: is_cuda is all the normaliser asks)
        is_cuda = True
    rp = _mk()
    ok = torch.tensor([1, 2, 99]).as_subclass(_Dev)
    assert rp._ids(ok, "x").data_ptr() == ok.data_ptr() and rp._ids(ok, "x", True) is None       # used in place, range unchecked
    for bad in (torch.tensor([1, 2], dtype=torch.int32), torch.tensor([[1, 2]])):
        with pytest.raises(ValueError) as e:
            rp._ids(bad.as_subclass(_Dev), "x")
        assert str(e.value) == "x: device ids must be a one-dimensional int64 tensor"


def test_readout_flags():
    from tpnet_amd import _lib
    rp = _mk()
    assert rp._readout_flags() == 0
    assert rp._readout_flags(raw=True) == _lib.FLAG_NOT_SCALE
    assert rp._readout_flags(packed=True) == _lib.FLAG_NOT_SCALE | _lib.FLAG_PACKED
    assert rp._readout_flags(matrix_cores=False) == _lib.FLAG_NO_MFMA_READOUT
    rp.not_scale = True
    assert rp._readout_flags() == _lib.FLAG_NOT_SCALE
    assert rp._readout_flags(True, True, False) == _lib.FLAG_NOT_SCALE | _lib.FLAG_PACKED | _lib.FLAG_NO_MFMA_READOUT


def test_advanced_marks_clock_layers_and_table():
    rp = _mk()
    sig = rp._table_sig
    rp._advanced(99.0)
    assert rp._now_host == 99.0 and rp._params_valid is False and rp._now_dirty is True
    assert rp._table_sig != sig and rp._table_sig % 2 == 0
    assert float(rp.now_time) == 99.0 and rp._now_dirty is False          # (the stale clock Parameter is filled when it is read)


def test_bare_table_has_every_field_of_the_constructor():
    """matrix_memory._bare_table builds an instance without the constructor: it must leave every attribute the constructor
    leaves, the engine-side bookkeeping included (no class-level defaults stand in for them)."""
    full = _mk()
    bare = RandomProjectionModule.__new__(RandomProjectionModule)
    _bare_table(bare, 6, 2, "cpu")
    assert set(full.__dict__) <= set(bare.__dict__), set(full.__dict__) - set(bare.__dict__)
    engine_side = ("_eng", "_engine_valid", "_params_valid", "_param_sig", "_now_host", "_launch_id", "_now_dirty", "_params_exposed",
                   "_table_sig", "_sig_counter", "_plan_tag", "_rows_plan_sig")
    fresh = RandomProjectionModule.__new__(RandomProjectionModule)
    fresh._init_engine_side(0.0)
    assert set(fresh.__dict__) == set(engine_side)
    for name in engine_side:
        assert name in bare.__dict__ and name not in vars(RandomProjectionModule), name
        assert bare.__dict__[name] == fresh.__dict__[name], name
    assert bare._now_host == 0.0 and full._now_host == 12.5
    assert (bare.node_num, bare.dim, bare.num_layer, len(bare._plist())) == (6, 6, 2, 3)
    bare._drop_plan()
    bare._table_written()
    assert bare._table_sig == 4
    assert R._StateRef._fields == ("p0", "eng", "st", "ref", "addr")
