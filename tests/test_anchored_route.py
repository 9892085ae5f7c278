"""GPU test of the anchored readout's route (csrc/encoder.hip: anchored_route): what tpnet_anchored_route reports is what
tpnet_anchored_features does.  Where it reports a one-launch kind the call needs no feature buffer; where it does not, the call
without one is refused with TPNET_ERR_NEED_GRAM (an error return before any launch); with a buffer every shape gives self.mlp of
the buffer's features.  The table itself is tests/test_anchored_route_host.py."""
import numpy as np
import pytest
import torch

from test_fused_feature import _module, _stream

WALK, MFMA = 2, 3
# (d, rows8_readout, rows, K) -> (Gram kernel, one-launch kind): the fused kernel; the same on 8-byte rows; a wide row, whose one-launch
# kernel is no geometry class's route; K < 4, which only the walk reads
SHAPES = [((64, False, 3, 4), (MFMA, 1)), ((110, True, 3, 4), (MFMA, 1)), ((172, False, 3, 4), (WALK, 0)), ((64, False, 3, 3), (WALK, 0))]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,want_route", SHAPES)
def test_the_call_does_what_the_route_reports(shape, want_route):
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    from tpnet_amd import _lib
    d, rows8, rows, K = shape
    rng = np.random.RandomState(d + K)
    N = 300
    rp = _module(N, d, 3)
    rp.rows8_readout = rows8
    for src, dst, t in _stream(rng, N, 150, 3):
        rp.update(src, dst, t)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    wd = dev(rng.randint(0, N, rows * K).astype(np.int64))
    a1, a2 = dev(rng.randint(1, N, rows).astype(np.int64)), dev(rng.randint(1, N, rows).astype(np.int64))
    prep = rp._overlapped_mlp()
    assert prep is not None
    flags, served, one_launch = rp._anchored_route(rows, K, prep.ref)
    route = _lib.load().tpnet_anchored_route(rp._st_ref(), rows, K, flags, prep.ref)
    assert (route & 15, route >> 4) == want_route
    assert served and one_launch == (route >> 4 != 0) and bool(flags & _lib.FLAG_ROWS8) == rows8
    launch = rp._anchored_launch(wd, a1, a2, rows, K, prep, flags)
    gram = torch.empty((2 * rows * K, 64), dtype=torch.float32, device="cuda:0")
    with torch.no_grad():
        outs = [launch(gram)]
        if route >> 4:
            outs.append(launch(None))
        else:
            with pytest.raises(_lib.NeedGramBuffer):
                launch(None)
        want = rp.mlp(gram)
    scale = float(want.abs().max())
    for got in outs:
        err = (got - want).abs()
        print("error / scale %.3g" % (float(err.max()) / scale))
        assert bool((err <= 2e-5 * scale + 1e-4 * want.abs()).all()), (float(err.max()), scale)   # (test_encoder_widths.py's bound)
    rp.check_device_errors()
