"""The small shared pieces of the row-shard runner (tpnet_amd/sharded.py) on the CPU: the placement of rows that arrive without
RCCL, the output buffers of a call, and the finished exchange plan against the arrays recorded before the plan had one spelling
(tests/golden/sharded_exchange_plan.npz, made by tests/golden/make_sharded_plan.py)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from test_sharded import _stream  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sharded_exchange_plan.npz")
PLAN_RANKS = [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]
PLAN_FIELDS = ("send_cnt", "recv_cnt", "stot", "rtot", "sstart", "smax", "pack_ids", "unpack_ids", "src", "dst", "neg")


def exchange_plan_of(runner_cls, world, rank):
    """_exchange_plan of rank `rank` of `world` on the stream of test_targeted_relabelling_gloo (torch plan: CPU ids)."""
    N, E, B = 97, 300, 40

    class _Stub:                                   # stands in for the local module (no GPU in this tier)
        node_num = (N + world - 1) // world + 3 * B

        def _drop_plan(self):
            pass
    src, dst, neg, t = (torch.from_numpy(x) for x in _stream(2, N, E))
    return runner_cls(_Stub(), N, 3 * B, world=world, rank=rank)._exchange_plan(src, dst, neg, t, B)


@pytest.mark.parametrize("world,rank", PLAN_RANKS)
def test_finished_exchange_plan_equals_the_recorded_one(world, rank):
    from tpnet_amd.sharded import ShardedStreamRunner
    want = np.load(GOLDEN)
    R, _ = exchange_plan_of(ShardedStreamRunner, world, rank)
    for f in PLAN_FIELDS:
        got = R[f].numpy() if isinstance(R[f], torch.Tensor) else np.asarray(R[f])
        w = want[f"w{world}_r{rank}_{f}"]
        assert got.dtype == w.dtype and got.shape == w.shape, (f, got.dtype, w.dtype, got.shape, w.shape)
        np.testing.assert_array_equal(got, w, err_msg=f)
    assert R["send_cnt"].flags.c_contiguous and R["recv_cnt"].flags.c_contiguous and R["sstart"].flags.c_contiguous  # (C reads them)
    # the same record from the relabelling alone, and a halo too small is the one ValueError
    run = ShardedStreamRunner.__new__(ShardedStreamRunner)
    run.G, run.me, run.N, run.n_cap, run.H = world, rank, 97, (97 + world - 1) // world, int(R["rtot"].max())
    src, dst, neg, _ = (torch.from_numpy(x) for x in _stream(2, 97, 300))
    R2 = run.relabel_targeted(src, dst, neg, 40)
    assert all(np.array_equal(np.asarray(R2[f]), np.asarray(R[f])) for f in PLAN_FIELDS)
    run.H -= 1
    with pytest.raises(ValueError, match=f"a batch reads {run.H + 1} rows of other ranks but the shard has {run.H} halo rows"):
        run.relabel_targeted(src, dst, neg, 40)


@pytest.mark.parametrize("G", [2, 3, 5])
@pytest.mark.parametrize("shared", [False, True])
def test_place_rows_against_a_restatement(G, shared):
    """Every destination row comes from the owner and source row the rule names -- what owner o packed for reader r sits behind what it
    packed for the readers < r (shared: from its row 0) and lands behind what the owners < o sent -- and no other row is written."""
    from tpnet_amd.sharded import place_rows
    rng = np.random.RandomState(10 * G + int(shared))
    for case in range(12):
        cnt = rng.randint(0, 5, (G, G))                                    # cnt[o][r]: rows owner o packed for reader r
        cnt[np.arange(G), np.arange(G)] = 0                                # (a rank sends itself nothing)
        if case % 3 == 1:
            cnt[rng.randint(G)] = 0                                        # an owner that sends nothing
        if case % 3 == 2:
            cnt[:, rng.randint(G)] = 0                                     # a reader that receives nothing
        if case == 11:
            cnt[:] = 0
        widths = (3, 2)
        # row k of owner o's buffer w holds 1000 * o + 10 * k + w in every column
        bufs = [tuple(torch.from_numpy(np.repeat((1000 * o + 10 * np.arange(cnt[o].sum() + 4) + w)[:, None], wd, 1).astype(np.float32))
                      for w, wd in enumerate(widths)) for o in range(G)]
        for me in range(G):
            row0, total = int(rng.randint(0, 4)), int(cnt[:, me].sum())
            dst = tuple(torch.full((row0 + total + 3, wd), -1.0) for wd in widths)
            before = [b.clone() for o in range(G) for b in bufs[o]]
            assert place_rows(dst, row0, bufs, cnt, me, shared=shared) == total
            want = [np.full((row0 + total + 3, wd), -1.0, dtype=np.float32) for wd in widths]
            row = row0
            for o in range(G):
                for k in range(cnt[o][me]):
                    src_row = k if shared else int(cnt[o][:me].sum()) + k
                    for w in range(len(widths)):
                        want[w][row] = 1000 * o + 10 * src_row + w
                    row += 1
            for w in range(len(widths)):
                np.testing.assert_array_equal(dst[w].numpy(), want[w])
            assert all(torch.equal(a, b) for a, b in zip(before, [b for o in range(G) for b in bufs[o]]))


def test_output_buffers_accept_raise_and_zero():
    from tpnet_amd.sharded import output_buffers
    E, NG, cpu = 5, 16, torch.device("cpu")
    # fresh buffers: zeroed by default, `alloc`'s otherwise; no out_neg without negatives
    op, on = output_buffers(E, NG, cpu, True)
    assert op.shape == on.shape == (E, NG) and op.dtype == on.dtype == torch.float32 and not op.any() and not on.any()
    op, on = output_buffers(E, NG, cpu, False)
    assert on is None and op.shape == (E, NG)
    seen = []
    op, on = output_buffers(E, NG, cpu, True, alloc=lambda *a, **k: seen.append(1) or torch.full(*a, 7.0, **k))
    assert len(seen) == 2 and bool((op == 7).all()) and bool((on == 7).all())
    # a caller's buffers: the same objects, zeroed only if asked; a caller's out_neg is dropped without negatives
    for zero in (False, True):
        mine_p, mine_n = torch.full((E, NG), 3.0), torch.full((E, NG), 4.0)
        op, on = output_buffers(E, NG, cpu, True, mine_p, mine_n, zero)
        assert op is mine_p and on is mine_n
        assert bool((op == (0.0 if zero else 3.0)).all()) and bool((on == (0.0 if zero else 4.0)).all())
    mine_p, mine_n = torch.full((E, NG), 3.0), torch.full((E, NG), 4.0)
    op, on = output_buffers(E, NG, cpu, False, mine_p, mine_n, True)
    assert op is mine_p and on is None and bool((mine_n == 4.0).all())
    op, on = output_buffers(E, NG, cpu, True, mine_p, None, False)
    assert op is mine_p and on.shape == (E, NG) and not on.any()
    # refused: wrong shape, dtype, layout or device -- out_neg even where it would not be used, and nothing is zeroed before the error
    bad = [torch.zeros((E + 1, NG)), torch.zeros((E, NG + 1)), torch.zeros(E * NG), torch.zeros((E, NG), dtype=torch.float64),
           torch.zeros((NG, E)).t(), torch.zeros((E, NG), device="meta")]
    for b in bad:
        for name, kw in (("out_pos", dict(out_pos=b)), ("out_neg", dict(out_pos=torch.full((E, NG), 3.0), out_neg=b))):
            for have_neg in (True, False):
                with pytest.raises(ValueError, match=rf"{name} must be a contiguous float32 tensor of shape \({E}, {NG}\) on cpu"):
                    output_buffers(E, NG, cpu, have_neg, zero=True, **kw)
                assert kw["out_pos"] is b or bool((kw["out_pos"] == 3.0).all())
