"""One source against many candidates in one launch, without a GPU: the new C symbols (declared, exported, bound), the served sizes of
tpnet_score_one_to_many_supported, the argument checks, `score_one_to_many_host` (the float64 restatement the kernel is held to on
the GPU) against the torch layers in float64, and the skip rule of tpnet_lp_ranking_skip -- the host rule with one candidate column
per query marked absent -- on hand-worked cases.  Shared with tests/test_score_fanout.py: `skip_cases`, `skip_valid`, `score_bound`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_link_ranking_host import FLAG_EMPTY, FLAG_NAN, FLAG_NO_QUERY, assert_record, brute_force_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tpnet_score_one_to_many", "tpnet_score_one_to_many_supported", "tpnet_lp_ranking_skip")


def test_new_symbols_declared_exported_and_bound_with_matching_arity(hip_lib):
    from tpnet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tpnet_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert m, f"{name} is not declared in include/tpnet_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert getattr(hip_lib, name) is not None
    header = open(os.path.join(ROOT, "include", "tpnet_hip.h")).read()
    head = header[:header.index("#define TPNET_MAX_LAYERS")]
    assert "tpnet_score_one_to_many*" in head and "tpnet_lp_ranking_skip" in head          # the list of additions to ABI 7


def _state(d, L=3, N=64):
    from tpnet_amd import _lib
    return _lib.State(p0=16, q=16, meta=16, N=N, d=d, L=L, err=16)


def _mlp(F=64, H=256, w1=16, w2f=16):
    from tpnet_amd import _lib
    return _lib.Mlp(w1t=16, b1=16, w2t=16, b2=16, F=F, H=H, w1=w1, w2f=w2f, wimg=None)


def test_served_and_unserved_sizes(hip_lib):
    q = lambda d, L=3, H=172, off=344, ldw=408, mlp=None: hip_lib.tpnet_score_one_to_many_supported(
        ctypes.byref(_state(d, L)), ctypes.byref(_mlp() if mlp is None else mlp), H, off, ldw)
    for d in (36, 64, 100, 120, 128, 132, 160, 252, 256, 260, 384, 512):   # the four geometries, exact fit and masked
        assert q(d) == 1, d
    for d in (16, 30, 32, 110, 130, 258, 516, 1024):                       # narrow, odd, more than one chunk
        assert q(d) == 0, d
    for L in (1, 2, 4):
        assert q(128, L=L) == 0, L
    for H in (1, 16, 33, 172, 256):
        assert q(128, H=H) == 1, H
    for H in (0, -1, 257):
        assert q(128, H=H) == 0, H
    assert q(128, off=0, ldw=64) == 1 and q(128, off=8, ldw=72) == 1       # (D = 0 and D = 4)
    for off, ldw in ((342, 408), (344, 406), (344, 404), (-4, 64), (2, 66)):
        assert q(128, off=off, ldw=ldw) == 0, (off, ldw)
    for bad in (_mlp(F=36, H=144), _mlp(H=128), _mlp(w1=None), _mlp(w2f=None)):
        assert q(128, mlp=bad) == 0
    assert hip_lib.tpnet_score_one_to_many_supported(None, ctypes.byref(_mlp()), 172, 344, 408) == 0
    assert hip_lib.tpnet_score_one_to_many_supported(ctypes.byref(_state(128)), None, 172, 344, 408) == 0


def test_bad_arguments_are_rejected_without_a_gpu(hip_lib):
    st, mlp = _state(128, N=64), _mlp()
    call = lambda **kw: hip_lib.tpnet_score_one_to_many(*[kw.get(k, v) for k, v in (
        ("st", ctypes.byref(st)), ("src", 16), ("cand", 16), ("cand_lo", 0), ("lead", None), ("n_rows", 4), ("C", 5), ("now", 0.0),
        ("lam", 1e-6), ("flags", 0), ("mlp", ctypes.byref(mlp)), ("wd", 256), ("ldw", 408), ("off", 344), ("bd", 16), ("wd2", 16),
        ("bd2", 16), ("H", 172), ("gram", None), ("out", 256), ("stream", None))])
    wide, two = _state(516), _state(128, L=2)
    for bad in (dict(st=None), dict(src=None), dict(out=None), dict(mlp=None), dict(wd=None), dict(bd=None), dict(wd2=None),
                dict(bd2=None), dict(C=0), dict(C=-3), dict(n_rows=-1), dict(n_rows=1 << 40), dict(n_rows=(1 << 31) // 6 + 1),
                dict(flags=8), dict(out=258), dict(gram=260), dict(wd=260), dict(bd=18), dict(H=0), dict(H=257), dict(off=342),
                dict(ldw=406), dict(st=ctypes.byref(wide)), dict(st=ctypes.byref(two)),
                dict(cand=None, cand_lo=-1), dict(cand=None, cand_lo=60), dict(cand=None, cand_lo=64)):       # the range leaves [0, N)
        assert call(**bad) == -1, bad                                # (nothing is launched: there is no GPU here)
        if "n_rows" not in bad:
            assert call(n_rows=0, **bad) == -1, bad                  # ... and an empty call does not excuse them
    assert call(n_rows=0) == 0 and call(n_rows=0, cand=None, cand_lo=59) == 0 and call(n_rows=0, lead=16, gram=256) == 0
    # ---- the skip record takes tpnet_lp_ranking's checks, and needs its skip column
    rank = lambda **kw: hip_lib.tpnet_lp_ranking_skip(*[kw.get(k, v) for k, v in (
        ("logits", 8), ("B", 4), ("C1", 5), ("skip", 8), ("k1", 1), ("k2", 3), ("k3", 10), ("scratch", 8), ("bytes", 1 << 20),
        ("record", 64), ("stream", None))])
    for bad in (dict(logits=None), dict(B=-1), dict(C1=0), dict(k1=0), dict(k2=-1), dict(k3=0), dict(scratch=None), dict(scratch=12),
                dict(record=None), dict(record=68), dict(skip=None), dict(skip=12)):
        assert rank(**bad) == -1, bad
    assert rank(bytes=16) == -2


def test_surface_on_a_cpu_module():
    """The switch exists and is off; without not_encode forward_one_to_all refuses; a CPU module takes no kernel route."""
    from tpnet_amd import RandomProjectionModule
    from tpnet_amd.callers import LinkPredictor_v1
    rp = RandomProjectionModule(node_num=20, edge_num=50, dim_factor=10, num_layer=3, time_decay_weight=1e-6, device="cpu",
                                use_matrix=False, beginning_time=np.float64(0.0), not_scale=False, enforce_dim=64)
    dec = LinkPredictor_v1(4, 4, 8, 1, rp, not_encode=False)
    assert dec.fused_scores is False and LinkPredictor_v1.SCORE_ALL_FUSED in (False, True)
    with pytest.raises(ValueError):
        dec.forward_one_to_all(np.array([1, 2]), 1, 20)
    dec = LinkPredictor_v1(4, 4, 8, 1, rp, not_encode=True)
    dec.fused_scores = True
    assert dec._scores_fused(False, True) is False                          # not on a GPU
    with pytest.raises(ValueError):
        dec.forward_one_to_all(np.array([1, 2]), 5, 5)


# ------------------------------------------------------------------------------------------------------- the float64 restatement

def score_bound(want, mags, c=4e-5, floor=1e-6):
    """The per-entry bound of a logit of the fp32 class against `want` (score_one_to_many_host's logits and magnitudes): the
    project's fp32-class bound c mag + floor max|want| (tests/test_decoder_f32.py) applied per stage and carried through the later
    stages by their absolute-value weights, ReLU being 1-Lipschitz:
      e_y = c (|W2m| relu(|W1m||f| + |b1m|) + |b2m|);  e_a = |Wd_f| e_y + c (|Wd_f||y| + |bd|);
      e   = |wd2| e_a + c (|wd2| (|Wd_f||y| + |bd|) + |bd2|) + floor max|want|."""
    e_y = c * mags["mag_y"]
    e_a = e_y @ mags["abs_wdf"].T + c * mags["mag_a"]
    return e_a @ mags["abs_wd2"] + c * (mags["mag_a"] @ mags["abs_wd2"] + mags["abs_bd2"]) + floor * float(np.abs(want).max())


@pytest.mark.parametrize("D,H", [(172, 172), (8, 16), (4, 1), (4, 33), (4, 256)])
def test_host_restatement_against_the_torch_layers_in_float64(D, H):
    from tpnet_amd.score_fanout import score_one_to_many_host
    gen = torch.Generator().manual_seed(100 * D + H)
    mlp = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.ReLU(), torch.nn.Linear(256, 64)).double()
    fc1, fc2 = torch.nn.Linear(2 * D + 64, H).double(), torch.nn.Linear(H, 1).double()
    f = torch.rand(50, 64, generator=gen, dtype=torch.float64) * 6.0 - 1.0
    with torch.no_grad():
        x = torch.cat([torch.zeros(50, 2 * D, dtype=torch.float64), mlp(f)], dim=1)
        want = fc2(torch.relu(fc1(x)))[:, 0].numpy()
        y = mlp(f).numpy()
    got, mags = score_one_to_many_host(f, (mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias), (fc1.weight, fc1.bias),
                                       (fc2.weight, fc2.bias), 2 * D)
    assert got.shape == (50,) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.abs(mags["y"] - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
    assert mags["mag_y"].shape == (50, 64) and mags["mag_a"].shape == (50, H) and (mags["mag_y"] >= np.abs(y) - 1e-12).all()
    a = y @ fc1.weight[:, 2 * D:].detach().numpy().T + fc1.bias.detach().numpy()
    assert (mags["mag_a"] >= np.abs(a) - 1e-12).all()
    bound = score_bound(want, mags)
    assert bound.shape == (50,) and (bound > 0).all() and (bound < 1e-2 * max(1.0, np.abs(want).max()) + 1.0).all()


# ----------------------------------------------------------------------------------------------------------------- the skip rule

def skip_valid(B, C, skip):
    """The mask of the host rule: valid[i, skip[i]] = False where 0 <= skip[i] < C."""
    v = np.ones((B, C), dtype=bool)
    for i, s in enumerate(skip):
        if 0 <= s < C:
            v[i, s] = False
    return v


def skip_cases():
    """name -> (logits [B, 1 + C] fp32, skip [B] int64, hits_at, the hand-worked record or None)."""
    nan = np.float32(np.nan)
    cases = {}
    x = np.array([[1.0, 3.0, 0.0, 2.0], [0.0, 1.0, 1.0, 1.0]], dtype=np.float32)
    # q1: g = 2 -> m = 6; q2: g = 3 -> m = 8
    cases["skip_none"] = (x, np.array([-1, -1]), (1, 3, 10),
                          dict(m_sum=14, n=2, n_valid_candidates=6, flags=0, mrr=(2 / 6 + 2 / 8) / 2, hits=(0.0, 0.5, 1.0)))
    # q1 without its first candidate (3.0): g = 1 -> m = 4; q2 without its last: g = 2 -> m = 6
    cases["skip_first_and_last"] = (x, np.array([0, 2]), (1, 3, 10),
                                    dict(m_sum=10, n=2, n_valid_candidates=4, flags=0, mrr=(2 / 4 + 2 / 6) / 2, hits=(0.0, 1.0, 1.0)))
    # the destination's own copy ties with the lead and is skipped: rank 1, not 1.5; the second query keeps its tie: m = 3
    t = np.array([[2.0, 2.0, 1.0, 0.0], [2.0, 1.0, 2.0, 0.0]], dtype=np.float32)
    cases["tie_with_the_lead"] = (t, np.array([0, 0]), (1, 3, 10),
                                  dict(m_sum=5, n=2, n_valid_candidates=4, flags=0, mrr=(2 / 2 + 2 / 3) / 2, hits=(0.5, 1.0, 1.0)))
    # a NaN under the skipped column is not looked at; the same NaN unskipped disqualifies its query
    n = np.array([[1.0, nan, 0.0, 2.0], [1.0, nan, 0.0, 2.0]], dtype=np.float32)
    cases["nan_under_the_skipped_column"] = (n, np.array([0, 1]), (1, 3, 10),
                                             dict(m_sum=4, n=1, n_valid_candidates=4, flags=FLAG_NAN, mrr=0.5, hits=(0.0, 1.0, 1.0)))
    # C1 = 2 and the only candidate skipped: an empty query; the other one ranks second
    e = np.array([[1.0, 5.0], [1.0, 5.0]], dtype=np.float32)
    cases["only_candidate_skipped"] = (e, np.array([0, -1]), (1, 3, 10),
                                       dict(m_sum=4, n=1, n_valid_candidates=1, flags=FLAG_EMPTY, mrr=0.5, hits=(0.0, 1.0, 1.0)))
    cases["B0"] = (np.zeros((0, 4), dtype=np.float32), np.zeros(0, dtype=np.int64), (1, 3, 10),
                   dict(m_sum=0, n=0, n_valid_candidates=0, flags=FLAG_NO_QUERY, mrr=float("nan"), hits=(float("nan"),) * 3))
    rng = np.random.RandomState(12)
    r = np.round(rng.randn(40, 14) * 2).astype(np.float32) / 2
    cases["random_grid"] = (r, rng.randint(-1, 13, 40).astype(np.int64), (1, 2, 5), None)
    return {k: (x, np.asarray(s, dtype=np.int64), ks, w) for k, (x, s, ks, w) in cases.items()}


@pytest.mark.parametrize("name", sorted(skip_cases()))
def test_skip_rule_on_hand_worked_cases(name):
    from tpnet_amd.metrics import link_ranking_metrics_host
    x, skip, ks, hand = skip_cases()[name]
    valid = skip_valid(x.shape[0], x.shape[1] - 1, skip)
    got = link_ranking_metrics_host(x, valid, hits_at=ks)
    assert_record(got, brute_force_record(x, valid, ks), name)
    if hand is not None:
        assert_record(got, hand, name + " (by hand)")
