"""EdgeBank on the device (tpnet_amd/edge_bank.py, csrc/edgebank.hip: tpnet_edgebank_*) against fixture G15
(tests/golden/make_golden_edge_bank.py: the reference's own `edge_bank_link_prediction`, its window start read from its frame) and
against the numpy statement of the rule, `edge_bank_host`.

The rule is deterministic, so predictions are compared for equality.  The 'fixed_proportion' window start is np.quantile's, bit for
bit.  The 'repeat_interval' window start t[h - 1] - S / n_present is held within 1e-12 relative: S is a float64 sum of at most a few
thousand terms of one sign, each good to 2^-53, summed in another order than the reference's dict order (n 2^-53 < 1e-12 for
n < 9000); where no fixture guards against it, a prediction is compared only if its deciding stamp is further than 1e-6 from the
window start.  Loss: 1e-12 max(1, loss); AP / AUC: 1e-10, the bounds tests/test_metrics.py uses for G14."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tpnet_amd import _lib
from tpnet_amd.edge_bank import GpuEdgeBank, edge_bank_host, edge_bank_link_prediction
from tpnet_amd.metrics import LinkPredictionMeter, link_prediction_metrics_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("unlimited_memory", "fixed_proportion", 0.15), ("time_window_memory", "fixed_proportion", 0.15),
           ("time_window_memory", "repeat_interval", 0.15), ("repeat_threshold_memory", "fixed_proportion", 0.15)]
REPEAT_INTERVAL = 2
AP_TOL = 1e-10
WINDOW_RTOL = 1e-12

_cache = {}


def g15():
    """Fixture G15: loaded once, never written."""
    if "g" not in _cache:
        _cache["g"] = dict(np.load(os.path.join(ROOT, "tests", "golden", "g15_edge_bank.npz")))
    return _cache["g"]


def big_stream():
    """E = 6000 over 60 x 60 nodes (U > 1024: the unique edges span several workgroups), stamps to one decimal (ties), 1025 queries of
    which a third are stream pairs; per (configuration, h) the host rule's predictions and bound: computed once, never written."""
    if "big" not in _cache:
        rng = np.random.RandomState(6000)
        E = 6000
        src, dst = rng.randint(1, 61, E).astype(np.int64), rng.randint(61, 121, E).astype(np.int64)
        t = np.round(np.sort(rng.uniform(0.0, 1.0e4, E)), 1)
        qs, qd = rng.randint(0, 63, 1025).astype(np.int64), rng.randint(59, 123, 1025).astype(np.int64)
        own = rng.permutation(1025)[:340]
        at = rng.randint(0, E, 340)
        qs[own], qd[own] = src[at], dst[at]
        host = {(c, h): edge_bank_host(src, dst, t, h, qs, qd, *CONFIGS[c]) for c in range(4) for h in BIG_H}
        _cache["big"] = (src, dst, t, qs, qd, host)
    return _cache["big"]


BIG_H = (1, 255, 256, 257, 3000, 6000)
BIG_Q = (1, 63, 64, 65, 257, 1025)


def loss_tol(loss):
    return 1e-12 * max(1.0, abs(loss))


def rel(x, y):
    return abs(x - y) / max(abs(y), 1e-300)


def latest_stamp(src, dst, t, h, qs, qd):
    """Stamp of each query pair's latest occurrence among the first h edges (NaN: none)."""
    last = {}
    for p in range(h):
        last[(int(src[p]), int(dst[p]))] = t[p]
    return np.array([last.get((int(a), int(b)), np.nan) for a, b in zip(qs, qd)])


# ------------------------------------------------------------------------------------------------------------------- CPU

def test_fixture_holds_the_cases():
    g = g15()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g15_edge_bank.npz")) < 200_000
    assert [(str(m), str(w), float(p)) for m, w, p in zip(g["config_memory"], g["config_window"], g["config_proportion"])] == CONFIGS
    E = len(g["src"])
    assert E == 400 and (np.diff(g["t"]) >= 0).all() and 80 <= len(set(zip(g["src"], g["dst"]))) <= 90      # a pool of 90 pairs
    for c in range(4):
        hs = g[f"h_{c}"]
        assert list(hs[:39]) == list(range(1, 40)) and hs[-1] == E and len(hs) >= 0.95 * 91
        assert g[f"pred_{c}"].shape == (len(hs), 60) and set(np.unique(g[f"pred_{c}"])) == {0.0, 1.0}
        for part in (g[f"loop_pos_{c}"], g[f"loop_neg_{c}"]):
            assert part.shape == (6, 25) and set(np.unique(part)) == {0.0, 1.0}


@pytest.mark.parametrize("c", range(4))
def test_host_rule_against_g15(c):
    """Every recorded (configuration, h): the predictions equal the reference's; the bound is the reference's -- bit for bit where it
    is a quantile or a threshold, within 1e-12 relative where it holds the float64 sum."""
    g = g15()
    src, dst, t = g["src"], g["dst"], g["t"]
    worst = 0.0
    for k, h in enumerate(g[f"h_{c}"]):
        pred, bound = edge_bank_host(src, dst, t, int(h), g[f"query_src_{c}"][k], g[f"query_dst_{c}"][k], *CONFIGS[c])
        np.testing.assert_array_equal(pred, g[f"pred_{c}"][k], err_msg=f"h = {h}")
        want = g[f"bound_{c}"][k]
        if c == 0:
            assert bound == float("-inf") and np.isnan(want)
        elif c == REPEAT_INTERVAL:
            worst = max(worst, rel(bound, want))
            assert rel(bound, want) <= WINDOW_RTOL, (h, bound, want)
        else:
            assert bound == want, (h, bound, want)
        if c == 3:
            assert bound == float(h) / float(len(set(zip(src[:h], dst[:h]))))
    print(CONFIGS[c], "worst relative difference of the bound", worst)


@pytest.mark.parametrize("p", [0.03, 0.15, 0.5, 1.0, 0.0])
def test_host_quantile_is_numpys_bit_for_bit(p):
    g = g15()
    src, dst, t = g["src"], g["dst"], g["t"]
    none = np.zeros(0, dtype=np.int64)
    for h in range(1, len(t) + 1):
        _, bound = edge_bank_host(src, dst, t, h, none, none, "time_window_memory", "fixed_proportion", p)
        assert bound == float(np.quantile(t[:h], 1 - p)), (h, p)
    u = np.sort(np.random.RandomState(3).uniform(0.0, 1.0e9, 500))             # stamps that are no integers: both _lerp branches round
    for h in range(1, 501):
        _, bound = edge_bank_host(np.ones(500, dtype=np.int64), np.ones(500, dtype=np.int64), u, h, none, none, "time_window_memory",
                                  "fixed_proportion", p)
        assert bound == float(np.quantile(u[:h], 1 - p)), (h, p)


def test_host_rule_on_ids_outside_the_table():
    g = g15()
    qs = np.array([-1, 1, 2 ** 31, 3, 2 ** 40, int(g["src"][0])], dtype=np.int64)
    qd = np.array([16, -16, 20, 2 ** 31, 1, int(g["dst"][0])], dtype=np.int64)
    pred, _ = edge_bank_host(g["src"], g["dst"], g["t"], 400, qs, qd)
    assert list(pred) == [0, 0, 0, 0, 0, 1]


def test_size_helpers_and_refusals_without_a_gpu(hip_lib):
    """Argument errors come back before anything touches a device -- so this holds on a machine without one."""
    assert hip_lib.tpnet_edgebank_bytes(0) == 0 and hip_lib.tpnet_edgebank_bytes(-5) == 0 and hip_lib.tpnet_edgebank_bytes(1 << 30) == 0
    assert hip_lib.tpnet_edgebank_bytes(400) >= 400 * (8 + 4 + 4 + 8 + 4)
    assert hip_lib.tpnet_edgebank_scratch_bytes(0) == 0 and hip_lib.tpnet_edgebank_scratch_bytes(1 << 30) == 0
    need = hip_lib.tpnet_edgebank_scratch_bytes(400)
    assert need >= 8
    counts = (C.c_int64 * 1)()
    assert hip_lib.tpnet_edgebank_build(None, 1 << 30, 8, 8, 8, 10, counts, None) == -1
    assert hip_lib.tpnet_edgebank_build(8, 1 << 30, 8, 8, None, 10, counts, None) == -1
    assert hip_lib.tpnet_edgebank_build(8, 1 << 30, 8, 8, 8, 0, counts, None) == -1
    assert hip_lib.tpnet_edgebank_build(8, 1 << 30, 8, 8, 8, 10, None, None) == -1
    assert hip_lib.tpnet_edgebank_build(8, 64, 8, 8, 8, 10, counts, None) == -2
    ok = dict(eb=8, E=10, mem=1, win=1, prop=0.15, h=5, s0=8, d0=8, Q0=4, o0=8, s1=8, d1=8, Q1=4, o1=8, scratch=8, nbytes=need, win_out=None)

    def call(**over):
        a = dict(ok, **over)
        return hip_lib.tpnet_edgebank_predict(a["eb"], a["E"], a["mem"], a["win"], a["prop"], a["h"], a["s0"], a["d0"], a["Q0"], a["o0"],
                                              a["s1"], a["d1"], a["Q1"], a["o1"], a["scratch"], a["nbytes"], a["win_out"], None)
    for over in (dict(eb=None), dict(E=0), dict(E=1 << 30), dict(h=0), dict(h=11), dict(prop=-0.01), dict(prop=1.5), dict(prop=float("nan")),
                 dict(mem=3), dict(mem=-1), dict(win=2), dict(win=-1), dict(Q0=-1), dict(Q1=-1), dict(o0=None), dict(o1=None),
                 dict(s0=None), dict(d1=None), dict(scratch=None)):
        assert call(**over) == -1, over
    assert call(nbytes=need - 1) == -2
    assert call(Q0=0, Q1=0) == 0                                                   # nothing to do, nothing launched
    assert call(Q0=0, Q1=0, s0=None, d0=None, o0=None, s1=None, d1=None, o1=None) == 0


def test_modes_and_devices_are_checked():
    one = np.ones(3, dtype=np.int64)
    with pytest.raises(ValueError, match="Not implemented error for edge_bank_memory_mode nope!"):
        GpuEdgeBank(one, one, np.zeros(3), edge_bank_memory_mode="nope")
    with pytest.raises(ValueError, match="Not implemented error for time_window_mode nope!"):
        GpuEdgeBank(one, one, np.zeros(3), edge_bank_memory_mode="time_window_memory", time_window_mode="nope")
    with pytest.raises(ValueError, match="Not implemented error for edge_bank_memory_mode nope!"):
        edge_bank_host(one, one, np.zeros(3), 1, one, one, "nope")
    with pytest.raises(_lib.TPNetHipError):
        GpuEdgeBank(one, one, np.zeros(3), device="cpu")


# ------------------------------------------------------------------------------------------------------------------- GPU

def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")


def _ids(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to("cuda:0")


def _bank(src, dst, t, c):
    return GpuEdgeBank(src, dst, t, *CONFIGS[c], device="cuda:0")


def _check_bound(c, got, want, t_end, what):
    """The device's double[2] against a bound of the host rule or of the fixture."""
    if c == 0:
        assert got[0] == float("-inf") and got[1] == t_end, what
    elif c == REPEAT_INTERVAL:
        assert rel(got[0], want) <= WINDOW_RTOL and got[1] == t_end, (what, got, want)
    elif c == 1:
        assert got[0] == want and got[1] == t_end, (what, got, want)                # bit for bit
    else:
        assert got[0] == want, (what, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("c", range(4))
def test_device_against_g15(c):
    """Every recorded (configuration, h) of the toy stream: the device's predictions equal the reference's, its written-out window
    start equals the reference's (bit for bit for 'fixed_proportion', 1e-12 relative for 'repeat_interval')."""
    _need_gpu()
    g = g15()
    bank = _bank(g["src"], g["dst"], g["t"], c)
    assert bank.num_unique_edges == len(set(zip(g["src"], g["dst"])))
    hs = g[f"h_{c}"]
    qs, qd = _ids(g[f"query_src_{c}"]), _ids(g[f"query_dst_{c}"])
    preds, wins = [], []
    for k, h in enumerate(hs):
        p, n = bank.predict_device(int(h), qs[k, :20], qd[k, :20], qs[k, 20:], qd[k, 20:])       # the stream's pairs, the uniform ones
        preds.append(torch.cat([p, n]))
        wins.append(bank.window_device().clone())
    preds, wins = torch.stack(preds).cpu().numpy(), torch.stack(wins).cpu().numpy()
    assert preds.dtype == np.float32
    np.testing.assert_array_equal(preds, g[f"pred_{c}"])
    worst = 0.0
    for k, h in enumerate(hs):
        _check_bound(c, wins[k], g[f"bound_{c}"][k], g["t"][h - 1], f"h = {h}")
        if c == 3:
            assert wins[k][1] == len(set(zip(g["src"][:h], g["dst"][:h])))
        if c == REPEAT_INTERVAL:
            worst = max(worst, rel(wins[k][0], g[f"bound_{c}"][k]))
    print(CONFIGS[c], "worst relative difference of the window start", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("c", range(4))
def test_device_on_special_prefixes_and_lists(c):
    """h = 1 and h = E, a list of one pair, an empty second list, two empty lists (nothing launched)."""
    _need_gpu()
    g = g15()
    src, dst, t = g["src"], g["dst"], g["t"]
    E = len(src)
    bank = _bank(src, dst, t, c)
    qs, qd = g[f"query_src_{c}"][-1], g[f"query_dst_{c}"][-1]
    for h in (1, E):
        want, bound = edge_bank_host(src, dst, t, h, qs, qd, *CONFIGS[c])
        got = bank.predict_device(h, _ids(qs), _ids(qd))                             # no second list: ONE tensor comes back
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        _check_bound(c, bank.window_device().cpu().numpy(), bound, t[h - 1], f"h = {h}")
        one = bank.predict_device(h, _ids(src[:1]), _ids(dst[:1]))                   # one pair: edge 0, history from h = 1 on
        assert one.shape == (1,) and float(one) == edge_bank_host(src, dst, t, h, src[:1], dst[:1], *CONFIGS[c])[0][0]
        p, n = bank.predict_device(h, _ids(qs[:0]), _ids(qd[:0]), _ids(qs), _ids(qd))  # an empty FIRST list
        assert p.numel() == 0
        np.testing.assert_array_equal(n.cpu().numpy(), want)
    bank.window_device().fill_(-7.0)
    p, n = bank.predict_device(5, _ids(qs[:0]), _ids(qd[:0]), _ids(qs[:0]), _ids(qd[:0]))
    assert p.numel() == 0 and n.numel() == 0
    torch.cuda.synchronize()
    assert (bank.window_device().cpu().numpy() == -7.0).all()                        # nothing was launched
    r = edge_bank_link_prediction(type("D", (), dict(src_node_ids=src, dst_node_ids=dst, node_interact_times=t)), (qs[:20], qd[:20]),
                                  (qs[20:], qd[20:]), *CONFIGS[c])
    want = edge_bank_host(src, dst, t, E, qs, qd, *CONFIGS[c])[0]
    assert r[0].dtype == r[1].dtype == np.float64
    np.testing.assert_array_equal(np.concatenate(r), want)


@pytest.mark.gpu
def test_device_refusals_launch_nothing():
    _need_gpu()
    g = g15()
    lib = _lib.load()
    bank = _bank(g["src"], g["dst"], g["t"], REPEAT_INTERVAL)
    E = bank.E
    qs, qd = _ids(g["query_src_2"][0]), _ids(g["query_dst_2"][0])
    out0 = torch.full((60,), -1.0, dtype=torch.float32, device="cuda:0")
    out1 = torch.full((60,), -1.0, dtype=torch.float32, device="cuda:0")
    window = torch.full((2,), -7.0, dtype=torch.float64, device="cuda:0")
    scratch = torch.zeros(lib.tpnet_edgebank_scratch_bytes(E), dtype=torch.uint8, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = dict(eb=bank._buf.data_ptr(), E=E, mem=1, win=1, prop=0.15, h=200, s0=qs.data_ptr(), d0=qd.data_ptr(), Q0=60, o0=out0.data_ptr(),
              s1=qs.data_ptr(), d1=qd.data_ptr(), Q1=60, o1=out1.data_ptr(), scratch=scratch.data_ptr(), nbytes=scratch.numel())

    def call(**over):
        a = dict(ok, **over)
        return lib.tpnet_edgebank_predict(a["eb"], a["E"], a["mem"], a["win"], a["prop"], a["h"], a["s0"], a["d0"], a["Q0"], a["o0"],
                                          a["s1"], a["d1"], a["Q1"], a["o1"], a["scratch"], a["nbytes"], window.data_ptr(), stream)
    for over in (dict(eb=None), dict(E=0), dict(h=0), dict(h=E + 1), dict(prop=-0.01), dict(prop=1.01), dict(mem=3), dict(win=2),
                 dict(Q0=-1), dict(Q1=-1), dict(o0=None), dict(o1=None), dict(scratch=None)):
        assert call(**over) == -1, over
    assert call(nbytes=scratch.numel() - 1) == -2
    assert call(Q0=0, Q1=0) == 0
    torch.cuda.synchronize()
    assert (out0.cpu() == -1).all() and (out1.cpu() == -1).all() and (window.cpu() == -7).all()   # nothing was launched
    assert call() == 0                                                               # ... and the same arguments, whole, run
    want = edge_bank_host(g["src"], g["dst"], g["t"], 200, g["query_src_2"][0], g["query_dst_2"][0], *CONFIGS[REPEAT_INTERVAL])[0]
    np.testing.assert_array_equal(out0.cpu().numpy(), want)
    np.testing.assert_array_equal(out1.cpu().numpy(), want)
    with pytest.raises(ValueError):
        bank.predict_device(0, qs, qd)
    with pytest.raises(ValueError):
        bank.predict_device(E + 1, qs, qd)
    with pytest.raises(TypeError):
        bank.predict_device(5, qs.int(), qd)
    with pytest.raises(TypeError):
        bank.predict_device(5, qs.cpu(), qd)


@pytest.mark.gpu
def test_build_refuses_a_decreasing_stamp_and_a_bad_id():
    _need_gpu()
    g = g15()
    t = g["t"].copy()
    t[200] = t[199] - 1.0
    with pytest.raises(_lib.TPNetHipError, match="edgebank_build"):
        _bank(g["src"], g["dst"], t, 0)
    t = g["t"].copy()
    t[7] = np.nan
    with pytest.raises(_lib.TPNetHipError, match="edgebank_build"):
        _bank(g["src"], g["dst"], t, 0)
    src = g["src"].copy()
    src[399] = 2 ** 31
    with pytest.raises(IndexError):
        _bank(src, g["dst"], g["t"], 0)
    dst = g["dst"].copy()
    dst[0] = -1
    with pytest.raises(IndexError):
        _bank(g["src"], dst, g["t"], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("c", range(4))
def test_device_on_shapes_that_span_workgroups(c):
    """E = 6000, U > 1024; Q in {1, 63, 64, 65, 257, 1025} split over the two lists; h in {1, 255, 256, 257, 3000, 6000}: the
    device equals the host rule.  'repeat_interval': the window start within 1e-12, and a prediction is compared only where its
    deciding stamp is further than 1e-6 from the host's window start (or the prefix has no repeat: S = 0 in any order)."""
    _need_gpu()
    src, dst, t, qs, qd, host = big_stream()
    bank = _bank(src, dst, t, c)
    assert bank.num_unique_edges == len(set(zip(src, dst))) > 1024
    qs_d, qd_d = _ids(qs), _ids(qd)
    got, wins = {}, {}
    for h in BIG_H:
        for Q in BIG_Q:
            Q1 = Q // 3
            p, n = bank.predict_device(h, qs_d[:Q - Q1], qd_d[:Q - Q1], qs_d[Q - Q1:Q], qd_d[Q - Q1:Q])
            got[h, Q] = torch.cat([p, n])
            wins[h, Q] = bank.window_device().clone()
    total = skipped = 0
    for h in BIG_H:
        want, bound = host[c, h]
        keep = np.ones(1025, dtype=bool)
        if c == REPEAT_INTERVAL and bound != t[h - 1]:
            keep = ~(np.abs(latest_stamp(src, dst, t, h, qs, qd) - bound) <= 1e-6)
        for Q in BIG_Q:
            _check_bound(c, wins[h, Q].cpu().numpy(), bound, t[h - 1], f"h = {h}, Q = {Q}")
            np.testing.assert_array_equal(got[h, Q].cpu().numpy()[keep[:Q]], want[:Q][keep[:Q]], err_msg=f"h = {h}, Q = {Q}")
            total, skipped = total + Q, skipped + int((~keep[:Q]).sum())
        assert 0.0 < want.mean() < 1.0 or h < 3000                                   # both outcomes, once the history is long enough
    print(CONFIGS[c], "queries left out:", skipped, "of", total)
    assert skipped < 0.01 * total


@pytest.mark.gpu
def test_same_call_twice_gives_the_same_bits():
    _need_gpu()
    src, dst, t, qs, qd, _ = big_stream()
    qs_d, qd_d = _ids(qs), _ids(qd)
    for c in range(4):
        bank = _bank(src, dst, t, c)
        runs = []
        for _ in range(2):
            bank._scratch.fill_(255)
            p, n = bank.predict_device(3000, qs_d[:700], qd_d[:700], qs_d[700:], qd_d[700:])
            runs.append((p.cpu().numpy().tobytes(), n.cpu().numpy().tobytes(), bank.window_device().cpu().numpy().tobytes()))
        assert runs[0] == runs[1]
        other = _bank(src, dst, t, c)                                                # ... and so does a second table of the same stream
        p, n = other.predict_device(3000, qs_d[:700], qd_d[:700], qs_d[700:], qd_d[700:])
        assert (p.cpu().numpy().tobytes(), n.cpu().numpy().tobytes(), other.window_device().cpu().numpy().tobytes()) == runs[0]


@pytest.mark.gpu
def test_predict_and_add_probabilities_do_not_synchronise():
    _need_gpu()
    g = g15()
    banks = [_bank(g["src"], g["dst"], g["t"], c) for c in range(4)]
    qs, qd = _ids(g["query_src_0"][50]), _ids(g["query_dst_0"][50])
    meter = LinkPredictionMeter(4, "cuda:0")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")              # a synchronising torch call inside would raise
    try:
        for c, bank in enumerate(banks):
            p, n = bank.predict_device(300, qs[:20], qd[:20], qs[20:], qd[20:])
            assert meter.add_probabilities(p, n.reshape(-1, 1)) == c
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    losses, metrics = meter.results()
    for c in range(4):
        want = edge_bank_host(g["src"], g["dst"], g["t"], 300, g["query_src_0"][50], g["query_dst_0"][50], *CONFIGS[c])[0]
        h = link_prediction_metrics_host(want[:20], want[20:])
        assert metrics[c]["roc_auc"] == h["auc"] and abs(metrics[c]["average_precision"] - h["ap"]) <= AP_TOL
        assert losses[c] == 100.0 * ((want[:20] == 0).sum() + (want[20:] == 1).sum()) / 60


class ReplaySampler:
    """The fixture's stored negatives, batch after batch, behind the reference sampler's interface."""
    negative_sample_strategy = "historical"

    def __init__(self, neg_src, neg_dst):
        self.neg_src, self.neg_dst, self.at = neg_src, neg_dst, 0

    def sample(self, size, batch_src_node_ids, batch_dst_node_ids, current_batch_start_time, current_batch_end_time):
        assert len(batch_src_node_ids) == len(batch_dst_node_ids) == size and current_batch_start_time <= current_batch_end_time
        s = slice(self.at, self.at + size)
        self.at += size
        return self.neg_src[s], self.neg_dst[s]


@pytest.mark.gpu
@pytest.mark.parametrize("c", range(4))
def test_evaluation_loop_against_g15(c):
    """`evaluate_edge_bank_link_prediction` on the fixture's loop (history 250, test 150, batches of 25, stored negatives): the
    reference's per-batch BCELoss, average precision and ROC-AUC."""
    _need_gpu()
    from tpnet_amd.callers import evaluate_edge_bank_link_prediction
    g = g15()
    nh, B = int(g["n_history"]), int(g["batch"])
    bank = _bank(g["src"], g["dst"], g["t"], c)
    losses, metrics = res = evaluate_edge_bank_link_prediction(bank, ReplaySampler(g["neg_src"], g["neg_dst"]), nh, g["src"][nh:],
                                                               g["dst"][nh:], g["t"][nh:], B)
    assert len(losses) == len(metrics) == 6 and res.flags == [0] * 6
    for b in range(6):
        print(CONFIGS[c], "batch", b, "dloss", abs(losses[b] - g[f"loop_loss_{c}"][b]), "dAP",
              abs(metrics[b]["average_precision"] - g[f"loop_ap_{c}"][b]), "dAUC", abs(metrics[b]["roc_auc"] - g[f"loop_auc_{c}"][b]))
        assert abs(losses[b] - g[f"loop_loss_{c}"][b]) <= loss_tol(g[f"loop_loss_{c}"][b])
        assert abs(metrics[b]["average_precision"] - g[f"loop_ap_{c}"][b]) <= AP_TOL
        assert abs(metrics[b]["roc_auc"] - g[f"loop_auc_{c}"][b]) <= AP_TOL


class _DeferredMeter(LinkPredictionMeter):
    """results() is the loop's one synchronisation: taken outside the guarded region."""

    def results(self):
        return None


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", ["historical", "random"])
def test_evaluation_loop_with_the_device_sampler_stays_on_the_device(strategy):
    _need_gpu()
    from tpnet_amd import GpuNegativeEdgeSampler
    from tpnet_amd.callers import evaluate_edge_bank_link_prediction
    g = g15()
    src, dst, t = g["src"], g["dst"], g["t"]
    nh, B = 250, 25
    bank = _bank(src, dst, t, REPEAT_INTERVAL)
    sampler = GpuNegativeEdgeSampler(src, dst, t, negative_sample_strategy=strategy, seed=0, device="cuda:0")
    meter = _DeferredMeter(6, "cuda:0")
    ts, td = _ids(src[nh:]), _ids(dst[nh:])
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        assert evaluate_edge_bank_link_prediction(bank, sampler, nh, ts, td, t[nh:], B, meter=meter) is None
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    losses, metrics = LinkPredictionMeter.results(meter)
    sampler.reset_random_state()                                                     # the same negatives again, scored on the host
    for b in range(6):
        s = slice(b * B, b * B + B)
        if strategy == "random":
            ns, nd = ts[s], sampler.sample_device(B)[1]
        else:
            ns, nd = sampler.sample_device(B, ts[s], td[s], float(t[nh:][s][0]), float(t[nh:][s][-1]))
        p, n = bank.predict_device(nh + b * B, ts[s], td[s], ns, nd)
        p, n = p.cpu().numpy(), n.cpu().numpy()
        want_p = edge_bank_host(src, dst, t, nh + b * B, src[nh:][s], dst[nh:][s], *CONFIGS[REPEAT_INTERVAL])[0]
        np.testing.assert_array_equal(p, want_p)
        h = link_prediction_metrics_host(p, n)
        assert metrics[b]["roc_auc"] == h["auc"] and abs(metrics[b]["average_precision"] - h["ap"]) <= AP_TOL
        assert losses[b] == 100.0 * ((p == 0).sum() + (n == 1).sum()) / (2 * B)


@pytest.mark.gpu
def test_add_probabilities_against_bceloss():
    """Probabilities other than 0 / 1, and exact 0 among the positives and exact 1 among the negatives (the -100 clamp), against
    torch.nn.BCELoss on float64 CPU copies; they are ranked as they are."""
    _need_gpu()
    rng = np.random.RandomState(5)
    meter = LinkPredictionMeter(3, "cuda:0")
    cases = []
    for P, N in ((300, 257), (1, 1), (64, 1000)):
        p, q = rng.uniform(0, 1, P).astype(np.float32), rng.uniform(0, 1, N).astype(np.float32)
        p[0], q[0] = 0.0, 1.0                                                       # each on the wrong side
        if P > 2:
            p[1], p[2], q[1], q[2] = 1.0, np.float32(1e-30), 0.0, np.float32(1.0 - 2.0 ** -24)
        cases.append((p, q))
        meter.add_probabilities(torch.from_numpy(p).to("cuda:0"), torch.from_numpy(q).to("cuda:0"))
    losses, metrics = meter.results()
    for k, (p, q) in enumerate(cases):
        x = torch.from_numpy(np.concatenate([p, q]).astype(np.float64))
        y = torch.cat([torch.ones(len(p), dtype=torch.float64), torch.zeros(len(q), dtype=torch.float64)])
        want = float(torch.nn.BCELoss()(x, y))
        h = link_prediction_metrics_host(p, q)
        print("case", k, "loss", losses[k], "dloss", abs(losses[k] - want), "dAP", abs(metrics[k]["average_precision"] - h["ap"]))
        assert want > 100.0 / (len(p) + len(q))                                      # the clamp was hit
        assert abs(losses[k] - want) <= loss_tol(want)
        assert metrics[k]["roc_auc"] == h["auc"] and abs(metrics[k]["average_precision"] - h["ap"]) <= AP_TOL
    with pytest.raises(IndexError):
        meter.add_probabilities(torch.zeros(1, device="cuda:0"), torch.zeros(1, device="cuda:0"))
    with pytest.raises(TypeError):
        LinkPredictionMeter(1, "cuda:0").add_probabilities(torch.zeros(1, device="cuda:0").double(), torch.zeros(1, device="cuda:0"))
