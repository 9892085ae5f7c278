"""The host-array calls (update, pair_gram, get_pair_wise_feature, encoder_pair_features: what the reference's training loop
passes, models/TPNet.py:67-129, 280-324) at every route and on both sides of every size threshold, against the float64-class
numpy oracle -- and every case says WHICH route served it.

The routes are found out without touching the product: the instance's own bound methods (_host_readout, _pair_feature_launch,
_encoder_pattern_features, _anchored_launch, pair_gram_anchored, get_pair_wise_feature_shared, pair_gram, _to_device, _workspace)
and fused_mlp.fused_readout_mlp are wrapped by recorders (monkeypatch), and the sequence of recorded calls is read as a
(route, sub-route) pair.  Thresholds are read from the live objects (rp._eng["stage"].max_pairs / .max_batch / .max_host_batch,
fused_feature.MAX_PAIRS, random_projection._BIG_SLOT_BYTES); only 8192 and 16384 are literals here, as they are in the product.

The table that test_every_route_of_the_table_was_reached holds the file to -- route numbers as in get_pair_wise_feature:

  pair_gram              staged                     host ids through the staging ring, one readout launch (n <= max_pairs)
  pair_gram              upload                     one pinned copy of the ids, tpnet_pair_gram
  1                      bf16 one launch            fused_mlp: readout + bf16 layers (tpnet_pair_feature_bf16)
  2                      device ids                 src a device tensor: tpnet_pair_gram, then self.mlp
  3                      staged, one launch         tpnet_host_pair_feature with self.mlp
  4                      device ids, one launch     wide rows, not tiled: tpnet_pair_feature
  5                      one crossing               tpnet_host_anchored_features served the call
  5                      device ids                 the crossing declined; tpnet_anchored_features in one launch, no feature buffer
  5                      device ids, scratch        the same as two launches with a feature buffer between them
  6                      anchored, 5 declined       pair_gram_anchored, then self.mlp
  7                      shared                     tiled src on wide rows below 8192 pairs: route 5 is not asked
  7                      shared, 5 declined         pair_gram_shared, then self.mlp
  8                      staged                     pair_gram from the ring, then self.mlp
  8                      staged, 5 declined
  8                      upload
  8                      upload, 5 declined
  8                      upload, bf16 layers        fused_mlp on a list too long for route 1
  update                 slot                       planned straight from the staging slot (B <= max_batch)
  update                 staged copy                staged, copied to the workspace tail, chunk planner (B <= max_host_batch)
  update                 upload                     one pinned copy, tpnet_update
  encoder_pair_features  staged                     tpnet_host_encoder_features
  encoder_pair_features  upload                     B > max_host_batch: one pinned copy, tpnet_encoder_features

Where a case does not sit at the size its threshold's name suggests, and why (what the routing does, found while writing the cases):
  * L = 3 on rows of whole 16-byte vectors from 36 floats (d = 64, 132, 256 here): route 3 serves EVERY list up to max_pairs, the
    encoder's pattern included, so routes 4 to 7 begin above max_pairs (16 384), not above 8192 -- the pattern cases of d = 64 /
    132 / 256 at L = 3, and the gradient cases of routes 4 and 5, sit just above max_pairs.  At L = 2, d = 16 and d = 130 the
    threshold is fused_feature.MAX_PAIRS and the pattern cases sit just above 8192.
  * max_pairs + 2 = 16 386 pairs are two halves of 8193 = 3 x 2731 neighbours: the pattern case there has 3 rows of K = 2731.
  * The big slot: K = 4 needs n % 8 == 0, and 48 (n / 8) = 1 MiB has no solution: the two sizes are the largest n whose ids fit the
    slot (174 760 pairs: 1 048 560 bytes) and the next pattern length (174 768: 1 048 608 bytes).
  * d = 256, L = 3 without gradients: tpnet_encoder_fused_supported is 0 (the wide one-launch kernel is not routed), so the
    crossing declines and the device-id sub-route runs with a scratch buffer -- what the case asserts from the library's own
    answer.  With gradients the crossing serves d = 256 too (the autograd node brings the feature buffer).

Tolerances: the project's own.  Pre-mlp features: _assert_features (1e-4 relative + the Gram bound); raw / not_scale entries: the
same three terms without the log's derivative.  State: _assert_state at 1e-4 (5e-6 in exact mode); clock: equal as float64.
Post-mlp outputs: the reference is self.mlp in float64 on the CPU applied to the oracle's features; the bound per output is the
Lipschitz propagation of the feature tolerance through the layers, |W2| (|W1| tol_x), plus C_DENSE * max(1, |want|.max()).
C_DENSE = 2e-5 is what the suite grants between two fp32-class implementations of the layers.  Whether it also covers fp32
against float64 is measured by test_fp32_layers_against_float64_on_the_feature_cases below (torch's float32 layers on the CPU on
the oracle's features of every get_pair_wise_feature case of this file, against the float64 layers on the same inputs): the worst
ratio |y32 - y64| / max(1, |y64|.max()) over all cases is 5.7e-7, a thirty-fifth of 2e-5 and far below half of it, so C_DENSE stays
2e-5.  The bf16 layers (fused_mlp) are held to the 2e-2 of tests/test_fused_mlp.py in its place."""
import copy
import gc
import inspect
import zlib

import numpy as np
import pytest
import torch

from oracle import tpnet_oracle as O
from test_fused_feature import _assert_mlp_grads_close
from test_gpu_parity import DEV, _assert_features, _assert_state, _gram_bound, _layers, _module, _need_gpu, _random_stream

LAM, T0 = 2e-6, 1.0e6
C_DENSE = 2e-5          # see the docstring: measured fp32-against-float64 ratio 5.7e-7
C_BF16 = 2e-2           # tests/test_fused_mlp.py
CHUNK = 4096            # pairs per evaluation of the oracle

TABLE = {
    ("pair_gram", "staged"), ("pair_gram", "upload"),
    ("1", "bf16 one launch"), ("2", "device ids"), ("3", "staged, one launch"), ("4", "device ids, one launch"),
    ("5", "one crossing"), ("5", "device ids"), ("5", "device ids, scratch"),
    ("6", "anchored, 5 declined"), ("7", "shared"), ("7", "shared, 5 declined"),
    ("8", "staged"), ("8", "staged, 5 declined"), ("8", "upload"), ("8", "upload, 5 declined"), ("8", "upload, bf16 layers"),
    ("update", "slot"), ("update", "staged copy"), ("update", "upload"),
    ("encoder_pair_features", "staged"), ("encoder_pair_features", "upload"),
}
_REACHED = {}           # (route, sub-route) -> the first case that reached it
_RAN = set()            # ids of the cases that ran in this process


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """The tables of this file are built once and kept (_GPU): dropped when the file is done, with what the collector still holds,
    so that the tests behind it meet the caching allocator without this file's blocks coming free under them."""
    yield
    _GPU.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


# ---------------------------------------------------------------------------------------------------------
# thresholds, tables, oracle
# ---------------------------------------------------------------------------------------------------------
def _thresholds(rp=None):
    """The size thresholds of the routes.  With a module: from the live objects.  Without (the CPU tier builds the same index lists):
    from the product's own defaults -- the staging ring's slot size is _Stage's default argument."""
    from tpnet_amd import fused_feature as ff
    from tpnet_amd import random_projection as R
    th = dict(MAX_PAIRS=ff.MAX_PAIRS, BIG=R._BIG_SLOT_BYTES)
    if rp is not None:
        rp._ensure_engine()
        s = rp._eng["stage"]
        th.update(max_pairs=s.max_pairs, max_batch=s.max_batch, max_host_batch=s.max_host_batch)
    else:
        slot = inspect.signature(R._Stage.__init__).parameters["slot_bytes"].default
        th.update(max_pairs=slot // 16, max_host_batch=slot // 24)
    return th


def _setup_stream(N, seed):
    """Three host updates of 100, 150 and 200 edges with hubs and self pairs (test_gpu_parity._random_stream)."""
    src, dst, _, t = _random_stream(np.random.RandomState(seed), N, 450, 3.0e5)
    return [(src[a:b], dst[a:b], t[a:b]) for a, b in ((0, 100), (100, 250), (250, 450))]


_CPU = {}


def _cpu_side(d, L, N=300, not_scale=False, use_matrix=False, extra_layer=False, fused=False):
    """What a table of the feature cases is on the CPU: P[0], the oracle's state after the three set-up updates, self.mlp (float32,
    seeded) and its float64 layers."""
    key = (d, L, N, not_scale, use_matrix, extra_layer, fused)
    if key not in _CPU:
        rng = np.random.RandomState(_seed("P0", key))
        P0 = np.eye(N, dtype=np.float32) if use_matrix else (rng.randn(N, d) / np.sqrt(d)).astype(np.float32)
        st = O.OracleState(P0, L, LAM, T0)
        for src, dst, t in _setup_stream(N, _seed("setup", key)):
            O.update(st, src, dst, t)
        F = (2 * L + 2) ** 2
        gen = torch.Generator().manual_seed(_seed("mlp", key))
        mods = [torch.nn.Linear(F, 4 * F), torch.nn.ReLU(), torch.nn.Linear(4 * F, F)]
        if extra_layer:
            mods += [torch.nn.ReLU(), torch.nn.Linear(F, F)]
        mlp = torch.nn.Sequential(*mods)
        with torch.no_grad():
            for m in mlp:                         # (nn.Linear's own law, uniform in +-1 / sqrt(fan_in), from a generator of the table's own)
                for p in m.parameters():
                    p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) / np.sqrt(m.in_features))
        _CPU[key] = (key, P0, st, mlp, _layers64(mlp))
    return _CPU[key]


_GPU = {}


def _table(**cfg):
    """The module of a table (built once per process: the readouts do not change it), the oracle's state, the float64 layers and
    the live thresholds."""
    key, P0, st, mlp, layers = _cpu_side(**cfg)
    if key not in _GPU:
        d, L, N, not_scale, use_matrix, _, fused = key
        rp = _module(N, d, L, LAM, T0, P0=None if use_matrix else P0, not_scale=not_scale, use_matrix=use_matrix)
        rp.mlp = copy.deepcopy(mlp).to(DEV)
        rp.fused_mlp = bool(fused)
        for src, dst, t in _setup_stream(N, _seed("setup", key)):
            rp.update(src, dst, t)
        assert float(rp.now_time.item()) == float(st.now_time)
        _GPU[key] = rp
    rp = _GPU[key]
    return rp, st, layers, _thresholds(rp)


def _wrapped(ids, N):
    """Python-style negative ids as ATen indexing reads them."""
    ids = np.asarray(ids, dtype=np.int64)
    return np.where(ids < 0, ids + N, ids)


def _oracle_features(st, u, v, not_scale=False):
    """The oracle's pre-mlp features of the pairs and the tolerance the project grants each of them (_assert_features' terms:
    1e-4 relative, 1e-5 absolute, and 1e-6 |R_a| |R_b| of the raw Gram entry carried through d/dx log(1 + x); raw entries: the
    same without the derivative), in chunks of CHUNK pairs."""
    want, tol = [], []
    for c in range(0, len(u), CHUNK):
        uc, vc = u[c:c + CHUNK], v[c:c + CHUNK]
        raw = O.pair_gram(st, uc, vc, not_scale=True)
        gb = _gram_bound(st.P, uc, vc, st.L, 1e-6)
        if not_scale:
            w = O.pair_gram(st, uc, vc, not_scale=True, accumulate=np.float64)
            want.append(w)
            tol.append(1e-4 * np.abs(w) + 1e-5 + gb)
        else:
            w = O.pair_gram(st, uc, vc)
            want.append(w)
            tol.append(1e-4 * np.abs(w) + 1e-5 + gb / (1.0 + np.maximum(raw, 0)))
    return np.concatenate(want).astype(np.float64), np.concatenate(tol)


def _check_features(got, st, u, v, not_scale=False, what=""):
    """Pre-mlp features against the oracle: _assert_features chunk by chunk (raw entries: the same terms, see _oracle_features)."""
    if not_scale:
        want, tol = _oracle_features(st, u, v, True)
        err = np.abs(got - want)
        assert (err <= tol).all(), f"{what}: {int((err > tol).sum())} raw entries off, worst {float((err / tol).max()):.3g} of the bound"
        return
    for c in range(0, len(u), CHUNK):
        _assert_features(got[c:c + CHUNK], st, u[c:c + CHUNK], v[c:c + CHUNK], f"{what} pairs {c}..")


def _layers64(mlp):
    out = []
    for m in mlp:
        if isinstance(m, torch.nn.Linear):
            out.append((m.weight.detach().double().cpu().numpy(), m.bias.detach().double().cpu().numpy()))
        else:
            assert isinstance(m, torch.nn.ReLU)
            out.append(None)
    return out


def _mlp64(layers, x, tol):
    """self.mlp in float64 on x, and the Lipschitz propagation of x's per-entry tolerance: |W| tol through a Linear, unchanged
    through a ReLU."""
    for lay in layers:
        if lay is None:
            x = np.maximum(x, 0)
        else:
            x = x @ lay[0].T + lay[1]
            tol = tol @ np.abs(lay[0]).T
    return x, tol


def _check_outputs(got, layers, st, u, v, not_scale, c, what):
    x, tol_x = _oracle_features(st, u, v, not_scale)
    want, tol = _mlp64(layers, x, tol_x)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    err = np.abs(got - want)
    print(f"{what}: worst |got - want| {float(err.max()):.3e} = {float(err.max()) / scale:.2e} of scale {scale:.3g}; "
          f"worst error / bound {float((err / (tol + c * scale)).max()):.3g}")
    bad = err > tol + c * scale
    assert not bad.any(), f"{what}: {int(bad.sum())} outputs off, worst {float(err.max()):.3e} (scale {scale:.3g})"


# ---------------------------------------------------------------------------------------------------------
# which route served a call
# ---------------------------------------------------------------------------------------------------------
class _Recorder:
    """Wraps the instance's own bound methods (and fused_mlp.fused_readout_mlp) with recorders: `events` = [(name, what)]."""
    NAMES = ("_host_readout", "_pair_feature_launch", "_encoder_pattern_features", "_anchored_launch", "pair_gram_anchored",
             "get_pair_wise_feature_shared", "pair_gram", "_to_device", "_workspace")

    def __init__(self, rp, monkeypatch):
        from tpnet_amd import fused_mlp as fm
        self.events = []
        self.rp = rp
        for name in self.NAMES:
            # (setattr on the instance, spelled as an item of its __dict__: monkeypatch then REMOVES the entry afterwards instead of
            # putting the bound method there, which would leave every module in a reference cycle -- its memory would go back to the
            # allocator whenever the collector next runs, in the middle of a later test)
            monkeypatch.setitem(rp.__dict__, name, self._wrap(name, getattr(rp, name)))
        inner = fm.fused_readout_mlp

        def readout_mlp(*a, **kw):
            self.events.append(("fused_readout_mlp", None))
            return inner(*a, **kw)
        monkeypatch.setattr(fm, "fused_readout_mlp", readout_mlp)

    def _wrap(self, name, inner):
        ev = self.events

        def wrapper(*a, **kw):
            if name == "_host_readout":
                ev.append((name, (a[5] if len(a) > 5 else kw.get("mlp_ref")) is not None))
            elif name == "_workspace":
                ev.append((name, int(kw.get("tail", a[3] if len(a) > 3 else 0))))
            elif name == "pair_gram":
                ev.append((name, "tensor" if isinstance(a[0] if a else kw["src_node_ids"], torch.Tensor) else "host"))
            elif name == "_to_device":
                ev.append((name, not all(isinstance(x, torch.Tensor) for x in a)))           # (True: a copy is enqueued)
            elif name not in ("_encoder_pattern_features", "_anchored_launch"):
                ev.append((name, None))
            res = inner(*a, **kw)
            if name == "_encoder_pattern_features":
                ev.append((name, res is not None))
            elif name == "_anchored_launch":
                ev.append((name, None))
                launch = res

                def recorded(gram):
                    ev.append(("_anchored_launch.launch", gram is not None))
                    return launch(gram)
                return recorded
            return res
        return wrapper

    def clear(self):
        del self.events[:]

    def _what(self, name):
        return [w for n, w in self.events if n == name]

    def feature_route(self):
        """The (route, sub-route) of the get_pair_wise_feature call recorded since clear()."""
        names = {n for n, _ in self.events}
        pattern = self._what("_encoder_pattern_features")
        tail = ", 5 declined" if pattern == [False] else ""
        staged = self._what("_host_readout")
        if "fused_readout_mlp" in names:
            return "1", "bf16 one launch"
        if staged == [True]:
            return "3", "staged, one launch"
        if "_pair_feature_launch" in names:
            return "4", "device ids, one launch"
        if pattern == [True]:
            if "_anchored_launch" not in names:
                return "5", "one crossing"
            return "5", "device ids, scratch" if self._what("_anchored_launch.launch")[-1] else "device ids"
        if "pair_gram_anchored" in names:
            return "6", "anchored" + tail
        if "get_pair_wise_feature_shared" in names:
            return "7", "shared" + tail
        assert self._what("pair_gram"), self.events
        if self._what("pair_gram")[0] == "tensor":
            return "2", "device ids"
        sub = "staged" if staged == [False] else "upload"
        assert sub == "staged" or True in self._what("_to_device"), self.events
        return "8", sub + tail + (", bf16 layers" if self.rp.fused_mlp else "")

    def gram_route(self):
        if self._what("_host_readout") == [False]:
            return "pair_gram", "staged"
        assert True in self._what("_to_device"), self.events
        return "pair_gram", "upload"

    def update_route(self):
        tails = self._what("_workspace")
        assert len(tails) == 1, self.events
        if True in self._what("_to_device"):
            assert tails[0] == 0, self.events
            return "update", "upload"
        return "update", ("staged copy" if tails[0] > 0 else "slot")

    def encoder_route(self):
        return "encoder_pair_features", ("upload" if True in self._what("_to_device") else "staged")


def _reached(route, case, expected):
    assert route == expected, f"{case}: served by route {route}, expected {expected}"
    _REACHED.setdefault(route, case)


# ---------------------------------------------------------------------------------------------------------
# index lists
# ---------------------------------------------------------------------------------------------------------
def _random_pairs(rng, N, n, negative=True):
    """Random pairs with the padding id 0, pairs u == v and (negative) one python-style negative id."""
    u, v = rng.randint(0, N, n).astype(np.int64), rng.randint(0, N, n).astype(np.int64)
    u[0] = 0
    if n > 8:
        v[1] = u[1]
        v[n // 2] = u[n // 2]
        v[5] = 0
        if negative:
            u[2] = -1
            v[7] = -N
    return u, v


def _other(x, N):
    return x % (N - 1) + 1 if x % (N - 1) + 1 != x else (x + 1) % (N - 1) + 1


def _pattern_pairs(rng, N, n, K, flaw=None):
    """The encoder's lists (models/TPNet.py:311-316): src = tile(neigh, 2), dst = concat(repeat(a1, K), repeat(a2, K)) for n / (2 K)
    rows whose consecutive anchors differ (so that K is the pattern's K), with padding ids among the neighbours and pairs u == v;
    `flaw`: the departures of tools/soak_encoder.py."""
    h = n // 2
    assert n % 2 == 0 and h % K == 0, (n, K)
    m = h // K
    neigh = rng.randint(0, N, (m, K)).astype(np.int64)
    neigh[rng.rand(m, K) < 0.1] = 0
    neigh[0, 0] = 0
    a1 = 1 + np.cumsum(rng.randint(1, N - 1, m)) % (N - 1)            # steps of 1 .. N-2 modulo N-1: neighbours in the list differ
    a2 = 1 + np.cumsum(rng.randint(1, N - 1, m)) % (N - 1)
    a1, a2 = a1.astype(np.int64), a2.astype(np.int64)
    neigh[m // 2, 0] = a1[m // 2]                                       # u == v
    neigh[m // 3, K - 1] = a2[m // 3]
    if flaw == "first two anchors equal":                               # the first run is 2 K
        a1[1] = a1[0]
    elif flaw == "first three anchors equal":
        assert m % 3 != 0
        a1[1] = a1[2] = a1[0]
    elif flaw == "second half one anchor":
        a2[:] = a2[0]
    u = np.tile(neigh.reshape(-1), 2)
    v = np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])
    if flaw == "broken tile":                                           # one neighbour of the second half changed
        u[h + 3] = (u[h + 3] + 1) % N
    elif flaw == "broken repeat":
        v[h + K + 1] = _other(int(v[h + K + 1]), N)
    elif flaw == "last element":
        v[-1] = _other(int(v[-1]), N)
    else:
        assert flaw is None or flaw.endswith("equal") or flaw == "second half one anchor", flaw
    return u, v


def _as_kind(u, v, kind):
    """The same pairs as another kind of argument."""
    if kind == "lists":
        return u.tolist(), v.tolist()
    if kind == "int32":
        return u.astype(np.int32), v.astype(np.int32)
    if kind == "strided":
        bu, bv = np.zeros(2 * len(u), dtype=np.int64), np.zeros(3 * len(v), dtype=np.int64)
        bu[::2], bv[::3] = u, v
        assert not bu[::2].flags.c_contiguous
        return bu[::2], bv[::3]
    if kind == "dst cpu tensor":
        return u, torch.from_numpy(v.copy())
    if kind == "src device tensor":
        return torch.from_numpy(u).to(DEV), torch.from_numpy(v).to(DEV)
    assert kind is None, kind
    return u, v


# ---------------------------------------------------------------------------------------------------------
# group 2 / 3: get_pair_wise_feature.  A case = (id, table, list, size, expected route); sizes are functions of the thresholds
# ---------------------------------------------------------------------------------------------------------
def _above(n, K):
    """The shortest pattern list of more than n pairs: the next multiple of 2 K."""
    return (n // (2 * K) + 1) * (2 * K)


def _big_slot_n(th):
    """The largest n (K = 4: n % 8 == 0) with (n // 2 + 2 * (n // 8)) * 8 <= _BIG_SLOT_BYTES."""
    n = th["BIG"] // 48 * 8
    assert (n // 2 + 2 * (n // 8)) * 8 <= th["BIG"] < ((n + 8) // 2 + 2 * ((n + 8) // 8)) * 8
    return n


def _case(cid, cfg, size, route, K=None, flaw=None, kind=None, negative=None, c=C_DENSE):
    if negative is None:       # a negative id where the route is documented to wrap it: not in the pattern (the crossing declines it), not on the device
        negative = K is None and kind != "src device tensor"
    return dict(id=cid, cfg=cfg, size=size, route=route, K=K, flaw=flaw, kind=kind, negative=negative, c=c)


_D64 = dict(d=64, L=3)
_D16 = dict(d=16, L=3)
_D64L2 = dict(d=64, L=2)
_D256 = dict(d=256, L=3)
_D256L2 = dict(d=256, L=2)
_D132 = dict(d=132, L=3)
_D130 = dict(d=130, L=3)
_R3 = ("3", "staged, one launch")
_R4 = ("4", "device ids, one launch")
FUSED_256 = "what tpnet_encoder_fused_supported says"       # (resolved in the case: ("5", "one crossing") or ("5", "device ids, scratch"))

FEATURE_CASES = [
    # d = 64, L = 3: the matrix-core one-launch kernel up to max_pairs
    _case("d64 max_pairs-1", _D64, lambda th: th["max_pairs"] - 1, _R3),
    _case("d64 max_pairs", _D64, lambda th: th["max_pairs"], _R3),
    _case("d64 max_pairs+1", _D64, lambda th: th["max_pairs"] + 1, ("8", "upload")),
    _case("d64 max_pairs+2 pattern", _D64, lambda th: th["max_pairs"] + 2, ("5", "one crossing"), K=2731),
    _case("d64 max_pairs+2 broken tile", _D64, lambda th: th["max_pairs"] + 2, ("8", "upload, 5 declined"), K=2731, flaw="broken tile"),
    # d = 16, L = 3: the plain fused kernel up to MAX_PAIRS; no anchored readout on rows of 16 floats
    _case("d16 MAX_PAIRS-1", _D16, lambda th: th["MAX_PAIRS"] - 1, _R3),
    _case("d16 MAX_PAIRS", _D16, lambda th: th["MAX_PAIRS"], _R3),
    _case("d16 MAX_PAIRS+1", _D16, lambda th: th["MAX_PAIRS"] + 1, ("8", "staged")),
    _case("d16 MAX_PAIRS+2 pattern", _D16, lambda th: th["MAX_PAIRS"] + 2, ("8", "staged, 5 declined"), K=17),
    # d = 64, L = 2: no prepared image
    _case("d64 L2 MAX_PAIRS-1", _D64L2, lambda th: th["MAX_PAIRS"] - 1, _R3),
    _case("d64 L2 MAX_PAIRS", _D64L2, lambda th: th["MAX_PAIRS"], _R3),
    _case("d64 L2 MAX_PAIRS+1", _D64L2, lambda th: th["MAX_PAIRS"] + 1, ("8", "staged")),
    _case("d64 L2 pattern above 8192", _D64L2, lambda th: _above(8192, 4), ("8", "staged, 5 declined"), K=4),
    # d = 256, L = 3
    _case("d256 max_pairs-1", _D256, lambda th: th["max_pairs"] - 1, _R3),
    _case("d256 max_pairs", _D256, lambda th: th["max_pairs"], _R3),
    _case("d256 max_pairs+1", _D256, lambda th: th["max_pairs"] + 1, _R4),
    _case("d256 pattern K4 just above 8192", _D256, lambda th: _above(8192, 4), _R3, K=4, negative=False),
    _case("d256 pattern K4", _D256, lambda th: _above(th["max_pairs"], 4), FUSED_256, K=4),
    _case("d256 pattern K20", _D256, lambda th: _above(th["max_pairs"], 20), FUSED_256, K=20),
    _case("d256 pattern K2", _D256, lambda th: _above(th["max_pairs"], 2), ("7", "shared, 5 declined"), K=2),
    _case("d256 pattern K3", _D256, lambda th: _above(th["max_pairs"], 3), ("7", "shared, 5 declined"), K=3),
    _case("d256 broken repeat", _D256, lambda th: _above(th["max_pairs"], 4), ("7", "shared, 5 declined"), K=4, flaw="broken repeat"),
    # d = 256, L = 2
    _case("d256 L2 pattern K5", _D256L2, lambda th: _above(8192, 5), ("6", "anchored, 5 declined"), K=5),
    _case("d256 L2 pattern K3", _D256L2, lambda th: _above(8192, 3), ("7", "shared, 5 declined"), K=3),
    _case("d256 L2 tiled below 8192", _D256L2, lambda th: _above(th["MAX_PAIRS"], 4) - 16, _R3, K=4, negative=False),
    # d = 132 (dim > 128, whole 16-byte vectors) and d = 130 (dim % 4 != 0: no anchored readout)
    _case("d132 max_pairs+1", _D132, lambda th: th["max_pairs"] + 1, _R4),
    _case("d132 pattern K4", _D132, lambda th: _above(th["max_pairs"], 4), ("5", "one crossing"), K=4),
    _case("d130 n500", _D130, lambda th: 500, _R3),
    _case("d130 MAX_PAIRS+1", _D130, lambda th: th["MAX_PAIRS"] + 1, ("8", "staged")),
    _case("d130 pattern K4", _D130, lambda th: _above(th["MAX_PAIRS"], 4), ("7", "shared, 5 declined"), K=4),
    _case("d130 short tiled", _D130, lambda th: 600, _R3, K=4, negative=False),
    # one case each
    _case("not_scale", dict(d=64, L=3, not_scale=True), lambda th: 500, _R3),
    _case("use_matrix", dict(d=40, L=3, N=40, use_matrix=True), lambda th: 500, _R3),
    _case("extra layer", dict(d=64, L=3, extra_layer=True), lambda th: 500, ("8", "staged")),
    _case("extra layer, tiled wide rows", dict(d=256, L=3, extra_layer=True), lambda th: 600, ("7", "shared"), K=4),
    _case("fused_mlp 16384", dict(d=64, L=3, fused=True), lambda th: 16384, ("1", "bf16 one launch"), c=C_BF16),
    _case("fused_mlp 16385", dict(d=64, L=3, fused=True), lambda th: 16385, ("8", "upload, bf16 layers"), c=C_BF16),
    # kinds of arguments
    _case("python lists", _D64, lambda th: 3000, _R3, kind="lists"),
    _case("int32 arrays", _D64, lambda th: 3000, _R3, kind="int32"),
    _case("strided int64 views", _D64, lambda th: 3000, _R3, kind="strided"),
    _case("dst a cpu tensor", _D64, lambda th: 3000, ("8", "upload"), kind="dst cpu tensor"),
    _case("src a device tensor", _D64, lambda th: 3000, ("2", "device ids"), kind="src device tensor"),
    # the pattern's edge cases (the "equal anchors" law of tools/soak_encoder.py), just above max_pairs
    _case("d64 first two anchors equal", _D64, lambda th: _above(th["max_pairs"], 4), ("5", "device ids"), K=4,
          flaw="first two anchors equal"),
    _case("d64 first three anchors equal", _D64, lambda th: _above(th["max_pairs"], 4) + 8, ("5", "device ids"), K=4,
          flaw="first three anchors equal"),
    _case("d64 second half one anchor", _D64, lambda th: _above(th["max_pairs"], 4), ("5", "one crossing"), K=4,
          flaw="second half one anchor"),
    _case("d64 last element", _D64, lambda th: _above(th["max_pairs"], 4), ("8", "upload, 5 declined"), K=4, flaw="last element"),
    _case("d256 first two anchors equal", _D256, lambda th: _above(th["max_pairs"], 4), ("5", "device ids, scratch"), K=4,
          flaw="first two anchors equal"),
    _case("d256 first three anchors equal", _D256, lambda th: _above(th["max_pairs"], 4) + 8, ("5", "device ids, scratch"), K=4,
          flaw="first three anchors equal"),
    _case("d256 second half one anchor", _D256, lambda th: _above(th["max_pairs"], 4), FUSED_256, K=4, flaw="second half one anchor"),
    _case("d256 last element", _D256, lambda th: _above(th["max_pairs"], 4), ("7", "shared, 5 declined"), K=4, flaw="last element"),
    # the big slot of the crossing
    _case("d64 big slot", _D64, _big_slot_n, ("5", "one crossing"), K=4),
    _case("d64 above the big slot", _D64, lambda th: _big_slot_n(th) + 8, ("5", "device ids"), K=4),
]

GRAD_CASES = [
    _case("route 3", _D64, lambda th: 700, _R3),
    _case("route 4", _D256, lambda th: th["max_pairs"] + 1, _R4),
    _case("route 5 crossing d64", _D64, lambda th: _above(th["max_pairs"], 4), ("5", "one crossing"), K=4),
    _case("route 5 crossing d256", _D256, lambda th: _above(th["max_pairs"], 4), ("5", "one crossing"), K=4),
    _case("route 5 device ids", _D64, lambda th: _above(th["max_pairs"], 4), ("5", "device ids, scratch"), K=4,
          flaw="first two anchors equal"),
    _case("route 6", _D256L2, lambda th: _above(8192, 5), ("6", "anchored, 5 declined"), K=5),
    _case("route 7", _D256L2, lambda th: _above(8192, 3), ("7", "shared, 5 declined"), K=3),
    _case("route 8", _D64L2, lambda th: th["MAX_PAIRS"] + 1, ("8", "staged")),
]


def _case_pairs(case, th, N):
    n = int(case["size"](th))
    rng = np.random.RandomState(_seed("pairs", case["id"]))
    if case["K"] is None:
        return _random_pairs(rng, N, n, case["negative"])
    return _pattern_pairs(rng, N, n, case["K"], case["flaw"])


def _run_feature_case(case, monkeypatch, grad=False):
    from tpnet_amd import _lib
    rp, st, layers, th = _table(**case["cfg"])
    N = rp.node_num
    u, v = _case_pairs(case, th, N)
    n = len(u)
    assert n <= 180000
    expected = case["route"]
    if expected == FUSED_256:
        prep = rp._overlapped_mlp()
        one = _lib.load().tpnet_encoder_fused_supported(rp._st_ref(), (n // 2) // case["K"], case["K"], prep.ref)
        expected = ("5", "one crossing") if one else ("5", "device ids, scratch")
    au, av = _as_kind(u, v, case["kind"])
    rec = _Recorder(rp, monkeypatch)
    what = ("grad " if grad else "") + case["id"]
    if grad:
        got = rp.get_pair_wise_feature(au, av)
        assert got.requires_grad
    else:
        with torch.no_grad():
            got = rp.get_pair_wise_feature(au, av)
    route = rec.feature_route()
    rp.check_device_errors()
    uw, vw = _wrapped(u, N), _wrapped(v, N)
    _check_outputs(got.detach().cpu().numpy(), layers, st, uw, vw, rp.not_scale, case["c"], what)
    if grad:
        ud, vd = torch.from_numpy(uw).to(DEV), torch.from_numpy(vw).to(DEV)
        gram = rp.pair_gram(ud, vd)
        _check_features(gram.cpu().numpy(), st, uw, vw, rp.not_scale, what + " pre-mlp")
        want = rp.mlp(gram)
        gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(n)).to(DEV)
        params = list(rp.mlp.parameters())
        _assert_mlp_grads_close(rp.mlp, gram, gy, torch.autograd.grad(got, params, gy), torch.autograd.grad(want, params, gy))
    _reached(route, what, expected)                  # (last: a call served by another route has had its numbers checked all the same)
    _RAN.add(what)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FEATURE_CASES, ids=[c["id"] for c in FEATURE_CASES])
def test_get_pair_wise_feature_route_and_oracle(case, monkeypatch):
    """Group 2: the route table under no_grad -- the route the case names, and the outputs against self.mlp in float64 on the
    oracle's features."""
    _need_gpu()
    _run_feature_case(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRAD_CASES, ids=[c["id"] for c in GRAD_CASES])
def test_get_pair_wise_feature_with_gradients(case, monkeypatch):
    """Group 3: the same call with gradients recorded -- route, forward as in group 2, and the gradients of self.mlp's four tensors
    against autograd over rp.mlp(rp.pair_gram(...)) on device ids."""
    _need_gpu()
    _run_feature_case(case, monkeypatch, grad=True)


def test_fp32_layers_against_float64_on_the_feature_cases():
    """The measurement behind C_DENSE (CPU): torch's float32 layers on the oracle's features of the feature cases above against the
    float64 layers on the same inputs, as a fraction of max(1, |y64|.max()).  The docstring's figure was taken over every pair of
    every case; the suite repeats it on the first CHUNK pairs of each case whose list is no longer than 20 000 pairs.  Half of
    2e-5 is the line above which C_DENSE would have to grow."""
    th = _thresholds()
    worst = 0.0
    for case in FEATURE_CASES:
        n = int(case["size"](th))
        if n > 20000 or case["c"] != C_DENSE:
            continue
        key, _, st, mlp, layers = _cpu_side(**case["cfg"])
        N = key[2]
        u, v = _case_pairs(case, th, N)
        x, _ = _oracle_features(st, _wrapped(u[:CHUNK], N), _wrapped(v[:CHUNK], N), key[3])
        with torch.no_grad():
            y32 = mlp(torch.from_numpy(x.astype(np.float32))).numpy()
        y64, _ = _mlp64(layers, x, np.zeros_like(x))
        ratio = float(np.abs(y32 - y64).max()) / max(1.0, float(np.abs(y64).max()))
        worst = max(worst, ratio)
    print(f"fp32 layers against float64 layers, worst ratio {worst:.3e}")
    assert worst <= 0.5 * C_DENSE, worst


# ---------------------------------------------------------------------------------------------------------
# group 1: pair_gram from host arrays
# ---------------------------------------------------------------------------------------------------------
GRAM_SIZES = {"1": lambda th: 1, "max_pairs-1": lambda th: th["max_pairs"] - 1, "max_pairs": lambda th: th["max_pairs"],
              "max_pairs+1": lambda th: th["max_pairs"] + 1, "2*max_pairs+5": lambda th: 2 * th["max_pairs"] + 5}
GRAM_CASES = [(d, flag, size) for d in (16, 30, 64) for flag in ("default", "raw", "packed", "not_scale") for size in GRAM_SIZES]


def _run_gram_case(d, flag, size, monkeypatch):
    rp, st, _, th = _table(d=d, L=3, not_scale=flag == "not_scale")
    N = rp.node_num
    n = int(GRAM_SIZES[size](th))
    what = f"pair_gram d={d} {flag} n={size}"
    u, v = _random_pairs(np.random.RandomState(_seed(what)), N, n)
    kw = dict(raw=flag == "raw", packed=flag == "packed")
    rec = _Recorder(rp, monkeypatch)
    got = rp.pair_gram(u, v, **kw)
    route = rec.gram_route()
    uw, vw = _wrapped(u, N), _wrapped(v, N)
    dev = rp.pair_gram(torch.from_numpy(uw).to(DEV), torch.from_numpy(vw).to(DEV), **kw)
    assert torch.equal(got, dev), what + ": host ids and device ids give different bits"
    got = got.cpu().numpy()
    if flag == "packed":
        NN = 2 * rp.num_layer + 2
        assert got.shape == (n, rp.packed_feature_dim)
        full = np.zeros((n, NN, NN), dtype=np.float32)
        a, b = np.triu_indices(NN)                                 # row-major upper triangle (include/tpnet_hip.h: TPNET_FLAG_PACKED)
        full[:, a, b] = got
        full[:, b, a] = got
        got = full.reshape(n, NN * NN)
    _check_features(got, st, uw, vw, flag != "default", what)
    rp.check_device_errors()
    _reached(route, what, ("pair_gram", "staged" if n <= th["max_pairs"] else "upload"))
    _RAN.add(what)


@pytest.mark.gpu
@pytest.mark.parametrize("d,flag,size", GRAM_CASES)
def test_pair_gram_from_host_arrays(d, flag, size, monkeypatch):
    """Group 1: _host_readout on one side of max_pairs, upload + tpnet_pair_gram on the other: against the oracle, and bit for bit
    against the call on device ids."""
    _need_gpu()
    _run_gram_case(d, flag, size, monkeypatch)


# ---------------------------------------------------------------------------------------------------------
# group 4: update from host arrays
# ---------------------------------------------------------------------------------------------------------
UPDATE_SIZES = {"1": lambda th: 1, "1024": lambda th: 1024, "1025": lambda th: 1025,
                "max_batch-1": lambda th: th["max_batch"] - 1, "max_batch": lambda th: th["max_batch"],
                "max_batch+1": lambda th: th["max_batch"] + 1, "max_host_batch-1": lambda th: th["max_host_batch"] - 1,
                "max_host_batch": lambda th: th["max_host_batch"], "max_host_batch+1": lambda th: th["max_host_batch"] + 1}
UPDATE_CASES = [(d, exact, N, size) for d in (16, 64) for exact in (False, True) for N in (300, 30000) for size in UPDATE_SIZES]


def _update_table(d, N, exact, what):
    rng = np.random.RandomState(_seed(what))
    P0 = (rng.randn(N, d) / np.sqrt(d)).astype(np.float32)
    rp = _module(N, d, 3, LAM, T0, P0=P0, exact=exact)
    st = O.OracleState(P0, 3, LAM, T0)
    return rng, rp, st, _thresholds(rp)


def _saved_state(rp):
    """(layers 1..L, clock) as backup_random_projections hands them out: clones, so the engine keeps its per-row state (reading
    random_projections[i] would have the next call import the layers again, and the second update would meet a fresh table)."""
    now, layers = rp.backup_random_projections()
    return np.stack([x.cpu().numpy() for x in layers]), float(now.item())


def _run_update_case(d, exact, N, size, monkeypatch):
    what = f"update d={d} exact={exact} N={N} B={size}"
    rng, rp, st, th = _update_table(d, N, exact, what)
    B = int(UPDATE_SIZES[size](th))
    assert B <= 11000
    src, dst, _, t = _random_stream(rng, N, 450 + 2 * B, 5.0e5, hub_frac=0.2 if N == 300 else 0.02)
    for a, b in ((0, 100), (100, 250), (250, 450)):
        rp.update(src[a:b], dst[a:b], t[a:b])
        O.update(st, src[a:b], dst[a:b], t[a:b])
    expected = ("update", "slot" if B <= th["max_batch"] else ("staged copy" if B <= th["max_host_batch"] else "upload"))
    rec = _Recorder(rp, monkeypatch)
    rtol = 5e-6 if exact else 1e-4
    routes = []
    for k in range(2):
        sl = slice(450 + k * B, 450 + (k + 1) * B)
        rec.clear()
        rp.update(src[sl], dst[sl], t[sl])
        routes.append(rec.update_route())
        O.update(st, src[sl], dst[sl], t[sl])
        layers, now = _saved_state(rp)
        _assert_state(layers, np.stack(st.P[1:]), rtol, f"{what}, update {k}")
        assert now == float(st.now_time)
    u, v = _random_pairs(rng, N, 64)
    _check_features(rp.pair_gram(u, v).cpu().numpy(), st, _wrapped(u, N), _wrapped(v, N), False, what + " readout")
    _assert_state(_layers(rp), np.stack(st.P[1:]), rtol, what + ", as the Parameters")
    assert float(rp.now_time.item()) == float(st.now_time)
    rp.check_device_errors()
    for route in routes:
        _reached(route, what, expected)
    _RAN.add(what)


@pytest.mark.gpu
@pytest.mark.parametrize("d,exact,N,size", UPDATE_CASES)
def test_update_from_host_arrays(d, exact, N, size, monkeypatch):
    """Group 4: tpnet_host_update's two branches and the upload behind them, two consecutive updates each (the second meets rows in
    the other copy): state and clock after each against O.update, one readout after the second."""
    _need_gpu()
    _run_update_case(d, exact, N, size, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True])
def test_update_rejects_an_id_out_of_range_on_the_staged_branch(exact):
    """B = max_batch + 1 with one id out of range: IndexError, state and clock untouched -- and the table still follows the oracle."""
    _need_gpu()
    N, d = 300, 64
    rng, rp, st, th = _update_table(d, N, exact, f"bad id exact={exact}")
    B = th["max_batch"] + 1
    src, dst, _, t = _random_stream(rng, N, 450 + B, 5.0e5)
    for a, b in ((0, 100), (100, 250), (250, 450)):
        rp.update(src[a:b], dst[a:b], t[a:b])
        O.update(st, src[a:b], dst[a:b], t[a:b])
    before, now = _saved_state(rp)
    sl = slice(450, 450 + B)
    for bad_at, bad_id in ((B - 1, N), (B // 2, -N - 1)):
        bad = dst[sl].copy()
        bad[bad_at] = bad_id
        with pytest.raises(IndexError):
            rp.update(src[sl], bad, t[sl])
        after, now2 = _saved_state(rp)
        np.testing.assert_array_equal(after, before)
        assert now2 == now == float(st.now_time)
    rp.check_device_errors()
    rp.update(src[sl], dst[sl], t[sl])
    O.update(st, src[sl], dst[sl], t[sl])
    layers, now = _saved_state(rp)
    _assert_state(layers, np.stack(st.P[1:]), 5e-6 if exact else 1e-4, "after the rejected calls")
    assert now == float(st.now_time)


# ---------------------------------------------------------------------------------------------------------
# group 5: encoder_pair_features from host arrays
# ---------------------------------------------------------------------------------------------------------
ENCODER_SIZES = {"max_host_batch-1": -1, "max_host_batch": 0, "max_host_batch+1": 1}


def _run_encoder_case(size, monkeypatch):
    from tpnet_amd.callers import RecentNeighborSampler, encoder_pair_indices
    from tpnet_amd.sampler import GpuRecentNeighborSampler
    what = f"encoder_pair_features B={size}"
    rp, st, layers, th = _table(**_D64)
    N, K = rp.node_num, 4
    B = th["max_host_batch"] + ENCODER_SIZES[size]
    assert 4 * B * K <= 180000
    rng = np.random.RandomState(_seed(what))
    hs, hd, _, ht = _random_stream(rng, N, 2000, 3.0e5)
    host = RecentNeighborSampler(hs, hd, ht)
    gpu = GpuRecentNeighborSampler(hs, hd, ht, device=DEV, num_nodes=N)
    src = rng.randint(0, N, B).astype(np.int64)                  # (the padding id among them)
    other = rng.randint(1, N, B).astype(np.int64)
    other[::7] = src[::7]
    times = rng.uniform(ht[0], ht[-1] + 1.0e4, B)
    rec = _Recorder(rp, monkeypatch)
    with torch.no_grad():
        got, neigh = rp.encoder_pair_features(gpu, src, other, times, K)
    route = rec.encoder_route()
    neigh_h, _, _ = host.get_historical_neighbors(np.concatenate([src, other]), np.tile(times, 2), K)
    np.testing.assert_array_equal(neigh.cpu().numpy(), neigh_h)
    u, v = encoder_pair_indices(neigh_h, src, other)
    _check_outputs(got.cpu().numpy(), layers, st, u, v, False, C_DENSE, what)
    rp.check_device_errors()
    _reached(route, what, ("encoder_pair_features", "staged" if B <= th["max_host_batch"] else "upload"))
    _RAN.add(what)


@pytest.mark.gpu
@pytest.mark.parametrize("size", list(ENCODER_SIZES))
def test_encoder_pair_features_from_host_arrays(size, monkeypatch):
    """Group 5: the staged path (tpnet_host_encoder_features) and the upload fallback above max_host_batch, K = 4 over a 2 000-edge
    history: neighbour ids equal to the host sampler's, features against the oracle through them."""
    _need_gpu()
    _run_encoder_case(size, monkeypatch)


# ---------------------------------------------------------------------------------------------------------
# the closing test: the whole table was reached
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_route_of_the_table_was_reached(monkeypatch):
    """The set of (route, sub-route) pairs reached by the cases above is the table of the file's docstring, no more and no less
    (they run first: file order; a case that did not run in this process -- the test run alone, or a selection -- is run here)."""
    _need_gpu()
    for case in FEATURE_CASES:
        if case["id"] not in _RAN:
            _run_feature_case(case, monkeypatch)
    for case in GRAD_CASES:
        if "grad " + case["id"] not in _RAN:
            _run_feature_case(case, monkeypatch, grad=True)
    for d, flag, size in GRAM_CASES:
        if f"pair_gram d={d} {flag} n={size}" not in _RAN:
            _run_gram_case(d, flag, size, monkeypatch)
    for d, exact, N, size in UPDATE_CASES:
        if f"update d={d} exact={exact} N={N} B={size}" not in _RAN:
            _run_update_case(d, exact, N, size, monkeypatch)
    for size in ENCODER_SIZES:
        if f"encoder_pair_features B={size}" not in _RAN:
            _run_encoder_case(size, monkeypatch)
    reached = set(_REACHED)
    assert reached == TABLE, f"never reached: {sorted(TABLE - reached)}; not in the table: {sorted(reached - TABLE)}"


# ---------------------------------------------------------------------------------------------------------
# group 6, CPU tier: tpnet_host_encoder_pattern is pure host arithmetic
# ---------------------------------------------------------------------------------------------------------
def _pattern_ref(src, dst):
    """The pattern's K as numpy states it: the halves of src equal and K = gcd(h, positions where either half of dst changes) >= 2,
    else 0."""
    n = len(src)
    if n < 4 or n % 2:
        return 0
    h = n // 2
    if not np.array_equal(src[:h], src[h:]):
        return 0
    ch = np.concatenate([np.flatnonzero(x[1:] != x[:-1]) + 1 for x in (dst[:h], dst[h:])])
    K = int(np.gcd.reduce(ch, initial=h))
    return K if K >= 2 else 0


def _pattern_lists():
    rng = np.random.RandomState(20240)
    N = 50
    lists = []

    def add(what, src, dst):
        lists.append((what, np.ascontiguousarray(src, dtype=np.int64), np.ascontiguousarray(dst, dtype=np.int64)))

    def pattern(h, K, front=1, second=None):
        m = h // K
        a1, a2 = (1 + np.cumsum(rng.randint(1, N - 1, m)) % (N - 1) for _ in range(2))
        a1[:min(front, m)] = a1[0]
        if second is not None:
            a2[:] = second
        neigh = rng.randint(0, N, h)
        return np.tile(neigh, 2), np.concatenate([np.repeat(a1, K), np.repeat(a2, K)])

    for h in range(2, 65):                                        # every divisor structure of h, K = 1 included
        for K in [k for k in range(1, h + 1) if h % k == 0]:
            if h <= 32 or rng.rand() < 0.25:
                add(f"h={h} K={K}", *pattern(h, K))
    for h, K in ((24, 4), (36, 4), (60, 5), (64, 2), (48, 3), (63, 7), (40, 4)):
        add(f"h={h} K={K} front 2K", *pattern(h, K, front=2))
        add(f"h={h} K={K} front 3K", *pattern(h, K, front=3))
        add(f"h={h} K={K} second half one anchor", *pattern(h, K, second=9))
    for h in (2, 3, 17, 64):
        add(f"h={h} all equal", np.tile(rng.randint(0, N, h), 2), np.full(2 * h, 7))
        add(f"h={h} halves equal, each constant", np.tile(rng.randint(0, N, h), 2), np.repeat([3, 4], h))
    for n in (0, 1, 2, 3, 5, 9, 25):                              # odd n, n < 4
        add(f"n={n}", np.arange(n) // 2 % max(1, n // 2), np.zeros(n))
    src, dst = pattern(12, 4)
    for i in range(24):                                           # a single changed entry at each position in turn
        s, d = src.copy(), dst.copy()
        d[i] = _other(int(d[i]), N)
        add(f"dst[{i}] changed", src, d)
        s[i] = (s[i] + 1) % N
        add(f"src[{i}] changed", s, dst)
    return lists, N


def test_host_encoder_pattern_against_numpy(hip_lib):
    """tpnet_host_encoder_pattern against the numpy restatement on seeded lists of h <= 64.  The C fast path may return any K'
    that tiles both halves and is a multiple (or a divisor) of the restatement's K; where the restatement says 0, so must it."""
    lists, N = _pattern_lists()
    assert len(lists) >= 200
    zeros = 0
    for what, src, dst in lists:
        n = len(src)
        want = _pattern_ref(src, dst)
        got = int(hip_lib.tpnet_host_encoder_pattern(src.ctypes.data, dst.ctypes.data, n, N))
        if want == 0:
            zeros += 1
            assert got == 0, (what, got)
            continue
        assert got >= 2 and (got % want == 0 or want % got == 0), (what, got, want)
        h = n // 2
        assert h % got == 0, (what, got)
        blocks = dst.reshape(2, h // got, got)
        assert (blocks == blocks[:, :, :1]).all(), (what, got, want)
    assert zeros >= 30 and len(lists) - zeros >= 100, zeros        # both answers are well represented
    assert int(hip_lib.tpnet_host_encoder_pattern(None, None, 8, N)) == 0
