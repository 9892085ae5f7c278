"""Device-side negative edge sampler (C ABI: tpnet_neg_build / tpnet_neg_sample / tpnet_neg_check, csrc/negsampler.hip).

Drop-in for the reference's `NegativeEdgeSampler` (utils/utils.py:315-505) with its three `negative_sample_strategy` values.  The
reference rebuilds Python sets over every edge seen so far for each batch and keeps |unique src| x |unique dst| tuples from
construction on; here the unique edges live in HBM as one sorted table with their occurrence times, and a call is four kernel
launches whatever the history's length."""
import ctypes as C

import numpy as np
import torch

from . import _lib

_STRATEGY = {"random": 0, "historical": 1, "inductive": 2}
FILTER_MODES = {"same_time": 1, "known": 2}          # TPNET_FILTER_SAME_TIME, TPNET_FILTER_KNOWN


def filter_lists_host(src, dst, t, batch_src, batch_dst, batch_t, mode: str, candidate_range, capacity: int):
    """tpnet_neg_filter_lists' rule in numpy, on the stream (src, dst, t) a sampler would be built on: query i = (s, d, t_i) gets the
    destinations d' != d inside candidate_range = (lo, hi) that `mode` excludes -- 'known': (s, d') occurs in the stream at any time;
    'same_time': at time exactly t_i -- ascending and distinct, the first F = capacity of them, the rest of the row -1.
    -> (fil [B, F] int64, n_fil [B] int32): n_fil is the TRUE count, which may exceed F (overflow)."""
    if mode not in FILTER_MODES:
        raise ValueError(f"filter mode {mode!r} is none of {sorted(FILTER_MODES)}")
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    t = np.zeros(len(src)) if t is None else np.asarray(t, dtype=np.float64)
    lo, hi, F = int(candidate_range[0]), int(candidate_range[1]), int(capacity)
    B = len(batch_src)
    fil = np.full((B, F), -1, dtype=np.int64)
    n_fil = np.zeros(B, dtype=np.int32)
    for i in range(B):
        m = src == int(batch_src[i])
        if mode == "same_time":
            m &= t == float(batch_t[i])
        ds = np.unique(dst[m])
        ds = ds[(ds != int(batch_dst[i])) & (ds >= lo) & (ds < hi)]
        n_fil[i] = len(ds)
        fil[i, :min(F, len(ds))] = ds[:F]
    return fil, n_fil


class GpuNegativeEdgeSampler:
    """The reference's keywords, attributes and `sample` signature.  'historical' draws among the edges seen up to the batch's start
    that do not occur inside the batch's window, 'inductive' also leaves out the edges first seen up to `last_observed_time`; when
    fewer than `size` exist, uniformly drawn pairs of (unique src) x (unique dst) that are not pairs of the batch come first and ALL
    candidates follow.

    The draws come from a counter-based generator (Philox4x32-10) keyed by the seed and indexed by (call, slot), through a keyed
    permutation (include/tpnet_hip.h spells the rule out): the same seed replays the same negatives, `reset_random_state()` restarts
    the sequence of calls, and a call's output does not depend on the sizes of earlier calls.  They follow the reference's
    probabilities but are NOT numpy's `RandomState.choice` stream, and the candidates' order (Python-set order in the reference) is
    the edges' (src, dst) order here."""

    def __init__(self, src_node_ids, dst_node_ids, interact_times=None, last_observed_time: float = None,
                 negative_sample_strategy: str = "random", seed: int = None, device="cuda:0"):
        if negative_sample_strategy not in _STRATEGY:
            raise ValueError(f"Not implemented error for negative_sample_strategy {negative_sample_strategy}!")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.TPNetHipError("GpuNegativeEdgeSampler needs a cuda device (no CPU fallback)")
        lib = _lib.load()
        self.seed = seed
        self.negative_sample_strategy = negative_sample_strategy
        self.last_observed_time = last_observed_time
        if negative_sample_strategy == "inductive":
            assert last_observed_time is not None and interact_times is not None
        to = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(self.device) \
            if not isinstance(a, torch.Tensor) else a.to(self.device, dt).contiguous()
        src, dst = to(src_node_ids, torch.int64), to(dst_node_ids, torch.int64)
        t = to(interact_times, torch.float64) if interact_times is not None else None
        self.E = int(src.numel())
        self._built_on = (src, dst, t)                # (filter_capacity reads the stream once, when first asked)
        self._filter_capacity = {}
        assert self.E > 0 and int(dst.numel()) == self.E and (t is None or int(t.numel()) == self.E)
        self.earliest_time = float(t.min().item()) if t is not None else None
        nbytes = lib.tpnet_neg_bytes(self.E)
        self._buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        counts = (C.c_int64 * 3)()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(lib.tpnet_neg_build(self._buf.data_ptr(), nbytes, src.data_ptr(), dst.data_ptr(),
                                       t.data_ptr() if t is not None else None, self.E,
                                       float(last_observed_time) if last_observed_time is not None else 0.0,
                                       1 if last_observed_time is not None else 0, counts, stream), "neg_build")
        self.num_unique_edges, n_src, n_dst = int(counts[0]), int(counts[1]), int(counts[2])
        unique_src = torch.empty(n_src, dtype=torch.int64, device=self.device)
        unique_dst = torch.empty(n_dst, dtype=torch.int64, device=self.device)
        _lib.check(lib.tpnet_neg_uniques(self._buf.data_ptr(), self.E, n_src, n_dst, unique_src.data_ptr(), unique_dst.data_ptr(), stream),
                   "neg_uniques")
        self.unique_src_node_ids = unique_src.cpu().numpy()
        self.unique_dst_node_ids = unique_dst.cpu().numpy()
        # an unseeded 'random' sampler of the reference draws from numpy's global generator (utils/utils.py:394-396): one key from it
        self._key = int(seed) & (2 ** 64 - 1) if seed is not None else int(np.random.randint(0, 2 ** 64, dtype=np.uint64))
        self._calls = 0
        self._scratch = None

    def reset_random_state(self):
        """utils/utils.py:500-505: the next call is call 0 of the seed again."""
        self._calls = 0

    def _scratch_for(self, size: int, B: int):
        need = _lib.load().tpnet_neg_scratch_bytes(self.E, size, B)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._scratch

    def sample_device(self, size: int, batch_src: torch.Tensor = None, batch_dst: torch.Tensor = None, t0: float = 0.0,
                      t1: float = 0.0):
        """-> (negative src, negative dst), two int64 device tensors of `size`; batch_src / batch_dst int64 device tensors.  Nothing
        synchronises.  A fill whose every possible pair is a pair of the batch (only when |unique src| |unique dst| <= len(batch))
        leaves -1 in its slots and sets the sampler's error word: `tpnet_neg_check` (`check()`) is the caller's to call then.
        Every call advances the call index, whatever its size.  The scratch buffer is the sampler's own: calls belong on one stream."""
        size = int(size)
        strategy = _STRATEGY[self.negative_sample_strategy]
        if strategy:
            assert self.seed is not None
            assert batch_src is not None and batch_dst is not None
        out_src = torch.empty(max(size, 0), dtype=torch.int64, device=self.device)
        out_dst = torch.empty(max(size, 0), dtype=torch.int64, device=self.device)
        call = self._calls & 0xFFFFFFFF
        self._calls += 1
        if size == 0:
            return out_src, out_dst
        B = int(batch_src.numel()) if strategy else 0
        scratch = self._scratch_for(size, B) if strategy else None
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().tpnet_neg_sample(self._buf.data_ptr(), self.E, strategy, size,
                                                batch_src.data_ptr() if strategy and B else None,
                                                batch_dst.data_ptr() if strategy and B else None, B, float(t0), float(t1), self._key,
                                                call, scratch.data_ptr() if strategy else None,
                                                scratch.numel() if strategy else 0, out_src.data_ptr(), out_dst.data_ptr(), stream),
                   "neg_sample")
        return out_src, out_dst

    def sample_many_device(self, batch_src: torch.Tensor, batch_dst: torch.Tensor, batch_t: torch.Tensor, num_negatives: int,
                           num_historical: int = None):
        """Per-query candidates of the ranking protocol (tpnet_neg_sample_many; include/tpnet_hip.h spells the rule out): every
        positive (s, d, t) of the batch gets its own row of Q = num_negatives destinations -> (cand [B, Q] int64, n_hist [B] int32) on
        the device.  The first n_hist[i] <= Qh = num_historical (default Q // 2) entries of a row are destinations `s` was seen with
        before t, the rest are drawn from the unique destinations; a row's entries are distinct, never d and never a destination `s`
        has an edge to at exactly t; slots that cannot be filled hold -1.  `negative_sample_strategy` is not consulted.  A row depends
        on (seed, call index, its index in the batch) and its own (s, d, t) alone.  batch_src / batch_dst: int64 device tensors,
        batch_t: a float64 device tensor.  Nothing synchronises; the call advances the call index like `sample_device`."""
        Q = int(num_negatives)
        Qh = Q // 2 if num_historical is None else int(num_historical)
        if not (1 <= Q < 1 << 16 and 0 <= Qh <= Q):
            raise ValueError(f"sample_many_device: 1 <= num_negatives < 65536 and 0 <= num_historical <= num_negatives, not {Q}, {Qh}")
        for x, dt, what in ((batch_src, torch.int64, "batch_src"), (batch_dst, torch.int64, "batch_dst"), (batch_t, torch.float64, "batch_t")):
            if not isinstance(x, torch.Tensor) or x.dtype != dt or not x.is_cuda or x.dim() != 1:
                raise TypeError(f"sample_many_device: {what} must be a one-dimensional {dt} tensor on {self.device}")
        B = int(batch_src.numel())
        if int(batch_dst.numel()) != B or int(batch_t.numel()) != B:
            raise ValueError("sample_many_device: batch_src, batch_dst and batch_t must have the same length")
        bs, bd, bt = batch_src.contiguous(), batch_dst.contiguous(), batch_t.contiguous()
        cand = torch.empty((B, Q), dtype=torch.int64, device=self.device)
        n_hist = torch.empty(B, dtype=torch.int32, device=self.device)
        call = self._calls & 0xFFFFFFFF
        self._calls += 1
        if B == 0:
            return cand, n_hist
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().tpnet_neg_sample_many(self._buf.data_ptr(), self.E, bs.data_ptr(), bd.data_ptr(), bt.data_ptr(), B, Q, Qh,
                                                     self._key, call, cand.data_ptr(), n_hist.data_ptr(), stream), "neg_sample_many")
        return cand, n_hist

    def filter_capacity(self, mode: str) -> int:
        """The longest filter list `mode` can give on the stream the sampler was built on: the largest number of distinct
        destinations of one source ('known') or of one (source, instant) ('same_time'); at least 1.  Computed once per mode (torch
        on the device; synchronises that once) -- `filter_lists_device`'s default capacity, with which no row overflows."""
        if mode not in FILTER_MODES:
            raise ValueError(f"filter mode {mode!r} is none of {sorted(FILTER_MODES)}")
        if mode not in self._filter_capacity:
            src, dst, t = self._built_on
            cols = [src] + ([t.view(torch.int64)] if (mode == "same_time" and t is not None) else []) + [dst]
            rows = torch.unique(torch.stack(cols, dim=1), dim=0)
            _, n = torch.unique(rows[:, :-1], dim=0, return_counts=True)
            self._filter_capacity[mode] = max(1, int(n.max().item()))
        return self._filter_capacity[mode]

    def filter_lists_device(self, batch_src: torch.Tensor, batch_dst: torch.Tensor, batch_t: torch.Tensor, mode: str, candidate_range,
                            capacity: int = None):
        """Per-query filter lists of the all-node ranking protocol (tpnet_neg_filter_lists; `filter_lists_host` is the rule): query
        (s, d, t) gets the destinations d' != d inside candidate_range = (lo, hi) that `mode` excludes from its candidates --
        'same_time': the table holds (s, d') at exactly t, `sample_many_device`'s exclusion; 'known': at any time -- ascending,
        distinct, -1 behind them -> (fil [B, F] int64, n_fil [B] int32) on the device, F = capacity (default: filter_capacity(mode));
        n_fil is the true count, n_fil[i] > F = overflow.  One launch, nothing synchronises, the call index does not advance."""
        if mode not in FILTER_MODES:
            raise ValueError(f"filter mode {mode!r} is none of {sorted(FILTER_MODES)}")
        for x, dt, what in ((batch_src, torch.int64, "batch_src"), (batch_dst, torch.int64, "batch_dst"), (batch_t, torch.float64, "batch_t")):
            if not isinstance(x, torch.Tensor) or x.dtype != dt or not x.is_cuda or x.dim() != 1:
                raise TypeError(f"filter_lists_device: {what} must be a one-dimensional {dt} tensor on {self.device}")
        B = int(batch_src.numel())
        if int(batch_dst.numel()) != B or int(batch_t.numel()) != B:
            raise ValueError("filter_lists_device: batch_src, batch_dst and batch_t must have the same length")
        F = self.filter_capacity(mode) if capacity is None else int(capacity)
        lo, hi = int(candidate_range[0]), int(candidate_range[1])
        if not (1 <= F < 1 << 16) or hi < lo:
            raise ValueError(f"filter_lists_device: 1 <= capacity < 65536 and lo <= hi, not {F}, ({lo}, {hi})")
        bs, bd, bt = batch_src.contiguous(), batch_dst.contiguous(), batch_t.contiguous()
        fil = torch.empty((B, F), dtype=torch.int64, device=self.device)
        n_fil = torch.empty(B, dtype=torch.int32, device=self.device)
        if B == 0:
            return fil, n_fil
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().tpnet_neg_filter_lists(self._buf.data_ptr(), self.E, bs.data_ptr(), bd.data_ptr(), bt.data_ptr(), B,
                                                      FILTER_MODES[mode], lo, hi, F, fil.data_ptr(), n_fil.data_ptr(), stream),
                   "neg_filter_lists")
        return fil, n_fil

    def check(self):
        """tpnet_neg_check: synchronises; raises if a fill since the last check found no pair outside its batch."""
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().tpnet_neg_check(self._buf.data_ptr(), stream), "neg_sample: every possible edge is an edge of the batch")

    def sample(self, size: int, batch_src_node_ids: np.ndarray = None, batch_dst_node_ids: np.ndarray = None,
               current_batch_start_time: float = 0.0, current_batch_end_time: float = 0.0):
        """The reference's signature and return types (two numpy int64 arrays): utils/utils.py:361-386."""
        if self.negative_sample_strategy == "random":
            s, d = self.sample_device(size)
            return s.cpu().numpy(), d.cpu().numpy()
        assert self.seed is not None
        assert batch_src_node_ids is not None and batch_dst_node_ids is not None
        dev = lambda a: a.to(self.device, torch.int64).contiguous() if isinstance(a, torch.Tensor) \
            else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int64).to(self.device)
        bs, bd = dev(batch_src_node_ids), dev(batch_dst_node_ids)
        s, d = self.sample_device(size, bs, bd, float(current_batch_start_time), float(current_batch_end_time))
        if len(self.unique_src_node_ids) * len(self.unique_dst_node_ids) <= int(bs.numel()):      # else the set cannot be empty
            self.check()
        return s.cpu().numpy(), d.cpu().numpy()
