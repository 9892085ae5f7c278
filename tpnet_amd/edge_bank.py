"""Device-side EdgeBank, the memorisation baseline (C ABI: tpnet_edgebank_build / tpnet_edgebank_predict, csrc/edgebank.hip).

Drop-in for the reference's `edge_bank_link_prediction` (models/EdgeBank.py) with its three `edge_bank_memory_mode` values and two
`time_window_mode` values.  The reference rebuilds a Python set (or a dict of lists) over train + val + test[:batch_start] for every
test batch; here the whole chronological stream is one table in HBM, built once, and a call names how many of its edges are history.

The rule (include/tpnet_hip.h spells it out), for a history of the first h edges and a query pair with c occurrences among them, the
latest at position p: c == 0 predicts 0; 'unlimited_memory' predicts 1; 'time_window_memory' predicts 1 iff t[p] >= window_start, with
window_start = np.quantile(t[:h], 1 - proportion) ('fixed_proportion') or t[h - 1] - S / n_present ('repeat_interval': S = the sum of
the repeated edges' mean inter-occurrence intervals, n_present = the distinct edges of the prefix); 'repeat_threshold_memory' predicts
1 iff c >= h / n_present."""
import ctypes as C

import numpy as np
import torch

from . import _lib

_MEMORY = {"unlimited_memory": 0, "time_window_memory": 1, "repeat_threshold_memory": 2}
_WINDOW = {"fixed_proportion": 0, "repeat_interval": 1}


def _modes(edge_bank_memory_mode, time_window_mode):
    """The reference's error texts (models/EdgeBank.py:70, 116); the window mode matters to 'time_window_memory' only, as there."""
    if edge_bank_memory_mode not in _MEMORY:
        raise ValueError(f"Not implemented error for edge_bank_memory_mode {edge_bank_memory_mode}!")
    if edge_bank_memory_mode == "time_window_memory" and time_window_mode not in _WINDOW:
        raise ValueError(f"Not implemented error for time_window_mode {time_window_mode}!")
    return _MEMORY[edge_bank_memory_mode], _WINDOW.get(time_window_mode, 0)


def edge_bank_host(src, dst, t, h, query_src, query_dst, memory_mode="unlimited_memory", window_mode="fixed_proportion",
                   proportion=0.15):
    """The rule in numpy on the first `h` edges of the stream (src, dst, t; t non-decreasing) -> (predictions float64[Q],
    window_start or threshold; -inf for 'unlimited_memory').  This is what the device is held to where no fixture exists.  The
    'repeat_interval' sum runs over the unique edges in (src, dst) order."""
    mem, win = _modes(memory_mode, window_mode)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    t = np.asarray(t, dtype=np.float64)
    h = int(h)
    assert 1 <= h <= len(src) and len(dst) == len(src) == len(t)
    key = (src[:h] << 32) | dst[:h]
    ukey, first, count = np.unique(key, return_index=True, return_counts=True)
    last = h - 1 - np.unique(key[::-1], return_index=True)[1]
    n_present = len(ukey)
    if mem == 0:
        bound = float("-inf")
    elif mem == 2:
        bound = float(h) / float(n_present)
    elif win == 0:
        q = 1 - proportion
        v = (h - 1) * q
        i = int(np.floor(v))
        g = v - np.floor(v)
        a, b = t[min(i, h - 1)], t[min(i + 1, h - 1)]
        bound = float(b - (b - a) * (1 - g) if g >= 0.5 else a + (b - a) * g)
    else:
        rep = count > 1
        S = float(np.sum((t[last[rep]] - t[first[rep]]) / (count[rep] - 1))) if rep.any() else 0.0
        bound = float(t[h - 1] - S / n_present)
    qs, qd = np.asarray(query_src, dtype=np.int64).reshape(-1), np.asarray(query_dst, dtype=np.int64).reshape(-1)
    ok = (qs >= 0) & (qs < 2 ** 31) & (qd >= 0) & (qd < 2 ** 31)
    qkey = np.where(ok, (qs << 32) | qd, -1)
    at = np.minimum(np.searchsorted(ukey, qkey), n_present - 1)
    seen = ok & (ukey[at] == qkey)
    if mem == 0:
        pred = seen
    elif mem == 2:
        pred = seen & (count[at].astype(np.float64) >= bound)
    else:
        pred = seen & (t[last[at]] >= bound)
    return pred.astype(np.float64), bound


class GpuEdgeBank:
    """The whole chronological stream (train ‖ val ‖ test) as one device table; `predict_device(history_len, ...)` answers from the
    memory the reference would build over the first `history_len` edges.  Keywords as in the reference's `edge_bank_link_prediction`.
    The stamps must be non-decreasing (a stream that is not is refused, not sorted).  There is no CPU fallback."""

    def __init__(self, src_node_ids, dst_node_ids, node_interact_times, edge_bank_memory_mode: str = "unlimited_memory",
                 time_window_mode: str = "fixed_proportion", time_window_proportion: float = 0.15, device="cuda:0"):
        self._mem, self._win = _modes(edge_bank_memory_mode, time_window_mode)
        self.edge_bank_memory_mode = edge_bank_memory_mode
        self.time_window_mode = time_window_mode
        self.time_window_proportion = float(time_window_proportion)
        if not 0.0 <= self.time_window_proportion <= 1.0:
            raise ValueError(f"time_window_proportion {time_window_proportion} is outside [0, 1]")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.TPNetHipError("GpuEdgeBank needs a cuda device (no CPU fallback; edge_bank_host is the numpy statement of the rule)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        lib = _lib.load()
        to = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(self.device) \
            if not isinstance(a, torch.Tensor) else a.to(self.device, dt).contiguous()
        src, dst = to(src_node_ids, torch.int64), to(dst_node_ids, torch.int64)
        t = to(node_interact_times, torch.float64)
        self.E = int(src.numel())
        assert self.E > 0 and int(dst.numel()) == self.E and int(t.numel()) == self.E
        nbytes = lib.tpnet_edgebank_bytes(self.E)
        if nbytes == 0:
            raise _lib.TPNetHipError(f"tpnet_hip edgebank_build: {self.E} edges are more than one table holds (2^30)")
        self._buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        counts = (C.c_int64 * 1)()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(lib.tpnet_edgebank_build(self._buf.data_ptr(), nbytes, src.data_ptr(), dst.data_ptr(), t.data_ptr(), self.E, counts,
                                            stream), "edgebank_build (ids in [0, 2^31), stamps non-decreasing)")
        self.num_unique_edges = int(counts[0])
        self._scratch = torch.empty(lib.tpnet_edgebank_scratch_bytes(self.E), dtype=torch.uint8, device=self.device)
        self._window = torch.full((2,), float("nan"), dtype=torch.float64, device=self.device)

    @property
    def table_bytes(self) -> int:
        return int(self._buf.numel())

    def predict_device(self, history_len: int, pos_src: torch.Tensor, pos_dst: torch.Tensor, neg_src: torch.Tensor = None,
                       neg_dst: torch.Tensor = None):
        """-> fp32 device tensor(s) of 0 / 1: one for (pos_src, pos_dst), and a second one when (neg_src, neg_dst) are given; int64
        device tensors in.  At most two launches for both lists; nothing synchronises and nothing is copied to the host.  The scratch
        buffer and the window record are the bank's own: calls belong on one stream."""
        h = int(history_len)
        if not 1 <= h <= self.E:
            raise ValueError(f"history_len {h} is outside [1, {self.E}]")
        lists = [(pos_src, pos_dst)] + ([(neg_src, neg_dst)] if neg_src is not None or neg_dst is not None else [])
        flat = []
        for s, d in lists:
            for v in (s, d):
                if not isinstance(v, torch.Tensor) or v.dtype != torch.int64 or v.device != self.device:
                    raise TypeError(f"predict_device: int64 tensors on {self.device} are expected")
            s, d = s.reshape(-1).contiguous(), d.reshape(-1).contiguous()
            if s.numel() != d.numel():
                raise ValueError("predict_device: one destination per source")
            flat.append((s, d, torch.empty(s.numel(), dtype=torch.float32, device=self.device)))
        if len(flat) == 1:
            flat.append((None, None, None))
        (s0, d0, o0), (s1, d1, o1) = flat
        ptr = lambda v: v.data_ptr() if v is not None and v.numel() else None
        n = lambda v: int(v.numel()) if v is not None else 0
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().tpnet_edgebank_predict(self._buf.data_ptr(), self.E, self._mem, self._win, self.time_window_proportion, h,
                                                      ptr(s0), ptr(d0), n(s0), ptr(o0), ptr(s1), ptr(d1), n(s1), ptr(o1),
                                                      self._scratch.data_ptr(), self._scratch.numel(), self._window.data_ptr(), stream),
                   "edgebank_predict")
        return o0 if o1 is None else (o0, o1)

    def window_device(self) -> torch.Tensor:
        """The last call's record, a float64 device tensor of 2: {window_start, window_end} ('time_window_memory'), {threshold,
        n_present} ('repeat_threshold_memory'), {-inf, t[h - 1]} ('unlimited_memory'); NaN before the first call.  The bank's own
        buffer: the next call overwrites it."""
        return self._window


def edge_bank_link_prediction(history_data, positive_edges: tuple, negative_edges: tuple, edge_bank_memory_mode: str,
                              time_window_mode: str, time_window_proportion: float, device="cuda:0"):
    """The reference's function (models/EdgeBank.py:94-121), its signature and return types: `history_data` has `src_node_ids`,
    `dst_node_ids` and `node_interact_times`; -> (positive_probabilities, negative_probabilities), two float64 numpy arrays.  Builds a
    bank over the history and asks with all of it: a script that calls this per batch pays the build per batch (and a
    synchronisation, by nature) -- `GpuEdgeBank` over the whole stream is the path that does not."""
    bank = GpuEdgeBank(history_data.src_node_ids, history_data.dst_node_ids, history_data.node_interact_times, edge_bank_memory_mode,
                       time_window_mode, time_window_proportion, device=device)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int64).to(bank.device)
    pos, neg = bank.predict_device(bank.E, dev(positive_edges[0]), dev(positive_edges[1]), dev(negative_edges[0]), dev(negative_edges[1]))
    return pos.cpu().numpy().astype(np.float64), neg.cpu().numpy().astype(np.float64)
