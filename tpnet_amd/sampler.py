"""Device-side neighbour samplers (SURVEY.md §8 f-3, C ABI: tpnet_sampler_build / tpnet_sample_recent / tpnet_sample_random).

Drop-in for what TPNet's encoder asks of the reference's `NeighborSampler` built by `get_neighbor_sampler(data,
'recent')` (utils/utils.py:82-224, 293-312; call site models/TPNet.py:291-294): the same
`get_historical_neighbors(node_ids, node_interact_times, num_neighbors)` -> three [n, K] arrays.  The adjacency lives
in HBM as one CSR; a query batch is one kernel launch instead of a Python loop over the nodes.  `GpuNeighborSampler` adds the
reference's 'uniform' and 'time_interval_aware' strategies on the same CSR."""
import ctypes as C

import numpy as np
import torch

from . import _lib


class GpuRecentNeighborSampler:
    sample_neighbor_strategy = "recent"      # attributes TPNet.set_neighbor_sampler looks at (models/TPNet.py:223-232)
    seed = None

    def __init__(self, src_node_ids, dst_node_ids, node_interact_times, edge_ids=None, device="cuda:0",
                 num_nodes: int = None):
        lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.TPNetHipError("GpuRecentNeighborSampler needs a cuda device (no CPU fallback)")
        to = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(self.device) \
            if not isinstance(a, torch.Tensor) else a.to(self.device, dt).contiguous()
        src, dst = to(src_node_ids, torch.int64), to(dst_node_ids, torch.int64)
        t = to(node_interact_times, torch.float64)
        eid = to(edge_ids, torch.int64) if edge_ids is not None else None
        self.E = int(src.numel())
        if num_nodes is None:
            num_nodes = (int(max(src.max().item(), dst.max().item())) + 1) if self.E else 1
        self.num_nodes = int(num_nodes)
        nbytes = lib.tpnet_sampler_bytes(self.E, self.num_nodes)
        self._buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(lib.tpnet_sampler_build(self._buf.data_ptr(), nbytes, src.data_ptr(), dst.data_ptr(), t.data_ptr(),
                                           eid.data_ptr() if eid is not None else None, self.E, self.num_nodes, stream),
                   "sampler_build")
        self._keep = (src, dst, t, eid)      # inputs must outlive the asynchronous build

    def sample_device(self, node_ids: torch.Tensor, times: torch.Tensor, num_neighbors: int, with_edges: bool = True):
        """node_ids int64 [n], times float64 [n] on the device -> (ids, edge_ids, times), each [n, K] on the device."""
        assert num_neighbors > 0, "Number of sampled neighbors for each node should be greater than 0!"
        n = int(node_ids.numel())
        ids = torch.empty((n, num_neighbors), dtype=torch.int64, device=self.device)
        eids = torch.empty((n, num_neighbors), dtype=torch.int64, device=self.device) if with_edges else None
        ts = torch.empty((n, num_neighbors), dtype=torch.float64, device=self.device) if with_edges else None
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().tpnet_sample_recent(self._buf.data_ptr(), self.E, self.num_nodes, node_ids.data_ptr(),
                                                   times.data_ptr(), n, num_neighbors, ids.data_ptr(),
                                                   eids.data_ptr() if with_edges else None,
                                                   ts.data_ptr() if with_edges else None, stream), "sample_recent")
        return ids, eids, ts

    def get_historical_neighbors(self, node_ids: np.ndarray, node_interact_times: np.ndarray, num_neighbors: int = 20):
        """The reference's signature and return types (numpy [n, K] x 3): utils/utils.py:160-224."""
        nid = torch.as_tensor(np.ascontiguousarray(node_ids), dtype=torch.int64).to(self.device)
        tq = torch.as_tensor(np.ascontiguousarray(node_interact_times), dtype=torch.float64).to(self.device)
        ids, eids, ts = self.sample_device(nid, tq, num_neighbors)
        return ids.cpu().numpy(), eids.cpu().numpy(), ts.cpu().numpy()


class GpuNeighborSampler(GpuRecentNeighborSampler):
    """The reference's three `sample_neighbor_strategy` values on the device (utils/utils.py:82-224): 'recent' is the parent;
    'uniform' and 'time_interval_aware' draw K positions with replacement from the interactions before the query time and return
    them sorted by time (C ABI: tpnet_sampler_build_weights / tpnet_sample_random, on the parent's CSR).

    The draws come from a counter-based generator (Philox4x32-10) keyed by the seed and indexed by (call, row, slot): the same
    seed replays the same neighbours, `reset_random_state()` restarts the sequence of calls, and a query's draws do not depend on
    the other rows of its call.  They follow the reference's probabilities but are NOT numpy's `RandomState.choice` stream, which
    is sequential and cannot be produced by parallel threads."""

    def __init__(self, src_node_ids, dst_node_ids, node_interact_times, edge_ids=None, device="cuda:0", num_nodes: int = None,
                 sample_neighbor_strategy: str = "uniform", time_scaling_factor: float = 0.0, seed: int = None):
        if sample_neighbor_strategy not in ("recent", "uniform", "time_interval_aware"):
            raise ValueError(f"Not implemented error for sample_neighbor_strategy {sample_neighbor_strategy}!")
        super().__init__(src_node_ids, dst_node_ids, node_interact_times, edge_ids=edge_ids, device=device, num_nodes=num_nodes)
        self.sample_neighbor_strategy = sample_neighbor_strategy
        self.time_scaling_factor = float(time_scaling_factor)
        self.seed = seed
        # an unseeded reference sampler draws from numpy's global generator (utils/utils.py:195-196): one 64-bit key from it
        self._key = int(seed) & (2 ** 64 - 1) if seed is not None else int(np.random.randint(0, 2 ** 64, dtype=np.uint64))
        self._calls = 0
        self._weights = None
        if sample_neighbor_strategy == "time_interval_aware":
            lib = _lib.load()
            nbytes = lib.tpnet_sampler_weights_bytes(self.E)
            self._weights = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(lib.tpnet_sampler_build_weights(self._buf.data_ptr(), self.E, self.num_nodes, self.time_scaling_factor,
                                                       self._weights.data_ptr(), nbytes, stream), "sampler_build_weights")

    def reset_random_state(self):
        """utils/utils.py:285-290: the next `sample_device` call is call 0 of the seed again."""
        self._calls = 0

    def sample_device(self, node_ids: torch.Tensor, times: torch.Tensor, num_neighbors: int, with_edges: bool = True):
        """As the parent's; every call of a random strategy advances the call index, whatever its size."""
        if self.sample_neighbor_strategy == "recent":
            return super().sample_device(node_ids, times, num_neighbors, with_edges)
        n, K = int(node_ids.numel()), int(num_neighbors)
        shape = (n, max(K, 0))
        ids = torch.empty(shape, dtype=torch.int64, device=self.device)
        eids = torch.empty(shape, dtype=torch.int64, device=self.device) if with_edges else None
        ts = torch.empty(shape, dtype=torch.float64, device=self.device) if with_edges else None
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        call = self._calls & 0xFFFFFFFF
        _lib.check(_lib.load().tpnet_sample_random(self._buf.data_ptr(), self._weights.data_ptr() if self._weights is not None else None,
                                                   self.E, self.num_nodes, node_ids.data_ptr(), times.data_ptr(), n, K, self._key,
                                                   call, ids.data_ptr(), eids.data_ptr() if with_edges else None,
                                                   ts.data_ptr() if with_edges else None, stream), "sample_random")
        self._calls += 1
        return ids, eids, ts
