"""tpnet_amd -- MI355X (gfx950) implementation of TPNet's temporal-walk-matrix hot path.

Only what the path needs: the HIP kernels + C ABI (csrc/, include/tpnet_hip.h), the ctypes binding (_lib) and the
drop-in `RandomProjectionModule` mirroring /root/reference/models/TPNet.py:9-157.
"""
from .random_projection import RandomProjectionModule  # noqa: F401
from ._lib import TPNetHipError, load as load_library  # noqa: F401
from .sampler import GpuRecentNeighborSampler, GpuNeighborSampler  # noqa: F401
from .negative_sampler import GpuNegativeEdgeSampler, filter_lists_host  # noqa: F401
from .metrics import LinkPredictionMeter, get_link_prediction_metrics, link_prediction_metrics_host  # noqa: F401
from .metrics import LinkRankingMeter, link_ranking_counts_host, link_ranking_metrics_host  # noqa: F401
from .edge_bank import GpuEdgeBank, edge_bank_host, edge_bank_link_prediction  # noqa: F401
from .encoder import TimeEncoder, FeedForwardNet, MLPMixer, TPNetEmbedding, TPNet  # noqa: F401
from .callers import evaluate_link_prediction, evaluate_edge_bank_link_prediction, create_optimizer  # noqa: F401
from .callers import evaluate_link_ranking  # noqa: F401
from .optimizer import DeviceAdam, DeviceSGD, DeviceRMSprop, optimizer_step_host  # noqa: F401

__all__ = ["RandomProjectionModule", "TPNetHipError", "load_library", "TimeEncoder", "FeedForwardNet", "MLPMixer", "TPNetEmbedding",
           "TPNet", "GpuRecentNeighborSampler", "GpuNeighborSampler", "GpuNegativeEdgeSampler", "LinkPredictionMeter",
           "get_link_prediction_metrics", "link_prediction_metrics_host", "evaluate_link_prediction", "GpuEdgeBank", "edge_bank_host",
           "edge_bank_link_prediction", "evaluate_edge_bank_link_prediction", "create_optimizer", "DeviceAdam", "DeviceSGD",
           "DeviceRMSprop", "optimizer_step_host", "LinkRankingMeter", "link_ranking_metrics_host", "link_ranking_counts_host", "filter_lists_host", "evaluate_link_ranking"]
