"""TPNet's encoder as a drop-in (models/TPNet.py:160-416, models/modules.py:8-42): `TimeEncoder`, `FeedForwardNet`, `MLPMixer`,
`TPNetEmbedding` and `TPNet`, restated the way callers.py restates `LinkPredictor_v1` -- the reference's constructor keywords,
attributes, method names and state-dict keys (the shared `random_projections` and `time_encoder` registered under two prefixes
each), so `TPNet(...)` at train_link_prediction.py:166 can be this class.

What differs is where the work runs:
* sampler -> readout: with a `GpuRecentNeighborSampler` the neighbour ids, edge ids and times never leave the device
  (`sample_device` -> `RandomProjectionModule.get_pair_wise_feature_anchored`); a host sampler's three [2B, K] arrays are
  copied to the device once.  The call is one launch on rows of 36..160 floats, and on rows of 164..512 floats where
  `tpnet_encoder_fused_supported` says so (csrc/anchored_feature.hip; else the anchored walk and `rp.mlp`'s dense layers as two
  launches).  Row widths the anchored readout does not serve (d < 36, d > 512, d % 4 != 0) take the general pair
  readout and `rp.mlp` as the stock torch layers.
* the input stage behind the readout (gathers, time encoding, concat, `projection_layer`; TPNet.py:297-330): under
  `torch.no_grad()` / inference mode, with the module on the GPU, `fused_input` set and a served shape, ONE launch on the matrix
  cores (tpnet_amd/fused_input.py, csrc/encoder_input.hip) that never writes the [2B, K, Din] concat.  When gradients are recorded
  the torch layers serve, and autograd reaches `projection_layer`, the time encoder and `rp.mlp` as in the reference.
* with `TPNetEmbedding.fused_input_training` set (it defaults to False), when a gradient IS recorded, with the module on the GPU,
  relative encodings present in a served shape (the forward's, with time_feat_dim + random_feature_dim <= 256), contiguous float32
  Parameters and raw feature tables that take no gradient, the input stage is ONE launch forward and TWO backward on the matrix
  cores in the project's fp32 class (fused_input.encoder_input_train, csrc/encoder_input_train.hip).  The forward stores one bit
  per (row, hidden unit), the ReLU's decision; the concat and the hidden layer are not kept, the backward rebuilds the concat from
  the sources in a workspace it allocates and frees.  Gradients reach `projection_layer`, the time encoder and, through the
  relative encodings, `rp.mlp`.  It combines freely with the other switches.
* the MLP-Mixer layers are stock torch unless `TPNetEmbedding.fused_mixer` is set (it defaults to False): then, under
  `torch.no_grad()` / inference mode, on contiguous float32 embeddings on the GPU, with no dropout active (eval mode, or dropout 0)
  and a served shape, every layer is TWO launches (tpnet_amd/fused_mixer.py, csrc/mixer.hip): token mixing in exact fp32, channel
  mixing on the matrix cores in the project's fp32 class.  Any other call runs `mlp_mixer(embeddings)` as before.
* with `TPNetEmbedding.fused_token_training` set (it defaults to False), when a gradient IS recorded, on contiguous float32
  embeddings on the GPU, with a served shape and both dropouts of the token FFN at the same p < 1, the token-mixing half of every
  layer is ONE launch forward and ONE backward in exact fp32 (fused_mixer.token_train, csrc/mixer_token_train.hip); the backward
  recomputes the forward, so the layer's input is the only activation kept.  In train mode its dropout masks follow nn.Dropout's
  probabilities but come from a counter-based generator on the device, keyed from torch's default CPU generator
  (torch.manual_seed reproduces a run): they are NOT torch's dropout stream.
* with `TPNetEmbedding.fused_channel_training` set (it defaults to False), under the same conditions (the channel FFN's two
  dropouts at the same p < 1), the channel-mixing half of every layer is ONE launch forward and TWO backward on the matrix
  cores in the project's fp32 class (fused_mixer.channel_train, csrc/mixer_channel_train.hip); the backward recomputes the forward
  in a workspace it allocates and frees, so the half's input is the only activation kept.  Its dropout masks are again
  nn.Dropout's probabilities from the device's generator, NOT torch's dropout stream.  The two switches combine freely: either
  half of a layer is fused or stock torch.
* the mean over the K tokens is stock torch.
"""
import numpy as np
import torch
import torch.nn as nn

from . import fused_input as _fi
from . import fused_mixer as _fm


class TimeEncoder(nn.Module):
    """cos(Linear(1, time_dim)) with the reference's initial weights 1 / 10^linspace(0, 9, time_dim) and zero bias
    (models/modules.py:8-42)."""

    def __init__(self, time_dim: int, parameter_requires_grad: bool = True):
        super().__init__()
        self.time_dim = time_dim
        self.w = nn.Linear(1, time_dim)
        self.w.weight = nn.Parameter(torch.from_numpy(1 / 10 ** np.linspace(0, 9, time_dim, dtype=np.float32)).reshape(time_dim, -1))
        self.w.bias = nn.Parameter(torch.zeros(time_dim))
        if not parameter_requires_grad:
            self.w.weight.requires_grad = False
            self.w.bias.requires_grad = False

    def forward(self, timestamps: torch.Tensor):
        """timestamps [batch, seq_len] -> [batch, seq_len, time_dim]"""
        return torch.cos(self.w(timestamps.unsqueeze(dim=2)))


class FeedForwardNet(nn.Module):
    """Linear -> GELU -> Dropout -> Linear -> Dropout (models/TPNet.py:341-368); keys ffn.0.*, ffn.3.*."""

    def __init__(self, input_dim: int, dim_expansion_factor: float, dropout: float = 0.0):
        super().__init__()
        self.input_dim = input_dim
        self.dim_expansion_factor = dim_expansion_factor
        self.dropout = dropout
        hidden = int(dim_expansion_factor * input_dim)
        self.ffn = nn.Sequential(nn.Linear(in_features=input_dim, out_features=hidden), nn.GELU(), nn.Dropout(dropout),
                                 nn.Linear(in_features=hidden, out_features=input_dim), nn.Dropout(dropout))

    def forward(self, x: torch.Tensor):
        return self.ffn(x)


class MLPMixer(nn.Module):
    """Token mixing then channel mixing, each LayerNorm -> FeedForwardNet -> residual (models/TPNet.py:371-416)."""

    def __init__(self, num_tokens: int, num_channels: int, token_dim_expansion_factor: float = 0.5,
                 channel_dim_expansion_factor: float = 4.0, dropout: float = 0.0):
        super().__init__()
        self.token_norm = nn.LayerNorm(num_tokens)
        self.token_feedforward = FeedForwardNet(input_dim=num_tokens, dim_expansion_factor=token_dim_expansion_factor, dropout=dropout)
        self.channel_norm = nn.LayerNorm(num_channels)
        self.channel_feedforward = FeedForwardNet(input_dim=num_channels, dim_expansion_factor=channel_dim_expansion_factor,
                                                  dropout=dropout)

    def forward(self, input_tensor: torch.Tensor):
        """[batch, num_tokens, num_channels] -> the same shape"""
        hidden_tensor = self.token_norm(input_tensor.permute(0, 2, 1))
        hidden_tensor = self.token_feedforward(hidden_tensor).permute(0, 2, 1)
        output_tensor = hidden_tensor + input_tensor
        hidden_tensor = self.channel_norm(output_tensor)
        hidden_tensor = self.channel_feedforward(hidden_tensor)
        return hidden_tensor + output_tensor


def _on(x, dev, dtype):
    """A host array or a tensor as a contiguous tensor of `dtype` on `dev` (one copy at most)."""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype={torch.int64: np.int64, torch.float64: np.float64}[dtype]))
    return x.to(device=dev, dtype=dtype).contiguous()


class TPNetEmbedding(nn.Module):
    """The embedding module (models/TPNet.py:236-338): projection_layer over [node | time | edge | r(w|u), r(w|v)] of every
    sampled neighbour, `num_layers` MLP-Mixers over the K tokens, mean over the tokens.  Same constructor keywords and state-dict
    keys (time_encoder.*, random_projections.*, projection_layer.{0,2}.*, mlp_mixers.*)."""

    # the one-launch input stage when no gradient is recorded: measured against the stock-torch expression at B = 1000, K = 20
    # (profiles/encoder_input.md)
    fused_input = True
    # the two-launch MLP-Mixer layers when no gradient is recorded and no dropout is active: opt-in (profiles/mixer.md; the
    # channel FFN is the fp32 class, and the bound of the end-to-end fixture test with it on is a measurement of its own)
    fused_mixer = False
    # the token-mixing half of every mixer as one launch forward and one backward when a gradient IS recorded: opt-in
    # (profiles/mixer_token_training.md); its dropout masks are the device generator's, not torch's stream
    fused_token_training = False
    # the channel-mixing half of every mixer as one launch forward and two backward on the matrix cores (fp32 class) when a
    # gradient IS recorded: opt-in (profiles/mixer_channel_training.md); its dropout masks are the device generator's too
    fused_channel_training = False
    # the input stage as one launch forward (that records the ReLU's decisions, one bit per hidden unit) and two backward on the
    # matrix cores (fp32 class) when a gradient IS recorded: opt-in (profiles/encoder_input_training.md); the concat and the
    # hidden layer are not kept for the backward
    fused_input_training = False

    def __init__(self, node_raw_features: torch.Tensor, edge_raw_features: torch.Tensor, neighbor_sampler, time_encoder: nn.Module,
                 node_feat_dim: int, edge_feat_dim: int, time_feat_dim: int, num_layers: int, num_neighbors: int, dropout: float,
                 random_projections):
        super().__init__()
        self.node_raw_features = node_raw_features
        self.edge_raw_features = edge_raw_features
        self.neighbor_sampler = neighbor_sampler
        self.time_encoder = time_encoder
        self.node_feat_dim = node_feat_dim
        self.edge_feat_dim = edge_feat_dim
        self.time_feat_dim = time_feat_dim
        self.num_layers = num_layers
        self.num_neighbors = num_neighbors
        self.dropout = dropout
        self.random_projections = random_projections
        self.random_feature_dim = 0 if random_projections is None else random_projections.pair_wise_feature_dim * 2
        self.projection_layer = nn.Sequential(
            nn.Linear(node_feat_dim + edge_feat_dim + time_feat_dim + self.random_feature_dim, self.node_feat_dim * 2), nn.ReLU(),
            nn.Linear(self.node_feat_dim * 2, self.node_feat_dim))
        self.mlp_mixers = nn.ModuleList([
            MLPMixer(num_tokens=self.num_neighbors, num_channels=self.node_feat_dim, token_dim_expansion_factor=0.5,
                     channel_dim_expansion_factor=4.0, dropout=self.dropout) for _ in range(self.num_layers)])

    def compute_node_temporal_embeddings(self, node_ids: np.ndarray, src_node_ids: np.ndarray, dst_node_ids: np.ndarray,
                                         node_interact_times: np.ndarray):
        """Embeddings [len(node_ids), node_feat_dim] of `node_ids` at `node_interact_times`; src_node_ids / dst_node_ids are the
        edge's two ends per row (the anchors of the relative encodings).  Sampler, readout, then embed_from_features
        (TPNet.py:280-338)."""
        dev = self.node_raw_features.device
        K = self.num_neighbors
        sampler = self.neighbor_sampler
        tq = _on(node_interact_times, dev, torch.float64)
        if dev.type == "cuda" and hasattr(sampler, "sample_device"):
            neigh, eids, tn = sampler.sample_device(_on(node_ids, dev, torch.int64), tq, K, with_edges=True)
        else:
            neigh, eids, tn = sampler.get_historical_neighbors(node_ids=node_ids, node_interact_times=node_interact_times,
                                                               num_neighbors=K)
            neigh, eids, tn = _on(neigh, dev, torch.int64), _on(eids, dev, torch.int64), _on(tn, dev, torch.float64)
        feats = None
        rp = self.random_projections
        if rp is not None:
            # TPNet.py:313-316, [2 n K, F]: every neighbour against the row's two anchors
            # (the module says which widths its anchored call serves: dim % 4 == 0 in 36..512, and with its `rows8_readout` set the
            # default rule's 110 / 130 / 150; at num_layer 1, 2, 4 its `layers_readout` puts the readout of rows of 36..160 floats on
            # the matrix cores, K >= 4)
            if dev.type == "cuda" and hasattr(rp, "get_pair_wise_feature_anchored") and (
                    rp.anchored_call_served(neigh.shape[0], K) if hasattr(rp, "anchored_call_served")
                    else getattr(rp, "engine_dim", rp.dim) % 4 == 0 and 36 <= getattr(rp, "engine_dim", rp.dim) <= 512):
                feats = rp.get_pair_wise_feature_anchored(neigh, src_node_ids, dst_node_ids)
            else:
                # row widths the anchored readout does not serve (or another module): the general pair readout, then self.mlp as
                # the stock torch layers -- true fp32 forward and backward, where the anchored path's dense layers are the fp32
                # class on the matrix cores (2^-16 per product)
                a1, a2 = _on(src_node_ids, dev, torch.int64), _on(dst_node_ids, dev, torch.int64)
                u, v = neigh.reshape(-1).repeat(2), torch.cat([a1.repeat_interleave(K), a2.repeat_interleave(K)])
                if dev.type == "cuda" and hasattr(rp, "pair_gram"):
                    feats = rp.mlp(rp.pair_gram(u, v))
                else:                                                    # (a host module takes the reference's numpy arrays)
                    feats = rp.get_pair_wise_feature(src_node_ids=u.cpu().numpy(), dst_node_ids=v.cpu().numpy())
        return self.embed_from_features(neigh, eids, tn, tq, feats)

    def _input_stage_prepared(self, dev, pair_features, backward=False):
        """fused_input.prepared of projection_layer where what both routes ask holds -- module on the GPU, relative encodings
        present, `random_feature_dim` even and twice their width -- else None."""
        if dev.type != "cuda" or pair_features is None or self.random_feature_dim % 2 \
                or pair_features.shape[1] * 2 != self.random_feature_dim:
            return None
        return _fi.prepared(self.projection_layer, self.node_feat_dim, self.time_feat_dim, self.edge_feat_dim,
                            self.random_feature_dim // 2, backward=backward)

    def _fused_prep(self, dev, pair_features):
        """The prepared weight image if the one-launch input stage serves this call, else None: no gradient recorded, module on
        the GPU, `fused_input` set, relative encodings present and a shape tpnet_encoder_input_supported accepts."""
        if torch.is_grad_enabled() or not self.fused_input:
            return None
        return self._input_stage_prepared(dev, pair_features)

    def _fused_input_training(self, dev, pair_features):
        """Whether fused_input.encoder_input_train serves this call: `fused_input_training` set, a gradient recorded, module on the
        GPU, relative encodings present (contiguous float32) in a shape the forward AND the backward serve, the Parameters of
        projection_layer and of the time encoder contiguous float32, and raw feature tables that take no gradient."""
        if not self.fused_input_training or not torch.is_grad_enabled() or pair_features is None:
            return False
        if pair_features.dtype != torch.float32 or not pair_features.is_contiguous():
            return False
        if self.node_raw_features.requires_grad or self.edge_raw_features.requires_grad:
            return False
        w = getattr(self.time_encoder, "w", None)
        if not isinstance(w, nn.Linear) or w.bias is None:
            return False
        if not all(p.is_cuda and p.is_contiguous() and p.dtype == torch.float32 for p in (w.weight, w.bias)):
            return False
        return self._input_stage_prepared(dev, pair_features, backward=True) is not None

    def _fused_mixer_prep(self, mixer, x):
        """The prepared channel image if the two-launch layer serves `mixer` on `x`, else None: `fused_mixer` set, no gradient
        recorded, x contiguous float32 on the GPU, no dropout active (eval mode, or every dropout of the mixer 0 -- a no_grad call in
        train mode keeps torch's dropout) and a shape tpnet_mixer_supported accepts."""
        if not self.fused_mixer or torch.is_grad_enabled() or not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
            return None
        if self.training:
            ls = _fm.layers_of(mixer)
            if ls is None or ls.dropout != 0:
                return None
        return _fm.prepared(mixer)

    def _fused_training_rate(self, switch, ffn, mixer, x):
        """The dropout rate at which a half of `mixer` (its FeedForwardNet's layers `ffn`) runs as token_train / channel_train on
        `x`, else None: `switch` set, a gradient recorded, x contiguous float32 on the GPU, a shape tpnet_mixer_supported accepts
        and both dropouts of `ffn` at the same p < 1.  In eval mode the rate is 0."""
        if not switch or not torch.is_grad_enabled() or not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
            return None
        if _fm.layers_of(mixer) is None:
            return None
        p = float(ffn[2].p)
        if p != float(ffn[4].p) or not 0.0 <= p < 1.0 or not _fm.supported(mixer):
            return None
        return p if self.training else 0.0

    def embed_from_features(self, neighbor_node_ids, neighbor_edge_ids, neighbor_times, node_interact_times, pair_features):
        """The tail behind the readout (TPNet.py:297-338).  neighbor_node_ids / neighbor_edge_ids int64 [n, K], neighbor_times
        float64 [n, K], node_interact_times float64 [n] (host arrays or tensors), pair_features [2 n K, F] in the reference's row
        order (all first anchors, then all second anchors) or None without relative encodings."""
        dev = self.node_raw_features.device
        neigh, eids = _on(neighbor_node_ids, dev, torch.int64), _on(neighbor_edge_ids, dev, torch.int64)
        tn, tq = _on(neighbor_times, dev, torch.float64), _on(node_interact_times, dev, torch.float64)
        n, K = neigh.shape
        prep = self._fused_prep(dev, pair_features)
        if prep is not None:
            w = self.time_encoder.w
            embeddings = _fi.encoder_input(prep, self.node_raw_features, self.edge_raw_features, neigh, eids, tn, tq, w.weight, w.bias,
                                           pair_features)
        elif self._fused_input_training(dev, pair_features):
            embeddings = _fi.encoder_input_train(self.projection_layer, self.time_encoder, self.node_raw_features, self.edge_raw_features,
                                                 neigh, eids, tn, tq, pair_features)
        else:
            neighbor_node_features = self.node_raw_features[neigh]
            # the delta in f64, cast to f32, then log(x + 1) (TPNet.py:299-301)
            neighbor_delta_times = torch.log((tq[:, None] - tn).float() + 1.0)
            neighbor_time_features = self.time_encoder(neighbor_delta_times)
            neighbor_edge_features = self.edge_raw_features[eids]
            parts = [neighbor_node_features, neighbor_time_features, neighbor_edge_features]
            if pair_features is not None:
                half = n * K
                parts.append(torch.cat([pair_features[:half], pair_features[half:]], dim=1).reshape(n, K, -1))
            embeddings = self.projection_layer(torch.cat(parts, dim=2))
        # (TPNet.py:332 calls masked_fill out of place and drops the result: pad neighbours are NOT masked)
        for mlp_mixer in self.mlp_mixers:
            if self.fused_token_training or self.fused_channel_training:
                rate = self._fused_training_rate(self.fused_token_training, mlp_mixer.token_feedforward.ffn, mlp_mixer, embeddings)
                crate = self._fused_training_rate(self.fused_channel_training, mlp_mixer.channel_feedforward.ffn, mlp_mixer, embeddings)
            else:
                rate = crate = None
            if rate is not None or crate is not None:
                if rate is not None:
                    tokens = _fm.token_train(mlp_mixer, embeddings, rate)
                else:
                    hidden = mlp_mixer.token_feedforward(mlp_mixer.token_norm(embeddings.permute(0, 2, 1))).permute(0, 2, 1)
                    tokens = (hidden + embeddings).contiguous()
                if crate is not None:
                    embeddings = _fm.channel_train(mlp_mixer, tokens, crate)
                else:
                    embeddings = mlp_mixer.channel_feedforward(mlp_mixer.channel_norm(tokens)) + tokens
                continue
            prep = self._fused_mixer_prep(mlp_mixer, embeddings)
            embeddings = mlp_mixer(embeddings) if prep is None else _fm.mixer_forward(prep, mlp_mixer, embeddings)
        return torch.mean(embeddings, dim=1)

    def check_device_errors(self):
        """Raise IndexError if a fused input-stage launch met a neighbour or edge id outside the raw feature tables since the last
        check (such a row read row 0 instead, where the torch layers' gathers would have faulted).  Synchronises the stream: meant
        for once per evaluation pass, not per batch."""
        prep = _fi.cached(self.projection_layer)
        if prep is not None:
            _fi.check_errors(prep)


class TPNet(nn.Module):
    """models/TPNet.py:160-233: holds the raw features, the shared random projections and time encoder, and the embedding
    module; state-dict keys random_projections.*, time_encoder.*, embedding_module.*."""

    def __init__(self, node_raw_features: np.ndarray, edge_raw_features: np.ndarray, neighbor_sampler, time_feat_dim: int,
                 dropout: float, random_projections, num_layers: int, num_neighbors: int, device: str):
        super().__init__()
        self.node_raw_features = torch.from_numpy(node_raw_features.astype(np.float32)).to(device)
        self.edge_raw_features = torch.from_numpy(edge_raw_features.astype(np.float32)).to(device)
        self.node_feat_dim = self.node_raw_features.shape[1]
        self.edge_feat_dim = self.edge_raw_features.shape[1]
        self.time_feat_dim = time_feat_dim
        self.dropout = dropout
        self.device = device
        self.num_nodes = self.node_raw_features.shape[0]        # including the padded node
        self.random_projections = random_projections
        self.time_encoder = TimeEncoder(time_dim=time_feat_dim)
        self.embedding_module = TPNetEmbedding(node_raw_features=self.node_raw_features, edge_raw_features=self.edge_raw_features,
                                               neighbor_sampler=neighbor_sampler, time_encoder=self.time_encoder,
                                               node_feat_dim=self.node_feat_dim, edge_feat_dim=self.edge_feat_dim,
                                               time_feat_dim=self.time_feat_dim, num_layers=num_layers, num_neighbors=num_neighbors,
                                               dropout=self.dropout, random_projections=self.random_projections)

    def compute_src_dst_node_temporal_embeddings(self, src_node_ids: np.ndarray, dst_node_ids: np.ndarray,
                                                 node_interact_times: np.ndarray):
        """(src embeddings, dst embeddings), each [batch, node_feat_dim] (TPNet.py:206-222)."""
        node_embeddings = self.embedding_module.compute_node_temporal_embeddings(
            node_ids=np.concatenate([src_node_ids, dst_node_ids]), src_node_ids=np.tile(src_node_ids, 2),
            dst_node_ids=np.tile(dst_node_ids, 2), node_interact_times=np.tile(node_interact_times, 2))
        return node_embeddings[:len(src_node_ids)], node_embeddings[len(src_node_ids):]

    def check_device_errors(self):
        """embedding_module.check_device_errors(): IndexError if a fused input-stage launch met an id outside the raw feature tables."""
        self.embedding_module.check_device_errors()

    def set_neighbor_sampler(self, neighbor_sampler):
        """TPNet.py:224-233: the random strategies restart their seeded state."""
        self.embedding_module.neighbor_sampler = neighbor_sampler
        if getattr(neighbor_sampler, "sample_neighbor_strategy", "recent") in ["uniform", "time_interval_aware"]:
            assert neighbor_sampler.seed is not None
            neighbor_sampler.reset_random_state()
