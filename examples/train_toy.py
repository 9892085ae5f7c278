#!/usr/bin/env python3
"""Toy temporal link prediction with the drop-in pieces, in the reference's batch order
(train_link_prediction.py:246-386): reset at epoch start; per batch: negatives, encoder readouts (neighbour x src/dst
relative encodings), decoder readouts, update, the loss, then the optimiser step -- `callers.train_link_prediction_epoch`.  The
loss is the device meter's (`LinkPredictionMeter.add_training`): every batch's loss, average precision and ROC-AUC are logged on
the device and read once per epoch; nothing synchronises for them inside the loop.  The encoder here is a small stand-in for
the reference's MLP-Mixer (out of scope): mean over the K neighbours of an MLP of their relative encodings.

    python examples/train_toy.py            # needs a GPU; ~10 s
    python examples/train_toy.py --fused-decoder      # the same with LinkPredictor_v1.fused = "f32"
    python examples/train_toy.py --device-optimizer   # the same with Adam's step in one launch (tpnet_amd.DeviceAdam)
"""
import os, sys, time
import numpy as np, torch
import torch.nn as nn
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tpnet_amd import RandomProjectionModule
from tpnet_amd.callers import LinkPredictor_v1, RandomNegativeSampler, train_link_prediction_epoch
from tpnet_amd.sampler import GpuRecentNeighborSampler
from tpnet_amd.stream import synthetic_stream

dev = "cuda:0"
U, I, E, B, K, D = 600, 200, 24000, 200, 10, 32
src, dst, t, N = synthetic_stream(U, I, E, 2.0e6, seed=0)
torch.manual_seed(0); np.random.seed(0)
rp = RandomProjectionModule(node_num=N, edge_num=E, dim_factor=10, num_layer=3, time_decay_weight=1e-6, device=dev,
                            use_matrix=False, beginning_time=np.float64(t[0]), not_scale=False, enforce_dim=64).to(dev)
rp.fused_mlp = True                                   # self.mlp on the bf16 matrix cores
enc_mlp = nn.Sequential(nn.Linear(2 * 64, D), nn.ReLU(), nn.Linear(D, D)).to(dev)
decoder = LinkPredictor_v1(input_dim1=D, input_dim2=D, hidden_dim=D, output_dim=1, random_projections=rp,
                           not_encode=False).to(dev)
if "--fused-decoder" in sys.argv[1:]:                 # opt-in: the decoder's two layers in HIP, fp32 class, forward and backward
    decoder.fused = "f32"
params = list(enc_mlp.parameters()) + list(decoder.parameters())       # decoder.parameters() includes rp.mlp
Adam = torch.optim.Adam
if "--device-optimizer" in sys.argv[1:]:              # opt-in: every tensor's Adam step in one launch, same state_dict as torch's
    from tpnet_amd import DeviceAdam as Adam
opt = Adam([p for p in params if p.requires_grad], lr=2e-3)
sampler = GpuRecentNeighborSampler(src, dst, t, device=dev)
negs = RandomNegativeSampler(src, dst)
encoder = lambda feats, node_ids, times: enc_mlp(feats).mean(dim=1)    # [2B, K, 128] -> [2B, D]

for epoch in range(3):
    t0 = time.perf_counter()
    losses, metrics = train_link_prediction_epoch(rp, sampler, negs, src, dst, t, B, K, encoder, decoder, opt)   # one read, at the end
    dt = time.perf_counter() - t0
    half = len(losses) // 2
    print(f"epoch {epoch}: loss {np.mean(losses[half:]):.4f}  AP {np.mean([m['average_precision'] for m in metrics[half:]]):.3f}"
          f"  AUC {np.mean([m['roc_auc'] for m in metrics[half:]]):.3f}  (second half of {len(losses)} batches; first batch: loss "
          f"{losses[0]:.4f} AP {metrics[0]['average_precision']:.3f} AUC {metrics[0]['roc_auc']:.3f};"
          f" {E / dt / 1e3:.0f} k edges/s end to end, python loop)")
