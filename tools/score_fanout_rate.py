#!/usr/bin/env python3
"""Developer tool: one source against many candidates, the one-launch kernel against the composition, timed on the GPU with the
variants alternating in one process after every shape has been warmed.

  variants  (a) the composition: forward_one_to_many / forward_one_to_all with fused = False, slices of 2^18 pairs
            (b) the same with fused = "f32" (the decoder's fp32-class kernel behind the features)
            (c) tpnet_score_one_to_many (fused_scores = True)
  shapes    C2-shaped table (d = 128), B = 200 sources against all candidates: the id range [1, N)
            the same table, B = 1000, a list of C = 100 candidates per source (the existing ranking shape)
            C3-shaped table (d = 256), B = 200 against all candidates

Before a shape is timed, (c)'s and (a)'s logits are held to the float64 restatement on the kernel's own features within the bound of
tests/test_score_fanout.py (per stage 4e-5 of the magnitudes + 1e-6 max|want|), in row chunks, in float64 on the GPU.

    tools/score_fanout_rate.py [--reps 11] [--inner 50] [--kernel-only] [--json OUT]

One sample = HIP events around `inner` calls, then a synchronise; per case the median and the range over the samples, in us per call.
--kernel-only: a few calls of (c) per shape and nothing else (for a kernel trace of its own)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import tpnet_amd                                                    # noqa: E402
from tpnet_amd import score_fanout as sf                            # noqa: E402
from tpnet_amd.callers import LinkPredictor_v1                      # noqa: E402
from tpnet_amd.stream import CONFIGS, synthetic_stream             # noqa: E402

LinkPredictor_v1.SCORE_ALL_FUSED = False                           # the variants set the route themselves (fused_scores)
dev = torch.device("cuda:0")
D = lambda x, dt=torch.int64: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)
results = []


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.inner * 1e3


def alternate(group, calls):
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            times[k].append(events(fn))
    for k, v in times.items():
        r = dict(group=group, variant=k, median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), reps=len(v),
                 inner=args.inner)
        results.append(r)
        print(f"{group:44s} {k:18s} {r['median_us']:10.1f} us  [{r['min_us']:.1f} .. {r['max_us']:.1f}]", flush=True)


def table(cfg):
    c = CONFIGS[cfg]
    E = 6 * c["B"] if cfg == "C2" else 2 * c["B"]
    src, dst, t, N = synthetic_stream(c["U"], c["I"], E, c["span"] * E / c["E"], 0)
    torch.manual_seed(c["d"])
    rp = tpnet_amd.RandomProjectionModule(node_num=N, edge_num=c["E"], dim_factor=10, num_layer=3, time_decay_weight=c["lam"],
                                          device="cuda:0", use_matrix=False, beginning_time=np.float64(0.0), not_scale=False,
                                          enforce_dim=c["d"]).to(dev)
    rp.run_stream(D(src), D(dst), None, D(t, torch.float64), c["B"], want_neg=False, want_pos=False)
    dec = LinkPredictor_v1(172, 172, 172, 1, rp, not_encode=True).to(dev)
    return rp, dec, N


def bound64(dec, gram, c=4e-5, floor=1e-6):
    """score_one_to_many_host and tests/test_score_fanout_host.score_bound in float64 torch on the GPU -> (want, bound without the floor)."""
    rp = dec.random_projections
    w1, b1, w2, b2 = (p.detach().double() for p in (rp.mlp[0].weight, rp.mlp[0].bias, rp.mlp[2].weight, rp.mlp[2].bias))
    wdf, bd = dec.fc1.weight.detach().double()[:, -64:], dec.fc1.bias.detach().double()
    wd2, bd2 = dec.fc2.weight.detach().double()[0], dec.fc2.bias.detach().double()[0]
    f = gram.reshape(-1, 64).double()
    y = torch.relu(f @ w1.T + b1) @ w2.T + b2
    a = y @ wdf.T + bd
    want = torch.relu(a) @ wd2 + bd2
    mag_y = torch.relu(f.abs() @ w1.abs().T + b1.abs()) @ w2.abs().T + b2.abs()
    mag_a = y.abs() @ wdf.abs().T + bd.abs()
    e_a = (c * mag_y) @ wdf.abs().T + c * mag_a
    return want, e_a @ wd2.abs() + c * (mag_a @ wd2.abs() + bd2.abs())


def check(name, dec, src, comp, fused, cand=None, rng=None, rows=16):
    """(c) and (a) against float64 on the kernel's own features, `rows` sources at a time."""
    B = src.numel()
    wants, bounds = [], []
    for r0 in range(0, B, rows):
        s = src[r0:r0 + rows]
        out, gram = sf.score(dec, s, cand_ids=None if cand is None else cand[r0:r0 + rows], cand_range=rng, want_gram=True)
        assert torch.equal(out, fused[r0:r0 + rows]), "a pair's logit depends on its position"
        w, b = bound64(dec, gram)
        wants.append(w.view(out.shape))
        bounds.append(b.view(out.shape))
        del gram
    want, bound = torch.cat(wants), torch.cat(bounds)
    bound = bound + 1e-6 * want.abs().max()
    rc = ((fused.double() - want).abs() / bound).max().item()
    ra = ((comp.double() - want).abs() / bound).max().item()
    print(f"{name}: worst |logit - float64| / bound: kernel {rc:.2e}, composition {ra:.2e}; max |want| {want.abs().max().item():.3f}", flush=True)
    results.append(dict(group=name, variant="bound", kernel_ratio=rc, composition_ratio=ra))
    assert rc <= 1.0, "the kernel's logits leave the bound"


def bytes_per_call(name, B, C, d, D2=344):
    pairs = B * C
    comp = pairs * (256 * 4 + 2 * D2 * 4 * 2 + 8 * 2 + 4)          # features written and read twice each, two zero tensors written and read, expanded ids, logits
    kern = pairs * 4 + B * 8
    rows = pairs * 4 * d * 4                                        # the candidates' rows (both paths; from the caches where the table fits)
    print(f"{name}: {pairs} pairs; bytes beside the table rows: composition {comp / 1e6:.1f} MB, kernel {kern / 1e6:.2f} MB; "
          f"candidate rows read by either {rows / 1e6:.0f} MB", flush=True)
    results.append(dict(group=name, variant="bytes", composition=comp, kernel=kern, rows=rows))


def variants(dec, run):
    def a():
        dec.fused, dec.fused_scores = False, False
        return run()

    def b():
        dec.fused, dec.fused_scores = "f32", False
        return run()

    def c():
        dec.fused, dec.fused_scores = False, True
        return run()
    return {"(a) composition": a, "(b) fused='f32'": b, "(c) one launch": c}


work = []
with torch.no_grad():
    for cfg in ("C2", "C3"):
        rp, dec, N = table(cfg)
        rng = np.random.RandomState(len(cfg) + N)
        s200 = D(rng.randint(1, N, 200))
        work.append((f"{cfg}-shaped N={N} d={rp.dim} B=200 all [1, N)", dec, lambda dec=dec, s=s200, N=N: dec.forward_one_to_all(s, 1, N),
                     dict(src=s200, rng=(1, N)), (200, N - 1, rp.dim)))
        if cfg == "C2":
            s1000, cand = D(rng.randint(1, N, 1000)), D(rng.randint(1, N, (1000, 100)))
            work.append((f"{cfg}-shaped N={N} d={rp.dim} B=1000 list C=100", dec,
                         lambda dec=dec, s=s1000, c=cand: dec.forward_one_to_many(s, c), dict(src=s1000, cand=cand), (1000, 100, rp.dim)))
    if args.kernel_only:
        for name, dec, run, _, _ in work:
            c = variants(dec, run)["(c) one launch"]
            for _ in range(5):
                c()
        torch.cuda.synchronize()
        print("kernel-only: 5 calls per shape", flush=True)
        sys.exit(0)
    # ---- every shape: checked and warmed before anything is timed
    for name, dec, run, kw, shape in work:
        vs = variants(dec, run)
        assert sf.serves(dec)
        n0 = sf.calls["score"]
        comp, fused = vs["(a) composition"](), vs["(c) one launch"]()
        assert sf.calls["score"] == n0 + 1
        check(name, dec, kw["src"], comp, fused, cand=kw.get("cand"), rng=kw.get("rng"))
        bytes_per_call(name, *shape)
        for fn in vs.values():
            for _ in range(3):
                fn()
        del comp, fused
    torch.cuda.synchronize()
    for name, dec, run, kw, shape in work:
        alternate(name, variants(dec, run))

if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
