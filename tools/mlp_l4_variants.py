#!/usr/bin/env python3
"""Developer tool: the two instantiations of k_mlp_l4 (csrc/mlp_l4.hip) against each other -- the library as built (two passes of 7
hidden slices, 4 output tiles) and a second build of the first variant (passes of 8 slices, 6 output tiles):

    make -C tpnet_amd/csrc VARIANT=l4first VARFLAGS=-DTPNET_L4_FIRST_VARIANT        # -> tpnet_amd/libtpnet_hip_l4first.so
    tools/mlp_l4_variants.py [--first PATH] [--turns 3] [--limit 120]

A library is fixed per process (TPNET_DEV_LIB), so the variants alternate as child processes, each under its own time limit; the first
child that fails ends the tool.  Per child and n = 1 000 / 80 000 / 800 000, without and with relu_bits: tpnet_mlp_l4_f32 alone, one
untimed window and five timed ones of device events around the calls, median and min-max in us per call, and a hash of y (and
relu_bits): equal hashes = equal bits.  The spread to compare against is over the windows AND the turns."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--first", default=os.path.join(ROOT, "tpnet_amd", "libtpnet_hip_l4first.so"))
ap.add_argument("--turns", type=int, default=3)
ap.add_argument("--limit", type=int, default=120)
ap.add_argument("--one", default=None)
args = ap.parse_args()


def one(tag):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from tpnet_amd import _dense, _lib, fused_feature as ff
    if not torch.cuda.is_available():
        sys.exit("mlp_l4_variants.py measures on a GPU: none found")
    dev = torch.device("cuda:0")
    torch.manual_seed(100)
    mlp = torch.nn.Sequential(torch.nn.Linear(100, 400), torch.nn.ReLU(), torch.nn.Linear(400, 100)).to(dev)
    lib = _lib.load()
    rec = ff.l4_images(mlp)
    out = dict(variant=tag, image_bytes=int(lib.tpnet_mlp_l4_image_bytes()))
    for n in (1000, 80000, 800000):
        g = torch.Generator().manual_seed(n)
        x = torch.log1p(torch.expm1(torch.rand(n, 100, generator=g, dtype=torch.float64) * 20.0)).float().to(dev)
        y = torch.empty_like(x)
        bits = torch.empty((n, 13), dtype=torch.int32, device=dev)
        st = _dense.stream_ptr(dev)
        calls = max(20, min(1000, 20_000_000 // n))
        for name, bp in (("plain", None), ("bits", bits.data_ptr())):
            def call():
                return lib.tpnet_mlp_l4_f32(x.data_ptr(), n, rec.img.data_ptr(), y.data_ptr(), bp, st)
            if call() != 0:
                sys.exit("tpnet_mlp_l4_f32 declined the call")
            torch.cuda.synchronize()
            ts = []
            for w in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    call()
                e1.record()
                torch.cuda.synchronize()
                if w:                                               # (the first window is the warm-up)
                    ts.append(e0.elapsed_time(e1) / calls * 1e3)
            sha = hashlib.sha256(y.cpu().numpy().tobytes() + (bits.cpu().numpy().tobytes() if bp else b"")).hexdigest()[:16]
            out[f"{n}_{name}"] = dict(us=round(float(np.median(ts)), 2), min=round(min(ts), 2), max=round(max(ts), 2), sha=sha)
    print(json.dumps(out), flush=True)


if args.one is not None:
    one(args.one)
else:
    libs = {"as built": os.path.join(ROOT, "tpnet_amd", "libtpnet_hip.so"), "first": args.first}
    for tag, lib in libs.items():
        if not os.path.exists(lib):
            sys.exit(f"{lib} is missing: build it first (see the docstring)")
    for turn in range(args.turns):
        for tag, lib in libs.items():
            p = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", tag],
                               env=dict(os.environ, TPNET_DEV_LIB=lib))
            if p.returncode != 0:
                sys.exit(f"{tag}, turn {turn}: the measuring process ended with status {p.returncode}; nothing more is started")
