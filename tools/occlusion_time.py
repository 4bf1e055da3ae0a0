#!/usr/bin/env python
"""Per-request device times of POST /occlusion's engine call (engine/occlusion.py), one GPU, by hipEvents.

    python tools/occlusion_time.py [--layers block3_conv3,block5_conv3,predictions] [--patch 32] [--stride 16]
                                   [--dtype bf16] [--reps 10] [--limit 240] [--out FILE]

For every layer, at the given grid (default: 169 patches, 170 variants of one 224 x 224 image):
  * occlude_variants (and its achieved write bandwidth: the kernel is a pure 16-B store stream);
  * the forward: ``DeconvNet.forward`` on the variants plus the score reduction (channel_sum / fp32 cast);
  * heat + overlay (with the top-4 selection between them and the forward);
  * for comparison, ``DeconvNet.forward`` alone on a ready tensor of the same batch.
Each layer is measured by a child process of its own under ``--limit`` seconds (this process never opens the GPU;
a child that fails or runs out of time ends the run). Seeded random-init weights, a seeded noise image. Prints a text
table (``--out``: also written there); nothing is gated.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events(fn, reps: int) -> float:
    """Mean device time of one ``fn()`` in microseconds (3 unrecorded calls first)."""
    import torch

    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def child(a) -> None:
    import torch

    from deconv_api_amd import ops
    from deconv_api_amd.engine.deconvnet import DeconvNet
    from deconv_api_amd.engine.occlusion import Occlusion
    from deconv_api_amd.models.vgg16 import VGG16

    dev = torch.device("cuda", 0)
    ops.native.load()
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    layer = a.child
    net = DeconvNet(VGG16.random(0, include_top=layer in ("fc1", "fc2", "predictions")).build(dev, dt))
    occ = Occlusion(net)
    g = torch.Generator().manual_seed(7)
    x0 = torch.zeros(1, 224, 224, 8)
    x0[..., :3] = torch.randint(0, 256, (1, 224, 224, 3), generator=g).float() - torch.tensor(ops.CAFFE_MEAN)
    x0 = x0.to(dt).to(dev)
    xv = ops.occlude_variants(x0, a.patch, a.stride)
    V = xv.shape[0]
    sc = occ.variant_scores(xv, layer).view(1, V, -1)

    def maps():
        idx, _ = ops.topk_positive(sc[:, 0], 4)
        heat, part = ops.occlusion_heat(sc, idx, 224, a.patch, a.stride)
        return ops.occlusion_overlay(heat, part, idx, x0)

    row = {"layer": layer, "variants": V, "gpu": torch.cuda.get_device_name(0),
           "occlude_us": _events(lambda: ops.occlude_variants(x0, a.patch, a.stride), a.reps),
           "forward_us": _events(lambda: occ.variant_scores(xv, layer), a.reps),
           "maps_us": _events(maps, a.reps),
           "forward_alone_us": _events(lambda: net.forward(xv, layer), a.reps),
           "request_us": _events(lambda: occ.run(x0, layer, a.patch, a.stride), a.reps),
           "written_mb": xv.numel() * 2 / 1e6}
    print("ROW " + json.dumps(row), flush=True)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="block3_conv3,block5_conv3,predictions")
    ap.add_argument("--patch", type=int, default=32)
    ap.add_argument("--stride", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per layer's child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child:
        child(a)
        return 0
    lines, shown = [], 0
    for layer in a.layers.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", layer, "--patch", str(a.patch), "--stride",
               str(a.stride), "--dtype", a.dtype, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{layer}: no answer within {a.limit:.0f} s; stopping", file=sys.stderr)
            return 3
        rows = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not rows:
            print(f"{layer}: child ended with {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 3
        d = json.loads(rows[0])
        if not lines:
            lines.append(f"# occlusion request, {a.dtype}, patch {a.patch} stride {a.stride}: {d['variants']} variants of one "
                         f"224 x 224 image ({d['written_mb']:.1f} MB written by occlude_variants), {d['gpu']}; device "
                         f"times by hipEvents, mean of {a.reps}")
            lines.append(f"{'layer':14s} {'occlude us':>10s} {'TB/s':>6s} {'forward us':>10s} {'heat+overlay us':>15s} "
                         f"{'request us':>10s} {'forward alone us':>16s}")
        lines.append(f"{d['layer']:14s} {d['occlude_us']:10.1f} {d['written_mb'] / d['occlude_us']:6.2f} "
                     f"{d['forward_us']:10.1f} {d['maps_us']:15.1f} {d['request_us']:10.1f} {d['forward_alone_us']:16.1f}")
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
