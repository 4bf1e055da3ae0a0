#!/usr/bin/env python
"""Per-request device times of POST /activations' engine call (engine/activations.py), one GPU, by hipEvents.

    python tools/actmap_time.py [--layers block1_conv2,block3_conv3,block5_conv3] [--batches 1,32] [--dtype bf16]
                                [--reps 10] [--limit 240] [--out FILE]

For every layer and batch size B:
  * the forward: ``DeconvNet.forward`` of the B images;
  * the selection: ``select_filters`` (channel sums + top-4);
  * heat: ``ops.activation_heat`` (csrc/actmap.hip), and overlay: ``ops.occlusion_overlay``, each on ready inputs;
  * the whole request: ``ActivationMaps.run``.
Each layer is measured by a child process of its own under ``--limit`` seconds (this process never opens the GPU;
a child that fails or runs out of time ends the run). Seeded random-init weights, seeded noise images. Prints a text
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
    from deconv_api_amd.engine.activations import ActivationMaps
    from deconv_api_amd.engine.deconvnet import DeconvNet
    from deconv_api_amd.models.vgg16 import VGG16

    dev = torch.device("cuda", 0)
    ops.native.load()
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    layer = a.child
    net = DeconvNet(VGG16.random(0, include_top=False).build(dev, dt))
    maps = ActivationMaps(net)
    for B in [int(b) for b in a.batches.split(",")]:
        g = torch.Generator().manual_seed(7)
        x = torch.zeros(B, 224, 224, 8)
        x[..., :3] = torch.randint(0, 256, (B, 224, 224, 3), generator=g).float() - torch.tensor(ops.CAFFE_MEAN)
        x = x.to(dt).to(dev)
        out = net.forward(x, layer).out
        idx, _ = net.select_filters(out, 4, "per_image")
        heat, part = ops.activation_heat(out, idx, 224)
        row = {"layer": layer, "B": B, "map": list(out.shape[1:]), "gpu": torch.cuda.get_device_name(0),
               "forward_us": _events(lambda: net.forward(x, layer), a.reps),
               "select_us": _events(lambda: net.select_filters(out, 4, "per_image"), a.reps),
               "heat_us": _events(lambda: ops.activation_heat(out, idx, 224), a.reps),
               "overlay_us": _events(lambda: ops.occlusion_overlay(heat, part, idx, x), a.reps),
               "request_us": _events(lambda: maps.run(x, layer), a.reps)}
        print("ROW " + json.dumps(row), flush=True)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="block1_conv2,block3_conv3,block5_conv3")
    ap.add_argument("--batches", default="1,32")
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
        cmd = [sys.executable, os.path.abspath(__file__), "--child", layer, "--batches", a.batches, "--dtype", a.dtype,
               "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{layer}: no answer within {a.limit:.0f} s; stopping", file=sys.stderr)
            return 3
        rows = [json.loads(ln[4:]) for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not rows:
            print(f"{layer}: child ended with {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 3
        if not lines:
            lines.append(f"# activation-map request, {a.dtype}, B images of 224 x 224, {rows[0]['gpu']}; device times by "
                         f"hipEvents, mean of {a.reps}")
            lines.append(f"{'layer':14s} {'B':>3s} {'map':>14s} {'forward us':>10s} {'select us':>9s} {'heat us':>8s} "
                         f"{'overlay us':>10s} {'request us':>10s} {'forward %':>9s}")
        for d in rows:
            lines.append(f"{d['layer']:14s} {d['B']:3d} {'x'.join(map(str, d['map'])):>14s} {d['forward_us']:10.1f} "
                         f"{d['select_us']:9.1f} {d['heat_us']:8.1f} {d['overlay_us']:10.1f} {d['request_us']:10.1f} "
                         f"{100 * d['forward_us'] / d['request_us']:9.1f}")
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
