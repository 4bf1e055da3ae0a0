#!/usr/bin/env python
"""Guided against unguided DeepDream, config 3 (InceptionV3, batch 64, 299^2, 4 octaves x 20 steps), one GPU.

    python tools/dream_guide_time.py [--batch 64] [--size 299] [--octaves 4] [--steps 20] [--pairs 3]

Method of bench_dream.py (one timed run = the whole octave loop over the batch, synthetic uint8 images, seeded
random-init weights, hipGraph per octave, one warm-up run per mode that includes the captures), in ``--pairs``
interleaved (unguided, guided) pairs so drift hits both alike. The guided runs include the guide's feature pass
(once per run). Then:

  * the matching kernel alone: for every octave shape and loss layer, guide_match (loss tap form: addend +
    partials) against the sumsq_core_bwd launch it replaces, on a sub-batch's activations, by device events;
  * the losses the two objectives reach on the default random weights after each octave (per image, against
    DreamSettings.max_loss) and how many images the device-side max_loss flag stopped.

Prints text; nothing is gated. Neither benchmark (bench.py, bench_dream.py) is touched.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deconv_api_amd import ops  # noqa: E402
from deconv_api_amd.engine.deepdream import DeepDream, DreamSettings, inception_preprocess  # noqa: E402
from deconv_api_amd.ops.autograd import guide_index  # noqa: E402


def _timed(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _events(fn, reps: int = 20) -> float:
    """Mean device time of one ``fn()`` in microseconds (3 unrecorded calls first)."""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=299)
    ap.add_argument("--octaves", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    lib = ops.native.load()
    from deconv_api_amd.models.inception_v3 import InceptionV3

    net = InceptionV3(0).build(dev, torch.bfloat16)
    s = DreamSettings(octaves=a.octaves, iterations=a.steps)
    dd = DeepDream(net, s)
    g = torch.Generator(device=dev).manual_seed(7)
    x = inception_preprocess(torch.randint(0, 256, (a.batch, a.size, a.size, 3), dtype=torch.uint8, device=dev, generator=g))
    guide = inception_preprocess(torch.randint(0, 256, (a.batch, a.size, a.size, 3), dtype=torch.uint8, device=dev,
                                               generator=g))
    print(f"# guided vs unguided DeepDream: inception_v3 bf16, batch {a.batch}, {a.size}^2, {a.octaves} octaves x "
          f"{a.steps} steps, guide_size {s.guide_size}, {dd.split} sub-batch streams, {torch.cuda.get_device_name(0)}")
    print(f"warm-up (captures included): unguided {_timed(lambda: dd.run(x)):.1f} s, "
          f"guided {_timed(lambda: dd.run(x, guide)):.1f} s")
    rows = []
    for p in range(a.pairs):
        tu = _timed(lambda: dd.run(x))
        tg = _timed(lambda: dd.run(x, guide))
        rows.append((tu, tg))
        print(f"pair {p}: unguided {tu * 1e3:8.1f} ms {a.batch / tu:7.1f} img/s | guided {tg * 1e3:8.1f} ms "
              f"{a.batch / tg:7.1f} img/s | guided / unguided time {tg / tu:.3f}")
    bu, bg = min(r[0] for r in rows), min(r[1] for r in rows)
    print(f"best: unguided {a.batch / bu:.1f} img/s, guided {a.batch / bg:.1f} img/s, guided / unguided time {bg / bu:.3f}")

    # ---- losses reached (the fused states keep every octave's last loss / max_loss flag per image)
    print("\n# losses after each octave's last step (random-init weights; max_loss = %s)" % s.max_loss)
    for mode in ("unguided", "guided"):
        for key, st in dd._graphs.items():
            if ("guided" in key) != (mode == "guided"):
                continue
            ls = st.loss.float().cpu()
            print(f"{mode:9s} octave {key[1][0]:3d}x{key[1][1]:<3d} sub-batch {key[3]}: loss min {float(ls.min()):9.4f} "
                  f"mean {float(ls.mean()):9.4f} max {float(ls.max()):9.4f}  stopped by max_loss {int(st.done.sum())}/{ls.numel()}")

    # ---- the kernel alone, against the launch it replaces
    print("\n# guide_match vs the sumsq_core_bwd launch it replaces (tap form: addend + loss partials), per launch")
    names = list(s.layers)
    B = -(-a.batch // max(1, dd.split))
    gf = dd.guide_features(guide[:B], B)
    tot_g = tot_s = 0.0
    for hw in dd.octave_shapes(a.size, a.size):
        with torch.no_grad():
            xin = dd._net_input(torch.nn.functional.interpolate(x[:B].permute(0, 3, 1, 2), size=hw).permute(0, 2, 3, 1))
            acts = net.forward(xin.contiguous(), names)
        for n in names:
            act = acts[n].contiguous()
            y = gf.feats[n]
            scale = torch.full((B,), 1e-6, device=dev)
            gx, add = torch.empty_like(act), torch.randn_like(act)
            part = torch.empty(B, 32, device=dev)
            gidx = guide_index(range(B), B, dev)
            tg = _events(lambda: lib.guide_match(act, y, gidx, scale, gx, s.border, add, part, True))
            ts = _events(lambda: lib.sumsq_core_bwd(act, scale, gx, s.border, add, part))
            P = (act.shape[1] - 2 * s.border) * (act.shape[2] - 2 * s.border)
            fl = 2.0 * B * P * y.shape[1] * act.shape[3]
            tot_g += tg
            tot_s += ts
            print(f"octave {hw[0]:3d}x{hw[1]:<3d} {n}: a {tuple(act.shape)} Q {y.shape[1]:4d}: guide_match {tg:8.1f} us "
                  f"({fl / tg * 1e-6:6.1f} TFLOP/s) sumsq_core_bwd {ts:7.1f} us")
    print(f"sum over one step of every octave, sub-batch {B}: guide_match {tot_g:.0f} us, sumsq_core_bwd {tot_s:.0f} us")


if __name__ == "__main__":
    main()
