#!/usr/bin/env python
"""Record which kernel every conv of fixed, seeded workloads is routed to (``_C.conv_route()``).

A proxy around the extension module is installed as ``ops.native._mod``: it forwards everything and,
after each ``conv`` call, writes one text line with the call's scalar inputs and the route the binding
reports. No C++ is involved, so the same script runs at any commit; two recordings of the same device
are comparable byte for byte. ``tests/fixtures/conv_dma_routes.txt`` is such a recording; the CPU test
of the LDS-DMA planner (tests/test_conv_dma_plan.py) replays its rows.

Workloads: the VGG16 deconvnet to block5_conv3 at B = 1, 4, 256 (K = 4) and, with the classifier head, to
predictions at B = 1 and 256 (the dense layers as [M, 1, 1, K] GEMMs, M = B up, 4 B down); one InceptionV3 DeepDream octave
at 299^2; one ResNet-50 DeepDream step on 512^2 fp16 tiles; the shapes of the GPU tests that assert the
routes the models do not reach; a few launches under non-default knobs.

Line: g=<23 geometry ints> amode epi impl dt has=<optional tensors> relu_cols split_col ucode_div stats_div
      out / res / emask / out_code = <pointer mod 16>,<row stride>,<storage elements past the pointer>
      cus=<device CUs> knobs=<non-default knobs, '-' for none> | <route>

  python tools/record_conv_routes.py --out conv_dma_routes.txt
"""
from __future__ import annotations

import argparse
import contextlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deconv_api_amd import ops  # noqa: E402
from deconv_api_amd.ops.conv import ConvWeights  # noqa: E402

DEV = torch.device("cuda", 0)
# the per-launch knobs of the LDS-DMA family a row may carry (read by the C++ under DV_ABLATIONS=1;
# DV_NO_KW3_SK is read directly)
KNOB_ENV = ("DV_KW3", "DV_KW3_VAR", "DV_KW3_TILE", "DV_KW3_SK", "DV_NO_KW3_SK", "DV_KW3P_EPI", "DV_KW3P_UNP_NT",
            "DV_NO_KW3P_UNPOOL", "DV_KW3P_NO_PRE")


def _tinfo(t):
    if t is None:
        return "-"
    esz = t.element_size()
    avail = (t.untyped_storage().nbytes() - t.storage_offset() * esz) // esz
    ld = t.stride(-2) if t.dim() >= 2 else t.numel()
    return f"{t.data_ptr() % 16},{ld},{avail}"


class Recorder:
    """Stands in for the extension module: records conv() calls, forwards everything else."""

    def __init__(self, mod):
        self._mod = mod
        self._tune = (0, 0)
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.sections: dict = {}
        self.section = None

    def __getattr__(self, name):
        return getattr(self._mod, name)

    def dma_tune(self, cfg, ks):
        self._tune = (int(cfg), int(ks))
        return self._mod.dma_tune(cfg, ks)

    def _knobs(self):
        k = []
        if os.environ.get("DV_ABLATIONS") == "1":
            k += [f"{n}={os.environ[n]}" for n in KNOB_ENV if n in os.environ and n != "DV_NO_KW3_SK"]
        if "DV_NO_KW3_SK" in os.environ:
            k.append("DV_NO_KW3_SK=" + os.environ["DV_NO_KW3_SK"])
        if self._tune != (0, 0):
            k.append(f"cfg={self._tune[0]}")
            k.append(f"ks={self._tune[1]}")
        return ",".join(k) if k else "-"

    def conv(self, x, w, bias, out, out_code, code, mask, geom, amode, epi, impl, res, emask, stats, stats_div,
             ucode, ucode_div, relu_cols, out2, split_col, obits, ebits, w_kw3):
        r = self._mod.conv(x, w, bias, out, out_code, code, mask, geom, amode, epi, impl, res, emask, stats,
                           stats_div, ucode, ucode_div, relu_cols, out2, split_col, obits, ebits, w_kw3)
        opt = dict(bias=bias, out_code=out_code, code=code, mask=mask, res=res, emask=emask, stats=stats, ucode=ucode,
                   out2=out2, obits=obits, ebits=ebits, w_kw3=w_kw3)
        has = ",".join(n for n, t in opt.items() if t is not None) or "-"
        line = (f"g={','.join(str(int(v)) for v in geom)} amode={int(amode)} epi={int(epi)} impl={int(impl)} "
                f"dt={'f16' if x.dtype == torch.float16 else 'bf16'} has={has} relu_cols={int(relu_cols)} "
                f"split_col={int(split_col)} ucode_div={int(ucode_div)} stats_div={int(stats_div)} "
                f"out={_tinfo(out)} res={_tinfo(res)} emask={_tinfo(emask)} out_code={_tinfo(out_code)} "
                f"cus={self.cus} knobs={self._knobs()} | {self._mod.conv_route()}")
        self.sections.setdefault(self.section, set()).add(line)
        return r


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def vgg16(rec):
    from deconv_api_amd.engine.deconvnet import DeconvNet
    from deconv_api_amd.models.vgg16 import VGG16

    eng = DeconvNet(VGG16.random(0, include_top=False).build(DEV, torch.bfloat16))
    g = torch.Generator(device=DEV).manual_seed(1)
    for B in (1, 4, 256):
        rec.section = f"vgg16 deconvnet block5_conv3 B={B} K=4"
        x = torch.zeros(B, 224, 224, 8, dtype=torch.bfloat16, device=DEV)
        x[..., :3] = (torch.rand(B, 224, 224, 3, device=DEV, generator=g) * 255 - 115).to(torch.bfloat16)
        eng.run(x, "block5_conv3", k=4)
        torch.cuda.synchronize()


def vgg16_dense(rec):
    """The classifier head: fc1 / fc2 / predictions up at M = B rows and down at M = B K rows (H = W = 1)."""
    from deconv_api_amd.engine.deconvnet import DeconvNet
    from deconv_api_amd.models.vgg16 import VGG16

    eng = DeconvNet(VGG16.random(0).build(DEV, torch.bfloat16))
    g = torch.Generator(device=DEV).manual_seed(2)
    for B in (1, 256):
        rec.section = f"vgg16 deconvnet predictions B={B} K=4"
        x = torch.zeros(B, 224, 224, 8, dtype=torch.bfloat16, device=DEV)
        x[..., :3] = (torch.rand(B, 224, 224, 3, device=DEV, generator=g) * 255 - 115).to(torch.bfloat16)
        eng.run(x, "predictions", k=4)
        torch.cuda.synchronize()


def dream(rec):
    from deconv_api_amd.engine.deepdream import (RESNET_LAYERS, DeepDream, DreamSettings, TiledDeepDream,
                                                 inception_preprocess)
    from deconv_api_amd.models.inception_v3 import InceptionV3
    from deconv_api_amd.models.resnet50 import ResNet50

    g = torch.Generator(device=DEV).manual_seed(7)
    rec.section = "inception_v3 deepdream, one octave at 299^2, B=64"
    img = torch.randint(0, 256, (64, 299, 299, 3), dtype=torch.uint8, device=DEV, generator=g)
    dd = DeepDream(InceptionV3(0).build(DEV, torch.bfloat16), DreamSettings(octaves=1, iterations=1), use_graphs=False)
    dd.run(inception_preprocess(img))
    torch.cuda.synchronize()
    rec.section = "resnet50 deepdream fp16, one step on 512^2 tiles of 8 images at 1024^2"
    img = torch.randint(0, 256, (8, 1024, 1024, 3), dtype=torch.uint8, device=DEV, generator=g)
    s = DreamSettings(layers=dict(RESNET_LAYERS), octaves=1, iterations=1)
    dd = TiledDeepDream(ResNet50(0).build(DEV, torch.float16), s, tile=512, use_graphs=False)
    dd.run(inception_preprocess(img))
    torch.cuda.synchronize()


def _cw(oc, c, k=3, dt=torch.bfloat16, bias=True, seed=0):
    g = torch.Generator().manual_seed(seed + oc + c)
    w = torch.randn(oc, c, k, k, generator=g) / (k * k * c) ** 0.5
    return ConvWeights(w, torch.randn(oc, generator=g) if bias else None, "fwd").to_device(DEV, dt)


def _x(n, h, w, c, dt=torch.bfloat16):
    return torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(n + h + c)).to(dt).to(DEV)


def route_test_shapes(rec):
    """Shapes of the GPU tests that assert a route, under the knobs those tests set."""
    G = rec.cus
    BF, HF = torch.bfloat16, torch.float16
    rec.section = "shapes of the GPU route tests"
    # stream-K and whole-tile KW3P on about 1.5 rounds (tests/test_conv_exact_gpu.py test_exact_kw3p_stream_k)
    for H, W, C, OC, div, dt in [(14, 14, 32, 256, 0, BF), (12, 11, 32, 512, 2, HF)]:
        tiles_n, d = OC // 256, max(div, 1)
        if G % tiles_n:
            continue
        N = -(-(3 * G // (2 * tiles_n)) * 256 // (H * W * d)) * d
        kw = dict(relu=True, use_bias=not div)
        if div:
            kw.update(unpool_out=torch.zeros(N // div, H, W, OC, dtype=torch.uint8, device=DEV), unpool_div=div)
        with env(DV_ABLATIONS=1, DV_KW3=2):
            rec.dma_tune(0, 1)
            ops.conv2d(_x(N, H, W, C, dt), _cw(OC, C, dt=dt, bias=not div), **kw)
            with env(DV_NO_KW3_SK=1):
                ops.conv2d(_x(N, H, W, C, dt), _cw(OC, C, dt=dt, bias=not div), **kw)
            rec.dma_tune(0, 0)
    # full rounds + 128 x 128 tail, and the plain tile with the shared-tap kernels off (test_kernels_gpu.py
    # test_conv_kw3_tail_split)
    H, W, C, OC = 14, 14, 512, 256
    N = -(-(21 * G // 20 + 1) * 256 // (H * W))
    x, cw = _x(N, H, W, C), _cw(OC, C)
    ops.conv2d(x, cw, relu=True)  # default knobs: stream-K takes this grid whole
    with env(DV_NO_KW3_SK=1):
        ops.conv2d(x, cw, relu=True)
        with env(DV_ABLATIONS=1, DV_KW3=0):
            ops.conv2d(x, cw, relu=True)
    del x
    # forced shared-tap kernels on small shapes (test_conv_exact_gpu.py test_exact_kw3_epilogues /
    # test_exact_kw3p_persistent / test_exact_kw3p_unpool_out; test_kernels_gpu.py test_conv_kw3p_unpool_out)
    rec.dma_tune(0, 1)
    with env(DV_ABLATIONS=1, DV_KW3=2, DV_NO_KW3_SK=1):
        for N, H, W, C, OC, dt in [(3, 10, 9, 32, 256, BF), (3, 36, 35, 32, 128, HF)]:
            x, cw = _x(N, H, W, C, dt), _cw(OC, C, dt=dt)
            code = torch.zeros(N, H, W, OC, dtype=torch.uint8, device=DEV)
            with env(DV_KW3_VAR=0):
                ops.conv2d(x, cw, relu=True)
                ops.conv2d(x, cw, relu=False, epilogue="f32")
                ops.conv2d(x, cw, relu=True, unpool_out=code)
            ops.conv2d(x, cw, relu=True)
            with env(DV_KW3P_EPI="reg"):
                ops.conv2d(x, cw, relu=True)
            ops.conv2d(x, cw, relu=True, unpool_out=code)
            with env(DV_NO_KW3P_UNPOOL=1):
                ops.conv2d(x, cw, relu=True, unpool_out=code)
    rec.dma_tune(0, 0)
    # ReLU-masked dgrad tiles of every width (test_kernels_gpu.py test_conv_masked_dgrad_shapes)
    for C, OC, N, H in [(64, 16, 3, 20), (64, 64, 2, 33), (128, 128, 2, 17), (256, 512, 1, 14)]:
        x = _x(N, H, H + 3, C)
        ops.conv2d(x, _cw(OC, C, bias=False), relu=False, mask=x.clone(), use_bias=False)
    # forced tiles with the pooled-max epilogue and with split-K 0 (automatic) / 2
    # (test_conv_exact_gpu.py test_exact_pool_ties_dma, test_exact_dma_tile_matrix)
    for N, H, W, C, OC, cfg in [(2, 16, 14, 64, 128, 4), (3, 10, 14, 64, 192, 6), (1, 12, 12, 32, 48, 11)]:
        rec.dma_tune(cfg, 0)
        ops.conv2d(_x(N, H, W, C), _cw(OC, C), relu=True, epilogue="pool")
    for cfg, OC in [(8, 40), (3, 128), (1, 256), (17, 40)]:
        for ks in (0, 2):
            rec.dma_tune(cfg, ks)
            ops.conv2d(_x(2, 13, 11, 64), _cw(OC, 64), relu=True)
            ops.conv2d(_x(2, 13, 11, 64), _cw(OC, 64), relu=False, epilogue="f32")
    rec.dma_tune(0, 0)
    # grouped launches: both groupable configs (test_conv_routes_exact_gpu.py test_dma_groups)
    with ops.conv.conv_group(DEV):
        ops.conv2d(_x(1, 16, 16, 64), _cw(64, 64, k=1), relu=True)
        ops.conv2d(_x(1, 16, 16, 64), _cw(96, 64, k=1), relu=True)
        ops.conv2d(_x(2, 112, 112, 64), _cw(128, 64, k=1), relu=True)
        ops.conv2d(_x(2, 112, 112, 64), _cw(128, 64, k=1), relu=True)
    torch.cuda.synchronize()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="", help="comma list of vgg16, dense, dream, tests (default: all)")
    a = ap.parse_args(argv)
    rec = Recorder(ops.native.load())
    ops.native._mod = rec
    only = set(filter(None, a.only.split(",")))
    for name, fn in (("vgg16", vgg16), ("dense", vgg16_dense), ("dream", dream), ("tests", route_test_shapes)):
        if not only or name in only:
            fn(rec)
    ops.conv.check_stream_k()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for sec, lines in rec.sections.items():
            f.write(f"# {sec}\n")
            f.writelines(ln + "\n" for ln in sorted(lines))
    n = sum(len(v) for v in rec.sections.values())
    print(f"{n} distinct conv calls in {len(rec.sections)} workloads -> {a.out}")


if __name__ == "__main__":
    main()
