"""Command line for files on disk: the service's computations without HTTP.

    python -m deconv_api_amd.cli deconv photo.jpg [more.png ...] --layer block5_conv3 [--out-dir out/]
    python -m deconv_api_amd.cli dream photo.jpg --model inception_v3 --octaves 4 --steps 20 [--out-dir out/]
                                       [--guide other.jpg] [--lap-levels 4]
    python -m deconv_api_amd.cli occlusion photo.jpg --layer block5_conv3 [--patch 32 --stride 16] [--out-dir out/]
    python -m deconv_api_amd.cli activations photo.jpg [more.png ...] --layer block5_conv3 [--out-dir out/]
    python -m deconv_api_amd.cli layers

``deconv`` writes ``<stem>_<layer>.jpg``: the 2x2 mosaic of the top-4 deconvnet reconstructions, the same
image ``POST /`` returns as a data URL (reference: app/main.py:45-78), all files as one batch on the device.
``dream`` writes ``<stem>_dream_<model>.jpg`` (``POST /deepdream``); with ``--guide`` every image dreams towards
that image's features (the route's ``guide`` field), with ``--lap-levels N`` the gradient of every step is
Laplacian-pyramid normalised over N levels (the route's ``lap_levels`` field). ``occlusion`` writes
``<stem>_occlusion_<layer>.jpg``: the JPEG ``POST /occlusion`` returns (occlusion sensitivity maps of the same four
filters, one image after another). ``activations`` writes ``<stem>_activations_<layer>.jpg``: the JPEG
``POST /activations`` returns (the feature maps of the same four filters laid over the image), all files as one
batch on the device. Configuration as the server's
(``DV_*`` variables, config.py) with ``--device`` / ``--dtype`` / ``--weights`` overrides.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List

import numpy as np


def _read(paths: List[str], coeffs: bool = False) -> list:
    """Decoded images; with ``coeffs`` a baseline JPEG stays a JpegCoeffs for the GPU decode path."""
    from .codec import decode_image, parse_jpeg_coeffs

    out = []
    for p in paths:
        with open(p, "rb") as f:
            data = f.read()
        img = parse_jpeg_coeffs(data) if coeffs else None
        out.append(decode_image(data) if img is None else img)
    return out


def _stem(p: str) -> str:
    return os.path.splitext(os.path.basename(p))[0]


def cmd_deconv(a, cfg) -> int:
    from .codec import encode_jpeg
    from .serve.service import DeconvService

    svc = DeconvService(cfg)
    try:
        svc.engine._check_layer(a.layer)  # an unknown layer fails before any compute
        mos = svc.run_batch(a.layer, _read(a.images, svc.gpu_decode))
    finally:
        svc.close()
    os.makedirs(a.out_dir, exist_ok=True)
    from .runtime.staging import GpuScans

    for b, p in enumerate(a.images):
        if isinstance(mos, GpuScans):  # GPU service: the mosaics arrive JPEG-encoded on the device
            from .codec.image import gpu_jpeg_bytes

            jpeg = gpu_jpeg_bytes(mos.packed, mos.off, b, mos.H, mos.W, cfg.jpeg_quality)
        else:
            jpeg = encode_jpeg(np.ascontiguousarray(mos[b]), cfg.jpeg_quality)
        dst = os.path.join(a.out_dir, f"{_stem(p)}_{a.layer}.jpg")
        with open(dst, "wb") as f:
            f.write(jpeg)
        print(dst)
    return 0


def _route_jpeg(svc, mos, b: int = 0) -> bytes:
    """The JPEG inside the data URL the service's routes answer with for image ``b`` of the result ``mos`` as a
    request of its own: encoded the way serve/service.py's ``_encode_deliver`` does (GPU scans, the native encoder's
    restart segments, or PIL)."""
    import base64
    from urllib.parse import unquote

    from .codec import encode_data_url, encode_data_urls
    from .codec.image import gpu_data_urls
    from .runtime.staging import GpuScans

    q, th = svc.cfg.jpeg_quality, svc.cfg.encode_threads
    if isinstance(mos, GpuScans):
        url = gpu_data_urls(mos.packed, mos.off, mos.H, mos.W, q, th)[b]
    elif svc.native_codec:
        url = encode_data_urls(mos[b:b + 1], q, th)[0]
    else:
        url = encode_data_url(mos[b], q)
    if not isinstance(url, str):
        url = bytes(url).decode("ascii")
    return base64.b64decode(unquote(url.split(",", 1)[1]))


def cmd_occlusion(a, cfg) -> int:
    from .serve.service import DeconvService

    svc = DeconvService(cfg)
    try:
        svc.validate_occlusion(a.layer, a.patch, a.stride)  # fails before any decode or compute
        outs = [svc.run_occlusion(a.layer, img, a.patch, a.stride) for img in _read(a.images)]
    finally:
        svc.close()
    os.makedirs(a.out_dir, exist_ok=True)
    for p, mos in zip(a.images, outs):
        jpeg = _route_jpeg(svc, mos)
        dst = os.path.join(a.out_dir, f"{_stem(p)}_occlusion_{a.layer}.jpg")
        with open(dst, "wb") as f:
            f.write(jpeg)
        print(dst)
    return 0


def cmd_activations(a, cfg) -> int:
    from .serve.service import DeconvService

    svc = DeconvService(cfg)
    try:
        svc.validate_activations(a.layer)  # fails before any decode or compute
        mos = svc.run_activations(a.layer, _read(a.images))
    finally:
        svc.close()
    os.makedirs(a.out_dir, exist_ok=True)
    for b, p in enumerate(a.images):
        dst = os.path.join(a.out_dir, f"{_stem(p)}_activations_{a.layer}.jpg")
        with open(dst, "wb") as f:
            f.write(_route_jpeg(svc, mos, b))
        print(dst)
    return 0


def cmd_dream(a, cfg) -> int:
    from .codec import encode_jpeg
    from .serve.dream_service import DreamService

    imgs = _read(a.images)
    ds = DreamService(cfg)
    try:
        guides = [ds.prepare_guide(_read([a.guide])[0])] if a.guide else None
        kw = {"lap_levels": a.lap_levels} if a.lap_levels else {}
        outs = [ds.run_batch([ds.prepare(img, a.octaves)], a.model, a.octaves, a.steps, guides, **kw)[0] for img in imgs]
    finally:
        ds.close()
    os.makedirs(a.out_dir, exist_ok=True)
    for p, o in zip(a.images, outs):
        dst = os.path.join(a.out_dir, f"{_stem(p)}_dream_{a.model}.jpg")
        with open(dst, "wb") as f:
            f.write(encode_jpeg(np.ascontiguousarray(o), cfg.jpeg_quality))
        print(dst)
    return 0


def cmd_layers(a, cfg) -> int:
    from .models.vgg16 import VGG16_LAYER_NAMES

    print("\n".join(n for n in VGG16_LAYER_NAMES if n != "input_1"))
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m deconv_api_amd.cli")
    ap.add_argument("--device", default=None, help="auto | cuda | cpu (DV_DEVICE)")
    ap.add_argument("--dtype", default=None, help="bf16 | fp16 on a GPU (DV_DTYPE)")
    ap.add_argument("--weights", default=None, help="VGG16 weights (DV_WEIGHTS): .safetensors / .pt / Keras .h5")
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("deconv", help="deconvnet mosaic of each image")
    d.add_argument("images", nargs="+")
    d.add_argument("--layer", default="block5_conv3")
    d.add_argument("--mode", default=None, help="all | max (DV_MODE)")
    d.add_argument("--out-dir", default=".")
    d.add_argument("--gpu-decode", action="store_true", default=None,
                   help="baseline JPEGs: entropy-decode on the host, the rest on the GPU (DV_GPU_JPEG_DECODE)")
    r = sub.add_parser("dream", help="DeepDream of each image")
    r.add_argument("images", nargs="+")
    r.add_argument("--model", default="inception_v3", choices=["inception_v3", "resnet50"])
    r.add_argument("--octaves", type=int, default=4)
    r.add_argument("--steps", type=int, default=20)
    r.add_argument("--guide", default=None, help="dream towards this image's features (guided DeepDream)")
    r.add_argument("--lap-levels", type=int, default=0, choices=range(6), metavar="N",
                   help="Laplacian-pyramid gradient normalisation over N levels (0..5, 0 = off)")
    r.add_argument("--out-dir", default=".")
    o = sub.add_parser("occlusion", help="occlusion sensitivity mosaic of each image")
    o.add_argument("images", nargs="+")
    o.add_argument("--layer", default="block5_conv3")
    o.add_argument("--patch", type=int, default=32, help="side of the grey square (8 .. half the image side)")
    o.add_argument("--stride", type=int, default=16, help="step of the square (4 .. patch)")
    o.add_argument("--out-dir", default=".")
    v = sub.add_parser("activations", help="activation-map mosaic of each image")
    v.add_argument("images", nargs="+")
    v.add_argument("--layer", default="block5_conv3")
    v.add_argument("--out-dir", default=".")
    sub.add_parser("layers", help="the VGG16 layer names POST / accepts")
    a = ap.parse_args(argv)

    from .config import Config

    over = {k: v for k, v in (("device", a.device), ("dtype", a.dtype), ("weights", a.weights),
                              ("mode", getattr(a, "mode", None)),
                              ("gpu_jpeg_decode", getattr(a, "gpu_decode", None))) if v is not None}
    cfg = Config.from_env(**over)
    from .codec import ImageDecodeError
    from .engine.deconvnet import UnknownLayerError

    try:
        return {"deconv": cmd_deconv, "dream": cmd_dream, "occlusion": cmd_occlusion, "activations": cmd_activations,
                "layers": cmd_layers}[a.cmd](a, cfg)
    except (UnknownLayerError, ImageDecodeError, ValueError, OSError) as e:  # the HTTP routes' 400s
        print(f"error: {str(e).strip(chr(34))}", file=sys.stderr)
        return 2


if __name__ == "__main__":
    sys.exit(main())
