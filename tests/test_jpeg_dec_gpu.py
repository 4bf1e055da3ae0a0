"""GPU JPEG decode on the device: the HIP kernels (csrc/jpeg_dec_gpu.hip) are bit-identical to PIL, the
staging ring gives the same network input whichever path decoded an image, and the service answers the same
mosaics with the switch on."""
import asyncio
import os
import sys

import numpy as np
import pytest
import torch

from deconv_api_amd import ops
from deconv_api_amd.codec import JpegCoeffs, decode_image, make_data_url, parse_jpeg_coeffs, parse_result_data_url
from deconv_api_amd.utils import metrics as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_dec_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


def test_kernels_are_bit_identical_to_pil(native_lib):
    """The whole matrix as four mixed batches: one launch pair sees every sampling, greyscale, odd sizes,
    restart / optimized files and (rgb_align=1) destination offsets of every alignment at once."""
    dev = torch.device("cuda", 0)
    mat = cases.matrix()
    coeffs = [parse_jpeg_coeffs(d) for _, d, _ in mat]
    assert all(c is not None for c in coeffs)
    bad, offsets = [], set()
    n = len(mat) - 5  # the cross product; behind it 3 greyscale files and the two large images
    for k in range(4):  # every batch: a quarter of the cross product, the greyscale files, a large image
        idx = list(range(k, n, 4)) + [n, n + 1, n + 2, n + 3 + k % 2]
        outs = ops.jpeg_coeffs_to_rgb([coeffs[i] for i in idx], dev, rgb_align=1)
        torch.cuda.synchronize()
        assert {coeffs[i].kind for i in idx} == {0, 1, 2, 3}
        for i, o in zip(idx, outs):
            offsets.add(o.storage_offset() % 4)
            if o.shape != mat[i][2].shape or not torch.equal(o.cpu(), torch.from_numpy(mat[i][2])):
                bad.append(mat[i][0])
    assert not bad, (len(bad), bad[:10])
    assert offsets == {0, 1, 2, 3}
    # the aligned layout the staging ring uses takes the 4-byte store path for every full pixel group
    big = [coeffs[-1], coeffs[-2]]
    for o, (_, _, want) in zip(ops.jpeg_coeffs_to_rgb(big, dev), (mat[-1], mat[-2])):
        assert torch.equal(o.cpu(), torch.from_numpy(want))


def _mixed(n: int):
    """n images: JPEG coefficients of several samplings and sizes, raw pixels, a PNG-decoded array; and
    the same list as PIL would have decoded it."""
    mat = cases.matrix()
    rng = np.random.default_rng(5)
    png = decode_image(_png_bytes(rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)))
    pool = [("jpeg", mat[-2]), ("raw", rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)), ("jpeg", mat[-1]),
            ("png", png), ("jpeg", mat[200]), ("jpeg", mat[-3]), ("jpeg", mat[430])]
    mixed, plain = [], []
    for kind, v in pool[:n]:
        if kind == "jpeg":
            mixed.append(parse_jpeg_coeffs(v[1]))
            plain.append(np.ascontiguousarray(v[2]))
        else:
            mixed.append(v)
            plain.append(v)
    return mixed, plain


def _png_bytes(img):
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")
    return buf.getvalue()


@pytest.mark.parametrize("n", [1, 5])
def test_staging_ring_mixed_batch_equals_pil_decoded(native_lib, n):
    from deconv_api_amd.runtime.staging import StagingRing, resize_batch

    dev = torch.device("cuda", 0)
    mixed, plain = _mixed(n)
    assert isinstance(mixed[0], JpegCoeffs)
    ring = StagingRing(dev, slots=1, slot_bytes=1 << 20, max_images=8)  # one slot: every stage reuses it
    for dtype, C in ((torch.uint8, 3), (torch.bfloat16, 8)):
        want = torch.empty(n, 224, 224, C, dtype=dtype, device=dev)
        ring.stage(plain, want)
        for rep in range(2):  # twice through the same slot
            got = torch.empty_like(want)
            ring.stage(mixed, got)
            torch.cuda.synchronize()
            assert torch.equal(got, want), (dtype, rep)
        assert torch.equal(resize_batch(mixed, torch.empty_like(want)), want)


def test_service_with_gpu_decode_answers_the_same_mosaics(native_lib):
    from deconv_api_amd.config import Config
    from deconv_api_amd.engine.deconvnet import DeconvNet
    from deconv_api_amd.models.vgg16 import VGG16
    from deconv_api_amd.serve.service import DeconvService

    mat = cases.matrix()
    jpeg = "data:image/jpeg;base64,"
    import base64

    uris = [jpeg + base64.b64encode(mat[i][1]).decode() for i in (-1, -2, 430)]
    uris.append(make_data_url(np.random.default_rng(2).integers(0, 256, (60, 80, 3), dtype=np.uint8), "PNG"))
    eng = DeconvNet(VGG16.random(0, include_top=False).build("cuda", torch.bfloat16))

    def answers(svc):  # one request at a time: every batch is one image, whatever the timing
        return [asyncio.run(svc.deconv(u, "block1_conv1")) for u in uris]

    def paths():
        return {dict(k).get("path"): v for k, v in M.DECODE_PATH.values.items()}

    svc = DeconvService(Config.from_env(device="cuda", max_batch=8, batch_timeout_ms=2.0, gpu_jpeg_decode=False), engine=eng)
    try:
        assert not svc.gpu_decode
        ref, again = answers(svc), answers(svc)
    finally:
        svc.close()
    stable = ref == again
    print("default path run-to-run bit-stable at block1_conv1:", stable)
    svc = DeconvService(Config.from_env(device="cuda", max_batch=8, batch_timeout_ms=2.0, gpu_jpeg_decode=True), engine=eng)
    try:
        assert svc.gpu_decode and svc.status()["gpu_jpeg_decode"]
        before = paths()
        got = answers(svc)
        after = paths()
    finally:
        svc.close()
    assert after.get("gpu", 0) - before.get("gpu", 0) == 3
    assert after.get("pil", 0) - before.get("pil", 0) == 1
    assert after.get("pil_fallback", 0) == before.get("pil_fallback", 0)
    for g, r in zip(got, ref):
        a, b = parse_result_data_url(g), parse_result_data_url(r)
        assert a.shape == (448, 448, 3)
        if stable:
            assert g == r  # the engine is run-to-run bit-stable here: the responses are the same bytes
        else:  # tolerance of test_engine_gpu.py::test_service_end_to_end_gpu for the same comparison
            assert np.abs(a.astype(int) - b.astype(int)).mean() < 1.0
