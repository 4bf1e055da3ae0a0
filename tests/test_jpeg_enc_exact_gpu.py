"""The GPU JPEG encoder (csrc/jpeg_gpu.hip: jpeg_segment, jpeg_offsets, jpeg_copy) against the exact oracle of
tests/jpeg_ref.py, over the cases of tests/jpeg_enc_cases.py (whose conditions tests/test_jpeg_enc_exact.py asserts
on the CPU): every quantized coefficient outside the rounding allowance has its one right value, and the packed
scans, the restart markers, every off[b] and every segment's span equal the reference entropy encoder's bytes."""
import base64
import os
import sys
from urllib.parse import quote

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_cases as cases  # noqa: E402
import jpeg_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _encode(c):
    """-> (packed scans on the host, off as a list) of the whole batch of a case."""
    from deconv_api_amd.codec import image as ci

    packed, off = ci.encode_gpu(torch.from_numpy(c.images).cuda(), c.quality)
    torch.cuda.synchronize()
    assert off.dtype == torch.int64 and off.shape == (c.B + 1,)
    off_h = off.cpu()
    return packed[: int(off_h[-1])].cpu(), off_h


@pytest.mark.parametrize("name", cases.names())
def test_gpu_encoder(native_lib, name):
    from deconv_api_amd.codec import image as ci
    from deconv_api_amd.codec import parse_jpeg_coeffs

    c = cases.by_name(name)
    packed_h, off_h = _encode(c)
    off = off_h.tolist()
    assert off[0] == 0
    urls = ci.gpu_data_urls(packed_h, off_h, c.H, c.W, c.quality)
    assert len(urls) == c.B
    pos = 0
    for b in range(c.B):
        jpg = ci.gpu_jpeg_bytes(packed_h, off_h, b, c.H, c.W, c.quality)
        C, scan, spans = ref.check_stream(jpg, c.images[b], c.quality, 1, x=c.x[b],
                                          exact=c.coef[b] if c.exact else None, what=f"{name}[{b}]: ")
        # the offsets kernel: image b starts where the reference's scans of images 0 .. b - 1 end
        assert off[b] == pos and off[b + 1] == pos + len(scan), (b, off[b], off[b + 1], pos, len(scan))
        assert bytes(packed_h[off[b]:off[b + 1]].numpy()) == scan
        assert len(spans) == (c.H + 15) // 16
        pos += len(scan)
        assert urls[b] == ci.DATA_URL_PREFIX + quote(base64.b64encode(jpg).decode()), (name, b)
        parsed = parse_jpeg_coeffs(jpg)
        if parsed is not None:  # the native parser keeps to blocks inside its exactness bound
            assert all(np.array_equal(p, q) for p, q in zip(cases.natural_coeffs(parsed), C)), (name, b)
    assert off[c.B] == pos


@pytest.mark.parametrize("name", [n for n in cases.names()[:8]])
def test_gpu_and_host_streams_of_exact_cases_decode_alike(native_lib, name):
    from deconv_api_amd.codec import image as ci

    c = cases.by_name(name)
    assert c.exact
    packed_h, off_h = _encode(c)
    for b in range(c.B):
        g = ref.parse(ci.gpu_jpeg_bytes(packed_h, off_h, b, c.H, c.W, c.quality))
        h = ref.parse(native_lib.jpeg_encode(torch.from_numpy(c.images[b]), c.quality))
        assert all(np.array_equal(p, q) for p, q in zip(g.coef, h.coef))
        assert all(np.array_equal(p, q) for p, q in zip(g.coef, c.coef[b]))
        assert len(g.spans) == (c.H + 15) // 16 and len(h.spans) == 1
