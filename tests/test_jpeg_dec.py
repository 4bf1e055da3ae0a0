"""GPU JPEG decode, host side: the native entropy decoder (csrc/jpeg_dec.cpp) + the CPU reference of the
device steps (ops/jpeg_dec.py) are bit-identical to PIL; everything outside the accepted subset falls back
to PIL; the front-end transport carries coefficient frames (serve/ingest.py kind 6)."""
import base64
import io
import json
import os
import re
import socket
import sys
import tempfile
import threading

import numpy as np
import pytest
from PIL import Image

from deconv_api_amd.codec import ImageDecodeError, JpegCoeffs, decode_image, parse_jpeg_coeffs, read_data_url
from deconv_api_amd.codec import image as codec_image
from deconv_api_amd.ops import jpeg_coeffs_to_rgb, jpeg_dec
from deconv_api_amd.serve import ingest as I

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_dec_cases as cases  # noqa: E402



@pytest.fixture(autouse=True)
def _built(native_lib):
    """The parser is native code: a missing build is a failure here, not a skip."""


def _url(data: bytes, mime: str = "jpeg") -> str:
    return f"data:image/{mime};base64," + base64.b64encode(data).decode()


def test_parser_and_reference_are_bit_identical_to_pil():
    bad = []
    for name, data, want in cases.matrix():
        c = parse_jpeg_coeffs(data)
        if c is None:
            bad.append((name, "not accepted"))
            continue
        got = jpeg_dec.decode_ref(c)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append((name, "differs from PIL"))
    assert not bad, bad[:10]
    assert len(cases.matrix()) == 9 * 3 * 4 * 2 * 3 + 3 + 2


def test_ops_cpu_path_and_data_url_form():
    name, data, want = cases.matrix()[100]
    c = read_data_url(_url(data), coeffs=True)
    assert isinstance(c, JpegCoeffs) and c.shape == want.shape and c.size == want.size
    (out,) = jpeg_coeffs_to_rgb([c], "cpu")
    assert np.array_equal(out.numpy(), want)
    assert isinstance(read_data_url(_url(data)), np.ndarray)  # the default call is unchanged


def test_idct_weight_bound_quoted_by_the_parser():
    """csrc/jpeg_dec.cpp's exactness bound assumes a pass's output weights are <= 11400."""
    assert jpeg_dec.idct_gain() <= 11400


def _exif_orientation(o: int) -> bytes:
    ex = Image.Exif()
    ex[0x0112] = o
    return ex.tobytes()


def _segments(data: bytes):
    """[(marker, payload)] of the segments before the scan, and the rest (from SOS on)."""
    out, p = [], 2
    while data[p + 1] != 0xDA:
        n = int.from_bytes(data[p + 2:p + 4], "big")
        out.append((data[p + 1], data[p + 4:p + 2 + n]))
        p += 2 + n
    return out, data[p:]


def _rgb_ids_with_app0(app0: bytes) -> bytes:
    """A 4:4:4 file whose component ids are 'R', 'G', 'B' and whose APP0 payload is ``app0``: libjpeg takes it
    for YCbCr only if it honours the JFIF marker (14 bytes at least)."""
    segs, rest = _segments(cases.save(cases.picture(16, 16, False), quality=90, subsampling=0))
    out = b"\xff\xd8"
    for m, pl in segs:
        if m == 0xE0:
            pl = app0
        elif m == 0xC0:
            pl = bytearray(pl)
            pl[6], pl[9], pl[12] = b"RGB"
            pl = bytes(pl)
        out += bytes([0xFF, m]) + (len(pl) + 2).to_bytes(2, "big") + pl
    rest = bytearray(rest)  # SOS: FF DA, length, Ns, then (id, tables) pairs
    rest[5], rest[7], rest[9] = b"RGB"
    return out + bytes(rest)


def _fallback_files():
    img = cases.picture(40, 56, False)
    base = cases.save(img, quality=90)
    png = io.BytesIO()
    Image.fromarray(img).save(png, format="PNG")
    cmyk = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(cmyk, format="JPEG", quality=90)
    return {
        "progressive": cases.save(img, quality=90, progressive=True),
        "cmyk": cmyk.getvalue(),
        "exif_orientation_6": cases.save(img, quality=90, exif=_exif_orientation(6)),
        "png": png.getvalue(),
        "truncated_mid_scan": base[: len(base) - len(base) // 3],
        "jfif_5_byte_app0_rgb_ids": _rgb_ids_with_app0(b"JFIF\0"),
        "jfif_13_byte_app0_rgb_ids": _rgb_ids_with_app0(b"JFIF\0\1\1\0\0\1\0\1\0"),
    }


@pytest.mark.parametrize("kind", ["progressive", "cmyk", "exif_orientation_6", "png", "truncated_mid_scan",
                                  "jfif_5_byte_app0_rgb_ids", "jfif_13_byte_app0_rgb_ids"])
def test_unsupported_files_fall_back_to_pil(kind):
    data = _fallback_files()[kind]
    assert parse_jpeg_coeffs(data) is None
    try:
        want = decode_image(data)
    except ImageDecodeError as e:  # PIL decides the response: the same error either way
        with pytest.raises(ImageDecodeError) as got:
            read_data_url(_url(data), coeffs=True)
        strip = lambda m: re.sub(r"0x[0-9a-f]+", "0x", m)  # PIL quotes the BytesIO object's address
        assert strip(str(got.value)) == strip(str(e))
        return
    got = read_data_url(_url(data), coeffs=True)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)


def test_rgb_ids_with_a_full_jfif_app0_are_ycbcr():
    """The accepted side of the two JFIF fallbacks: 14 bytes of JFIF make libjpeg (and the parser) read YCbCr."""
    data = _rgb_ids_with_app0(b"JFIF\0\1\1\0\0\1\0\1\0\0")
    c = parse_jpeg_coeffs(data)
    assert c is not None and np.array_equal(jpeg_dec.decode_ref(c), decode_image(data))


# ---- the exactness bound (csrc/jpeg_dec.cpp:block_in_bounds) ----
def _heavy_block(targets: dict, img=None):
    """An 8x8 greyscale file whose quantizer columns are scaled so that the L1 norm of the dequantized
    values of column c is just below targets[c] (the other columns keep q = 1: norms of a few dozen).
    -> (file, the eight column norms)."""
    if img is None:
        img = np.random.default_rng(7).integers(120, 137, (8, 8)).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", qtables=[[1] * 64])
    data = buf.getvalue()
    co = np.abs(parse_jpeg_coeffs(data).coef.reshape(8, 8).astype(np.int64))  # [column, row]
    q = np.ones((8, 8), np.int64)  # natural order: [row, column]
    for c, t in targets.items():
        q[:, c] = t // co[c].sum()
    norms = (co * q.T).sum(1)
    natural = [int(v) for v in q.reshape(-1)]
    zz = sorted(range(64), key=lambda i: _ZIGZAG_RANK[i])
    seg = bytes([0x10]) + b"".join(natural[i].to_bytes(2, "big") for i in zz)  # one 16-bit table, id 0
    i = data.index(b"\xff\xdb")
    n = int.from_bytes(data[i + 2:i + 4], "big")
    return data[:i] + b"\xff\xdb" + (len(seg) + 2).to_bytes(2, "big") + seg + data[i + 2 + n:], norms


# rank of each natural index in zig-zag order
_ZIGZAG_RANK = [0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31,
                40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59,
                61, 35, 36, 48, 49, 57, 58, 62, 63]


@pytest.mark.parametrize("targets", [{0: 2930, 4: 2920}, {7: 2930, 3: 2920}, {5: 2930, 1: 2920}, {0: 5700}, {2: 5790},
                                     {6: 5790, 2: 5790}, {4: 5600}, {0: 2930, 4: 2920, 2: 5790}],
                         ids=lambda t: "-".join(f"c{c}_{v}" for c, v in t.items()))
def test_blocks_just_inside_the_exactness_bound_equal_pil(targets):
    """Column norms right below the bound (each <= 5800; the pairs (0, 4), (7, 3), (5, 1) that libjpeg-turbo's
    SIMD IDCT adds in 16 bits together <= about 5880): accepted, and still PIL's pixels."""
    data, norms = _heavy_block(targets)
    assert all(0.97 * t <= norms[c] <= t for c, t in targets.items()), norms
    c = parse_jpeg_coeffs(data)
    assert c is not None, norms
    assert np.array_equal(jpeg_dec.decode_ref(c), cases.oracle(data)), norms


@pytest.mark.parametrize("targets", [{0: 5760, 4: 5120}, {0: 3010, 4: 3010}, {7: 3010, 3: 3010}, {5: 3010, 1: 3010},
                                     {2: 5900}, {0: 5790, 4: 400}],
                         ids=lambda t: "-".join(f"c{c}_{v}" for c, v in t.items()))
def test_blocks_just_outside_the_exactness_bound_fall_back(targets):
    """One column norm above 5800, or a 16-bit pair above its sum: not accepted, and the caller gets PIL's
    decode."""
    data, norms = _heavy_block(targets)
    assert all(0.97 * t <= norms[c] <= t for c, t in targets.items()), norms
    assert parse_jpeg_coeffs(data) is None
    got = read_data_url(_url(data), coeffs=True)
    assert isinstance(got, np.ndarray) and np.array_equal(got, decode_image(data))


def test_the_pair_bound_is_needed():
    """Why the pairs are bounded: with all of columns 0 and 4 in one row (a flat image plus one horizontal
    cosine), in0 + in4 of that row leaves int16 in libjpeg-turbo's SIMD pass 2, and the exact integer IDCT of
    the same coefficients is no longer what PIL decodes. The parser hands such a file to PIL."""
    import dataclasses

    x = np.arange(8)
    img = np.tile(np.round(168 + 45 * np.cos((2 * x + 1) * 4 * np.pi / 16)), (8, 1)).astype(np.uint8)
    data, norms = _heavy_block({0: 5760, 4: 5120}, img)
    assert norms[0] > 5600 and norms[4] > 5000 and max(norms[c] for c in (1, 2, 3, 5, 6, 7)) < 50, norms
    assert parse_jpeg_coeffs(data) is None
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", qtables=[[1] * 64])
    c = parse_jpeg_coeffs(buf.getvalue())
    q = np.ones((8, 8), np.int64)
    co = np.abs(c.coef.reshape(8, 8).astype(np.int64))
    q[:, 0], q[:, 4] = 5760 // co[0].sum(), 5120 // co[4].sum()
    exact = jpeg_dec.decode_ref(dataclasses.replace(c, qt=q.reshape(1, 64).astype(np.uint16)))
    assert not np.array_equal(exact, cases.oracle(data))
    for targets in ({0: 2930, 4: 2920}, {0: 5700}, {4: 5400}):  # the same concentrated block inside the bound
        inside, norms = _heavy_block(targets, img)
        c = parse_jpeg_coeffs(inside)
        assert c is not None and np.array_equal(jpeg_dec.decode_ref(c), cases.oracle(inside)), (targets, norms)


def test_exif_orientation_1_is_accepted():
    data = cases.save(cases.picture(24, 40, False), quality=90, exif=_exif_orientation(1))
    c = parse_jpeg_coeffs(data)
    assert c is not None and np.array_equal(jpeg_dec.decode_ref(c), decode_image(data))


def test_file_over_max_pixels_falls_back(monkeypatch):
    data = cases.save(cases.picture(40, 56, False), quality=90)
    assert parse_jpeg_coeffs(data) is not None
    monkeypatch.setattr(codec_image, "MAX_PIXELS", 40 * 56 - 1)
    assert parse_jpeg_coeffs(data) is None  # refused from the SOF header, before decoding
    with pytest.raises(ImageDecodeError, match="too large"):
        decode_image(data)
    with pytest.raises(ImageDecodeError, match="too large"):
        read_data_url(_url(data), coeffs=True)


def test_http_load_corpus_is_accepted_whole():
    """Pillow's default baseline JFIF 4:2:0 output is inside the accepted subset: no fallback on the
    load generator's JPEGs, and the decode is PIL's."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from http_load import corpus

    urls = corpus(64, png_every=0)
    for i, (u, kind) in enumerate(urls):
        c = read_data_url(u, coeffs=True)
        assert isinstance(c, JpegCoeffs), (i, kind)
        if i % 8 == 0:
            assert np.array_equal(jpeg_dec.decode_ref(c), read_data_url(u)), (i, kind)


# ------------------------------------------------------------------ transport
class _Cfg:
    jpeg_quality = 95


class _Engine:
    names = ["input_1", "block1_conv1"]


class _Svc:
    cfg = _Cfg()
    engine = _Engine()
    gpu_decode = True

    def __init__(self):
        self.seen = []

    def submit(self, layer, img, done):
        self.seen.append(img)
        threading.Thread(target=done, args=("ok", None)).start()

    def layer_names(self):
        return ["block1_conv1"]


@pytest.fixture()
def server():
    d = tempfile.mkdtemp(prefix="dv-ingest-jpeg-")
    path = os.path.join(d, "s.sock")
    svc = _Svc()
    srv = I.IngestServer(path, svc)
    yield path, svc
    srv.close()
    os.rmdir(d)


def test_ingest_coefficient_frame_round_trip(server):
    path, svc = server
    c = parse_jpeg_coeffs(cases.matrix()[-2][1])  # 224x224, 4:2:0
    g = parse_jpeg_coeffs(cases.matrix()[-4][1])  # greyscale
    cli = I.IngestClient(path, connect_timeout=10)
    try:
        st, body = cli.call(I.LAYERS)
        assert st == 200 and json.loads(body)["gpu_jpeg_decode"] is True
        for src in (c, g):
            ev, box = threading.Event(), {}
            cli.send_jpeg(lambda s, d: (box.update(r=(s, d)), ev.set()), "block1_conv1", src, decode_s=0.001)
            assert ev.wait(10) and box["r"] == (200, b"ok")
            got = svc.seen[-1]
            assert isinstance(got, JpegCoeffs) and (got.H, got.W, got.ncomp, got.kind) == (src.H, src.W, src.ncomp, src.kind)
            assert np.array_equal(got.qt, src.qt) and np.array_equal(got.coef, src.coef)
            assert np.array_equal(jpeg_dec.decode_ref(got), jpeg_dec.decode_ref(src))
    finally:
        cli.close()


@pytest.mark.parametrize("lie", ["short", "kind", "pixels", "switch_off"])
def test_ingest_rejects_inconsistent_coefficient_frames(server, lie, monkeypatch):
    path, svc = server
    h, w, kind, ncomp = 16, 16, 2, 3
    nbytes = I.JPEG_HEAD.size + ncomp * 128 + 128 * jpeg_dec.total_blocks(h, w, kind)
    if lie == "short":
        nbytes -= 2
    elif lie == "kind":
        ncomp = 1  # three-component sampling, one component
    elif lie == "pixels":
        h = w = int(I.MAX_PIXELS ** 0.5) + 1
        nbytes = I.JPEG_HEAD.size + ncomp * 128 + 128 * jpeg_dec.total_blocks(h, w, kind)
    else:
        monkeypatch.setattr(svc, "gpu_decode", False, raising=False)
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.connect(path)
    try:
        s.sendall(I.REQ.pack(9, I.DECONV_JPEG, 0, 0, h, w, nbytes, 0) + I.JPEG_HEAD.pack(ncomp, kind, 0))
        rid, st, n = I.RESP.unpack(I._recv_exact(s, I.RESP.size))
        assert rid == 9 and st == 400 and I._recv_exact(s, n)
    finally:
        s.close()
    assert svc.seen == []


def test_decode_kernels_compile_with_debug_bounds_checks(tmp_path):
    """The DV_DEBUG build of the decode kernels (common.h DV_BOUNDS on every load and store) compiles for
    gfx950; the pattern of tests/test_debug_build.py."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed to compile the kernels"
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deconv_api_amd", "csrc")
    src = os.path.join(csrc, "jpeg_dec_gpu.hip")
    assert open(src).read().count("DV_BOUNDS(") >= 5
    obj = tmp_path / "jpeg_dec_gpu.o"
    cmd = [hipcc, "-O1", "-DDV_DEBUG=1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wno-unused-result",
           f"-I{csrc}", "-c", src, "-o", str(obj)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    assert obj.stat().st_size > 0
