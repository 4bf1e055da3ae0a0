"""The host JPEG encoder (csrc/jpeg_enc.cpp) against an exact oracle: tests/jpeg_ref.py splits the encoder at the
quantized coefficients, so the arithmetic half (colour, 4:2:0, DCT, quantization) is checked to the integer and the
entropy half (Huffman codes, ZRL / EOB, amplitude bits, padding, stuffing, restart markers) to the byte, over the
cases of tests/jpeg_enc_cases.py. The reference itself is checked first: on its own conditions, on PIL-encoded
files (which it must decode and re-encode bit for bit) and on damaged streams (which it must refuse)."""
import base64
import io
import os
import sys
from urllib.parse import quote

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_dec_cases as dec_cases  # noqa: E402
import jpeg_enc_cases as cases  # noqa: E402
import jpeg_ref as ref  # noqa: E402

from deconv_api_amd.codec.image import DATA_URL_PREFIX  # noqa: E402


def _native_or_skip():
    from deconv_api_amd.ops import native

    if not native.available():
        pytest.skip("native extension not built")
    return native.lib()


# ------------------------------------------------------------------ the reference on its own
def test_conditions():
    """Every builder's assertions (crafted coefficients, zero ambiguity of the exact cases, at most 1 % elsewhere)
    and the coverage of the whole set."""
    cs = cases.cases()
    assert [c.name for c in cs] == cases.names()
    assert max(c.ambiguous for c in cs) <= cases.MAX_AMBIGUOUS
    assert sum(c.exact for c in cs) == 8
    print("coverage:", cases.coverage())
    print("worst ambiguous share:", max((c.ambiguous, c.name) for c in cs))
    # the geometry the GPU kernel's two block slots need: 252 (one slot), 258 and 336 blocks (both) per segment
    assert sorted({6 * ((w + 15) // 16) for w in cases.GEOMETRY_W if w > 600}) == [252, 258, 336]
    assert (147 + 15) // 16 == 10  # more than 8 restart markers: RST7 -> RST0


def test_no_pixels_reach_ac_1023():
    """Why the coverage takes +-1020 for 2^10 - 1 and +-2040 for 2^11 - 1: no 8-bit block has a larger AC
    coefficient or DC difference, whatever the quantizer."""
    basis = np.einsum("vy,ux->vuyx", ref._DCT, ref._DCT).reshape(64, 64)
    assert abs(np.abs(basis[1:]).sum(1).max() * 127.5 - cases.AC_MAX) < 1e-9
    assert np.abs(basis[1:].sum(1)).max() < 1e-12
    assert abs(basis[0].sum() - 8) < 1e-12  # DC = 8 x the mean: -1024 .. 1016


def test_allowance_is_small_and_only_from_the_reference():
    for q, lo, hi in ((1, 1e-7, 1e-4), (50, 1e-6, 1e-4), (95, 1e-5, 1e-3), (100, 1e-4, 1e-3)):
        dl, dc = ref.delta(q)
        print(f"quality {q}: delta luma {dl:.3e} chroma {dc:.3e}")
        assert lo < dc <= dl < hi, (q, dl, dc)


def _pil(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_reference_round_trips_pil_files():
    """PIL's 4:2:0 files with the default tables are Annex K streams: the decoder reads them, its DHT tables are the
    ones typed into the reference, and the encoder writes PIL's scan back bit for bit (restart rows included)."""
    n = 0
    for h, w in ((16, 16), (17, 33), (100, 70), (1, 1), (147, 17)):
        for q in (30, 95, 100):
            for noisy in (False, True):
                for rows in (0, 1, 2):
                    data = _pil(dec_cases.picture(h, w, noisy), quality=q, subsampling=2, restart_marker_rows=rows)
                    r = ref.parse(data)
                    assert {k: r.dht[k] for k in ref.ANNEX_K} == ref.ANNEX_K
                    assert (r.H, r.W) == (h, w)
                    assert np.array_equal(r.qt[0], ref.quant_tables(q)[0]) and np.array_equal(r.qt[1], ref.quant_tables(q)[1])
                    spans = []
                    scan = ref.encode_scan(r.coef, rows, spans)
                    assert scan == data[r.scan[0]:r.scan[1]], (h, w, q, noisy, rows)
                    assert spans == r.spans
                    n += 1
    assert n == 90


def _same_as_native_parser(data, coef):
    """Where the native parser accepts a file its coefficients are the reference decoder's. -> accepted?"""
    from deconv_api_amd.codec import parse_jpeg_coeffs

    c = parse_jpeg_coeffs(data)
    if c is None:
        return False
    nat = cases.natural_coeffs(c)
    assert len(nat) == len(coef) and all(np.array_equal(a, b) for a, b in zip(nat, coef))
    return True


def test_reference_decoder_equals_native_parser_on_pil_files():
    """Every file of the decode tests' matrix (all samplings, optimized tables, restart intervals, greyscale)."""
    _native_or_skip()
    files = [f for f in dec_cases.matrix() if not f[0].startswith(("224x224", "480x640"))]
    accepted = sum(_same_as_native_parser(data, ref.parse(data).coef) for _, data, _ in files)
    assert accepted == len(files)


def _reference_stream():
    data = _pil(dec_cases.picture(40, 40, True), quality=95, subsampling=2, restart_marker_rows=1)
    r = ref.parse(data)
    assert len(r.spans) == 3 and any(r.pad)
    return data, r


def test_reference_decoder_refuses_damaged_streams():
    data, r = _reference_stream()
    s0, s1 = r.scan
    a1 = s0 + r.spans[1][0]  # first byte of the second segment; the RST0 marker ends at a1
    assert data[a1 - 2:a1] == b"\xff\xd0"
    si = next(i for i, p in enumerate(r.pad) if p and data[s0 + r.spans[i][1] - 2] != 0xFF)
    end = s0 + r.spans[si][1]
    bad = {
        "RST number": data[:a1 - 1] + b"\xd1" + data[a1:],
        "RST missing": data[:a1 - 2] + data[a1:],
        "0-bit padding": data[:end - 1] + bytes([data[end - 1] & ~1 & 0xFF]) + data[end:],
        "trailing byte before EOI": data[:s1] + b"\x7f" + data[s1:],
        "trailing byte before RST": data[:a1 - 2] + b"\x55" + data[a1 - 2:],
        "unstuffed FF": data[:s0 + 3] + b"\xff\x01" + data[s0 + 5:],
        "bytes after EOI": data + b"\x00",
        "truncated": data[:s0 + (s1 - s0) // 2] + b"\xff\xd9",
        "segment missing": data[:a1 - 2] + b"\xff\xd9",
    }
    for what, d in bad.items():
        with pytest.raises(ref.JpegError):
            ref.parse(d)
            pytest.fail(f"accepted: {what}")
    # an invalid code: sixteen 1-bits is no code of any Annex K table
    with pytest.raises(ref.JpegError, match="bad Huffman code"):
        ref.parse(data[:s0] + b"\xff\x00\xff\x00\xff\x00" + data[s0 + 6:])


def test_reference_encoder_and_decoder_agree_on_every_case():
    """decode(header + encode(coefficients)) gives the coefficients back, with a restart marker per MCU row and with
    none: the reference's two halves are written independently and check each other."""
    from deconv_api_amd.codec.image import encode_jpeg_pil

    for c in cases.cases():
        if c.B > 3:
            continue
        head = encode_jpeg_pil(c.images[0], c.quality)
        head = head[:ref.parse(head, header_only=True).scan[0]]
        i = head.index(b"\xff\xda")
        for rows in (0, 1):
            mcux, mcuy = (c.W + 15) // 16, (c.H + 15) // 16
            dri = b"\xff\xdd\x00\x04" + (rows * mcux).to_bytes(2, "big") if rows and mcuy > 1 else b""
            for co in c.coef:
                r = ref.parse(head[:i] + dri + head[i:] + ref.encode_scan(co, rows) + b"\xff\xd9")
                assert all(np.array_equal(a, b) for a, b in zip(r.coef, co)), (c.name, rows)


# ------------------------------------------------------------------ the host encoder
def _url_bytes(url: str) -> bytes:
    """The JPEG inside a response string, which must be exactly prefix + quote(base64(jpeg))."""
    assert url.startswith(DATA_URL_PREFIX)
    jpg = base64.b64decode(url[len(DATA_URL_PREFIX):].replace("%2B", "+").replace("%3D", "="), validate=True)
    assert url == DATA_URL_PREFIX + quote(base64.b64encode(jpg).decode())
    return jpg


def _rows_per_segment(threads: int, B: int, H: int) -> int:
    """encode_data_urls: with fewer images than threads each image is split into min(ceil(threads / B), MCU rows)
    restart segments of equal whole MCU rows. -> rows per segment, 0 for a single segment."""
    mcuy = (H + 15) // 16
    segments = max(1, min(-(-threads // B), mcuy))
    rows = -(-mcuy // segments)
    return rows if -(-mcuy // rows) > 1 else 0


@pytest.mark.parametrize("name", cases.names())
def test_host_encoder(name):
    lib = _native_or_skip()
    c = cases.by_name(name)
    batch = torch.from_numpy(c.images)
    coefs = []
    for b in range(c.B):
        jpg = lib.jpeg_encode(batch[b], c.quality)
        C, _, _ = ref.check_stream(jpg, c.images[b], c.quality, 0, x=c.x[b], exact=c.coef[b] if c.exact else None,
                                   what=f"{name}[{b}] jpeg_encode: ")
        coefs.append(C)
        _same_as_native_parser(jpg, C)
    for threads in (1, 3, 7):
        # one image per call: the threads share its MCU rows (restart segments); then the whole batch
        calls = [(b, batch[b:b + 1]) for b in range(min(c.B, 3))] + ([(0, batch)] if c.B > 1 else [])
        for b0, imgs in calls:
            urls = lib.jpeg_data_urls(imgs.contiguous(), c.quality, DATA_URL_PREFIX, threads)
            assert len(urls) == imgs.shape[0]
            rows = _rows_per_segment(threads, imgs.shape[0], c.H)
            for k, u in enumerate(urls):
                ref.check_stream(_url_bytes(u), c.images[b0 + k], c.quality, rows, x=c.x[b0 + k], coef=coefs[b0 + k],
                                 what=f"{name}[{b0 + k}] jpeg_data_urls({threads} threads): ")


def test_host_encoder_writes_restart_segments():
    """The cases do reach the restart path: 3 and 7 threads split the 147-row image into 3 and 5 segments."""
    assert [_rows_per_segment(t, 1, 147) for t in (1, 3, 7)] == [0, 4, 2]
    lib = _native_or_skip()
    c = cases.by_name("geo_147x17")
    for threads, nseg in ((3, 3), (7, 5)):
        jpg = _url_bytes(lib.jpeg_data_urls(torch.from_numpy(c.images), c.quality, DATA_URL_PREFIX, threads)[0])
        assert len(ref.parse(jpg).spans) == nseg
