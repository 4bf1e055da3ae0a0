"""A reference for baseline JPEG encoding, written from the standard (ITU-T T.81, JFIF / T.871) and independent
of csrc/jpeg_enc.cpp and csrc/jpeg_gpu.hip. It splits an encoder at the quantized coefficients:

  * ``parse``        a stream parser + Huffman decoder (T.81 B, C, F.2): raises ``JpegError`` on any anomaly;
  * ``forward``      colour, 4:2:0, 8x8 DCT-II by the cosine matrix and the division by the quantizer, all in
                     float64, returned UNROUNDED;
  * ``encode_scan``  an Annex F entropy encoder over the Annex K tables typed in below;
  * ``delta``        the rounding allowance of one quality: 8 x the worst deviation of a float32, FMA-free
                     AAN pipeline from ``forward`` on 4096 fixed noise blocks per table. It is measured against
                     this reference alone, never against an encoder;
  * ``check_stream`` the check both encoders are held to: every coefficient farther than delta from a .5 boundary
                     has one right value, and the scan bytes equal ``encode_scan`` of the decoded coefficients.

Coefficient arrays are int / float [block rows, block columns, 64] per component, natural (row-major) order.
"""
import functools

import numpy as np


class JpegError(ValueError):
    pass


# ---- T.81 Annex K.1 quantizers (natural order), Figure A.6 zig-zag, Annex K.3 Huffman tables ----
LUMA_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99])
CHROMA_Q = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def _zigzag():
    """zig-zag position -> natural index, walked along the anti-diagonals (Figure A.6)."""
    out = []
    for s in range(15):
        rows = range(max(0, s - 7), min(7, s) + 1)
        for r in (rows if s % 2 else reversed(rows)):  # even diagonals run upwards (row decreasing)
            out.append(r * 8 + s - r)
    return np.array(out)


ZIGZAG = _zigzag()

_AC_HEX_LUMA = (
    "01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 62 72 "
    "82 09 0a 16 17 18 19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 "
    "5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 "
    "a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 "
    "e3 e4 e5 e6 e7 e8 e9 ea f1 f2 f3 f4 f5 f6 f7 f8 f9 fa")
_AC_HEX_CHROMA = (
    "00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 15 62 72 d1 "
    "0a 16 24 34 e1 25 f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 "
    "59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 82 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a "
    "a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da "
    "e2 e3 e4 e5 e6 e7 e8 e9 ea f2 f3 f4 f5 f6 f7 f8 f9 fa")
# (class, id) -> (BITS: codes of each length 1..16, HUFFVAL); class 0 = DC, 1 = AC; id 0 = luminance, 1 = chrominance
ANNEX_K = {
    (0, 0): ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),                      # Table K.3
    (0, 1): ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),                      # Table K.4
    (1, 0): ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), tuple(bytes.fromhex(_AC_HEX_LUMA))),  # Table K.5
    (1, 1): ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), tuple(bytes.fromhex(_AC_HEX_CHROMA))),  # Table K.6
}
assert all(sum(b) == len(v) for b, v in ANNEX_K.values())


def quant_tables(quality: int):
    """The IJG scaling of the Annex K.1 tables -> (luma, chroma), natural order."""
    q = min(100, max(1, int(quality)))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (LUMA_Q, CHROMA_Q))


def huff_codes(bits, vals):
    """Annex C: symbol -> (code, length)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _decode_lut(bits, vals):
    """16-bit prefix -> length << 8 | symbol (0: no code has this prefix)."""
    lut = np.zeros(1 << 16, np.int32)
    for sym, (code, length) in huff_codes(bits, vals).items():
        lo = code << (16 - length)
        if lo + (1 << (16 - length)) > (1 << 16):
            raise JpegError("DHT: code lengths overflow 16 bits")
        lut[lo:lo + (1 << (16 - length))] = (length << 8) | sym
    return lut.tolist()


def round_half_away(x):
    x = np.asarray(x, np.float64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


# ------------------------------------------------------------------ parser / decoder
class Parsed:
    """H, W; comps [(id, h, v, quantizer id)]; qt {id: 64 values, natural order}; dht {(class, id): (BITS, HUFFVAL)};
    dri (MCUs, 0: none); scan_tabs [(DC id, AC id)] per component; coef [int32 [bh, bw, 64]] per component;
    scan = (first entropy-coded byte, offset of EOI); spans [(start, end)] of each restart segment's bytes, relative
    to scan[0], RSTm excluded; pad [padding bits of each segment]."""


def _segment_bits(raw: bytes, what: str):
    """Entropy-coded bytes of one restart segment -> unstuffed bytes; any marker inside is an error."""
    p = raw.find(b"\xff")
    while p >= 0:
        if p + 1 >= len(raw) or raw[p + 1] != 0:
            raise JpegError(f"{what}: FF not followed by 00 at byte {p}")
        p = raw.find(b"\xff", p + 2)
    return raw.replace(b"\xff\x00", b"\xff")


def parse(data: bytes, header_only: bool = False) -> Parsed:
    """The whole stream; ``header_only``: SOI .. SOS alone (``scan`` = (first entropy-coded byte, None))."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise JpegError("no SOI")
    r = Parsed()
    r.qt, r.dht, r.dri, r.comps = {}, {}, 0, None
    p = 2
    while True:
        if p + 4 > len(data) or data[p] != 0xFF:
            raise JpegError(f"marker expected at {p}")
        m = data[p + 1]
        n = int.from_bytes(data[p + 2:p + 4], "big")
        body = data[p + 4:p + 2 + n]
        if n < 2 or len(body) != n - 2:
            raise JpegError(f"segment {m:02x}: bad length")
        if m == 0xDB:
            q = 0
            while q < len(body):
                pq, tq = body[q] >> 4, body[q] & 15
                size = 128 if pq else 64
                if pq > 1 or tq > 3 or q + 1 + size > len(body):
                    raise JpegError("DQT: bad table")
                v = np.frombuffer(body[q + 1:q + 1 + size], ">u2" if pq else "u1").astype(np.int64)
                nat = np.zeros(64, np.int64)
                nat[ZIGZAG] = v
                r.qt[tq] = nat
                q += 1 + size
        elif m == 0xC0:
            if body[0] != 8 or r.comps is not None:
                raise JpegError("SOF0: precision / repeated")
            r.H, r.W = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            nc = body[5]
            if len(body) != 6 + 3 * nc or r.H < 1 or r.W < 1:
                raise JpegError("SOF0: bad size")
            r.comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nc)]
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise JpegError(f"frame type {m:02x} is not baseline")
        elif m == 0xC4:
            q = 0
            while q < len(body):
                tc, th = body[q] >> 4, body[q] & 15
                bits = tuple(body[q + 1:q + 17])
                if tc > 1 or th > 3 or len(bits) != 16 or q + 17 + sum(bits) > len(body):
                    raise JpegError("DHT: bad table")
                r.dht[(tc, th)] = (bits, tuple(body[q + 17:q + 17 + sum(bits)]))
                q += 17 + sum(bits)
        elif m == 0xDD:
            if n != 4:
                raise JpegError("DRI: bad length")
            r.dri = int.from_bytes(body, "big")
        elif m == 0xDA:
            if r.comps is None or body[0] != len(r.comps) or len(body) != 4 + 2 * body[0]:
                raise JpegError("SOS: components")
            if [body[1 + 2 * i] for i in range(body[0])] != [c[0] for c in r.comps]:
                raise JpegError("SOS: component order")
            r.scan_tabs = [(body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(body[0])]
            if tuple(body[-3:]) != (0, 63, 0):
                raise JpegError("SOS: not a sequential full-band scan")
            p += 2 + n
            break
        elif not (0xE0 <= m <= 0xEF or m == 0xFE):
            raise JpegError(f"unexpected marker {m:02x}")
        p += 2 + n
    if header_only:
        r.scan = (p, None)
    else:
        _decode_scan(r, data, p)
    return r


def _decode_scan(r: Parsed, data: bytes, start: int):
    nc = len(r.comps)
    hmax, vmax = max(c[1] for c in r.comps), max(c[2] for c in r.comps)
    if nc == 1:  # a single-component scan is not interleaved: one block per MCU
        mcux, mcuy, per = (r.W + 7) // 8, (r.H + 7) // 8, [(1, 1)]
    else:
        mcux, mcuy = -(-r.W // (8 * hmax)), -(-r.H // (8 * vmax))
        per = [(c[1], c[2]) for c in r.comps]
    r.mcux, r.mcuy = mcux, mcuy
    r.coef = [np.zeros((mcuy * v, mcux * h, 64), np.int32) for h, v in per]
    luts = []
    for (td, ta), c in zip(r.scan_tabs, r.comps):
        if (0, td) not in r.dht or (1, ta) not in r.dht or c[3] not in r.qt:
            raise JpegError("a table the scan names is missing")
        luts.append((_decode_lut(*r.dht[(0, td)]), _decode_lut(*r.dht[(1, ta)])))
    # cut the scan at its markers: FF 00 is data, FF D0..D7 ends a segment, FF D9 ends the scan
    pieces, rst, p, seg0 = [], [], start, start
    while True:
        p = data.find(b"\xff", p)
        if p < 0 or p + 1 >= len(data):
            raise JpegError("scan: no EOI")
        m = data[p + 1]
        if m == 0:
            p += 2
        elif 0xD0 <= m <= 0xD7:
            pieces.append((seg0, p))
            rst.append(m - 0xD0)
            p += 2
            seg0 = p
        elif m == 0xD9:
            pieces.append((seg0, p))
            break
        else:
            raise JpegError(f"scan: marker {m:02x} at {p}")
    if p + 2 != len(data):
        raise JpegError("bytes after EOI")
    total = mcux * mcuy
    ri = r.dri if r.dri else total
    if len(pieces) != -(-total // ri):
        raise JpegError(f"{len(pieces)} restart segments, {-(-total // ri)} expected")
    if rst != [i % 8 for i in range(len(rst))]:
        raise JpegError(f"RSTm sequence {rst[:12]}")
    r.scan = (start, p)
    r.spans = [(a - start, b - start) for a, b in pieces]
    r.pad = []
    zz = ZIGZAG.tolist()
    mcu = 0
    for si, (a, b) in enumerate(pieces):
        buf = _segment_bits(data[a:b], f"segment {si}")
        nbits = 8 * len(buf)
        acc = have = bp = used = 0  # acc holds `have` unread bits; `used` bits are consumed
        pred = [0] * nc
        for _ in range(min(ri, total - mcu)):
            my, mx = divmod(mcu, mcux)
            for ci in range(nc):
                h, v = per[ci]
                dlut, alut = luts[ci]
                plane = r.coef[ci]
                for by in range(v):
                    for bx in range(h):
                        blk = plane[my * v + by, mx * h + bx]
                        k = 0
                        while k < 64:
                            if have < 32:  # past the end the reader sees 1-bits; `used` is checked below
                                acc &= (1 << have) - 1
                                while have < 32:
                                    acc = (acc << 8) | (buf[bp] if bp < len(buf) else 0xFF)
                                    bp += 1
                                    have += 8
                            e = (alut if k else dlut)[(acc >> (have - 16)) & 0xFFFF]
                            ln, sym = e >> 8, e & 0xFF
                            if ln == 0:
                                raise JpegError(f"segment {si}: bad Huffman code at bit {used}")
                            have -= ln
                            size = sym & 15
                            if k == 0:
                                if sym > 11:
                                    raise JpegError(f"segment {si}: DC category {sym}")
                                size = sym
                            val = 0
                            if size:
                                bits = (acc >> (have - size)) & ((1 << size) - 1)
                                have -= size
                                val = bits if bits >> (size - 1) else bits - (1 << size) + 1
                            used += ln + size
                            if k == 0:
                                pred[ci] += val
                                blk[0] = pred[ci]
                                k = 1
                            elif size == 0:
                                if sym == 0xF0:
                                    k += 16
                                    if k > 63:
                                        raise JpegError(f"segment {si}: ZRL past coefficient 63")
                                elif sym == 0:
                                    break
                                else:
                                    raise JpegError(f"segment {si}: AC symbol {sym:02x}")
                            else:
                                k += sym >> 4
                                if k > 63:
                                    raise JpegError(f"segment {si}: run past coefficient 63")
                                blk[zz[k]] = val
                                k += 1
                        if used > nbits:
                            raise JpegError(f"segment {si}: ran out of bits")
            mcu += 1
        left = nbits - used
        if left >= 8:
            raise JpegError(f"segment {si}: {left // 8} trailing bytes")
        if left and (buf[-1] & ((1 << left) - 1)) != (1 << left) - 1:
            raise JpegError(f"segment {si}: padding bits are not 1")
        r.pad.append(left)


# ------------------------------------------------------------------ forward reference (float64)
def _dct_matrix():
    u, x = np.mgrid[0:8, 0:8].astype(np.float64)
    c = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    c[0] /= np.sqrt(2.0)
    return c


_DCT = _dct_matrix()


def _planes(rgb, dtype):
    """RGB [H, W, 3] -> level-shifted Y, Cb, Cr of the image replicated to multiples of 16; chroma: the mean of
    each 2x2 quad. JFIF / T.871 constants, six decimals."""
    rgb = np.asarray(rgb)
    H, W = rgb.shape[:2]
    p = np.pad(rgb, ((0, -H % 16), (0, -W % 16), (0, 0)), mode="edge").astype(dtype)
    f = dtype
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = f(0.299) * R + f(0.587) * G + f(0.114) * B - f(128)
    Cb = f(-0.168736) * R - f(0.331264) * G + f(0.5) * B
    Cr = f(0.5) * R - f(0.418688) * G - f(0.081312) * B
    quad = lambda c: f(0.25) * (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2])  # noqa: E731
    return Y, quad(Cb), quad(Cr)


def _blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)  # [bh, bw, y, x]


def forward(rgb, quality: int):
    """[xY, xCb, xCr]: the unrounded quantized coefficients of an RGB uint8 [H, W, 3] image."""
    ql, qc = quant_tables(quality)
    out = []
    for plane, q in zip(_planes(rgb, np.float64), (ql, qc, qc)):
        b = _blocks(plane)
        F = np.einsum("vy,ijyx,ux->ijvu", _DCT, b, _DCT)  # F[v, u]: vertical frequency v, natural index v * 8 + u
        out.append(F.reshape(F.shape[0], F.shape[1], 64) / q)
    return out


# ------------------------------------------------------------------ allowance
def _aan8_f32(d):
    """8-point scaled DCT (Arai, Agui, Nakajima; Pennebaker & Mitchell fig. 4-8) along axis -2, float32, every
    product and sum rounded on its own (numpy has no fused multiply-add)."""
    f = np.float32
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i, :] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1 = (e2 + e3) * f(0.707106781)
    o0, o1, o2 = t4 + t5, t5 + t6, t6 + t7
    z5 = (o0 - o2) * f(0.382683433)
    z2 = f(0.541196100) * o0 + z5
    z4 = f(1.306562965) * o2 + z5
    z3 = o1 * f(0.707106781)
    z11, z13 = t7 + z3, t7 - z3
    return np.stack([e0 + e1, z11 + z4, e3 + z1, z13 - z2, e0 - e1, z13 + z2, e3 - z1, z11 - z4], -2)


def forward_f32(rgb, quality: int):
    """The float32 pipeline the allowance is measured with: colour and quad means in float32, AAN on columns then
    rows, one multiply by the float32 reciprocal of quantizer x AAN scale."""
    a = np.array([1.0] + [np.sqrt(2.0) * np.cos(k * np.pi / 16) for k in range(1, 8)])
    ql, qc = quant_tables(quality)
    out = []
    for plane, q in zip(_planes(rgb, np.float32), (ql, qc, qc)):
        b = _blocks(plane)
        F = _aan8_f32(b)                                       # columns: axis -2 is y
        F = _aan8_f32(F.swapaxes(-1, -2)).swapaxes(-1, -2)     # rows
        recip = (1.0 / (q.reshape(8, 8) * 8.0 * np.outer(a, a))).astype(np.float32)
        assert F.dtype == np.float32
        out.append((F * recip).reshape(F.shape[0], F.shape[1], 64))
    return out


@functools.lru_cache(maxsize=None)
def _delta_sample():
    return np.random.default_rng(20240501).integers(0, 256, (1024, 1024, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def delta(quality: int):
    """(luma, chroma) allowance of one quality: 8 x the worst |float32 pipeline - float64 reference| over 4096 noise
    blocks per table (luma: the top-left 512 x 512 pixels; chroma: the whole 1024 x 1024 sample)."""
    img = _delta_sample()
    x64, x32 = forward(img, quality), forward_f32(img, quality)
    dl = np.abs(x32[0][:64, :64].astype(np.float64) - x64[0][:64, :64]).max()
    dc = max(np.abs(x32[c].astype(np.float64) - x64[c]).max() for c in (1, 2))
    assert x64[0][:64, :64].shape[:2] == (64, 64) and x64[1].shape[:2] == (64, 64)
    return 8.0 * float(dl), 8.0 * float(dc)


def allowed(x, quality: int):
    """(lo, hi, ambiguous mask) per component: the values a correct encoder may give each coefficient."""
    out = []
    for xc, d in zip(x, (delta(quality)[0],) + (delta(quality)[1],) * 2):
        lo, hi = round_half_away(xc - d), round_half_away(xc + d)
        out.append((lo, hi, lo != hi))
    return out


def ambiguous_share(x, quality: int) -> float:
    a = allowed(x, quality)
    return sum(int(m.sum()) for _, _, m in a) / sum(m.size for _, _, m in a)


# ------------------------------------------------------------------ entropy encoder (Annex F.1.2)
_CODES = {k: huff_codes(*v) for k, v in ANNEX_K.items()}


def _block_symbols(blk_zz, pred, dc, ac, out):
    """Append (code, length) pairs of one block (64 ints in zig-zag order)."""
    diff = blk_zz[0] - pred
    n = abs(diff).bit_length()
    out.append(dc[n])
    if n:
        out.append((diff if diff > 0 else diff + (1 << n) - 1, n))
    run = 0
    for k in range(1, 64):
        v = blk_zz[k]
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(ac[0xF0])
            run -= 16
        n = abs(v).bit_length()
        out.append(ac[(run << 4) | n])
        out.append((v if v > 0 else v + (1 << n) - 1, n))
        run = 0
    if run:
        out.append(ac[0x00])


def encode_scan(coef, restart_rows: int = 0, spans=None, raw=None):
    """Entropy-coded bytes of a 4:2:0 scan (SOS header and EOI excluded) of [Y, Cb, Cr] integer coefficients, a
    restart marker after every ``restart_rows`` MCU rows (0: none). ``spans``, a list, receives each segment's
    (start, end), RSTm excluded; ``raw``, a list, each segment's (bytes before stuffing, padding bits)."""
    Y, Cb, Cr = (np.asarray(c) for c in coef)
    mcuy, mcux = Cb.shape[:2]
    assert Y.shape[:2] == (2 * mcuy, 2 * mcux) and Cr.shape == Cb.shape
    assert max(int(np.abs(c[..., 1:]).max()) for c in (Y, Cb, Cr)) < 1024
    Yz, Cbz, Crz = (c[..., ZIGZAG].tolist() for c in (Y, Cb, Cr))
    rows = restart_rows if restart_rows > 0 else mcuy
    out = bytearray()
    nseg = -(-mcuy // rows)
    for s in range(nseg):
        sym = []
        pred = [0, 0, 0]
        for my in range(s * rows, min(mcuy, (s + 1) * rows)):
            for mx in range(mcux):
                for by in (0, 1):
                    for bx in (0, 1):
                        b = Yz[2 * my + by][2 * mx + bx]
                        _block_symbols(b, pred[0], _CODES[(0, 0)], _CODES[(1, 0)], sym)
                        pred[0] = b[0]
                for ci, plane in ((1, Cbz), (2, Crz)):
                    b = plane[my][mx]
                    _block_symbols(b, pred[ci], _CODES[(0, 1)], _CODES[(1, 1)], sym)
                    pred[ci] = b[0]
        chunks, acc, n = [], 0, 0
        for code, length in sym:
            acc = (acc << length) | code
            n += length
            if n >= 512:  # keep the accumulator short: move 64 whole bytes out
                n -= 512
                chunks.append((acc >> n).to_bytes(64, "big"))
                acc &= (1 << n) - 1
        pad = -n % 8
        acc = (acc << pad) | ((1 << pad) - 1)
        chunks.append(acc.to_bytes((n + pad) // 8, "big"))
        seg = b"".join(chunks)
        if raw is not None:
            raw.append((seg, pad))
        seg = seg.replace(b"\xff", b"\xff\x00")
        if spans is not None:
            spans.append((len(out), len(out) + len(seg)))
        out += seg
        if s + 1 < nseg:
            out += bytes([0xFF, 0xD0 + s % 8])
    return bytes(out)


# ------------------------------------------------------------------ the check
def check_header(r: Parsed, H: int, W: int, quality: int, restart_rows: int):
    ql, qc = quant_tables(quality)
    assert (r.H, r.W) == (H, W), (r.H, r.W)
    assert [c[1:] for c in r.comps] == [(2, 2, 0), (1, 1, 1), (1, 1, 1)], r.comps
    assert np.array_equal(r.qt[0], ql) and np.array_equal(r.qt[1], qc), "quantizers are not the IJG-scaled Annex K.1"
    assert r.scan_tabs == [(0, 0), (1, 1), (1, 1)], r.scan_tabs
    for k, v in ANNEX_K.items():
        assert r.dht.get(k) == v, f"DHT {k} is not the Annex K.3 table"
    mcux, mcuy = (W + 15) // 16, (H + 15) // 16
    nseg = -(-mcuy // restart_rows) if restart_rows > 0 else 1
    want = restart_rows * mcux if nseg > 1 else 0
    # one segment needs no DRI; an interval that covers the whole scan says the same
    assert r.dri == want or (nseg == 1 and r.dri >= mcux * mcuy), (r.dri, want)
    assert r.scan[1] is None or len(r.spans) == nseg


def check_coefficients(C, x, quality: int, what: str = ""):
    """Every decoded coefficient is round_half_away(x) where x is farther than delta from a .5 boundary, and one
    of the two neighbours elsewhere."""
    for k, (c, (lo, hi, _)) in enumerate(zip(C, allowed(x, quality))):
        bad = (c < lo) | (c > hi)
        if bad.any():
            i = tuple(int(v[0]) for v in np.nonzero(bad))
            raise AssertionError(f"{what}{('Y', 'Cb', 'Cr')[k]}: {int(bad.sum())} wrong coefficients; first at block "
                                 f"{i[:2]} index {i[2]}: got {int(c[i])}, x = {float(x[k][i]):.6f}, "
                                 f"delta = {delta(quality)}")


def _first_diff(a: bytes, b: bytes) -> str:
    n = min(len(a), len(b))
    i = next((i for i in range(n) if a[i] != b[i]), n)
    return f"lengths {len(a)} / {len(b)}, first difference at byte {i}: {a[i:i + 8].hex()} / {b[i:i + 8].hex()}"


def check_stream(jpg: bytes, rgb, quality: int, restart_rows: int, x=None, exact=None, coef=None, what: str = ""):
    """The whole check of one stream of one image. ``x``: forward(rgb, quality) when the caller has it.
    ``exact``: the coefficients of an unambiguous case (round_half_away(x), asserted by its builder): the scan must
    equal their encoding byte for byte, with no decoding in between. ``coef``: coefficients another stream of the
    same image already passed the check with: the scan must equal THEIR encoding (then it decodes to them, and
    nothing is left to compare); on a mismatch the stream is decoded for the message.
    -> (coefficients, scan bytes, spans of the segments within the scan)."""
    jpg = bytes(jpg)
    H, W = rgb.shape[:2]
    x = forward(rgb, quality) if x is None else x
    given = exact if exact is not None else coef
    if given is not None:
        head = parse(jpg, header_only=True)
        check_header(head, H, W, quality, restart_rows)
        start = head.scan[0]
        assert jpg[-2:] == b"\xff\xd9", what + "no EOI"
        spans = []
        want = encode_scan(given, restart_rows, spans)
        if jpg[start:-2] == want:
            return given, want, spans
        if exact is not None:
            raise AssertionError(f"{what}scan != encode(round(x)): {_first_diff(jpg[start:-2], want)}")
    r = parse(jpg)
    check_header(r, H, W, quality, restart_rows)
    C = [c.astype(np.int64) for c in r.coef]
    check_coefficients(C, x, quality, what)
    spans = []
    want = encode_scan(C, restart_rows, spans)
    scan = jpg[r.scan[0]:r.scan[1]]
    assert scan == want, f"{what}scan != encode(decoded coefficients): {_first_diff(scan, want)}"
    assert spans == r.spans, what + "segment spans"
    return C, scan, spans
