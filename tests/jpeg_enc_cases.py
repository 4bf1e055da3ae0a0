"""The images of the exact JPEG-encoder tests (test_jpeg_enc_exact.py on the host encoder, test_jpeg_enc_exact_gpu.py
on the GPU encoder). Every builder asserts its own conditions on the reference (tests/jpeg_ref.py), never on an
encoder: a crafted case really has the coefficients it was made for and not one coefficient near a rounding
boundary; no case has more than 1 % of its coefficients inside the allowance; and the set as a whole reaches every
Huffman category, padding length and stuffing position (``coverage``)."""
import functools
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref as ref  # noqa: E402

MAX_AMBIGUOUS = 0.01
# The largest AC magnitude 8-bit samples can produce: |F_k| <= 127.5 * sum |basis_k| (the -0.5 of the level shift
# meets sum basis_k = 0), and sum |basis_k| peaks at 8 for k = (0, 4), (4, 0) and (4, 4). So 1023 = 2^10 - 1 does not
# occur in any stream made from pixels; likewise a DC value lies in [-1024, 1016], a difference in [-2040, 2040].
AC_MAX, DC_DIFF_MAX = 1020, 2040


class Case:
    """images uint8 [B, H, W, 3]; ``exact``: no coefficient of the reference is within the allowance of a rounding
    boundary, so a stream has to equal ``encode_scan(coef)`` byte for byte."""

    def __init__(self, name, images, quality, exact=False):
        images = np.ascontiguousarray(images, dtype=np.uint8)
        self.name, self.quality, self.exact = name, int(quality), exact
        self.images = images[None] if images.ndim == 3 else images
        self.B, self.H, self.W = self.images.shape[:3]
        assert self.B * self.H * self.W <= 300_000 and self.H * self.W <= 100_000, name
        self.x = [ref.forward(im, self.quality) for im in self.images]
        self.coef = [[ref.round_half_away(c) for c in x] for x in self.x]  # THE answer only where exact
        self.ambiguous = max(ref.ambiguous_share(x, self.quality) for x in self.x)
        if exact:
            assert self.ambiguous == 0.0, (name, self.ambiguous)
        assert self.ambiguous <= MAX_AMBIGUOUS, (name, self.ambiguous)

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------ crafted blocks
def _grey(yblocks):
    """Level-shifted luma blocks [bh, bw, 8, 8] (integers in [-128, 127]) -> a grey image: Y = value, Cb = Cr = 0."""
    yb = np.asarray(yblocks)
    assert yb.min() >= -128 and yb.max() <= 127 and np.array_equal(yb, np.round(yb))
    bh, bw = yb.shape[:2]
    g = (yb.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8) + 128).astype(np.uint8)
    return np.repeat(g[..., None], 3, -1)


def _idct(target_zz, q):
    """Pixels (level-shifted, rounded) of the block whose quantized coefficients, zig-zag order, are ``target_zz``."""
    nat = np.zeros(64)
    nat[ref.ZIGZAG] = target_zz
    F = (nat * q).reshape(8, 8)
    return np.round(ref._DCT.T @ F @ ref._DCT)


def _target(**at):
    t = np.zeros(64)
    for k, v in at.items():
        t[int(k[1:])] = v
    return t


def _expect_zz(case, comp, by, bx, target_zz, img=0):
    got = case.coef[img][comp][by, bx][ref.ZIGZAG]
    assert np.array_equal(got, target_zz), (case.name, comp, by, bx, got.tolist())


def _c63_luma():
    ql, _ = ref.quant_tables(50)
    t = [_target(k0=5, k63=1), _target(k0=-3, k63=-1), _target(k0=0, k63=2), _target(k0=7)]
    c = Case("dc_c63_luma", _grey(np.array([_idct(v, ql) for v in t]).reshape(2, 2, 8, 8)), 50, exact=True)
    for i, v in enumerate(t):
        _expect_zz(c, 0, i // 2, i % 2, v)
    return c


def _c63_chroma():
    """Cb of the only MCU: DC and coefficient 63; Y flat, Cr flat (the inverse JFIF transform at Y = Cr = 0)."""
    _, qc = ref.quant_tables(50)
    t = _target(k0=-4, k63=1)
    cb = np.kron(_idct(t, qc), np.ones((2, 2)))
    rgb = np.stack([np.full_like(cb, 128.0), 128 - 0.344136 * cb, 128 + 1.772 * cb], -1)
    c = Case("dc_c63_chroma", np.clip(np.round(rgb), 0, 255), 50, exact=True)
    _expect_zz(c, 1, 0, 0, t)
    assert not c.coef[0][2].any() and not c.coef[0][0][..., 1:].any()
    return c


def _zero_runs():
    """Zero runs of exactly 15, 16, 31 and 32 before a nonzero coefficient (zig-zag positions 16, 17, 32, 33)."""
    ql, _ = ref.quant_tables(50)
    t = [_target(k0=2, k16=1), _target(k0=2, k17=-1), _target(k0=-1, k32=2), _target(k0=0, k33=-2),
         _target(k0=1, k16=-1, k33=1), _target(k0=1, k17=1, k50=-1), _target(k0=0, k15=1, k31=1, k47=1, k63=1),
         _target(k0=0, k16=1, k32=1, k48=-1)]
    c = Case("zero_runs", _grey(np.array([_idct(v, ql) for v in t]).reshape(2, 4, 8, 8)), 50, exact=True)
    for i, v in enumerate(t):
        _expect_zz(c, 0, i // 4, i % 4, v)
    return c


def _all_zero_ac():
    g = np.array([[100, 104, 180, 60], [128, 128, 20, 250]])
    c = Case("all_zero_ac", _grey(np.broadcast_to((g - 128)[..., None, None], (2, 4, 8, 8))), 50, exact=True)
    assert all(not p[..., 1:].any() for p in c.coef[0]) and len(set(c.coef[0][0][..., 0].ravel().tolist())) >= 6
    return c


def _flat_grey():
    c = Case("flat_grey", np.full((48, 16, 3), 128), 95, exact=True)
    assert all(not p.any() for p in c.coef[0])
    raw = []
    ref.encode_scan(c.coef[0], 1, raw=raw)
    assert [(len(s), pad) for s, pad in raw] == [(4, 0)] * 3  # 4 x (2 + 4) + 2 x (2 + 2) bits per MCU
    return c


_S4 = np.array([1, -1, -1, 1, 1, -1, -1, 1])
_SIGN44 = np.outer(_S4, _S4)  # sign of the (4, 4) basis function, whose magnitude is 1/8 everywhere


def _safe(blk) -> bool:
    """No coefficient of the block at quality 100 within 0.01 of a rounding boundary (far outside any allowance)."""
    F = ref._DCT @ blk @ ref._DCT.T
    return bool((np.abs(np.abs(F) % 1.0 - 0.5) > 0.01).all())


def _ac44(value):
    """A block whose coefficient (4, 4) at quality 100 is exactly ``value`` = sum(sign * sample) / 8: one amplitude
    along the sign pattern; a value that is no multiple of 8 takes the remainder out of one pixel, the first in
    raster order that leaves every other coefficient clear of a rounding boundary."""
    if abs(value) == AC_MAX:
        return np.where(_SIGN44 * np.sign(value) > 0, 127, -128)
    a, r = divmod(abs(value), 8)
    if r == 0:
        return a * _SIGN44 * (1 if value > 0 else -1)
    for at in np.ndindex(8, 8):
        blk = (a + 1) * _SIGN44
        blk[at] -= 8 * (8 - r) * _SIGN44[at]
        if _safe(blk):
            return blk * (1 if value > 0 else -1)
    raise AssertionError(value)


def _ac_cat10():
    """Quality 100 (every quantizer 1): AC coefficients at the boundaries of categories 9 and 10, both signs, by the
    (4, 4) sign pattern, and +-128-amplitude sign-of-cosine patterns of other frequencies."""
    vals = [AC_MAX, -AC_MAX, 512, -512, 511, -511, 256, -256, 255, -255]
    blocks = [_ac44(v) for v in vals]
    for u, v in ((1, 0), (0, 1), (1, 1), (4, 0), (0, 4), (7, 7), (3, 5)):
        s = np.sign(np.outer(ref._DCT[v], ref._DCT[u]))
        blocks += [np.where(s > 0, 127, -128), np.where(s > 0, -128, 127)]
    c = Case("ac_cat10_q100", _grey(np.array(blocks).reshape(4, 6, 8, 8)), 100, exact=True)
    for i, v in enumerate(vals):
        assert c.coef[0][0][i // 6, i % 6, 4 * 8 + 4] == v, (i, v)
    return c


def _dc_block(d):
    """A block with DC = d at quality 100: the samples sum to 8 d. d // 8 everywhere, and d % 8 whole rows one
    higher: the first choice of rows that leaves the seven vertical AC coefficients clear of a rounding boundary."""
    a, m = divmod(d, 8)
    for rows in itertools.combinations(range(8), m):
        blk = np.full((8, 8), a)
        blk[list(rows)] += 1
        if _safe(blk):
            return blk
    raise AssertionError(d)


_DC_ROWS = [  # DC differences of the luma blocks of one MCU row each, in coding order (the predictor starts at 0)
    [-512, 1023, -1023, 512, 255, -255, 256, -256, 511, -511, 1, -1],
    [-1024, 1024, 1016, -2040, 2040, -1016, 127, -127, 128, -128, 0, 0],
    [63, -63, 64, -64, 31, -31, 32, -32, 15, -15, 16, -16],
    [7, -7, 8, -8, 3, -3, 4, -4, 2, -2, 1, -1],
]


def _dc_luma():
    """Quality 100: every luma DC category 0..11 at both boundaries and both signs, white then black included.
    48 wide: 12 luma blocks per MCU row, and every MCU row is a restart segment of the GPU encoder."""
    yb = np.zeros((8, 6, 8, 8), np.int64)
    for row, diffs in enumerate(_DC_ROWS):
        dc = 0
        for i, d in enumerate(diffs):
            dc += d
            yb[2 * row + (i % 4 >> 1), 2 * (i // 4) + (i & 1)] = _dc_block(dc)
    c = Case("dc_luma_q100", _grey(yb), 100, exact=True)
    got = []
    for row in range(4):
        prev = 0
        for i in range(12):
            v = int(c.coef[0][0][2 * row + (i % 4 >> 1), 2 * (i // 4) + (i & 1), 0])
            got.append(v - prev)
            prev = v
    assert got == sum(_DC_ROWS, []), got
    return c


def _dc_chroma():
    """Quality 100: saturated blue then yellow (Cb DC 1020 -> -1020), then red / cyan for Cr."""
    cols = [(0, 0, 255), (255, 255, 0), (0, 0, 255), (255, 0, 0), (0, 255, 255), (255, 0, 0)]
    img = np.concatenate([np.broadcast_to(np.array(c), (16, 16, 3)) for c in cols], 1)
    c = Case("dc_chroma_q100", img, 100, exact=True)
    cb, cr = c.coef[0][1][0, :, 0], c.coef[0][2][0, :, 0]
    assert cb[0] - cb[1] == DC_DIFF_MAX and cb[2] - cb[1] == DC_DIFF_MAX, cb
    assert cr[3] - cr[4] == DC_DIFF_MAX and cr[5] - cr[4] == DC_DIFF_MAX, cr
    return c


# ------------------------------------------------------------------ noise, geometry, bulk
def _noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)


def _smooth(H, W, seed):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    g = np.random.default_rng(seed).uniform(0.5, 3.0, 6)
    return np.stack([(xx * g[0] + yy * g[1]) % 256, 128 + 100 * np.sin(xx / (3 * g[2]) + yy / (5 * g[3])),
                     255 - (xx * g[4] + yy * g[5]) % 256], -1).astype(np.uint8)


def _mix(B, H, W, seed):
    from test_jpeg_gpu import _images  # the mix of the tolerance tests: ramps, noise, noisy ramps, a saturated corner

    return _images(B, H, W, seed)


GEOMETRY_W = (1, 2, 15, 16, 17, 33, 672, 673, 688, 895, 896)  # mcux 42, 43, 56: 252, 258, 336 blocks per segment
GEOMETRY_H = (1, 16, 17)
TALL_H = (2, 15, 31, 147)  # with W = 17; 147: 10 MCU rows, RST7 -> RST0
# fixed seeds, found on the CPU: with these the set meets ``coverage``
SEED_NARROW, SEED_WIDE = 1, 2


def _geometry():
    out = []
    for W in GEOMETRY_W:
        for H in GEOMETRY_H:
            out.append(Case(f"geo_{H}x{W}", _noise(H, W, 1000 * H + W), 95))
    for H in TALL_H:
        out.append(Case(f"geo_{H}x17", _noise(H, 17, 1000 * H + 17), 95))
    return out


def _many_segments():
    """B = 65, H = 256, W = 16: 1040 one-MCU segments, past the offsets kernel's first chunk of 1024; smooth content
    that differs per image, so every image has its own length."""
    yy, xx = np.mgrid[0:256, 0:16]
    imgs = np.stack([np.stack([(yy * (1 + b % 5) + xx * 3 + 7 * b) % 256, (yy + 2 * xx * (b % 3) + 11 * b) % 256,
                               (3 * yy + xx + 5 * b) % 256], -1) for b in range(65)])
    c = Case("segments_65x256x16", imgs, 50)
    lens = {len(ref.encode_scan(co, 1)) for co in c.coef}
    assert len(lens) > 32
    return c


def _bulk():
    out = []
    for H, W in ((100, 70), (17, 33)):
        for q in (1, 50, 95, 100):
            out.append(Case(f"bulk_noise_{H}x{W}_q{q}", _noise(H, W, H + q), q))
            out.append(Case(f"bulk_smooth_{H}x{W}_q{q}", _smooth(H, W, H + q), q))
            out.append(Case(f"bulk_mix_{H}x{W}_q{q}", _mix(3, H, W, H + q), q))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = [_c63_luma(), _c63_chroma(), _zero_runs(), _all_zero_ac(), _flat_grey(), _ac_cat10(), _dc_luma(),
           _dc_chroma(),
           Case("noise_q100_640x16", _noise(640, 16, SEED_NARROW), 100),  # 40 one-MCU segments: the rare endings
           Case("noise_q100_16x896", _noise(16, 896, SEED_WIDE), 100),    # one segment of tens of KB
           Case("batch3_40x50", _mix(3, 40, 50, 5), 95)]
    out += _geometry() + [_many_segments()] + _bulk()
    assert len({c.name for c in out}) == len(out)
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)


def names():
    """Case names without building anything (for parametrize)."""
    n = ["dc_c63_luma", "dc_c63_chroma", "zero_runs", "all_zero_ac", "flat_grey", "ac_cat10_q100", "dc_luma_q100",
         "dc_chroma_q100", "noise_q100_640x16", "noise_q100_16x896", "batch3_40x50"]
    n += [f"geo_{H}x{W}" for W in GEOMETRY_W for H in GEOMETRY_H] + [f"geo_{H}x17" for H in TALL_H]
    n += ["segments_65x256x16"]
    for H, W in ((100, 70), (17, 33)):
        for q in (1, 50, 95, 100):
            n += [f"bulk_{kind}_{H}x{W}_q{q}" for kind in ("noise", "smooth", "mix")]
    return n


def natural_coeffs(c):
    """codec.image.JpegCoeffs of the native parser (component-major, blocks column-major) -> [bh, bw, 64] natural order per component."""
    hs, vs = {0: (1, 1), 1: (2, 1), 2: (2, 2), 3: (1, 1)}[c.kind]  # csrc/jpeg_dec.h DecKind: 4:4:4, 4:2:2, 4:2:0, grey
    mcux, mcuy = -(-c.W // (8 * hs)), -(-c.H // (8 * vs))
    out, p = [], 0
    for i in range(c.ncomp):
        bh, bw = (mcuy * vs, mcux * hs) if i == 0 else (mcuy, mcux)
        blk = c.coef[p:p + bh * bw * 64].reshape(bh, bw, 8, 8)
        out.append(blk.transpose(0, 1, 3, 2).reshape(bh, bw, 64).astype(np.int64))
        p += bh * bw * 64
    assert p == c.coef.size
    return out


# ------------------------------------------------------------------ coverage of the whole set
def _boundary_values(nmax, top):
    """+-2^(n-1) and +-(2^n - 1) of categories 1..nmax; ``top`` stands in for the unreachable 2^nmax - 1."""
    v = set()
    for n in range(1, nmax + 1):
        hi = (1 << n) - 1 if n < nmax else top
        v |= {1 << (n - 1), -(1 << (n - 1)), hi, -hi}
    return v


def coverage():
    """What the reference streams of the whole set (a restart marker per MCU row, as the GPU encoder writes them)
    contain; asserts the list of section 'Coverage' of the cases' design and returns the figures."""
    ac, dc = set(), set()
    pads, ff_mod4 = set(), set()
    ff_last_before_rst = 0
    long_ok = False
    for c in cases():
        for co in c.coef:
            for p in co:
                ac |= set(np.unique(p[..., 1:]).tolist())
            Y, Cb, Cr = co
            mcuy, mcux = Cb.shape[:2]
            # luma DC in coding order within an MCU row: [mcuy, mcux, 2, 2] -> 4 blocks per MCU
            yd = Y[..., 0].reshape(mcuy, 2, mcux, 2).transpose(0, 2, 1, 3).reshape(mcuy, -1)
            for d in (yd, Cb[..., 0], Cr[..., 0]):
                dc |= set(np.unique(np.diff(d, axis=1, prepend=0)).tolist())
            raw = []
            ref.encode_scan(co, 1, raw=raw)
            for i, (seg, pad) in enumerate(raw):
                pads.add(pad)
                ff = np.flatnonzero(np.frombuffer(seg, np.uint8) == 0xFF)
                ff_mod4 |= set((ff % 4).tolist())
                if i + 1 < len(raw) and seg[-1] == 0xFF:
                    ff_last_before_rst += 1
                if len(seg) > 2048 and (ff < 1024).any() and ((ff >= 1024) & (ff < 2048)).any() and (ff >= 2048).any():
                    long_ok = True
    assert max(abs(v) for v in ac) == AC_MAX and max(abs(v) for v in dc) == DC_DIFF_MAX
    missing_ac = _boundary_values(10, AC_MAX) - ac
    missing_dc = (_boundary_values(11, DC_DIFF_MAX) | {0}) - dc
    assert not missing_ac, sorted(missing_ac)
    assert not missing_dc, sorted(missing_dc)
    assert pads == set(range(8)), pads
    assert ff_mod4 == {0, 1, 2, 3}, ff_mod4
    assert ff_last_before_rst >= 1
    assert long_ok, "no segment over 2048 bytes with FF bytes in each of its first three 1024-byte chunks"
    return {"ac_values": len(ac), "dc_differences": len(dc), "ff_last_before_rst": ff_last_before_rst}
