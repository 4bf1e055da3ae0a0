"""Exact-oracle tests of the Laplacian-pyramid kernels (csrc/dream_lap.hip: lap_split, lap_merge, lap_normalize,
through the binding and through ops.lapnorm), in the style of test_dream_guide_exact_gpu.py.

The oracle is the naive float64 loop of lap_oracle.py. For integer inputs in [-2, 2] and n in {1, 2} every level
is a multiple of 2^-22 below 4 in magnitude, and every sum the kernels form has all its terms on one dyadic grid
with the sum of their magnitudes below 2^24 grid units: exact in fp32 in ANY summation order, fused multiply-adds
included, so the kernels must equal the oracle bit for bit. Those conditions, and the ones that keep the cases
worth running, are asserted on the oracle alone in the CPU tests at the top."""
import numpy as np
import pytest
import torch

import lap_oracle as O
from deconv_api_amd.ops import lapnorm as L
from exact_helpers import BF, DEV, HF, _same

gpu = pytest.mark.gpu
dtypes = pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
shapes = pytest.mark.parametrize("N,H,W", O.SHAPES)
SENTINEL = -77.0
GUARD = 64  # elements of sentinel on either side of an output (keeps 16-B alignment)
POW2 = (1.0, 0.5, 2.0)


def _uniform_scales(N, n):
    """Per-image power-of-two scales (image i: POW2[i % 3] on every level)."""
    return np.array([[POW2[i % 3]] * (n + 1) for i in range(N)])


def _mixed_scales(N, n):
    """Another power of two for every (image, level)."""
    return np.array([[POW2[(i + 2 * j) % 3] for j in range(n + 1)] for i in range(N)])


def _merge_stages(levels, s):
    """Per merge stage (grid bits q of its terms, max over outputs of the sum of the terms' magnitudes)."""
    img = s[:, 0, None, None, None] * levels[0]
    stages = []
    for i in range(1, len(levels)):
        hi = s[:, i, None, None, None] * levels[i]
        mag = O.up(np.abs(img), hi.shape[1:3]) + np.abs(hi)
        for k in range(img.shape[0]):  # per image: its scale moves its grid and its magnitudes together
            q = max(O.unit_bits(img[k]) + 6, O.unit_bits(hi[k]))  # up's weights are multiples of 1/64
            stages.append((q, float(mag[k].max())))
        img = O.up(img, hi.shape[1:3]) + hi
    return stages, img


# --------------------------------------------------------------------------- conditions (CPU)
@shapes
@pytest.mark.parametrize("n", [1, 2])
def test_conditions_split(N, H, W, n):
    x = O.int_case(N, H, W)[..., :3]
    levels = O.int_levels(N, H, W, n)
    for lv in levels:
        assert O.fp32_exact(lv) and O.unit_bits(lv) <= 22 and float(np.abs(lv).max()) < 4
    for hi in levels[1:]:
        assert bool((hi != 0).any()), "a level without detail"
    assert bool((O.down(x) != O.down(x, replicate=True)).any()), "the zero border changes nothing"
    # any summation order: per level the terms of down (grid: the input's / 256) and of x - up(lo) (grid: lo's
    # / 64, the input's) sum to less than 2^24 grid units in magnitude
    cur = x
    for _ in range(n):
        lo = O.down(cur)
        q = O.unit_bits(cur) + 8
        assert float(O.down(np.abs(cur)).max()) * 2.0 ** q < 2 ** 24
        q = max(O.unit_bits(lo) + 6, O.unit_bits(cur))
        assert float((np.abs(cur) + O.up(np.abs(lo), cur.shape[1:3])).max()) * 2.0 ** q < 2 ** 24
        cur = lo


@shapes
@pytest.mark.parametrize("n", [1, 2])
def test_conditions_merge(N, H, W, n):
    """Merging with all scales 1 reconstructs the integers, and that merge, the per-image power-of-two merge and
    (one level) the per-level power-of-two merge are exact in fp32 in any order."""
    levels = list(O.int_levels(N, H, W, n))
    x = O.int_case(N, H, W)[..., :3]
    assert np.array_equal(O.merge(levels, np.ones((N, n + 1))), x)
    sets = [np.ones((N, n + 1)), _uniform_scales(N, n)] + ([_mixed_scales(N, 1)] if n == 1 else [])
    for s in sets:
        stages, img = _merge_stages(levels, s)
        assert O.fp32_exact(img)
        for q, mag in stages:
            assert mag * 2.0 ** q < 2 ** 24, (q, mag)
    ref = O.merge(levels, _uniform_scales(N, n))
    for dt in (BF, HF):  # the packed 16-bit output of the all-ones merge is exact too
        t = torch.from_numpy(x)
        assert torch.equal(t.to(dt).double(), t)
    assert np.array_equal(ref, _uniform_scales(N, n)[:, 0, None, None, None] * x)


# --------------------------------------------------------------------------- GPU helpers
def _guarded(shape, dtype=torch.float32):
    """A sentinel-filled tensor of ``shape`` in the middle of a larger sentinel-filled buffer -> (view, buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(*shape), buf


def _guards_intact(bufs):
    return all(bool((b[:GUARD].float() == SENTINEL).all()) and bool((b[-GUARD:].float() == SENTINEL).all()) for b in bufs)


class _Guarded:
    """Guarded level buffers with the layout of ops.lapnorm.LapBuffers."""

    def __init__(self, N, H, W, n):
        shp = L.level_shapes(H, W, n)
        self.bufs = []

        def g(shape):
            v, b = _guarded(shape)
            self.bufs.append(b)
            return v

        self.hi = [g((N, *shp[l], 3)) for l in range(n)]
        self.lo = [g((N, *shp[l + 1], 3)) for l in range(n)]
        self.hpart = [g((N, L.parts_of(*shp[l]))) for l in range(n)]
        self.lpart = g((N, L.parts_of(*shp[n - 1])))
        self.merged = [g((N, *shp[l], 3)) for l in range(1, n)]

    def levels(self):
        return [self.lo[-1]] + self.hi[::-1]

    def partials(self):
        return [self.lpart] + self.hpart[::-1]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


# --------------------------------------------------------------------------- exact split
@gpu
@dtypes
@shapes
@pytest.mark.parametrize("n", [1, 2])
def test_exact_split(native_lib, N, H, W, n, dt):
    """Every level bit for bit (so every element is written: none keeps the sentinel), the intermediate lo levels
    too, partials written, guards intact, input unchanged; the fp32 3-channel input layout gives the same."""
    x8 = _t(O.int_case(N, H, W)).to(dt).to(DEV)
    keep = x8.clone()
    want = O.int_levels(N, H, W, n)
    b = _Guarded(N, H, W, n)
    native_lib.lap_split(x8, b.lo, b.hi, b.hpart, b.lpart)
    for got, ref in zip(b.levels(), want):
        _same(got, _t(ref))
    cur = O.int_case(N, H, W)[..., :3]
    for l in range(n):  # lo of every level, not only the last
        cur = O.down(cur)
        _same(b.lo[l], _t(cur))
    for p, ref in zip(b.partials(), want):  # exact levels, but the squares' sums round: to rounding only
        assert not bool((p == SENTINEL).any())
        ssq = (ref ** 2).sum(axis=(1, 2, 3))
        assert np.allclose(p.double().sum(1).cpu().numpy(), ssq, rtol=ref[0].size * 2.0 ** -24, atol=0)
    assert _guards_intact(b.bufs)
    assert torch.equal(x8, keep), "the input changed"
    for got, ref in zip(L.lap_split(x8[..., :3].float().contiguous(), n), want):
        _same(got, _t(ref))
    for got, ref in zip(L.lap_split(x8, n), want):
        _same(got, _t(ref))


# --------------------------------------------------------------------------- exact merge
@gpu
@shapes
@pytest.mark.parametrize("n", [1, 2])
def test_exact_merge(native_lib, N, H, W, n):
    """lap_merge on the oracle's exact levels: per-image power-of-two scales bit for bit, all scales 1 reproduces
    the integers (fp32 and both packed 16-bit layouts, channels 3..7 exactly zero), per-level powers of two bit for
    bit at one level and to rounding at two (16 roundings per level against the largest stage magnitude)."""
    levels = list(O.int_levels(N, H, W, n))
    x = O.int_case(N, H, W)[..., :3]
    lv = [_t(a).to(DEV) for a in levels]
    keep = [t.clone() for t in lv]
    shp = L.level_shapes(H, W, n)
    for name, s in (("ones", np.ones((N, n + 1))), ("uniform", _uniform_scales(N, n)), ("mixed", _mixed_scales(N, n))):
        ref = O.merge(levels, s)
        out, obuf = _guarded((N, H, W, 3))
        merged = [_guarded((N, *shp[l], 3)) for l in range(1, n)]
        native_lib.lap_merge(lv[0], lv[:0:-1], [m for m, _ in merged], out, torch.from_numpy(s).float().to(DEV))
        assert _guards_intact([obuf] + [b for _, b in merged])
        assert not bool((out == SENTINEL).any())
        if n == 1 or name != "mixed":
            _same(out, _t(ref))
        else:
            stages, _ = _merge_stages(levels, s)
            tol = 16 * n * 2.0 ** -24 * max(m for _, m in stages)
            assert float(np.abs(out.double().cpu().numpy() - ref).max()) <= tol
        _same(L.lap_merge(lv, torch.from_numpy(s).float()), out.cpu())
    ones = torch.ones(N, n + 1)
    _same(L.lap_merge(lv, ones), _t(x))  # perfect reconstruction
    for dt in (BF, HF):
        out, obuf = _guarded((N, H, W, 8), dt)
        merged = [torch.empty(N, *shp[l], 3, device=DEV) for l in range(1, n)]
        native_lib.lap_merge(lv[0], lv[:0:-1], merged, out, ones.to(DEV))
        _same(out[..., :3], _t(x))
        assert not bool(out[..., 3:].float().any()), "channels 3..7 not zero"
        assert _guards_intact([obuf])
        packed = L.lap_merge(lv, torch.from_numpy(_uniform_scales(N, n)).float(), out_dtype=dt)
        _same(packed[..., :3], _t(O.merge(levels, _uniform_scales(N, n))).to(dt))
        assert packed.shape == (N, H, W, 8) and not bool(packed[..., 3:].float().any())
    for t, t0 in zip(lv, keep):
        assert torch.equal(t, t0), "a level changed"


# --------------------------------------------------------------------------- deep levels, partials
@gpu
@dtypes
@shapes
@pytest.mark.parametrize("n", [3, 4, 5])
def test_deep_levels_and_partials(native_lib, N, H, W, n, dt):
    """n >= 3 on random 16-bit values. Levels: |got - oracle| <= 40 n 2^-24 max|x|, tighter than the 64 n of a
    25-term and a 9-term dot product taken term by term, from the kernel's order. With u = 2^-24 A, A = max|x|
    (no value of any level's input exceeds A: the weights of down, and of up per output, are positive and sum to
    1): down is a 5-term row chain and a 5-term column chain over the rows, 10 additions, each result at most A
    in magnitude, so at most 10 u when every multiply-add is fused and 20 u when none is; up is a chain of at
    most 3 and one of at most 3 over those, 6 u / 12 u, and the subtraction rounds a value below 2 A: 2 u. An
    input error E passes through down with norm 1 and through x - up(down(x)) with norm 2, so E grows by at most
    20 u per level and a hi level is off by at most 2 E + 20 u + 12 u + 2 u: below 40 n u for every level of an
    n-level split. Measured on an MI355X: at most 0.8 % of this bound.

    Partials: an image's partials summed in float64 against the float64 sum of squares of the level THE KERNEL
    WROTE, relative M 2^-24 (M elements: one rounding per square, at most M - 1 per running sum of non-negative
    terms, whatever the order). That is the bound's own argument: it speaks of the summation, so it holds against
    the summed terms; a pixel counted twice or not at all still breaks it. Against the oracle's sum of squares the
    same bound cannot hold for the small coarse levels (M = 3 at 5 x 5, n = 5: the coarse values themselves
    carry the level error above, relative to max|x| and not to their own size; measured on an MI355X at 5 x 5,
    n = 5: 1.80e-7 (bf16 input) and 1.85e-7 (fp16) against 3 x 2^-24 = 1.79e-7, while against the kernel's own level
    the same partials are within 3.8e-8), so there the level error is added as it propagates:
    |sum (l + e)^2 - sum l^2| <= 2 e sum|l| + M e^2 with e the level bound. Every other level of every case is
    within M 2^-24 of the oracle as well (largest ratio measured 0.32)."""
    x8, x = O.rand_case(N, H, W, dt)
    want = O.split(x, n)
    b = _Guarded(N, H, W, n)
    native_lib.lap_split(x8.to(DEV), b.lo, b.hi, b.hpart, b.lpart)
    e = 40 * n * 2.0 ** -24 * float(np.abs(x).max())
    for i, (got, p, ref) in enumerate(zip(b.levels(), b.partials(), want)):
        g = got.double().cpu().numpy()
        err = float(np.abs(g - ref).max())
        M = ref[0].size
        psum = p.double().sum(1).cpu().numpy()
        own = (g ** 2).sum(axis=(1, 2, 3))
        orc = (ref ** 2).sum(axis=(1, 2, 3))
        print(f"level {i}: err {err:.3g} (bound {e:.3g}), partial rel own {np.abs(psum / own - 1).max():.3g} "
              f"oracle {np.abs(psum / orc - 1).max():.3g} (M 2^-24 = {M * 2.0 ** -24:.3g})")
        assert err <= e, (i, err, e)
        assert not bool((p == SENTINEL).any())
        assert np.all(np.abs(psum - own) <= M * 2.0 ** -24 * own), (i, psum, own)
        slack = 2 * e * np.abs(ref).sum(axis=(1, 2, 3)) + M * e * e
        assert np.all(np.abs(psum - orc) <= M * 2.0 ** -24 * orc + slack), (i, psum, orc)
    assert _guards_intact(b.bufs)


# --------------------------------------------------------------------------- lap_normalize end to end
@gpu
@dtypes
@shapes
@pytest.mark.parametrize("n", [1, 4])
def test_lap_normalize(native_lib, N, H, W, n, dt):
    """|out - ref| <= u |ref| + (64 n + 3 H W) 2^-24 max|ref| with u = 2^-8 (bf16) / 2^-10 (fp16), one unit of the
    output format; the last image of every case with several images is all zero (eps decides: exactly zero, no NaN);
    channels 3..7 zero, guards intact, input unchanged."""
    x8, x = O.rand_case(N, H, W, dt, zero_image=N > 1)
    ref = O.lap_normalize(x, n)
    xg = x8.to(DEV)
    keep = xg.clone()
    b = _Guarded(N, H, W, n)
    out, obuf = _guarded((N, H, W, 8), dt)
    native_lib.lap_normalize(xg, b.lo, b.hi, b.hpart, b.lpart, b.merged, out, 1e-10)
    got = out[..., :3].double().cpu().numpy()
    u = 2.0 ** -8 if dt == BF else 2.0 ** -10
    tol = u * np.abs(ref) + (64 * n + 3 * H * W) * 2.0 ** -24 * float(np.abs(ref).max())
    print(f"max err / tol {float((np.abs(got - ref) / tol).max()):.3g}, max|ref| {float(np.abs(ref).max()):.3g}")
    assert np.isfinite(got).all() and np.all(np.abs(got - ref) <= tol)
    assert float(np.abs(ref).max()) > 0.5  # unit-RMS bands: the result is of order one
    if N > 1:
        assert not bool(out[-1].float().any()) and not np.any(ref[-1])
    assert not bool(out[..., 3:].float().any()), "channels 3..7 not zero"
    assert _guards_intact(b.bufs + [obuf]) and torch.equal(xg, keep)
    # the op surface: same bits with its own buffers, and the fp32 layout within the fp32 part of the bound
    assert torch.equal(L.lap_normalize(xg, n).view(torch.int16), out.view(torch.int16))
    f = L.lap_normalize(xg[..., :3].float().contiguous(), n).double().cpu().numpy()
    assert np.all(np.abs(f - ref) <= (64 * n + 3 * H * W) * 2.0 ** -24 * float(np.abs(ref).max()))


@gpu
def test_lap_normalize_all_zero(native_lib):
    x = torch.zeros(1, 9, 12, 8, dtype=BF, device=DEV)
    out = L.lap_normalize(x, 3)
    assert out.shape == x.shape and not bool(out.float().any())


@gpu
def test_binding_refuses_bad_arguments(native_lib):
    x = torch.zeros(1, 9, 12, 8, dtype=BF, device=DEV)
    b = L.LapBuffers(1, 9, 12, 2, DEV)
    with pytest.raises(RuntimeError):  # a level of the wrong shape
        native_lib.lap_split(x, [b.lo[0], b.lo[0]], b.hi, b.hpart, b.lpart)
    with pytest.raises(RuntimeError):  # partial extents
        native_lib.lap_split(x, b.lo, b.hi, [b.hpart[0], torch.zeros(1, 2, device=DEV)], b.lpart)
    with pytest.raises(RuntimeError):  # dtype
        native_lib.lap_split(x.float(), b.lo, b.hi, b.hpart, b.lpart)
    with pytest.raises(RuntimeError):  # device
        native_lib.lap_split(x.cpu(), b.lo, b.hi, b.hpart, b.lpart)
    with pytest.raises(RuntimeError):  # contiguity
        native_lib.lap_split(x.transpose(1, 2), b.lo, b.hi, b.hpart, b.lpart)
    with pytest.raises(RuntimeError):  # 1 <= n <= 5
        native_lib.lap_split(x, [], [], [], b.lpart)
    with pytest.raises(ValueError):
        L.lap_split(x, 6)
    with pytest.raises(ValueError):
        L.lap_normalize(x, 0)


# --------------------------------------------------------------------------- the torch reference (CPU)
@pytest.mark.parametrize("N,H,W", O.SHAPES[:5])
def test_torch_reference_equals_the_oracle(N, H, W):
    """ops.lapnorm's CPU path (F.conv2d / F.conv_transpose2d + crop) against the naive loops, in float64-exact
    integer arithmetic for the levels and to fp32 rounding for lap_normalize."""
    x = O.int_case(N, H, W)
    for got, ref in zip(L.lap_split(_t(x[..., :3]), 2), O.int_levels(N, H, W, 2)):
        _same(got, _t(ref))
    lv = [_t(a) for a in O.int_levels(N, H, W, 2)]
    _same(L.lap_merge(lv, torch.ones(N, 3)), _t(x[..., :3]))
    _, r = O.rand_case(N, H, W, BF)
    got = L.lap_normalize(_t(r), 3).double().numpy()
    ref = O.lap_normalize(r, 3)
    assert np.abs(got - ref).max() <= (64 * 3 + 3 * H * W) * 2.0 ** -24 * np.abs(ref).max()
