"""Helpers shared by the exact-oracle GPU tests (test_conv_exact_gpu.py, test_conv_routes_exact_gpu.py,
test_dream_exact_gpu.py, test_conv_rounding_exact_gpu.py, test_small_values_exact_gpu.py, test_engine_exact_gpu.py
through engine_oracle.py): seeded integer (and, for the rounding cases, fractional / lifted) operands, mask draws
(``_signs``; ``_signs_tiny`` for the predicate on tiny values), the method's conditions on a CPU reference,
the sentinel-framed launcher and bit equality with the reference. A plain module,
not a conftest: nothing here changes how the suite is collected or run."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import rounding_oracle as RO
from deconv_api_amd import ops
from deconv_api_amd.ops import conv as Cm
from deconv_api_amd.ops.conv import ConvWeights
from gpu_helpers import route as _route

DEV = "cuda"
BF, HF = torch.bfloat16, torch.float16
SENT = 7.0  # fill of the frame around an output view


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _weights(g, oc, c, kh=3, kw=3, kind="fwd", bias=True, taps=96):
    """Integer weights in [-2, 2] with about ``taps`` non-zero taps per output (density min(1, taps / K))
    and an integer bias in [-4, 4]."""
    K = c * kh * kw
    shape = (oc, c, kh, kw) if kind == "fwd" else (c, oc, kh, kw)
    w = _ints(g, shape, -2, 2)
    if taps < K:
        w = w * (torch.rand(shape, generator=g) < taps / K)
    b = _ints(g, (oc,), -4, 4) if bias else None
    return ConvWeights(w, b, kind)


def _signs(g, shape):
    """Mask values from {-1, -0.0, 0, 1}: the two zeros must mask like the negatives."""
    vals = torch.tensor([-1.0, -0.0, 0.0, 1.0])
    return vals[torch.randint(0, 4, shape, generator=g)]


TINY_BITS = {BF: (0x0001, 0x0080), HF: (0x0001, 0x0400)}  # dtype -> bits of the smallest subnormal / normal


def _signs_tiny(g, shape, dt):
    """Stored mask values +-1, +-0.0, +-(smallest subnormal, bits 0x0001 / 0x8001) and +-(smallest normal) of
    ``dt``, equally often, as a ``dt`` tensor (fp32 would hold them too, but the bits are the point). Positive as
    real numbers: 1 and the two positive tiny values; the six others must mask."""
    sub, nrm = TINY_BITS[dt]
    one = int(torch.ones((), dtype=dt).view(torch.int16))
    bits = torch.tensor([one, 0x0000, sub, nrm], dtype=torch.int32)
    bits = torch.cat([bits, bits | 0x8000])
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16)
    vals = bits.view(dt)
    assert int((vals.double() > 0).sum()) == 3 and bool(torch.isfinite(vals.float()).all())
    return vals[torch.randint(0, 8, shape, generator=g)]


def _absconv_max(x, cw, stride=1, pad=1):
    """max over outputs of sum |x| |w|: bounds every partial sum of every summation order."""
    X = x.float().abs().permute(0, 3, 1, 2)
    w = cw.w_oihw.float().abs()
    if cw.kind == "fwd":
        return float(F.conv2d(X, w, None, stride=stride, padding=pad).max())
    return float(F.conv_transpose2d(X, w, None, stride=stride, padding=pad, output_padding=stride - 1).max())


def _check_exact(ref, dt, x, cw, extra=0.0, stride=1, pad=1, dense=True):
    """The method's conditions on the CPU reference ``ref`` (fp32) of a case with output dtype ``dt``."""
    ref = ref.float()
    assert torch.equal(ref.to(dt).double(), ref.double()), "reference not representable in the output type"
    assert _absconv_max(x, cw, stride, pad) + extra < 2 ** 24, "partial sums not exact in fp32"
    if dense:
        assert float((ref != 0).float().mean()) >= 0.25, "too few non-zero outputs"
        # (16 distinct values among the first 64 Ki outputs settle it without sorting a large tensor)
        assert ref.flatten()[:65536].unique().numel() >= 16 or ref.unique().numel() >= 16, "too few distinct values"


def _dev(t, dt):
    return None if t is None else t.to(dt).to(DEV)


def _same(got, ref):
    """Bit equality with the reference (values compared as fp32: -0.0 == 0.0 is not a difference)."""
    g, r = got.float().cpu(), ref.float()
    if g.shape != r.shape or not torch.equal(g, r):
        bad = (g != r).nonzero()
        pytest.fail(f"{int((g != r).sum())} of {g.numel()} values differ, first at {bad[0].tolist()}: "
                    f"got {float(g[tuple(bad[0])])}, want {float(r[tuple(bad[0])])}")


def _geom(M, even=False):
    """Output geometry (N, OH, OW, crop) with N OH OW == M: both sides >= 3 (even sides for the pool
    epilogue) where M factors that way. Where it does not (M = 127, 199, 257, 1543, ...), one output row
    of M pixels (two for the pool) CROPPED from an input two rows taller (pad_h = 0, ``crop``): every
    output still sums all three kernel rows of real data, so the density conditions hold there too."""
    unit = 4 if even else 1
    q = M // unit
    for h in range(int(q ** 0.5), 2, -1):
        if q % h == 0:
            return (1, 2 * h, 2 * (q // h), False) if even else (1, h, q // h, False)
    return (1, 2, M // 2, True) if even else (1, 1, M, True)


def _check_ties(full):
    """The pooled cases' density condition on the full-resolution map ``full`` [N, H, W, OC]: at least one 2 x 2
    window in 20 has its maximum twice (a tie the first-max switch code must resolve)."""
    N, H, W, OC = full.shape
    win = full.view(N, H // 2, 2, W // 2, 2, OC).permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, OC)
    top2 = win.topk(2, dim=3).values
    # (half of the outputs are 0 after the ReLU: one window in 16 is all zeros, and more tie above zero)
    assert float((top2[..., 0, :] == top2[..., 1, :]).float().mean()) >= 0.05, "too few tied windows"


def _pool_case(g, N, H, W, C, OC, taps=96):
    x = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C, taps=taps)
    rp, rc = ops.conv2d(x, cw, relu=True, epilogue="pool")
    full = ops.conv2d(x, cw, relu=True)
    _check_exact(full, BF, x, cw, 4.0)
    _check_ties(full)
    return x, cw, rp, rc


def _representable(ref, what="reference"):
    """``ref`` (fp32 / fp64) is exactly representable in both 16-bit storage types."""
    for dt in (BF, HF):
        assert torch.equal(ref.detach().to(dt).double(), ref.detach().double()), f"{what} not representable in {dt}"


def _tap_weights(g, oc, c, kh=1, kw=1, taps=6, lim=1, live=None):
    """OIHW integer weights, non-zero values in [-lim, lim], thinned like ``_weights`` to about ``taps``
    non-zero taps per output, all of them on the first ``live`` input channels (default: every channel)."""
    live = c if live is None else live
    shape = (oc, c, kh, kw)
    w = _ints(g, shape, 1, lim) * (2 * torch.randint(0, 2, shape, generator=g) - 1)
    w = w * (torch.rand(shape, generator=g) < taps / (live * kh * kw))
    w[:, live:] = 0
    return w


def _recip_exact(m, cnt):
    """The pool kernels' fp32 formula m * (1.f / count) equals the exact integer quotient m / count (m fp32
    integers, cnt the window counts, broadcastable); returns the fp32 result."""
    inv = torch.ones((), dtype=torch.float32) / cnt.float()
    q = m.float() * inv
    assert torch.equal(q.double(), m.double() / cnt.double()), "sum * (1.f / count) is not the exact average"
    assert torch.equal(q, q.round()), "average is not an integer"
    return q


# ----------------------------------------------------------------------------------------
# launcher: a conv case on the GPU through sentinel-framed views
# ----------------------------------------------------------------------------------------

@contextlib.contextmanager
def _policy(impl):
    old = Cm.get_policy()
    Cm.set_policy(impl=impl)
    try:
        yield
    finally:
        Cm.set_policy(**old)


def _wide(t, dt, extra, fill=3.0):
    """``t`` on the device as a channel slice of a buffer ``extra`` channels wider (row stride C + extra)."""
    if not extra:
        return _dev(t, dt)
    buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + extra,), fill, dtype=dt, device=DEV)
    buf[..., : t.shape[-1]] = _dev(t, dt)
    return buf[..., : t.shape[-1]]


def _out_view(shape, odt, left, right):
    """A sentinel-filled buffer one image longer and ``left + right`` channels wider than ``shape`` and the view
    of it a conv writes through."""
    N, OC = shape[0], shape[-1]
    buf = torch.full((N + 1,) + tuple(shape[1:-1]) + (left + OC + right,), SENT, dtype=odt, device=DEV)
    return buf, buf[:N, ..., left: left + OC]


def _untouched(buf, shape, left):
    chk = buf.clone()
    chk[: shape[0], ..., left: left + shape[-1]] = SENT
    return bool((chk == SENT).all())


def _launch(c, policy="auto", x_extra=0, left=0, right=8, mask_extra=0, x_fill=3.0, x_tail=False, more_extra=0,
            mask_fill=1.0, more_fill=1.0, **extra_kw):
    """Run case ``c`` on the GPU under ``policy``: x (and its mask) as channel slices of buffers ``x_extra`` /
    ``mask_extra`` wider (x's extra channels hold ``x_fill``), the output through a sentinel-framed view.
    ``x_tail``: x is the last rows of a longer dense buffer, so it ends where the storage ends (its leading rows
    hold ``x_fill``). ``more_extra``: res / emask as channel slices of buffers that much wider (their row stride
    decides the epilogue with the output's). ``mask_fill`` / ``more_fill``: what the mask's and res / emask's extra
    channels hold.
    Returns (result, route, bits_flags)."""
    dt = c.dt
    kw = dict(c.kw)
    if "code" in kw:
        kw["code"] = kw["code"].to(DEV)
    if "mask" in kw:
        kw["mask"] = _wide(kw["mask"], dt, mask_extra, fill=mask_fill)
    for key, v in c.more.items():
        kw[key] = _wide(v, dt, more_extra, fill=more_fill)
    oshape = tuple((c.ref[0] if c.epi == "pool" else c.ref).shape)
    buf, view = _out_view(oshape, c.odt, left, right)
    if c.base is not None:
        view.copy_(_dev(c.base, c.odt))
        kw["accumulate"] = True
    if x_tail:
        xbuf = torch.full((c.x.shape[0] + 3,) + tuple(c.x.shape[1:]), x_fill, dtype=dt, device=DEV)
        xbuf[3:] = _dev(c.x, dt)
        xd = xbuf[3:]
    else:
        xd = _wide(c.x, dt, x_extra, fill=x_fill)
    with _policy(policy):
        got = ops.conv2d(xd, c.cw.to_device(DEV, dt), out=view, **kw, **extra_kw)
        r, bits = _route(), Cm.bits_flags()
    assert _untouched(buf, oshape, left), "wrote outside the output view"
    return got, r, bits


def _expect(c, got):
    if c.epi == "pool":
        _same(got[0], c.ref[0])
        assert torch.equal(got[1].cpu(), c.ref[1]), "switch codes differ"
    else:
        _same(got, c.ref)


PW_H = 61  # image height of the persistent 1x1 kernel's cases (one image of PW_H x W pixels)


def _pw_m(G, OC):
    """Rows for about 2.25 tiles per CU with an M tail: tiles_total strictly between 2 G and 4 G, so with two
    workgroups per CU some walk two tiles and others one."""
    BM, BN = (128, 128) if OC % 128 == 0 else (256, 64)
    tiles_n = -(-OC // BN)
    tiles_m = 9 * G // (4 * tiles_n) + 1
    W = ((tiles_m - 1) * BM + BM // 2) // PW_H  # PW_H rows of W pixels: the last row tile is about half full
    M = PW_H * W
    assert 2 * G < -(-M // BM) * tiles_n < 4 * G and M % BM != 0
    return M, BM, BN


# ----------------------------------------------------------------------------------------
# rounding cases (test_conv_rounding_exact_gpu.py): operands whose results are INEXACT in 16 bits yet exact in
# fp32 under any summation order, and the conditions that make bit equality with rounding_oracle.py a test of
# where a kernel rounds
# ----------------------------------------------------------------------------------------

FRAC_Q = {BF: (5, 4), HF: (8, 7)}          # dtype -> (q, q'): bias fractions are k 2^-q, res / base are k 2^-q'
LIFT = {BF: (256, 1024), HF: (4096, 16384)}  # the binades (spacing 2-8) the lifted biases sit in
DENSE_INT = {BF: (15, 7), HF: (63, 31)}    # |x|, |w| limits of the bias-free cases: sums pass 2^8 / 2^11


def _frac_bias(g, oc, dt):
    """fp32 bias: an integer in [-4, 4] plus a multiple of 2^-q."""
    q = FRAC_Q[dt][0]
    return _ints(g, (oc,), -4, 4) + _ints(g, (oc,), 0, 2 ** q - 1) * 2.0 ** -q


def _frac16(g, shape, dt):
    """A residual / accumulate base: multiples of 2^-q' of magnitude < 16, each a ``dt`` value."""
    qp = FRAC_Q[dt][1]
    lim = 2 ** (qp + 4) - 1
    v = _ints(g, shape, -lim, lim) * 2.0 ** -qp
    assert torch.equal(v.to(dt).float(), v)
    return v


def _lift_bias(g, oc, dt):
    """Three channels in four get an integer bias inside ``LIFT[dt]`` (distinct fp32 window values then often
    round to one stored value); the fourth keeps [-4, 4], so ReLU zeros and true ties remain."""
    lo, hi = LIFT[dt]
    b = _ints(g, (oc,), -4, 4)
    lifted = _ints(g, (oc,), lo, hi - 1)
    keep = torch.arange(oc) % 4 == 3
    return torch.where(keep, b, lifted)


def _check_fp32_exact(y, x, cw, gbits, stride=1, pad=1, others=()):
    """fp32-exactness: (max sum |x| |w| + max |bias| + max |res| + max |base|) 2^g < 2^24 with 2^-g the case's
    finest granularity (every partial sum of every order is then an fp32 value), and the float64 result ``y``
    survives fp32."""
    bound = _absconv_max(x, cw, stride, pad) + sum(float(t.abs().max()) for t in others if t is not None)
    assert bound * 2.0 ** gbits < 2 ** 24, "partial sums not exact in fp32"
    fin = torch.isfinite(y)
    assert torch.equal(y[fin].float().double(), y[fin]), "result not exact in fp32"
    for t in (y,) + tuple(t for t in others if t is not None):
        s = t.double() * 2.0 ** gbits
        assert torch.equal(s, s.round()), "operand finer than the stated granularity"


def _check_rounding(y, dt):
    """Rounding density of the float64 result ``y`` for output type ``dt``: >= 20 % not representable, >= 5 %
    exact ties, ties resolved downward and upward each >= 2 %; and _check_exact's density conditions."""
    inexact = ~RO.representable(y, dt)
    r = RO.round16(y, dt)
    assert torch.equal(inexact, r != y), "representability test disagrees with the conversion"
    tie = RO.ties(y, dt)
    n = y.numel()
    f = lambda m: float(m.sum()) / n
    assert f(inexact) >= 0.20, f"only {f(inexact):.3f} of the outputs are inexact in {dt}"
    assert f(tie) >= 0.05, f"only {f(tie):.3f} of the outputs are exact ties"
    assert f(tie & (r < y)) >= 0.02 and f(tie & (r > y)) >= 0.02, \
        f"ties resolve down / up in {f(tie & (r < y)):.3f} / {f(tie & (r > y)):.3f} of the outputs"
    assert f(y != 0) >= 0.25, "too few non-zero outputs"
    assert r.flatten()[:65536].unique().numel() >= 16, "too few distinct values"


def _check_separation(one, two, OC):
    """Model separation: the once- and twice-rounded oracles differ on >= 5 % of the outputs, and inside the last
    partial 8-channel chunk where OC % 8 != 0."""
    d = one != two
    assert float(d.float().mean()) >= 0.05, f"models differ on {float(d.float().mean()):.3f} of the outputs only"
    if OC % 8:
        assert bool(d[..., OC - OC % 8:].any()), "models agree on the last partial chunk"


def _check_pool_separation(full, dt):
    """Pool separation on the unrounded ReLU'd map ``full`` (float64): first-max codes of the ROUNDED map differ
    from those of the unrounded one in >= 1 % of the windows; the rounded map is tie-rich (_check_ties).
    Returns (pooled values, codes) of the rounded map: round, then pool."""
    rv, rc = RO.pool_first_max(RO.round16(full, dt))
    ev, ec = RO.pool_first_max(full)
    assert torch.equal(RO.round16(ev, dt), rv), "pooled values depend on the rounding point"
    sep = float((rc != ec).float().mean())
    assert sep >= 0.01, f"codes differ in {sep:.4f} of the windows only"
    _check_ties(RO.round16(full, dt))
    return rv, rc
