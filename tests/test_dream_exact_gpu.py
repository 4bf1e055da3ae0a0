"""GPU: the DeepDream-side kernels (k x k pooling, the direct stem convs, ResNet-50 conv1 forward and input
gradient, col2im, sub-pixel scatter, the sum-of-squares loss) against an EXACT oracle.

As in test_conv_exact_gpu.py the operands are small integers (or multiples chosen so that every division
the kernel makes is exact), so every product and partial sum is exact in fp32 under any summation order
and the results are exact in bf16 and fp16: a correct kernel reproduces the CPU reference bit for bit
(``torch.equal`` on values compared as fp32). One wrong border tap, parity class, window divisor or
first-max switch shows, however small it is next to the largest value of the tensor.

Every case is built by a ``_*_case`` function that draws the operands, computes the CPU reference and
asserts the method's conditions on the reference alone, for both dtypes: the reference is representable in
the output type, every partial sum is bounded below 2^24, the reference is not degenerate (>= 25 %
non-zero outputs, except where structure forces zeros), and for the max pools >= 5 % of the windows tie.
``test_conditions`` (no GPU) builds every case of every table, so a condition failure is never mistaken
for a kernel failure; the GPU tests build the same cases (cached: the reference is computed once and never
modified) before they look at a GPU result.
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from deconv_api_amd.ops import autograd as AG
from exact_helpers import BF, DEV, HF, _dev, _gen, _ints, _same, _signs, _weights

gpu = pytest.mark.gpu
dtypes = pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
SENTINEL = 7.0


# ----------------------------------------------------------------------------------------
# conditions
# ----------------------------------------------------------------------------------------

def _representable(ref, what="reference"):
    """``ref`` (fp32 / fp64) is exactly representable in both 16-bit output types."""
    for dt in (BF, HF):
        assert torch.equal(ref.to(dt).double(), ref.double()), f"{what} not representable in {dt}"


def _conditions(ref, bound, where=None):
    """The method's conditions on a CPU reference: representable, partial sums (bounded by ``bound``) exact
    in fp32, and at least a quarter of the outputs non-zero (of those at ``where`` when structure forces
    zeros elsewhere)."""
    _representable(ref)
    assert float(bound) < 2 ** 24, "partial sums not exact in fp32"
    live = ref if where is None else ref[where]
    assert live.numel() > 0 and float((live != 0).double().mean()) >= 0.25, "too few non-zero outputs"


def _case(**kw):
    return types.SimpleNamespace(**kw)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _untouched(buf, before, lo, hi):
    """No byte of ``buf`` outside channels [lo, hi) differs from ``before`` (compared as bit patterns)."""
    a, b = buf.view(torch.int16).clone(), before.view(torch.int16).clone()
    a[..., lo:hi] = 0
    b[..., lo:hi] = 0
    return torch.equal(a, b)


# ----------------------------------------------------------------------------------------
# 1. k x k pooling
# ----------------------------------------------------------------------------------------

POOL_SHAPES = [(N, H, W, C) for N in (2, 3) for H, W in [(13, 11), (14, 16), (9, 10), (3, 3), (2, 5)] for C in (8, 24)]
POOL_K3 = [(3, 2, 0), (3, 2, 1), (3, 1, 1), (3, 1, 0)]        # the unrolled KC = 3 template
POOL_GENERIC = [(2, 2, 0), (4, 2, 1), (5, 1, 2), (5, 3, 1), (7, 2, 3)]  # the generic KC = 0 template
# average pools: inputs are multiples of the lcm of the window counts (k -> multiple, integer range), so
# sum * (1.f / count) is an exact integer; 5 x 5 and 7 x 7 have no usable multiple within bf16's integers
AVG_MULT = {3: (36, 3), 4: (144, 1), 2: (4, 8)}


def _pool_out(L, k, s, p):
    return (L + 2 * p - k) // s + 1


def _pool_cases(geoms):
    """geometry x shape, without the geometries whose output would be empty"""
    return [(k, s, p, N, H, W, C) for k, s, p in geoms for N, H, W, C in POOL_SHAPES
            if _pool_out(H, k, s, p) >= 1 and _pool_out(W, k, s, p) >= 1]


MAX_CASES = _pool_cases(POOL_K3 + POOL_GENERIC)
AVG_CASES = _pool_cases(POOL_K3 + [(2, 2, 0), (4, 2, 1)])
# one geometry per kernel on channel-slice views (the Inception blocks' max 3x3 / 2 and avg 3x3 / 1 pad 1)
SLICE_CASES = [("max_fwd", (3, 2, 0, 2, 13, 11, 24)), ("max_bwd", (3, 2, 0, 2, 13, 11, 24)),
               ("avg_fwd", (3, 1, 1, 2, 13, 11, 24)), ("avg_bwd", (3, 1, 1, 2, 13, 11, 24)),
               ("max_fwd", (5, 3, 1, 3, 9, 10, 8)), ("avg_bwd", (4, 2, 1, 3, 9, 10, 8))]


def _geom(c):
    return [c.N, c.H, c.W, c.C, c.OH, c.OW, c.k, c.s, c.p]


@functools.lru_cache(maxsize=None)
def _max_case(k, s, p, N, H, W, C):
    g = _gen(1000 * k + 100 * s + 10 * p + N * H * W + C)
    x = _ints(g, (N, H, W, C), -4, 4)
    xg = x.clone().requires_grad_(True)
    y, flat = F.max_pool2d(_nchw(xg), k, s, p, return_indices=True)
    OH, OW = y.shape[2:]
    assert (OH, OW) == (_pool_out(H, k, s, p), _pool_out(W, k, s, p))
    # the switch the kernel header promises: the window position kh * k + kw of the FIRST max in row-major
    # order (the CPU max_pool2d keeps the first max: it replaces on val > maxval only)
    ih, iw = flat // W, flat % W
    kh = ih - (torch.arange(OH).view(1, 1, OH, 1) * s - p)
    kw = iw - (torch.arange(OW).view(1, 1, 1, OW) * s - p)
    assert bool(((kh >= 0) & (kh < k) & (kw >= 0) & (kw < k)).all())
    idx = _nhwc((kh * k + kw).to(torch.uint8))
    win = F.unfold(F.pad(_nchw(x), (p, p, p, p), value=float("-inf")), k, stride=s).view(N, C, k * k, OH * OW)
    top = win.max(dim=2, keepdim=True).values
    assert torch.equal(top.view(N, C, OH, OW), y.detach())
    # (the same switch once more, straight from the windows: the smallest position that holds the max)
    first = torch.where(win == top, torch.arange(k * k).view(1, 1, -1, 1), k * k).min(dim=2).values
    assert torch.equal(_nhwc(first.view(N, C, OH, OW)).to(torch.uint8), idx)
    assert float(((win == top).sum(dim=2) >= 2).double().mean()) >= 0.05, "too few tied windows"
    gy = _ints(g, (N, OH, OW, C), -3, 3)
    (gx,) = torch.autograd.grad(_nhwc(y), xg, gy)
    base = _ints(g, (N, H, W, C), -4, 4)
    chosen = torch.zeros(N * C, H * W).scatter_(1, flat.reshape(N * C, -1), 1.0).view(N, C, H, W) > 0
    nwin = (-(-k // s)) ** 2  # windows that contain one pixel, at most
    _conditions(_nhwc(y.detach()), 4)
    _conditions(gx, 3 * nwin, where=_nhwc(chosen))
    _conditions(base + gx, 3 * nwin + 4)
    return _case(k=k, s=s, p=p, N=N, H=H, W=W, C=C, OH=OH, OW=OW, x=x, y=_nhwc(y.detach()), idx=idx, gy=gy, gx=gx,
                 base=base)


FWD_EPILOGUES = [(False, False), (True, False), (True, True), (False, True)]  # (bias, relu)


def _avg_epilogue(y, bias, relu):
    y = y if bias is None else y + bias.double()
    return y.clamp_min(0) if relu else y


def _recip_exact(m, cnt):
    """The kernel's fp32 formula m * (1.f / count) equals the exact quotient m / count (m fp32 integers,
    cnt the window counts, broadcastable); returns the fp32 result."""
    inv = torch.ones((), dtype=torch.float32) / cnt.float()
    q = m.float() * inv
    assert torch.equal(q.double(), m.double() / cnt.double()), "sum * (1.f / count) is not the exact average"
    assert torch.equal(q, q.round()), "average is not an integer"
    return q


@functools.lru_cache(maxsize=None)
def _avg_case(k, s, p, N, H, W, C):
    mult, r = AVG_MULT[k]
    g = _gen(2000 * k + 100 * s + 10 * p + N * H * W + C)
    x = mult * _ints(g, (N, H, W, C), -r, r)
    xg = x.double().requires_grad_(True)
    y = F.avg_pool2d(_nchw(xg), k, s, p, count_include_pad=False)
    OH, OW = y.shape[2:]
    assert (OH, OW) == (_pool_out(H, k, s, p), _pool_out(W, k, s, p))
    cnt = F.avg_pool2d(torch.ones(1, 1, H, W, dtype=torch.float64), k, s, p, divisor_override=1)  # [1, 1, OH, OW]
    assert all(mult % int(c) == 0 for c in cnt.unique()), "the window counts must divide the input multiple"
    wsum = F.avg_pool2d(_nchw(x), k, s, p, divisor_override=1)  # fp32 window sums: integers, exact
    y32 = _recip_exact(wsum, cnt)
    assert torch.equal(y32.double(), y.detach())
    bias = _ints(g, (C,), -4, 4)
    gy = mult * _ints(g, (N, OH, OW, C), -r, r)
    (gx,) = torch.autograd.grad(_nhwc(y), xg, gy.double())
    # the backward kernels sum inv * gy per window: each term an exact integer
    _recip_exact(_nchw(gy), cnt)
    base = _ints(g, (N, H, W, C), -4, 4)
    yb = _nhwc(y.detach())
    nwin = (-(-k // s)) ** 2
    _conditions(yb, k * k * mult * r)
    for b, relu in FWD_EPILOGUES:
        _conditions(_avg_epilogue(yb, bias if b else None, relu), k * k * mult * r + 4,
                    where=(yb + (bias if b else 0)) > 0 if relu else None)
    _conditions(gx, nwin * mult * r)
    _conditions(base.double() + gx, nwin * mult * r + 4)
    return _case(k=k, s=s, p=p, N=N, H=H, W=W, C=C, OH=OH, OW=OW, x=x, y=yb, bias=bias, gy=gy, gx=gx, base=base)


@gpu
@dtypes
@pytest.mark.parametrize("k,s,p,N,H,W,C", MAX_CASES)
def test_exact_maxpool_fwd(native_lib, k, s, p, N, H, W, C, dt):
    """maxpool_fwd_kernel: values equal F.max_pool2d, switches equal the window position of the first max
    in row-major order (ties in >= 5 % of the windows; on 3 x 3 windows of nine values, in most)."""
    c = _max_case(k, s, p, N, H, W, C)
    y = torch.full((N, c.OH, c.OW, C), SENTINEL, dtype=dt, device=DEV)
    idx = torch.full((N, c.OH, c.OW, C), 255, dtype=torch.uint8, device=DEV)
    native_lib.pool(_dev(c.x, dt), y, idx, 0, 0, _geom(c))
    _same(y, c.y)
    assert torch.equal(idx.cpu(), c.idx), f"{int((idx.cpu() != c.idx).sum())} of {idx.numel()} switches differ"
    yd = AG.max_pool(_dev(c.x, dt), k, s, p)
    assert yd.dtype == dt
    _same(yd, c.y)


@gpu
@dtypes
@pytest.mark.parametrize("k,s,p,N,H,W,C", MAX_CASES)
def test_exact_maxpool_bwd(native_lib, monkeypatch, k, s, p, N, H, W, C, dt):
    """maxpool_bwd_kernel from the REFERENCE's switches (independent of the forward kernel), plain and
    accumulated onto an integer base, and through ops.autograd.max_pool (the kernel's own switches); the
    3 x 3 / 2 cases on the unrolled 2 x 2 window path and on the generic loop (DV_NO_POOL_UNROLL=1)."""
    c = _max_case(k, s, p, N, H, W, C)
    for generic in (False, True) if (k, s) == (3, 2) else (False,):
        if generic:
            monkeypatch.setenv("DV_NO_POOL_UNROLL", "1")
        gx = torch.full((N, H, W, C), SENTINEL, dtype=dt, device=DEV)
        native_lib.pool(_dev(c.gy, dt), gx, c.idx.to(DEV), 0, 1, _geom(c))
        _same(gx, c.gx)
        acc = _dev(c.base, dt)
        native_lib.pool(_dev(c.gy, dt), acc, c.idx.to(DEV), 0, 1, _geom(c), None, False, True)
        _same(acc, c.base + c.gx)
        xd = _dev(c.x, dt).requires_grad_(True)
        (gd,) = torch.autograd.grad(AG.max_pool(xd, k, s, p), xd, _dev(c.gy, dt))
        assert gd.dtype == dt
        _same(gd, c.gx)


@gpu
@dtypes
@pytest.mark.parametrize("k,s,p,N,H,W,C", AVG_CASES)
def test_exact_avgpool_fwd(native_lib, k, s, p, N, H, W, C, dt):
    """avgpool_fwd_kernel, count_include_pad = False: the divisor of every border window (4, 6, 9 for
    3 x 3), without and with the fp32 bias and the ReLU the Inception pool branches fuse."""
    c = _avg_case(k, s, p, N, H, W, C)
    for b, relu in FWD_EPILOGUES:
        y = torch.full((N, c.OH, c.OW, C), SENTINEL, dtype=dt, device=DEV)
        native_lib.pool(_dev(c.x, dt), y, None, 1, 0, _geom(c), c.bias.to(DEV) if b else None, relu)
        _same(y, _avg_epilogue(c.y, c.bias if b else None, relu))
    _same(AG.avg_pool(_dev(c.x, dt), k, s, p), c.y)


@gpu
@dtypes
@pytest.mark.parametrize("k,s,p,N,H,W,C", AVG_CASES)
def test_exact_avgpool_bwd(native_lib, monkeypatch, k, s, p, N, H, W, C, dt):
    """avgpool_bwd_kernel: plain, accumulated onto an integer base and through ops.autograd.avg_pool; the
    3 x 3 / 1 cases on the unrolled 3 x 3 window path and on the generic loop (DV_NO_POOL_UNROLL=1).

    Gradients that cancel to 0 are the sharp part: with ``acc += inv * gy`` contracted into an FMA (the
    product unrounded: a share of 108 / 9 is 12 + 9e-8) 142 of these 240 cases left 3.6e-7 to 1.9e-6 at
    8 to 802 such elements; the kernel now rounds each share (docs/KERNELS.md, round 8)."""
    c = _avg_case(k, s, p, N, H, W, C)
    for generic in (False, True) if (k, s) == (3, 1) else (False,):
        if generic:
            monkeypatch.setenv("DV_NO_POOL_UNROLL", "1")
        gx = torch.full((N, H, W, C), SENTINEL, dtype=dt, device=DEV)
        native_lib.pool(_dev(c.gy, dt), gx, None, 1, 1, _geom(c))
        _same(gx, c.gx)
        acc = _dev(c.base, dt)
        native_lib.pool(_dev(c.gy, dt), acc, None, 1, 1, _geom(c), None, False, True)
        _same(acc, c.base.double() + c.gx)
        xd = _dev(c.x, dt).requires_grad_(True)
        (gd,) = torch.autograd.grad(AG.avg_pool(xd, k, s, p), xd, _dev(c.gy, dt))
        assert gd.dtype == dt
        _same(gd, c.gx)


def _slice_of(t, dt, extra):
    """``t`` as the channel slice [8, 8 + C) of a sentinel-filled buffer with pixel stride C + extra."""
    C = t.shape[3]
    buf = torch.full(t.shape[:3] + (C + extra,), SENTINEL, dtype=dt, device=DEV)
    buf[..., 8:8 + C] = _dev(t, dt)
    return buf, buf[..., 8:8 + C]


@gpu
@dtypes
@pytest.mark.parametrize("kernel,geom", SLICE_CASES, ids=[f"{n}-{'-'.join(map(str, c))}" for n, c in SLICE_CASES])
def test_exact_pool_channel_slices(native_lib, kernel, geom, dt):
    """The four pool kernels on channel-slice views of wider buffers (x_ld = C + 8, y_ld = C + 16, slices
    from channel 8: how ops/inception.py pools out of and into its concat buffers; the avg forward with
    its bias and ReLU, the max backward accumulating): exact inside the slice, no byte changed outside
    it, nor in the input buffer. The switches stay dense."""
    k, s, p, N, H, W, C = geom
    kind = 0 if kernel.startswith("max") else 1
    c = (_max_case if kind == 0 else _avg_case)(*geom)
    if kernel.endswith("fwd"):
        src, dst, want = c.x, torch.zeros_like(c.y), c.y
        if kind == 1:
            want = _avg_epilogue(c.y, c.bias, True)
    else:
        src, dst = c.gy, (c.base if kind == 0 else torch.zeros_like(c.gx))
        want = c.base + c.gx if kind == 0 else c.gx
    fwd = kernel.endswith("fwd")
    sbuf, sv = _slice_of(src, dt, 8 if fwd else 16)
    dbuf, dv = _slice_of(dst, dt, 16 if fwd else 8)
    s0, d0 = sbuf.clone(), dbuf.clone()
    idx = None
    if kind == 0:
        idx = torch.full((N, c.OH, c.OW, C), 255, dtype=torch.uint8, device=DEV) if fwd else c.idx.to(DEV)
    if kernel == "avg_fwd":
        native_lib.pool(sv, dv, None, 1, 0, _geom(c), c.bias.to(DEV), True)
    else:
        native_lib.pool(sv, dv, idx, kind, 0 if fwd else 1, _geom(c), None, False, kernel == "max_bwd")
    assert _untouched(dbuf, d0, 8, 8 + C), "wrote outside the output's channel slice"
    assert torch.equal(sbuf.view(torch.int16), s0.view(torch.int16)), "changed its input"
    _same(dv, want)
    if kernel == "max_fwd":
        assert torch.equal(idx.cpu(), c.idx)


# ----------------------------------------------------------------------------------------
# 2. direct stem kernels (csrc/conv_stem.hip)
# ----------------------------------------------------------------------------------------

STEM_FWD_CASES = [(N, H, W, pad, bias, relu) for N, H, W in [(2, 9, 8), (2, 17, 23), (1, 35, 33)] for pad in (0, 1)
                  for bias in (False, True) for relu in (False, True)]
# (N, H, W, pad): H, W odd / even / mixed; one class of more than 256 pixels; H = 1 and W = 1 (pad 1 only:
# without padding a 3 x 3 window needs three rows), where two of the four parity classes have no pixel
STEM_DGRAD_CASES = [(N, H, W, pad) for N, H, W in [(2, 9, 7), (2, 8, 10), (1, 9, 8), (2, 8, 9), (1, 35, 33)]
                    for pad in (0, 1)] + [(2, 1, 9, 1), (2, 9, 1, 1), (1, 1, 1, 1)]
STEM_DGRAD7_CASES = [(2, 9, 12), (1, 16, 17)]


def _rgb8(x):
    """[N, H, W, 3] -> the 8-channel padded input (channels 3 .. 7 zero)"""
    return F.pad(x, (0, 5))


def _conv_dgrad_ref(gy, w, H, W, stride, pad):
    """CPU autograd input gradient of F.conv2d(x [N, H, W, 3], w, stride, pad) for the output gradient gy (NHWC)"""
    x = torch.zeros(gy.shape[0], w.shape[1], H, W, requires_grad=True)
    y = F.conv2d(x, w, None, stride=stride, padding=pad)
    assert y.shape[2:] == gy.shape[1:3]
    (gx,) = torch.autograd.grad(y, x, _nchw(gy))
    return _nhwc(gx)


def _abs_dgrad_bound(gy, w, H, W, stride, pad):
    return float(_conv_dgrad_ref(gy.abs(), w.abs(), H, W, stride, pad).max())


@functools.lru_cache(maxsize=None)
def _stem_fwd_case(N, H, W, pad, bias, relu):
    g = _gen(N * H * W + pad)  # (one x and w per shape: the four epilogues differ in the epilogue only)
    x = _ints(g, (N, H, W, 3), -3, 3)
    cw = _weights(g, 32, 3, bias=True)  # K = 27 taps: nothing to thin, |y| <= 27 * 6 + 4
    b = cw.bias if bias else None
    y = _nhwc(F.conv2d(_nchw(x), cw.w_oihw, b, stride=2, padding=pad))
    ref = y.relu() if relu else y
    _conditions(ref, 27 * 6 + 4, where=y > 0 if relu else None)
    assert float((ref != 0).float().mean()) >= 0.25
    return _case(x=x, w=cw.w_oihw, b=b, ref=ref)


@functools.lru_cache(maxsize=None)
def _stem_dgrad_case(N, H, W, pad, cout=32, k=3):
    g = _gen(N * H * W + pad + k)
    # 3 x 3: <= 4 taps x 32 channels meet one pixel; 7 x 7: <= 16 x 64, thinned to about 96 non-zero terms
    cw = _weights(g, cout, 3, k, k, bias=False, taps=3 * k * k if k == 3 else 14)
    OH, OW = (H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1
    # about half zeros, as a premasked gradient arrives
    gy = _ints(g, (N, OH, OW, cout), -3, 3) * (torch.rand(N, OH, OW, cout, generator=g) < 0.5)
    gx = _conv_dgrad_ref(gy, cw.w_oihw, H, W, 2, pad)
    # (rows and columns that no window reads get no gradient: structure; the others are dense)
    _conditions(gx, _abs_dgrad_bound(gy, cw.w_oihw, H, W, 2, pad),
                where=_conv_dgrad_ref(torch.ones_like(gy), torch.ones_like(cw.w_oihw), H, W, 2, pad) > 0)
    return _case(w=cw.w_oihw, gy=gy, gx=gx, OH=OH, OW=OW)


@gpu
@dtypes
@pytest.mark.parametrize("N,H,W,pad,bias,relu", STEM_FWD_CASES)
def test_exact_stem_conv_fwd(native_lib, N, H, W, pad, bias, relu, dt):
    """stem_conv_fwd_kernel (3 -> 32, 3 x 3 / 2) through the unit that owns its weight layout: pad 0 and 1,
    bias and ReLU on and off, one output pixel per thread up to past one 256-thread block."""
    c = _stem_fwd_case(N, H, W, pad, bias, relu)
    unit = AG.ConvUnit("u", c.w, c.b, 2, (pad, pad), relu=relu).build(DEV, dt)
    assert unit.stem_w is not None and unit.stem7_w is None
    y = AG._stem_fwd(_dev(_rgb8(c.x), dt), unit)
    assert y is not None and y.dtype == dt, "the direct kernel refused its own geometry"
    _same(y, c.ref)


@gpu
@dtypes
@pytest.mark.parametrize("N,H,W,pad", STEM_DGRAD_CASES)
def test_exact_stem_conv_dgrad(native_lib, N, H, W, pad, dt):
    """stem_conv_dgrad_s2_kernel<32, 3>: every stride-2 parity class at both pads, rows and columns no
    window reads, classes without a pixel; channels 3 .. 7 of gx are written as zeros."""
    c = _stem_dgrad_case(N, H, W, pad)
    unit = AG.ConvUnit("u", c.w, None, 2, (pad, pad), relu=False).build(DEV, dt)
    assert unit.stem_w is not None
    gx = torch.full((N, H, W, 8), SENTINEL, dtype=dt, device=DEV)
    geom = [N, H, W, c.OH, c.OW, 8, 3, 32, 3, 2, pad, 0]
    assert native_lib.stem_conv(_dev(c.gy, dt), unit.stem_w, None, gx, geom, 1)
    _same(gx[..., :3], c.gx)
    assert not bool(gx[..., 3:].float().any()), "padding channels must get a zero gradient"
    # and by the route the autograd takes (ops/autograd.py _dgrad_strided)
    _same(AG._dgrad_strided(unit, _dev(c.gy, dt), None, (H, W))[..., :3], c.gx)


@gpu
@dtypes
@pytest.mark.parametrize("N,H,W", STEM_DGRAD7_CASES)
def test_exact_stem_conv_dgrad_7x7(native_lib, N, H, W, dt):
    """The 7 x 7 / 64-channel instantiation of the same kernel (pad 3), through the binding with fp32
    [7][7][3][64] weights: the autograd does not route to it, the launcher accepts it."""
    c = _stem_dgrad_case(N, H, W, 3, 64, 7)
    w = c.w.permute(2, 3, 1, 0).contiguous().to(DEV)
    gx = torch.full((N, H, W, 8), SENTINEL, dtype=dt, device=DEV)
    assert native_lib.stem_conv(_dev(c.gy, dt), w, None, gx, [N, H, W, c.OH, c.OW, 8, 3, 64, 7, 2, 3, 0], 1)
    _same(gx[..., :3], c.gx)
    assert not bool(gx[..., 3:].float().any())


# ----------------------------------------------------------------------------------------
# 3. ResNet-50 conv1 forward (csrc/conv_stem7.hip, 16 x 32 output tiles)
# ----------------------------------------------------------------------------------------

# (H, W): one partial tile; exactly one tile; 2 x 2 tiles, the second row and column one pixel deep
STEM7_CASES = [(H, W, bias, relu) for H, W in [(5, 7), (32, 64), (33, 65)] for bias in (False, True)
               for relu in (False, True)]


@functools.lru_cache(maxsize=None)
def _stem7_case(H, W, bias, relu):
    g = _gen(H * W)
    x = _ints(g, (2, H, W, 3), -3, 3)
    cw = _weights(g, 64, 3, 7, 7, taps=48)  # 147 taps thinned to about 48: |y| <= 256
    b = cw.bias if bias else None
    y = _nhwc(F.conv2d(_nchw(x), cw.w_oihw, b, stride=2, padding=3))
    ref = y.relu() if relu else y
    assert float(ref.abs().max()) <= 256
    bound = float(F.conv2d(_nchw(x).abs(), cw.w_oihw.abs(), None, stride=2, padding=3).max()) + 4
    _conditions(ref, bound, where=y > 0 if relu else None)
    assert float((ref != 0).float().mean()) >= 0.25
    return _case(x=x, w=cw.w_oihw, b=b, ref=ref)


@gpu
@dtypes
@pytest.mark.parametrize("H,W,bias,relu", STEM7_CASES)
def test_exact_stem7_fwd(native_lib, H, W, bias, relu, dt):
    """stem7_fwd_kernel (3 -> 64, 7 x 7 / 2, pad 3) on partial, whole and several tiles."""
    c = _stem7_case(H, W, bias, relu)
    unit = AG.ConvUnit("u", c.w, c.b, 2, (3, 3), relu=relu).build(DEV, dt)
    assert unit.stem7_w is not None and AG.STEM7
    y = AG._stem_fwd(_dev(_rgb8(c.x), dt), unit)
    assert y is not None and y.dtype == dt, "the conv1 kernel refused its own geometry"
    _same(y, c.ref)


# ----------------------------------------------------------------------------------------
# 4. conv1 input gradient: fused kernel, GEMM + col2im, both col2im kernels
# ----------------------------------------------------------------------------------------

STEM_FUSED_CASES = [(H, W, masked) for H, W in [(7, 9), (17, 33), (32, 64), (37, 41)] for masked in (False, True)]
# (k, pad, H, W, lds): J_ld a multiple of 8 (the LDS kernel) or the dense J = k k 3 (147, 27: the simple one);
# (9, 70) and (17, 33) cross the LDS kernel's 8 x 64 tile in both directions
COL2IM_CASES = [(k, pad, H, W, lds) for k, pad in [(7, 3), (3, 0), (3, 1)] for H, W in [(9, 70), (17, 33)]
                for lds in (True, False)]


@functools.lru_cache(maxsize=None)
def _stem_fused_case(H, W, masked):
    g = _gen(H * W + masked)
    N, k, pad = 2, 7, 3
    cw = _weights(g, 64, 3, k, k, bias=False, taps=14)  # <= 16 taps x 64 channels per pixel, about 96 non-zero
    OH, OW = (H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1
    gy = _ints(g, (N, OH, OW, 64), -3, 3)
    mask = _signs(g, (N, OH, OW, 64)) if masked else None
    gym = gy * (mask > 0) if masked else gy  # both zeros mask like the negatives
    gx = _conv_dgrad_ref(gym, cw.w_oihw, H, W, 2, pad)
    # the intermediate cols (dy @ W^T per tap, [N, OH, OW, (kh, kw, c)]) are rounded to 16 bits in both paths
    cols = torch.einsum("nhwo,ocyx->nhwyxc", gym, cw.w_oihw)
    _representable(cols, "intermediate cols")
    assert float(torch.einsum("nhwo,ocyx->nhwyxc", gym.abs(), cw.w_oihw.abs()).max()) < 2 ** 24
    _conditions(gx, _abs_dgrad_bound(gym, cw.w_oihw, H, W, 2, pad))
    return _case(N=N, w=cw.w_oihw, gy=gy, mask=mask, gx=gx, OH=OH, OW=OW)


@functools.lru_cache(maxsize=None)
def _col2im_case(k, pad, H, W, lds):
    g = _gen(100 * k + 10 * pad + H + W + lds)
    N, Cr = 2, 3
    J = k * k * Cr
    J_ld = -(-J // 8) * 8 if lds else J
    assert (J_ld % 8 == 0) == lds
    OH, OW = (H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1
    cols = _ints(g, (N, OH, OW, J_ld), -3, 3)  # (columns J .. J_ld - 1 are padding: never read)
    # a pure-torch fold: column (kh k + kw) Cr + c -> fold's (c, kh, kw) channel order
    blocks = cols[..., :J].reshape(N, OH * OW, k, k, Cr).permute(0, 4, 2, 3, 1).reshape(N, Cr * k * k, OH * OW)
    gx = _nhwc(F.fold(blocks, (H, W), k, padding=pad, stride=2))
    covered = _nhwc(F.fold(torch.ones_like(blocks), (H, W), k, padding=pad, stride=2)) > 0
    _conditions(gx, 3 * (-(-k // 2)) ** 2, where=covered)
    return _case(N=N, cols=cols, gx=gx)


@gpu
@dtypes
@pytest.mark.parametrize("H,W,masked", STEM_FUSED_CASES)
def test_exact_stem_dgrad_fused(native_lib, monkeypatch, H, W, masked, dt):
    """ResNet-50 conv1's input gradient by the fused kernel (16 x 32 dx tiles: a partial tile, tiles one
    pixel deep, exactly 2 x 2 tiles, 3 x 2 with tails) AND by the 1 x 1 GEMM + col2im_lds_kernel, each
    against the CPU autograd gradient; without a mask and with a ReLU mask from {-1, -0.0, 0, 1}."""
    c = _stem_fused_case(H, W, masked)
    unit = AG.ConvUnit("u", c.w, None, 2, (3, 3), relu=True).build(DEV, dt)
    assert unit.stem_w is None and unit.col_w is not None
    gy, mask = _dev(c.gy, dt), _dev(c.mask, dt)
    gx = torch.full((c.N, H, W, 8), SENTINEL, dtype=dt, device=DEV)
    assert native_lib.stem_dgrad_fused(gy, mask, unit.col_w.w_gemm, gx, [7, 7, 2, 3, 3])
    _same(gx[..., :3], c.gx)
    assert not bool(gx[..., 3:].float().any()), "padding channels must get a zero gradient"
    monkeypatch.setattr(AG, "STEM_FUSED", False)
    g2 = AG._col2im_dgrad(gy, mask, unit, (H, W))
    _same(g2[..., :3], c.gx)
    assert not bool(g2[..., 3:].float().any())


@gpu
@dtypes
@pytest.mark.parametrize("k,pad,H,W,lds", COL2IM_CASES)
def test_exact_col2im(native_lib, k, pad, H, W, lds, dt):
    """lib.col2im alone on integer cols against a pure-torch fold: col2im_lds_kernel (J_ld % 8 == 0) and
    the simple col2im_kernel (dense J_ld = 147 / 27)."""
    c = _col2im_case(k, pad, H, W, lds)
    gx = torch.full((c.N, H, W, 8), SENTINEL, dtype=dt, device=DEV)
    native_lib.col2im(_dev(c.cols, dt), gx, [k, k, 2, pad, pad, 3])
    _same(gx[..., :3], c.gx)
    assert not bool(gx[..., 3:].float().any())


# ----------------------------------------------------------------------------------------
# 5. sub-pixel scatter (csrc/pool.hip)
# ----------------------------------------------------------------------------------------

SCATTER_CASES = [(C, s, H, W, masked) for C in (8, 24) for s in (1, 2, 3) for H, W in [(7, 9), (8, 8), (1, 5)]
                 for masked in (False, True)]


@functools.lru_cache(maxsize=None)
def _scatter_case(C, s, H, W, masked):
    g = _gen(100 * C + 10 * s + H * W + masked)
    N = 2
    E = _ints(g, (N, -(-H // s), -(-W // s), C), -4, 4)
    em = _signs(g, (N, H, W, C)) if masked else None
    gx = torch.zeros(N, H, W, C)
    gx[:, ::s, ::s] = E
    if masked:
        gx[em <= 0] = 0
    live = torch.zeros(N, H, W, C, dtype=torch.bool)
    live[:, ::s, ::s] = True
    _conditions(gx, 4, where=live & (em > 0) if masked else live)
    return _case(N=N, E=E, em=em, gx=gx)


@gpu
@dtypes
@pytest.mark.parametrize("C,s,H,W,masked", SCATTER_CASES)
def test_exact_subpixel_scatter(native_lib, C, s, H, W, masked, dt):
    """subpixel_scatter_kernel: E at every s-th pixel, zero elsewhere (all of gx is written), zero where
    emask <= 0 with zeros of both signs."""
    c = _scatter_case(C, s, H, W, masked)
    gx = torch.full((c.N, H, W, C), SENTINEL, dtype=dt, device=DEV)
    native_lib.subpixel_scatter(_dev(c.E, dt), _dev(c.em, dt), gx, s)
    _same(gx, c.gx)


# ----------------------------------------------------------------------------------------
# 6. loss kernels (csrc/dream.hip)
# ----------------------------------------------------------------------------------------

SUMSQ_CASES = [(2, 6, 6, 8, 1), (3, 9, 11, 24, 2), (1, 5, 7, 8, 2)]  # (N, H, W, C, b)
SUMSQ_PARTS = (1, 3, 5)


@functools.lru_cache(maxsize=None)
def _sumsq_case(N, H, W, C, b):
    g = _gen(N * H * W * C + b)
    x = _ints(g, (N, H, W, C), -3, 3)
    core = torch.zeros(N, H, W, C, dtype=torch.bool)
    core[:, b:H - b, b:W - b] = True
    loss = (x.double() ** 2 * core).sum(dim=(1, 2, 3))
    scale = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (N,), generator=g)]
    addend = _ints(g, (N, H, W, C), -4, 4)
    grad = 2 * scale.view(N, 1, 1, 1) * x * core
    assert float(loss.max()) < 2 ** 24 and float(loss.min()) > 0
    _conditions(grad, 6 * 2, where=core)
    _conditions(addend + grad, 6 * 2 + 4)
    return _case(x=x, core=core, loss=loss, scale=scale, addend=addend, grad=grad)


@gpu
@dtypes
@pytest.mark.parametrize("N,H,W,C,b", SUMSQ_CASES)
def test_exact_sumsq_core_fwd(native_lib, N, H, W, C, b, dt):
    """sumsq_core_kernel through the binding with 1, 3 and 5 partial sums per image, and through
    ops.autograd.sumsq_core: the exact integer sum of squares over the core."""
    c = _sumsq_case(N, H, W, C, b)
    for P in SUMSQ_PARTS:
        part = torch.full((N, P), SENTINEL, dtype=torch.float32, device=DEV)
        native_lib.sumsq_core(_dev(c.x, dt), part, b)
        assert torch.equal(part.double().sum(1).cpu(), c.loss), (P, part.tolist(), c.loss.tolist())
    got = AG.sumsq_core(_dev(c.x, dt), b)
    assert got.dtype == torch.float32 and torch.equal(got.double().cpu(), c.loss)


@gpu
@dtypes
@pytest.mark.parametrize("N,H,W,C,b", SUMSQ_CASES)
def test_exact_sumsq_core_bwd(native_lib, N, H, W, C, b, dt):
    """sumsq_core_bwd_kernel and sumsq_core_fused_kernel: 2 scale[n] x in the core and exactly 0 on the
    border; with an addend, addend + 2 scale[n] x in the core and the addend bit for bit on the border;
    the fused kernel writes the same gradient and the forward's partial sums."""
    c = _sumsq_case(N, H, W, C, b)
    x, scale = _dev(c.x, dt), c.scale.to(DEV)
    for addend in (None, c.addend):
        want = c.grad if addend is None else addend + c.grad
        gx = torch.full((N, H, W, C), SENTINEL, dtype=dt, device=DEV)
        native_lib.sumsq_core_bwd(x, scale, gx, b, _dev(addend, dt))
        _same(gx, want)
        border = ~c.core.to(DEV)
        if addend is None:
            assert not bool(gx[border].float().any())
        else:
            assert torch.equal(gx[border].view(torch.int16), _dev(addend, dt)[border].view(torch.int16))
        for P in SUMSQ_PARTS:
            fx = torch.full((N, H, W, C), SENTINEL, dtype=dt, device=DEV)
            part = torch.full((N, P), SENTINEL, dtype=torch.float32, device=DEV)
            native_lib.sumsq_core_bwd(x, scale, fx, b, _dev(addend, dt), part)
            assert torch.equal(fx.view(torch.int16), gx.view(torch.int16)), "fused gradient != unfused, bit for bit"
            assert torch.equal(part.double().sum(1).cpu(), c.loss), (P, part.tolist(), c.loss.tolist())
    # through the autograd function: the gradient of sum_n scale[n] * sumsq_core(x)[n]
    xd = x.clone().requires_grad_(True)
    (gd,) = torch.autograd.grad(AG.sumsq_core(xd, b), xd, scale)
    _same(gd, c.grad)


@gpu
@dtypes
@pytest.mark.parametrize("N,H,W,C,b", SUMSQ_CASES)
@pytest.mark.parametrize("with_part", [False, True], ids=["bwd", "fused"])
def test_exact_loss_tap(native_lib, N, H, W, C, b, with_part, dt):
    """loss_tap: the gradient that reaches the input is the upstream gradient plus the loss term (and, with
    ``part``, the backward leaves the layer's loss partials there)."""
    c = _sumsq_case(N, H, W, C, b)
    a = _dev(c.x, dt).requires_grad_(True)
    part = torch.full((N, 3), SENTINEL, dtype=torch.float32, device=DEV) if with_part else None
    out = AG.loss_tap(a, c.scale.to(DEV), b, part)
    assert torch.equal(out.detach(), a.detach())
    (ga,) = torch.autograd.grad(out, a, _dev(c.addend, dt))
    _same(ga, c.addend + c.grad)
    if with_part:
        assert torch.equal(part.double().sum(1).cpu(), c.loss)


@gpu
@dtypes
@pytest.mark.parametrize("H,W,b", [(4, 7, 2), (7, 4, 2), (2, 2, 1)])
def test_sumsq_core_refuses_empty_core(native_lib, H, W, b, dt):
    """A map with H <= 2 b or W <= 2 b has no core: sumsq_core and the fused kernel raise (their launchers
    return -1) and write nothing."""
    x = _dev(_ints(_gen(H + W), (2, H, W, 8), -3, 3), dt)
    part = torch.full((2, 1), SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="launch failed with code -1"):
        native_lib.sumsq_core(x, part, b)
    gx = torch.full((2, H, W, 8), SENTINEL, dtype=dt, device=DEV)
    with pytest.raises(RuntimeError, match="launch failed with code -1"):
        native_lib.sumsq_core_bwd(x, torch.ones(2, device=DEV), gx, b, None, part)
    torch.cuda.synchronize()
    assert bool((part == SENTINEL).all()) and bool((gx.float() == SENTINEL).all())


# ----------------------------------------------------------------------------------------
# the conditions of every case, on the CPU alone
# ----------------------------------------------------------------------------------------

CASE_TABLES = {
    "maxpool": (_max_case, MAX_CASES),
    "avgpool": (_avg_case, AVG_CASES),
    "pool_slices": (lambda kernel, geom: (_max_case if kernel.startswith("max") else _avg_case)(*geom), SLICE_CASES),
    "stem_conv_fwd": (_stem_fwd_case, STEM_FWD_CASES),
    "stem_conv_dgrad": (_stem_dgrad_case, STEM_DGRAD_CASES),
    "stem_conv_dgrad_7x7": (lambda N, H, W: _stem_dgrad_case(N, H, W, 3, 64, 7), STEM_DGRAD7_CASES),
    "stem7_fwd": (_stem7_case, STEM7_CASES),
    "stem_dgrad_fused": (_stem_fused_case, STEM_FUSED_CASES),
    "col2im": (_col2im_case, COL2IM_CASES),
    "subpixel_scatter": (_scatter_case, SCATTER_CASES),
    "sumsq_core": (_sumsq_case, SUMSQ_CASES),
}


@pytest.mark.parametrize("table", sorted(CASE_TABLES))
def test_conditions(table):
    """Every case of every table: generator, CPU reference and the method's conditions (asserted inside
    the case builders, for bf16 and fp16), without a GPU."""
    build, cases = CASE_TABLES[table]
    assert cases
    for case in cases:
        try:
            build(*case)
        except AssertionError as e:
            raise AssertionError(f"{table} case {case}: {e}") from e
