"""Helpers shared by the exact-oracle GPU tests (test_conv_exact_gpu.py, test_conv_routes_exact_gpu.py,
test_dream_exact_gpu.py, test_engine_exact_gpu.py through engine_oracle.py): seeded
integer operands, the method's conditions on a CPU reference, and bit equality with it. A plain module,
not a conftest: nothing here changes how the suite is collected or run."""
import pytest
import torch
import torch.nn.functional as F

from deconv_api_amd import ops
from deconv_api_amd.ops.conv import ConvWeights

DEV = "cuda"
BF, HF = torch.bfloat16, torch.float16


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
