"""Helpers shared by the exact-oracle GPU tests (test_conv_exact_gpu.py, test_dream_exact_gpu.py): seeded
integer operands, the method's conditions on a CPU reference, and bit equality with it. A plain module,
not a conftest: nothing here changes how the suite is collected or run."""
import pytest
import torch
import torch.nn.functional as F

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
        assert ref.unique().numel() >= 16, "too few distinct values"


def _dev(t, dt):
    return None if t is None else t.to(dt).to(DEV)


def _same(got, ref):
    """Bit equality with the reference (values compared as fp32: -0.0 == 0.0 is not a difference)."""
    g, r = got.float().cpu(), ref.float()
    if g.shape != r.shape or not torch.equal(g, r):
        bad = (g != r).nonzero()
        pytest.fail(f"{int((g != r).sum())} of {g.numel()} values differ, first at {bad[0].tolist()}: "
                    f"got {float(g[tuple(bad[0])])}, want {float(r[tuple(bad[0])])}")
