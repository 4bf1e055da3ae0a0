"""A float64 oracle of ``ops.conv2d`` that rounds at STATED points (tests/test_conv_rounding_exact_gpu.py).

Independent of ``ops.conv._conv2d_ref``: float64 ``F.conv2d`` / ``F.conv_transpose2d`` and the operation order of
the ``conv2d`` docstring: v = conv + bias; ReLU (without ``res``); += ``res``; += the old ``out``; ReLU (with
``res``); zero where ``emask`` <= 0. The operands of the rounding cases make every float64 value here exact, and
exact in fp32 as well under any summation order, so the only freedom a kernel has is WHERE it rounds to 16 bits:

  single  one conversion, at the end (the CPU path, the register epilogues, the split-K reduce, conv_igemm);
  staged  t = round16(v) after the first ReLU (the 16-bit C tile in LDS), then round16(act(t + res + out)),
          then emask (csrc/conv_dma_impl.h epilogue_lds / epi_combine / epi_tail).

Without ``res`` / ``accumulate`` the two coincide. Conversions are torch's ``.to(dtype)`` (round to nearest, ties
to even) of an fp32 tensor that holds the float64 value exactly (asserted)."""
import torch
import torch.nn.functional as F

SIG = {torch.bfloat16: 8, torch.float16: 11}  # significand bits, the implicit one included


def round16(v, dt):
    """float64 -> ``dt`` -> float64, through fp32 (which must hold ``v`` exactly: one rounding, not two)."""
    f = v.float()
    assert torch.equal(f.double(), v), "value not exact in fp32"
    return f.to(dt).double()


def unpool(p, code, div=1):
    """NHWC max-unpool of ``p`` by switch codes shared by ``div`` images."""
    N, PH, PW, C = p.shape
    code = code.repeat_interleave(div, dim=0).long()
    out = p.new_zeros(N, PH, 2, PW, 2, C)
    for pos in range(4):
        out[:, :, pos >> 1, :, pos & 1, :] = torch.where(code == pos, p, torch.zeros_like(p))
    return out.reshape(N, 2 * PH, 2 * PW, C)


def conv_acc(x, w_oihw, kind, stride, pad, out_hw):
    """The bias-free conv sum, NHWC float64. ``x`` NHWC (the conv's effective input), ``out_hw`` the output window."""
    X = x.double().permute(0, 3, 1, 2)
    w = w_oihw.double()
    KH, KW = w.shape[2:]
    H, W = X.shape[2:]
    OH, OW = out_hw
    if kind == "transpose":
        oph = OH - ((H - 1) * stride - 2 * pad[0] + KH)
        opw = OW - ((W - 1) * stride - 2 * pad[1] + KW)
        Y = F.conv_transpose2d(X, w, None, stride=stride, padding=pad, output_padding=(oph, opw))
    else:
        rb = (OH - 1) * stride + KH - H - pad[0]
        rr = (OW - 1) * stride + KW - W - pad[1]
        Y = F.conv2d(F.pad(X, (pad[1], rr, pad[0], rb)), w, None, stride=stride)
    assert tuple(Y.shape[2:]) == (OH, OW)
    return Y.permute(0, 2, 3, 1).contiguous()


def _act(v, relu, relu_cols):
    if not relu:
        return v
    if relu_cols > 0:
        return torch.cat([v[..., :relu_cols].clamp_min(0), v[..., relu_cols:]], dim=-1)
    return v.clamp_min(0)


def _mask(v, emask):
    return v if emask is None else torch.where(emask.double() > 0, v, torch.zeros_like(v))


def exact(acc, bias, relu, res=None, base=None, emask=None, relu_cols=0):
    """The unrounded float64 result in the documented order."""
    v = acc if bias is None else acc + bias.double()
    if res is None:
        v = _act(v, relu, relu_cols)
    else:
        v = v + res.double()
    if base is not None:
        v = v + base.double()
    if res is not None:
        v = _act(v, relu, relu_cols)
    return _mask(v, emask)


def single(acc, bias, relu, dt, res=None, base=None, emask=None, relu_cols=0):
    return round16(exact(acc, bias, relu, res, base, emask, relu_cols), dt)


def staged(acc, bias, relu, dt, res=None, base=None, emask=None, relu_cols=0):
    v = acc if bias is None else acc + bias.double()
    if res is None:
        v = _act(v, relu, relu_cols)
    t = round16(v, dt)
    if res is not None:
        t = t + res.double()
    if base is not None:
        t = t + base.double()
    if res is not None:
        t = _act(t, relu, relu_cols)
    return _mask(round16(t, dt), emask)


MIN_NORMAL_EXP = {torch.bfloat16: -126, torch.float16: -14}  # smallest normal 2^e; below it the grid is fixed
SUB_GRID_EXP = {dt: e - (SIG[dt] - 1) for dt, e in MIN_NORMAL_EXP.items()}  # 2^-133 (bf16), 2^-24 (fp16)


def _on_grid(v, dt, extra):
    """``v`` is a multiple of its ``dt`` spacing / 2^extra: the binade's spacing in the normal range (frexp: |v| =
    m 2^e with m in [0.5, 1), spacing 2^(e - SIG)), the fixed grid 2^SUB_GRID_EXP below the smallest normal."""
    m, e = torch.frexp(v)
    s = m * float(2 ** (SIG[dt] + extra))
    # below 2^MIN_NORMAL_EXP: e <= MIN_NORMAL_EXP, and the spacing stays 2^(MIN_NORMAL_EXP + 1 - SIG)
    shift = (MIN_NORMAL_EXP[dt] + 1 - e).clamp_min(0)
    s = torch.ldexp(s, -shift)
    return s == s.round()


def representable(v, dt):
    """Elementwise: float64 ``v`` is a finite ``dt`` value, normal or subnormal (0 included)."""
    return _on_grid(v, dt, 0)


def ties(v, dt):
    """Elementwise: ``v`` lies exactly half way between two neighbouring ``dt`` values (one more significand bit
    holds it, ``dt`` does not; below the smallest normal: an odd multiple of half the fixed grid)."""
    return _on_grid(v, dt, 1) & ~representable(v, dt)


def windows(full):
    N, H, W, C = full.shape
    return full.view(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)


def pool_first_max(full):
    """2 x 2 / stride 2 max and the row-major FIRST maximal position of each window of ``full`` [N, H, W, C]."""
    win = windows(full)
    val = win.max(dim=3).values
    code = (win == val.unsqueeze(3)).to(torch.int8).argmax(dim=3).to(torch.uint8)
    return val, code
