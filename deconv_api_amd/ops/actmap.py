"""Activation maps (Zeiler & Fergus, "Visualizing and Understanding Convolutional Networks", figure 7 (b)): the
feature map of a filter, upsampled to the network input and laid over the image.

``act [B, H, W, C]`` is the target layer's output (``DeconvNet.forward(x, layer).out``), ``S = r H`` the input side,
``r`` a power of two in 1..64. Bilinear with half-pixel centres (``cv2.INTER_LINEAR``,
``F.interpolate(align_corners=False)``), written in integers so nothing depends on float rounding of coordinates:
``t = 2 y + 1 - r``, ``y0 = floor(t / 2r)``, ``fy = (t - 2r y0) / 2r`` (exact in fp32), rows ``ya = clamp(y0, 0, H - 1)``
and ``yb = clamp(y0 + 1, 0, H - 1)``, the same for x, and with ``a = float(act[b, :, :, idx[b, k]])``

    heat[b, k, y, x] = (1 - fy) ((1 - fx) a[ya, xa] + fx a[ya, xb]) + fy ((1 - fx) a[yb, xa] + fx a[yb, xb])   (fp32)

A filter outside ``0 .. C - 1`` (-1 included) gives a zero map. ``part[b, k]`` holds maxima of ``|heat[b, k]|`` over
runs of 256 pixels: what ``occlusion_overlay`` takes.

Device tensors run csrc/actmap.hip; CPU tensors the torch reference below (what the CPU service uses)."""
from __future__ import annotations

from typing import Tuple

import torch

from . import native

MAX_RATIO = 64


def activation_ratio(S: int, H: int, W: int) -> int:
    """r = S / H; ValueError outside the definition (H != W, r not a power of two in 1..64, S outside 16..4096)."""
    if isinstance(S, bool) or not isinstance(S, int) or not 16 <= S <= 4096:
        raise ValueError(f"the image side must be an integer in 16..4096, got {S!r}")
    if H != W or H < 1 or S % H:
        raise ValueError(f"a {H} x {W} feature map does not upsample to {S} x {S} by a whole factor")
    r = S // H
    if r > MAX_RATIO or r & (r - 1):
        raise ValueError(f"the upsampling factor must be a power of two in 1..{MAX_RATIO}, got {r}")
    return r


def _taps(S: int, H: int, r: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per output coordinate: the two source coordinates (int64 [S]) and the weight of the second (fp32 [S])."""
    t = 2 * torch.arange(S) + 1 - r
    y0 = torch.div(t, 2 * r, rounding_mode="floor")
    f = (t - 2 * r * y0).float() / (2 * r)
    return y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1), f


def activation_heat(act: torch.Tensor, idx: torch.Tensor, S: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """act [B, H, W, C], idx int32 [B, 4] (-1: no filter) -> (heat fp32 [B, 4, S, S], part fp32 [B, 4, n] whose maximum
    over n is max |heat[b, k]|; n = kernel blocks on the GPU, 1 on the CPU)."""
    if act.dim() != 4:
        raise ValueError(f"expected a feature map [B, H, W, C], got {tuple(act.shape)}")
    B, H, W, C = act.shape
    r = activation_ratio(S, H, W)
    if tuple(idx.shape) != (B, 4):
        raise ValueError(f"idx must be [{B}, 4]")
    idx = idx.to(torch.int32)
    if act.is_cuda:
        if act.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("activation_heat on the GPU takes the 16-bit layer output (bf16 / fp16)")
        heat = torch.empty(B, 4, S, S, dtype=torch.float32, device=act.device)
        part = torch.empty(B, 4, native.lib().occlusion_parts(S), dtype=torch.float32, device=act.device)
        native.lib().activation_heat(act.contiguous(), idx.contiguous(), heat, part)
        return heat, part
    live = (idx >= 0) & (idx < C)
    fi = idx.long().clamp(0, C - 1)
    a = torch.gather(act.float().permute(0, 3, 1, 2), 1, fi.view(B, 4, 1, 1).expand(B, 4, H, W))  # [B, 4, H, W]
    ya, yb, fy = _taps(S, H, r)
    xa, xb, fx = _taps(S, W, r)
    fy, fx = fy.view(S, 1), fx.view(1, S)
    ra, rb = a[:, :, ya], a[:, :, yb]  # [B, 4, S, W]
    top = (1 - fx) * ra[..., xa] + fx * ra[..., xb]
    bot = (1 - fx) * rb[..., xa] + fx * rb[..., xb]
    heat = ((1 - fy) * top + fy * bot) * live.view(B, 4, 1, 1)
    return heat.contiguous(), heat.abs().amax(dim=(2, 3)).unsqueeze(-1)
