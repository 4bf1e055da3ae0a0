"""Occlusion sensitivity (Zeiler & Fergus, "Visualizing and Understanding Convolutional Networks", section 4.2): a
grey p x p patch slides over the S x S network input with stride s, and the drop of a filter's score under each
patch is spread over the pixels that patch covers.

Geometry: ``8 <= p <= S / 2``, ``4 <= s <= p``; per axis ``g = ceil((S - p) / s) + 1`` positions ``o_i = min(i s,
S - p)`` (every patch inside the image, the image covered, only the last position clamped), ``P = g^2 <= 255``.
Variant 0 of an image is the image, variant ``1 + i g + j`` has all 8 channels zero (the dataset mean colour in
preprocessed space) on rows ``o_i .. o_i + p - 1``, columns ``o_j .. o_j + p - 1``.
``heat[k, y, x]`` = mean over the covering patches of ``score[0, f_k] - score[1 + i g + j, f_k]`` (fp32, summed i
ascending then j ascending); the overlay blends red (score dropped) / blue (score rose) over the de-meaned image
with weight ``0.6 |heat| / max |heat[k]|``.

Device tensors run csrc/occlusion.hip; CPU tensors the torch reference below (what the CPU service uses)."""
from __future__ import annotations

from typing import Tuple

import torch

from . import native
from .misc import CAFFE_MEAN

MAX_PATCHES = 255
ALPHA = 0.6


def occlusion_grid(S: int, p: int, s: int) -> Tuple[int, ...]:
    """The patch origins per axis ``(o_0, ..., o_{g-1})``; ValueError outside the definition."""
    for name, v in (("image side", S), ("patch", p), ("stride", s)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"occlusion {name} must be an integer, got {v!r}")
    if not 8 <= p <= S // 2:
        raise ValueError(f"occlusion patch must be in 8..{S // 2} (half the image side), got {p}")
    if not 4 <= s <= p:
        raise ValueError(f"occlusion stride must be in 4..patch ({p}), got {s}")
    g = -(-(S - p) // s) + 1
    if g * g > MAX_PATCHES:
        raise ValueError(f"patch {p} / stride {s} give {g * g} patches; at most {MAX_PATCHES}")
    return tuple(min(i * s, S - p) for i in range(g))


def _check_x0(x0: torch.Tensor) -> None:
    if x0.dim() != 4 or x0.shape[1] != x0.shape[2] or x0.shape[3] != 8:
        raise ValueError(f"expected the network-input layout [B, S, S, 8], got {tuple(x0.shape)}")


def _cover(o: Tuple[int, ...], S: int, p: int, device) -> torch.Tensor:
    """fp32 [S, g]: 1 where position i covers coordinate y."""
    y = torch.arange(S, device=device).view(S, 1)
    ot = torch.tensor(o, device=device).view(1, -1)
    return ((y >= ot) & (y < ot + p)).float()


def occlude_variants(x0: torch.Tensor, patch: int = 32, stride: int = 16) -> torch.Tensor:
    """x0 [B, S, S, 8] -> [B (P + 1), S, S, 8]: each image followed by its P occluded variants."""
    _check_x0(x0)
    B, S = x0.shape[:2]
    o = occlusion_grid(S, patch, stride)
    V = len(o) ** 2 + 1
    if x0.is_cuda:
        if x0.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("occlude_variants on the GPU takes the 16-bit network input (bf16 / fp16)")
        xv = torch.empty(B * V, S, S, 8, dtype=x0.dtype, device=x0.device)
        native.lib().occlude_variants(x0.contiguous(), xv, patch, stride)
        return xv
    xv = x0.unsqueeze(1).repeat(1, V, 1, 1, 1)
    v = 1
    for oy in o:
        for ox in o:
            xv[:, v, oy:oy + patch, ox:ox + patch] = 0
            v += 1
    return xv.reshape(B * V, S, S, 8)


def occlusion_heat(scores: torch.Tensor, idx: torch.Tensor, S: int, patch: int = 32, stride: int = 16):
    """scores fp32 [B, P + 1, C], idx int32 [B, 4] (-1: no filter) -> (heat fp32 [B, 4, S, S], part fp32 [B, 4, n]
    whose maximum over n is max |heat[b, k]|; n = kernel blocks on the GPU, 1 on the CPU)."""
    o = occlusion_grid(S, patch, stride)
    g = len(o)
    if scores.dim() != 3 or scores.shape[1] != g * g + 1 or scores.dtype != torch.float32:
        raise ValueError(f"scores must be fp32 [B, {g * g + 1}, C], got {scores.dtype} {tuple(scores.shape)}")
    B, _, C = scores.shape
    if tuple(idx.shape) != (B, 4):
        raise ValueError(f"idx must be [{B}, 4]")
    idx = idx.to(torch.int32)
    if scores.is_cuda:
        heat = torch.empty(B, 4, S, S, dtype=torch.float32, device=scores.device)
        part = torch.empty(B, 4, native.lib().occlusion_parts(S), dtype=torch.float32, device=scores.device)
        native.lib().occlusion_heat(scores.contiguous(), idx.contiguous(), heat, part, patch, stride)
        return heat, part
    live = (idx >= 0) & (idx < C)
    sel = torch.gather(scores, 2, idx.long().clamp(0, C - 1).view(B, 1, 4).expand(B, g * g + 1, 4))  # [B, P + 1, 4]
    d = (sel[:, :1] - sel[:, 1:]).permute(0, 2, 1).reshape(B, 4, g, g)
    cov = _cover(o, S, patch, scores.device)  # [S, g]
    heat = torch.zeros(B, 4, S, S)
    for i in range(g):  # the definition's order: i ascending, then j ascending, one accumulator
        for j in range(g):
            heat += d[:, :, i, j].view(B, 4, 1, 1) * (cov[:, i].view(S, 1) * cov[:, j].view(1, S))
    n = cov.sum(1)
    heat = heat / (n.view(S, 1) * n.view(1, S)) * live.view(B, 4, 1, 1)
    return heat, heat.abs().amax(dim=(2, 3)).unsqueeze(-1)


def occlusion_overlay(heat: torch.Tensor, part: torch.Tensor, idx: torch.Tensor, x0: torch.Tensor) -> torch.Tensor:
    """heat [B, 4, S, S], part [B, 4, n] (from ``occlusion_heat``), idx [B, 4], x0 [B, S, S, 8] -> u8 RGB mosaic
    [B, 2 S, 2 S, 3], tiles [[0, 1], [2, 3]]; a tile with idx -1 is black, a tile whose heat is all zero shows the
    plain image. The background is x0 + the mean colour, clamped to 0..255: taken from the network input, so in
    bf16 it can be up to half a level off the resized u8 image."""
    _check_x0(x0)
    B, S = x0.shape[:2]
    if tuple(heat.shape) != (B, 4, S, S) or part.dim() != 3 or tuple(part.shape[:2]) != (B, 4) or \
            tuple(idx.shape) != (B, 4):
        raise ValueError("heat [B, 4, S, S], part [B, 4, n] and idx [B, 4] must match x0 [B, S, S, 8]")
    idx = idx.to(torch.int32)
    if x0.is_cuda:
        out = torch.empty(B, 2 * S, 2 * S, 3, dtype=torch.uint8, device=x0.device)
        native.lib().occlusion_overlay(heat.float().contiguous(), part.float().contiguous(), idx.contiguous(),
                                       x0.contiguous(), out)
        return out
    heat = heat.float()
    m = part.float().amax(dim=2).view(B, 4, 1, 1)
    t = torch.where(m > 0, heat / m.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(heat))
    a = (ALPHA * t.abs()).unsqueeze(-1)  # [B, 4, S, S, 1]
    bg = (x0[..., :3].float() + torch.tensor(CAFFE_MEAN)).clamp(0, 255).unsqueeze(1)  # [B, 1, S, S, 3]
    tint = torch.zeros(B, 4, S, S, 3)
    tint[..., 0] = (t >= 0) * 255.0
    tint[..., 2] = (t < 0) * 255.0
    px = torch.floor((1 - a) * bg + a * tint + 0.5).to(torch.uint8) * (idx >= 0).view(B, 4, 1, 1, 1).to(torch.uint8)
    return px.view(B, 2, 2, S, S, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * S, 2 * S, 3).contiguous()
