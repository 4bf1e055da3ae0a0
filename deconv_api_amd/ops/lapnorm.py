"""Laplacian-pyramid gradient normalisation ("lapnorm", the TensorFlow DeepDream tutorial's second control):
a gradient is split into frequency bands with a 5x5 binomial pyramid, every band is scaled to unit RMS per
image, and the bands are put back together, so low frequencies get as much of a DeepDream step as high ones.

All fp32, per image and channel, NHWC with 3 channels. ``k = [1, 4, 6, 4, 1] / 16``, filter ``k (x) k``; a side L
has the coarse side ``out(L) = ceil(L / 2)`` and the leading zero pad 1 (L even) or 2 (L odd): TensorFlow's SAME
for a 5-tap stride-2 filter. ``down`` is that strided convolution, ``up(lo, (H, W))`` 4 x its exact adjoint,
``split`` keeps ``hi = x - up(down(x))`` per level, ``merge`` is ``img = up(img) + s * hi`` from the coarsest level.

Device tensors run csrc/dream_lap.hip (one split and one merge launch per level); CPU tensors the torch
reference below (F.pad + F.conv2d(stride=2), F.conv_transpose2d + crop), which is also what the torch tail of
the DeepDream step uses."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import native

MAX_LEVELS = 5
_K = (1.0, 4.0, 6.0, 4.0, 1.0)


def out_side(L: int) -> int:
    return (L + 1) // 2


def _pad(L: int) -> int:
    return 2 if L % 2 else 1


def level_shapes(H: int, W: int, n: int) -> List[Tuple[int, int]]:
    """Sides of level 0 .. n (level 0 is the map itself)."""
    shapes = [(H, W)]
    for _ in range(n):
        shapes.append((out_side(shapes[-1][0]), out_side(shapes[-1][1])))
    return shapes


def parts_of(H: int, W: int) -> int:
    """Partials per image of an H x W level: one per kernel tile (csrc/kernels.h LAP_TILE_H x LAP_TILE_W)."""
    return native.lib().lap_parts(H, W)


def _check_levels(n: int) -> int:
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_LEVELS:
        raise ValueError(f"lap levels must be an integer in 1..{MAX_LEVELS}, got {n!r}")
    return int(n)


# --------------------------------------------------------------------------- torch reference (NHWC in and out)
def _kernel(x: torch.Tensor) -> torch.Tensor:
    k = torch.tensor(_K, dtype=x.dtype, device=x.device) / 16.0
    return (k[:, None] * k[None, :]).expand(3, 1, 5, 5).contiguous()


def down_ref(x: torch.Tensor) -> torch.Tensor:
    H, W = x.shape[1:3]
    ph, pw = _pad(H), _pad(W)
    # (right / bottom pads: whatever the last window needs, at most 2)
    xp = F.pad(x.permute(0, 3, 1, 2), (pw, 2 * out_side(W) + 3 - pw - W, ph, 2 * out_side(H) + 3 - ph - H))
    return F.conv2d(xp, _kernel(x), stride=2, groups=3).permute(0, 2, 3, 1).contiguous()


def up_ref(lo: torch.Tensor, hw: Tuple[int, int]) -> torch.Tensor:
    H, W = hw
    ph, pw = _pad(H), _pad(W)
    full = F.conv_transpose2d(lo.permute(0, 3, 1, 2), 4.0 * _kernel(lo), stride=2, groups=3)
    return full[:, :, ph:ph + H, pw:pw + W].permute(0, 2, 3, 1).contiguous()


def split_ref(x: torch.Tensor, n: int) -> List[torch.Tensor]:
    levels = []
    for _ in range(n):
        lo = down_ref(x)
        levels.append(x - up_ref(lo, x.shape[1:3]))
        x = lo
    levels.append(x)
    return levels[::-1]


def merge_ref(levels: Sequence[torch.Tensor], scales: torch.Tensor) -> torch.Tensor:
    img = scales[:, 0].view(-1, 1, 1, 1) * levels[0]
    for i in range(1, len(levels)):
        img = up_ref(img, levels[i].shape[1:3]) + scales[:, i].view(-1, 1, 1, 1) * levels[i]
    return img


def normalize_ref(g: torch.Tensor, n: int, eps: float = 1e-10) -> torch.Tensor:
    """lap_normalize of an fp32 [N, H, W, 3] tensor in plain torch (any device)."""
    levels = split_ref(g, n)
    scales = torch.stack([1.0 / lv.square().mean(dim=(1, 2, 3)).sqrt().clamp_min(eps) for lv in levels], dim=1)
    return merge_ref(levels, scales)


# --------------------------------------------------------------------------- device buffers
class LapBuffers:
    """The static buffers of one (N, H, W, n): level l = 0..n-1 has hi[l] [N, H_l, W_l, 3], lo[l] (= down of level l)
    [N, H_{l+1}, W_{l+1}, 3] and its partials hpart[l] [N, tiles]; lpart: the coarsest lo's partials; merged[l-1]:
    the merge's intermediate image of level l = 1..n-1. Nothing needs zeroing: the kernels write every element."""

    def __init__(self, N: int, H: int, W: int, n: int, device):
        n = _check_levels(n)
        shp = level_shapes(H, W, n)
        f = dict(dtype=torch.float32, device=device)
        self.n, self.shape = n, (N, H, W)
        self.hi = [torch.empty(N, *shp[l], 3, **f) for l in range(n)]
        self.lo = [torch.empty(N, *shp[l + 1], 3, **f) for l in range(n)]
        self.hpart = [torch.empty(N, parts_of(*shp[l]), **f) for l in range(n)]
        self.lpart = torch.empty(N, parts_of(*shp[n - 1]), **f)
        self.merged = [torch.empty(N, *shp[l], 3, **f) for l in range(1, n)]

    def levels(self) -> List[torch.Tensor]:
        return [self.lo[-1]] + self.hi[::-1]


def _src3(x: torch.Tensor) -> torch.Tensor:
    """The kernels' two input layouts: fp32 [N, H, W, 3] or 16-bit [N, H, W, 8] (channels 0..2 used)."""
    if x.dim() != 4 or not ((x.dtype == torch.float32 and x.shape[3] == 3) or
                            (x.dtype in (torch.bfloat16, torch.float16) and x.shape[3] == 8)):
        raise ValueError("expected fp32 [N, H, W, 3] or bf16 / fp16 [N, H, W, 8], got "
                         f"{x.dtype} {tuple(x.shape)}")
    return x.contiguous()


# --------------------------------------------------------------------------- op surface
def lap_split(x: torch.Tensor, n: int) -> List[torch.Tensor]:
    """``[lo_n, hi_{n-1}, ..., hi_0]`` (fp32 [N, h, w, 3] each) of x: fp32 [N, H, W, 3] or the 16-bit 8-channel
    gradient layout [N, H, W, 8]."""
    n = _check_levels(n)
    x = _src3(x)
    if not x.is_cuda:
        return split_ref(x[..., :3].float(), n)
    buf = LapBuffers(x.shape[0], x.shape[1], x.shape[2], n, x.device)
    native.lib().lap_split(x, buf.lo, buf.hi, buf.hpart, buf.lpart)
    return buf.levels()


def lap_merge(levels: Sequence[torch.Tensor], scales: torch.Tensor, out_dtype: Optional[torch.dtype] = None):
    """``merge(levels, scales)``: levels as ``lap_split`` returns them, scales fp32 [N, len(levels)] (column i
    scales levels[i]). fp32 [N, H, W, 3]; with ``out_dtype`` bf16 / fp16 the 8-channel layout [N, H, W, 8],
    channels 3..7 zero."""
    n = _check_levels(len(levels) - 1)
    N, H, W = levels[-1].shape[:3]
    shp = level_shapes(H, W, n)
    want = [(N, *shp[n], 3)] + [(N, *shp[l], 3) for l in range(n - 1, -1, -1)]
    if [tuple(lv.shape) for lv in levels] != want or any(lv.dtype != torch.float32 for lv in levels):
        raise ValueError(f"levels must be fp32 with shapes {want}")
    if tuple(scales.shape) != (N, n + 1):
        raise ValueError(f"scales must be [{N}, {n + 1}]")
    if out_dtype not in (None, torch.float32, torch.bfloat16, torch.float16):
        raise ValueError("out_dtype: None / float32, bfloat16 or float16")
    packed = out_dtype in (torch.bfloat16, torch.float16)
    if not levels[0].is_cuda:
        img = merge_ref(levels, scales.float())
        return F.pad(img, (0, 5)).to(out_dtype) if packed else img
    dev = levels[0].device
    out = torch.empty(N, H, W, 8 if packed else 3, dtype=out_dtype if packed else torch.float32, device=dev)
    merged = [torch.empty(N, *shp[l], 3, dtype=torch.float32, device=dev) for l in range(1, n)]
    hi = [lv.contiguous() for lv in levels[:0:-1]]
    native.lib().lap_merge(levels[0].contiguous(), hi, merged, out, scales.float().contiguous().to(dev))
    return out


def lap_normalize(g: torch.Tensor, n: int, eps: float = 1e-10, buffers: Optional[LapBuffers] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``merge(split(g, n), s)`` with ``s[i] = 1 / max(rms(level i), eps)`` per image. g: fp32 [N, H, W, 3] ->
    fp32, or the 16-bit 8-channel gradient layout [N, H, W, 8] -> the same layout (channels 3..7 zero).
    ``buffers`` / ``out`` (GPU): preallocated ``LapBuffers`` and result, so a captured graph replays them."""
    n = _check_levels(n)
    if not eps > 0:
        raise ValueError("eps must be positive")
    g = _src3(g)
    if not g.is_cuda:
        r = normalize_ref(g[..., :3].float(), n, eps)
        return r if g.shape[3] == 3 else F.pad(r, (0, 5)).to(g.dtype)
    if buffers is None:
        buffers = LapBuffers(g.shape[0], g.shape[1], g.shape[2], n, g.device)
    elif buffers.n != n or buffers.shape != tuple(g.shape[:3]):
        raise ValueError("buffers of another shape / level count")
    if out is None:
        out = torch.empty_like(g)
    native.lib().lap_normalize(g, buffers.lo, buffers.hi, buffers.hpart, buffers.lpart, buffers.merged, out, float(eps))
    return out
