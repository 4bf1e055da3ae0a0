"""The independent oracle of the Laplacian-pyramid tests: naive float64 numpy loops written straight from the
definitions (k = [1, 4, 6, 4, 1] / 16, out(L) = ceil(L / 2), pad(L) = 1 for even L and 2 for odd L, zeros outside).
It shares no code with deconv_api_amd.ops.lapnorm (neither the kernels nor the torch reference). A plain module,
not a conftest. Arrays are [N, H, W, C] float64; the loops run over positions and taps, vectorised only over N, C."""
import functools

import numpy as np
import torch

K = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0

# (N, H, W): even and odd sides, sides smaller than the filter at the coarse levels, non-square maps, several
# images; the last crosses two 16 x 32 kernel tiles plus one pixel on both sides (and one tile at level 1)
SHAPES = [(1, 5, 5), (2, 6, 9), (2, 16, 16), (3, 17, 33), (2, 40, 37), (1, 64, 130), (1, 35, 67)]


def out(L):
    return -(-L // 2)


def pad(L):
    return 1 if L % 2 == 0 else 2


def down(x, replicate=False):
    N, H, W, C = x.shape
    lo = np.zeros((N, out(H), out(W), C))
    for i in range(out(H)):
        for j in range(out(W)):
            acc = np.zeros((N, C))
            for a in range(5):
                y = 2 * i + a - pad(H)
                for b in range(5):
                    xx = 2 * j + b - pad(W)
                    if replicate:
                        acc += K[a] * K[b] * x[:, min(max(y, 0), H - 1), min(max(xx, 0), W - 1)]
                    elif 0 <= y < H and 0 <= xx < W:
                        acc += K[a] * K[b] * x[:, y, xx]
            lo[:, i, j] = acc
    return lo


def up(lo, hw):
    H, W = hw
    N, Hl, Wl, C = lo.shape
    assert (Hl, Wl) == (out(H), out(W))
    res = np.zeros((N, H, W, C))
    for i in range(Hl):
        for a in range(5):
            y = 2 * i + a - pad(H)
            if not 0 <= y < H:
                continue
            for j in range(Wl):
                for b in range(5):
                    xx = 2 * j + b - pad(W)
                    if 0 <= xx < W:
                        res[:, y, xx] += 4.0 * K[a] * K[b] * lo[:, i, j]
    return res


def split(x, n):
    levels = []
    for _ in range(n):
        lo = down(x)
        levels.append(x - up(lo, x.shape[1:3]))
        x = lo
    levels.append(x)
    return levels[::-1]


def merge(levels, s):
    """s: [N, len(levels)]"""
    img = s[:, 0, None, None, None] * levels[0]
    for i in range(1, len(levels)):
        img = up(img, levels[i].shape[1:3]) + s[:, i, None, None, None] * levels[i]
    return img


def scales_of(levels, eps=1e-10):
    return np.stack([1.0 / np.maximum(np.sqrt((lv ** 2).mean(axis=(1, 2, 3))), eps) for lv in levels], axis=1)


def lap_normalize(g, n, eps=1e-10):
    levels = split(g, n)
    return merge(levels, scales_of(levels, eps))


def unit_bits(a):
    """The smallest q with a * 2^q integral (a: float64 values that are dyadic rationals)."""
    for q in range(0, 64):
        if np.all(np.floor(a * 2.0 ** q) == a * 2.0 ** q):
            return q
    raise AssertionError("not dyadic within 2^-63")


def fp32_exact(a):
    return bool(np.all(a.astype(np.float32).astype(np.float64) == a))


@functools.lru_cache(maxsize=None)
def int_case(N, H, W):
    """Seeded integers in [-2, 2], [N, H, W, 8]: channels 0..2 are the map, 3..7 must be ignored by the kernels."""
    g = torch.Generator().manual_seed(10000 * N + 100 * H + W)
    return torch.randint(-2, 3, (N, H, W, 8), generator=g).double().numpy()


@functools.lru_cache(maxsize=None)
def int_levels(N, H, W, n):
    return tuple(split(int_case(N, H, W)[..., :3], n))


@functools.lru_cache(maxsize=None)
def rand_case(N, H, W, dt, zero_image=False):
    """Seeded normal values rounded to the 16-bit dtype ``dt`` -> (torch [N, H, W, 8] of dt, float64 [N, H, W, 3]);
    ``zero_image``: the last image is all zero."""
    g = torch.Generator().manual_seed(20000 * N + 100 * H + W)
    x = (torch.randn(N, H, W, 8, generator=g) * 0.75).to(dt)
    if zero_image:
        x[-1] = 0
    return x, x[..., :3].double().numpy()
