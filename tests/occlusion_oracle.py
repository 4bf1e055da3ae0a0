"""The independent oracle of the occlusion tests: plain float64 numpy loops written straight from the definition
(grid g = ceil((S - p) / s) + 1, o_i = min(i s, S - p); variant 1 + i g + j zeroed on its patch; heat = mean drop over
the covering patches; overlay = 0.6 |heat| / max |heat| of red / blue over the image plus the mean colour). It calls
nothing from deconv_api_amd.ops. A plain module, not a conftest."""
import functools

import numpy as np
import torch

MEAN = (103.939, 116.779, 123.68)
# (S, p, s): the default; count 1 everywhere; counts 1, 2 and 4; a clamped last position with count 3; P = 4
GRID_CASES = [(224, 32, 16), (24, 8, 8), (24, 8, 4), (27, 8, 6), (224, 112, 112)]
# the kernels' small geometries: count 1, overlapping patches, the clamped last position, an odd side
SMALL = [(24, 8, 8), (24, 8, 4), (27, 8, 6), (25, 12, 5)]
POW2 = [(24, 8, 8), (24, 8, 4)]  # every covering count is a power of two: heat of integer scores is exact


def grid(S, p, s):
    """Patch origins per axis, or ValueError."""
    if not (8 <= p and 2 * p <= S and 4 <= s <= p):
        raise ValueError("outside the definition")
    g = -((S - p) // -s) + 1
    if g * g > 255:
        raise ValueError("more than 255 patches")
    return [min(i * s, S - p) for i in range(g)]


def counts(S, p, s):
    o = grid(S, p, s)
    return np.array([sum(1 for a in o if a <= y < a + p) for y in range(S)])


def variants(x0, p, s):
    """x0 [S, S, 8] -> [P + 1, S, S, 8] (same dtype)."""
    S = x0.shape[0]
    o = grid(S, p, s)
    out = [x0.copy()]
    for oy in o:
        for ox in o:
            v = x0.copy()
            for y in range(oy, oy + p):
                for x in range(ox, ox + p):
                    v[y, x, :] = 0
            out.append(v)
    return np.stack(out)


def heat(scores, idx, S, p, s):
    """scores [P + 1, C], idx [4] -> float64 [4, S, S]."""
    o = grid(S, p, s)
    g = len(o)
    scores = np.asarray(scores, dtype=np.float64)
    h = np.zeros((4, S, S))
    for k in range(4):
        f = int(idx[k])
        if f < 0:
            continue
        cover = [[i for i in range(g) if o[i] <= y < o[i] + p] for y in range(S)]
        for y in range(S):
            iy = cover[y]
            for x in range(S):
                jx = cover[x]
                acc = 0.0
                for i in iy:
                    for j in jx:
                        acc += scores[0, f] - scores[1 + i * g + j, f]
                h[k, y, x] = acc / (len(iy) * len(jx))
    return h


def overlay(h, idx, x0):
    """h [4, S, S] float64, idx [4], x0 [S, S, 8] (any float dtype, values used as they are) -> u8 [2 S, 2 S, 3]."""
    S = h.shape[1]
    x0 = np.asarray(x0, dtype=np.float64)
    out = np.zeros((2 * S, 2 * S, 3), np.uint8)
    for k in range(4):
        if int(idx[k]) < 0:
            continue
        m = np.abs(h[k]).max()
        for y in range(S):
            for x in range(S):
                t = h[k, y, x] / m if m > 0 else 0.0
                a = 0.6 * abs(t)
                for c in range(3):
                    tint = 255.0 if (c == 0 and t >= 0) or (c == 2 and t < 0) else 0.0
                    bg = min(max(x0[y, x, c] + MEAN[c], 0.0), 255.0)
                    out[(k // 2) * S + y, (k % 2) * S + x, c] = int(np.floor((1 - a) * bg + a * tint + 0.5))
    return out


# ---- seeded cases shared by the CPU and GPU tests (computed once, never modified)
@functools.lru_cache(maxsize=None)
def image_case(B, S, dt=torch.bfloat16):
    """Seeded network inputs [B, S, S, 8] of the 16-bit dtype ``dt``: RGB minus the mean in channels 0..2 and NON-zero
    values in channels 3..7 (so "copy all 8 outside, zero all 8 inside" is what a variant test sees)."""
    g = torch.Generator().manual_seed(1000 * B + S)
    x = torch.randint(0, 256, (B, S, S, 8), generator=g).float()
    x[..., :3] -= torch.tensor(MEAN)
    x[..., 3:] = x[..., 3:] / 4 + 1  # 1 .. 64.75: never zero
    return x.to(dt)


@functools.lru_cache(maxsize=None)
def score_case(B, S, p, s, C):
    """Integer scores in [-8, 8] fp32 [B, P + 1, C] and idx int32 [B, 4]: distinct filters, the last image's second
    filter -1."""
    P = len(grid(S, p, s)) ** 2
    g = torch.Generator().manual_seed(S * 10000 + p * 100 + s + C)
    sc = torch.randint(-8, 9, (B, P + 1, C), generator=g).float()
    idx = torch.stack([torch.randperm(C, generator=g)[:4] for _ in range(B)]).to(torch.int32)
    idx[-1, 1] = -1
    return sc, idx


@functools.lru_cache(maxsize=None)
def heat_case(B, S, p, s, C):
    sc, idx = score_case(B, S, p, s, C)
    return np.stack([heat(sc[b].numpy(), idx[b].numpy(), S, p, s) for b in range(B)])


def ulp_diff(got, ref64):
    """Distance in fp32 units in the last place between fp32 ``got`` and the float64 reference rounded to fp32."""
    r = ref64.astype(np.float32)
    g = np.asarray(got, dtype=np.float32)
    return np.abs(g.astype(np.float64) - r.astype(np.float64)) / np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)


def overlay_case(S, p, s, dt=torch.bfloat16):
    """Overlay inputs (heat fp32 [2, 4, S, S], idx, x0): four tiles with different heats per image; tile 1 of the
    last image has idx -1, tile 2 of image 0 is all zero."""
    _, idx = score_case(2, S, p, s, 64)
    h = torch.from_numpy(heat_case(2, S, p, s, 64)).float()
    h[0, 2] = 0
    return h, idx, image_case(2, S, dt)


def overlay_within(got, h, idx, x0):
    """Every byte of ``got`` (u8 numpy [B, 2 S, 2 S, 3]) within 1 level of the float64 oracle and at most 0.5 % of the
    bytes different."""
    for b in range(got.shape[0]):
        ref = overlay(h[b].double().numpy(), idx[b].numpy(), x0[b].float().numpy())
        d = np.abs(got[b].astype(int) - ref.astype(int))
        assert d.max() <= 1, (b, int(d.max()))
        assert (d != 0).mean() <= 0.005, (b, float((d != 0).mean()))


@functools.lru_cache(maxsize=None)
def default_variants(dt, seed=7):
    """(x0 [1, 224, 224, 8] of dtype dt, its 170 default-grid variants by the oracle, as a dt tensor)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(1, 224, 224, 8)
    x[..., :3] = torch.randint(0, 256, (1, 224, 224, 3), generator=g).float() - torch.tensor(MEAN)
    x = x.to(dt)
    return x, torch.from_numpy(variants(x[0].float().numpy(), 32, 16)).to(dt)
