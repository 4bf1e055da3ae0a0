"""The independent oracle of the activation-map tests: plain float64 loops written straight from the definition
(bilinear upsampling with half-pixel centres by r = S / H in integer coordinates: t = 2 y + 1 - r, y0 = floor(t / 2r),
fy = (t - 2r y0) / 2r, rows clamp(y0) and clamp(y0 + 1), the same for x). It calls nothing from deconv_api_amd.ops.
A plain module, not a conftest.

``heat_map`` is the naive loop over every output pixel. ``heat_map_rows`` is the same arithmetic in the same order
with the loop over x written as a numpy float64 expression, for the 224 x 224 cases; test_actmap.py asserts the two
equal bit for bit. ``overlay_rows`` is likewise ``occlusion_oracle.overlay`` with the pixel loops as numpy float64
expressions, asserted equal to it there."""
import functools

import numpy as np
import torch

import occlusion_oracle as O

# (S, H): r = 1; r = 2 with S^2 = 2.25 blocks; r = 8; r = 8 with 6.25 blocks; r = 32 where every tap clamps on one side
# somewhere; r = 16 from a single value
CASES = [(32, 32), (24, 12), (24, 3), (40, 5), (64, 2), (16, 1)]
EPS = 8 * 2.0 ** -24  # at most five fp32 roundings of values bounded by max |a|


def ratio(S, H):
    r = S // H
    if r * H != S or r < 1 or r > 64 or r & (r - 1):
        raise ValueError("outside the definition")
    return r


def taps(S, H):
    """Per output coordinate y: (ya, yb, fy) with fy a Python float (exact: a multiple of 1 / 2r)."""
    r = ratio(S, H)
    out = []
    for y in range(S):
        t = 2 * y + 1 - r
        y0 = t // (2 * r)  # Python's floor division
        out.append((min(max(y0, 0), H - 1), min(max(y0 + 1, 0), H - 1), (t - 2 * r * y0) / (2 * r)))
    return out


def heat_map(a, S):
    """a [H, H] -> float64 [S, S], one pixel at a time."""
    a = np.asarray(a, dtype=np.float64)
    tp = taps(S, a.shape[0])
    h = np.zeros((S, S))
    for y, (ya, yb, fy) in enumerate(tp):
        for x, (xa, xb, fx) in enumerate(tp):
            h[y, x] = (1 - fy) * ((1 - fx) * a[ya, xa] + fx * a[ya, xb]) + fy * ((1 - fx) * a[yb, xa] + fx * a[yb, xb])
    return h


def heat_map_rows(a, S):
    """``heat_map`` with the loop over x as a numpy expression (same operations, same order)."""
    a = np.asarray(a, dtype=np.float64)
    tp = taps(S, a.shape[0])
    xa, xb = np.array([t[0] for t in tp]), np.array([t[1] for t in tp])
    fx = np.array([t[2] for t in tp])
    h = np.zeros((S, S))
    for y, (ya, yb, fy) in enumerate(tp):
        h[y] = (1 - fy) * ((1 - fx) * a[ya, xa] + fx * a[ya, xb]) + fy * ((1 - fx) * a[yb, xa] + fx * a[yb, xb])
    return h


def heat(act, idx, S, fn=heat_map):
    """act [B, H, H, C] (torch, any float dtype; values used as they are), idx [B, 4] -> float64 [B, 4, S, S]; a filter
    outside 0 .. C - 1 gives a zero map."""
    B, H, _, C = act.shape
    out = np.zeros((B, 4, S, S))
    for b in range(B):
        for k in range(4):
            f = int(idx[b, k])
            if 0 <= f < C:
                out[b, k] = fn(act[b, :, :, f].double().numpy(), S)
    return out


def overlay_rows(h, idx, x0):
    """``occlusion_oracle.overlay`` (h [4, S, S] float64, idx [4], x0 [S, S, 8] -> u8 [2 S, 2 S, 3]) with the pixel
    loops as numpy float64 expressions."""
    S = h.shape[1]
    x0 = np.asarray(x0, dtype=np.float64)
    out = np.zeros((2 * S, 2 * S, 3), np.uint8)
    for k in range(4):
        if int(idx[k]) < 0:
            continue
        m = np.abs(h[k]).max()
        t = h[k] / m if m > 0 else np.zeros_like(h[k])
        a = 0.6 * np.abs(t)
        for c in range(3):
            tint = np.where((t >= 0) if c == 0 else (t < 0) if c == 2 else np.zeros_like(t, dtype=bool), 255.0, 0.0)
            bg = np.minimum(np.maximum(x0[:, :, c] + O.MEAN[c], 0.0), 255.0)
            out[(k // 2) * S:(k // 2 + 1) * S, (k % 2) * S:(k % 2 + 1) * S, c] = np.floor((1 - a) * bg + a * tint + 0.5)
    return out


def overlay_within(got, h64, idx, x0, fn=O.overlay):
    """Every byte of ``got`` (u8 numpy [B, 2 S, 2 S, 3]) within 1 level of the float64 oracle on the float64 heat
    ``h64`` [B, 4, S, S] and at most 0.5 % of the bytes different; returns the largest fraction of differing bytes."""
    worst = 0.0
    for b in range(got.shape[0]):
        ref = fn(h64[b], idx[b].numpy(), x0[b].float().numpy())
        d = np.abs(got[b].astype(int) - ref.astype(int))
        assert d.max() <= 1, (b, int(d.max()))
        assert (d != 0).mean() <= 0.005, (b, float((d != 0).mean()))
        worst = max(worst, float((d != 0).mean()))
    return worst


def within_bound(got, ref64, act, idx):
    """|got - ref| <= 8 x 2^-24 max |a| per map (a: the selected channel); returns the largest error in units of the
    bound."""
    got = np.asarray(got, dtype=np.float64)
    B, _, _, C = act.shape
    worst = 0.0
    for b in range(B):
        for k in range(4):
            f = int(idx[b, k])
            err = float(np.abs(got[b, k] - ref64[b, k]).max())
            if not 0 <= f < C:
                assert err == 0.0, (b, k, err)
                continue
            amax = float(act[b, :, :, f].double().abs().max())
            assert err <= EPS * amax, (b, k, err, EPS * amax)
            if amax > 0:
                worst = max(worst, err / (EPS * amax))
    return worst


# ---- seeded cases shared by the CPU and GPU tests (computed once, never modified)
def filters(C, B=2):
    """idx int32 [B, 4]: channels 0, 7, 8 (mod C) and C - 1; the last image's second filter is -1 and its third is C."""
    idx = torch.tensor([[0, 7, 8 % C, C - 1]] * B, dtype=torch.int32)
    idx[-1] = torch.tensor([C - 1, -1, C, 7], dtype=torch.int32)
    return idx


@functools.lru_cache(maxsize=None)
def int_case(S, H, C, dt=torch.bfloat16, B=2):
    """Integer maps in [-64, 64] as the 16-bit dtype ``dt`` (exact in both) [B, H, H, C], and idx."""
    g = torch.Generator().manual_seed(S * 100000 + H * 1000 + C)
    return torch.randint(-64, 65, (B, H, H, C), generator=g).float().to(dt), filters(C, B)


@functools.lru_cache(maxsize=None)
def rand_case(S, H, C, dt=torch.bfloat16, B=2):
    """Random 16-bit-representable maps (normal, scale 3) [B, H, H, C] of dtype ``dt``, and idx."""
    g = torch.Generator().manual_seed(S * 100000 + H * 1000 + C + 1)
    return (3 * torch.randn(B, H, H, C, generator=g)).to(dt), filters(C, B)


@functools.lru_cache(maxsize=None)
def heat_case(kind, S, H, C, dt=torch.bfloat16, B=2):
    """float64 [B, 4, S, S]: the oracle's heat of ``int_case`` / ``rand_case``."""
    act, idx = (int_case if kind == "int" else rand_case)(S, H, C, dt, B)
    return heat(act, idx, S, heat_map if S <= 64 else heat_map_rows)
