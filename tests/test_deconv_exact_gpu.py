"""GPU: the deconvnet serving path's small kernels (csrc/misc.hip), the fused tail (conv_unpool_z in
csrc/conv_smalln.hip) and zsum3x3 against EXACT oracles.

As in test_conv_exact_gpu.py and test_dream_exact_gpu.py the operands are small integers, so every product
and partial sum is exact in fp32 under any summation order and the results are exact in bf16 and fp16: a
correct kernel reproduces the CPU reference bit for bit. One wrong border tap, swapped h / w, dropped tail
element or wrong tile quadrant shows, however small it is next to the tensor's norm.

Every case comes from a cached ``_*_case`` builder that draws the operands, computes a CPU reference in
fp32 / fp64 from the formula alone (``torch.nn.functional`` and plain indexing, never the ``ops.*`` GPU
wrappers) and asserts the method's conditions on the reference alone: representable in bf16 and fp16,
partial sums below 2^24, >= 25 % non-zero outputs where structure allows. ``test_conditions`` (no GPU)
builds every case of every table. Outputs are pre-filled with a sentinel. Where a launcher chooses between
two kernels the test asserts ``misc_route()``, so it cannot quietly become a test of the other kernel.

The deprocess kernels are fp32 chains that end in a truncation, so they have a banded oracle instead
(``_deprocess_case``); resize / preprocess are integer pipelines with one rounding (``from_f``) that the
NumPy model repeats; softmax keeps the project's fp64 comparison at rtol 1e-5, atol 1e-7.
"""
import functools
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from deconv_api_amd import ops
from exact_helpers import BF, DEV, HF, _dev, _gen, _ints, _same, _weights

gpu = pytest.mark.gpu
dtypes = pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
SENTINEL = 7.0
SENT_U8 = 0xA5


def _case(**kw):
    return types.SimpleNamespace(**kw)


def _representable(ref, what="reference"):
    for dt in (BF, HF):
        assert torch.equal(ref.to(dt).double(), ref.double()), f"{what} not representable in {dt}"


def _conditions(ref, bound, where=None, dense=True):
    """Representable in both 16-bit types, partial sums (bounded by ``bound``) exact in fp32, and (``dense``)
    at least a quarter of the outputs (of those at ``where``) non-zero."""
    _representable(ref)
    assert float(bound) < 2 ** 24, "partial sums not exact in fp32"
    if dense:
        live = ref if where is None else ref[where]
        assert live.numel() > 0 and float((live != 0).double().mean()) >= 0.25, "too few non-zero outputs"


def _misc_route():
    return ops.native.lib().misc_route()


def _bits(t):
    """16-bit patterns of a bf16 / fp16 tensor (on the CPU)."""
    return t.cpu().contiguous().view(torch.int16)


def _unpool(p, code, div=1):
    """out[n, 2ph+dy, 2pw+dx, c] = p[n, ph, pw, c] where code[n // div, ph, pw, c] == 2dy + dx, else 0."""
    N, PH, PW, C = p.shape
    cd = code.repeat_interleave(div, dim=0).long()
    out = torch.zeros(N, 2 * PH, 2 * PW, C, dtype=p.dtype)
    for dy in range(2):
        for dx in range(2):
            out[:, dy::2, dx::2] = torch.where(cd == 2 * dy + dx, p, torch.zeros_like(p))
    return out


# ----------------------------------------------------------------------------------------
# 2. seed_deconv3x3: the small-map kernel and the grid-stride kernel, each reached by shape
# ----------------------------------------------------------------------------------------

SEED_F = 4
SEED_SMALL = [(3, H, W, Cin) for H, W in [(1, 1), (1, 7), (5, 3), (3, 5), (14, 14), (64, 64)] for Cin in (8, 24, 64, 512)]
# grid-stride: a map of more than 4096 px; Cin / 8 > 256; and more 16-B chunks than the grid's 4096 * 256
# threads, so that the stride loop takes a second trip (17 MB of output)
SEED_GRID = [(3, 65, 64, 8), (3, 5, 7, 2056), (4, 65, 65, 512)]
assert 4 * 65 * 65 * (512 // 8) > 4096 * 256


def _seed_ref(S, f, wt):
    """out[b, h, w, ci] = relu(sum_{kh, kw} S[b, h+kh-1, w+kw-1] * wt[min(f_b, F-1), kh, kw, ci]), zero for f_b < 0."""
    B, H, W = S.shape
    out = torch.zeros(B, H, W, wt.shape[3], dtype=torch.float64)
    for b, fb in enumerate(f):
        if fb < 0:
            continue
        w = wt[min(fb, wt.shape[0] - 1)].double().permute(2, 0, 1).unsqueeze(1)  # [Cin, 1, 3, 3]
        y = F.conv2d(S[b].double().view(1, 1, H, W), w, padding=1)[0]
        out[b] = y.permute(1, 2, 0).clamp_min(0)
    return out


@functools.lru_cache(maxsize=None)
def _seed_case(B, H, W, Cin):
    g = _gen(31 * H + 7 * W + Cin + B)
    S = _ints(g, (B, H, W), -3, 3) * (torch.rand(B, H, W, generator=g) < 0.6)
    S[:, 0, 0] = torch.tensor([3.0, -2.0, 1.0, 2.0])[:B]  # a one-pixel map is not all zero
    wt = _ints(g, (SEED_F, 3, 3, Cin), -2, 2)
    # two index vectors over the same maps: {0, F-1, -1} and {F, 4096, -5} (clamped to F-1; negative: zero)
    fa = [0, SEED_F - 1, -1, 1][:B]
    fb = [SEED_F, 4096, -5, 2][:B]
    ra, rb = _seed_ref(S, fa, wt), _seed_ref(S, fb, wt)
    if B * H * W >= 100:  # about half of S is zero
        assert float(S.abs().max()) == 3 and 0.35 <= float((S == 0).double().mean()) <= 0.65
    for f, r in ((fa, ra), (fb, rb)):
        live = torch.tensor([v >= 0 for v in f])
        # (a map of a few pixels has a few taps per output: it need only be not all zero)
        _conditions(r, 9 * 3 * 2, where=live, dense=H * W >= 8)
        assert bool(r[live].any()) and not bool(r[~live].any())
    assert torch.equal(ra[1], rb[1])  # f = 4096 reads filter F-1
    return _case(S=S, wt=wt, fa=fa, fb=fb, ra=ra, rb=rb)


def _seed_run(native_lib, c, f, dt):
    B, H, W = c.S.shape
    out = torch.full((B, H, W, c.wt.shape[3]), SENTINEL, dtype=dt, device=DEV)
    native_lib.seed_deconv3x3(c.S.to(DEV), torch.tensor(f, dtype=torch.int32, device=DEV), _dev(c.wt, dt), out)
    return out


def _seed_check(native_lib, shape, dt, route):
    c = _seed_case(*shape)
    ga = _seed_run(native_lib, c, c.fa, dt)
    assert _misc_route() == route
    gb = _seed_run(native_lib, c, c.fb, dt)
    assert _misc_route() == route
    _same(ga, c.ra)
    _same(gb, c.rb)
    assert torch.equal(_bits(ga[1]), _bits(gb[1]))  # f >= F equals the F-1 map bit for bit
    assert not bool(_bits(ga[2]).any()) and not bool(_bits(gb[2]).any())  # f < 0: exactly (+)zero


@gpu
@dtypes
@pytest.mark.parametrize("B,H,W,Cin", SEED_SMALL)
def test_exact_seed_deconv_smallmap(native_lib, B, H, W, Cin, dt):
    """seed_deconv3x3_smallmap_kernel: non-square maps, one-pixel rows, 1 / 3 / 8 / 64 chunks per pixel
    (Cin = 24: 256 % cpp != 0, idle lanes), 4096 px (the largest map it takes)."""
    _seed_check(native_lib, (B, H, W, Cin), dt, "seed_deconv3x3 smallmap")


@gpu
@dtypes
@pytest.mark.parametrize("B,H,W,Cin", SEED_GRID)
def test_exact_seed_deconv_grid(native_lib, B, H, W, Cin, dt):
    """seed_deconv3x3_kernel (grid-stride), reached by shape; the last case wraps the stride loop."""
    _seed_check(native_lib, (B, H, W, Cin), dt, "seed_deconv3x3 grid")


# ----------------------------------------------------------------------------------------
# 3. seed_map
# ----------------------------------------------------------------------------------------

SEEDMAP_SHAPES = [(3, 17, 19, 16, 4), (2, 1, 1, 8, 2), (2, 33, 32, 24, 3)]  # HW = 323 (> 256), 1, 1056 (> 1024)
SEEDMAP_MODES = [0, 1, 2]


def _seedmap_ref(x, idx, code, mode):
    """Chain (b, k): channel f = idx[b, k] of image b (zero for f < 0 or f >= C); mode 1 keeps only the
    positions equal to the map's max, mode 2 to the max of channel f over the whole batch; with ``code``
    the map is max-unpooled by the switches of (b, f) and clamped at 0."""
    B, H, W, C = x.shape
    K = idx.shape[1]
    up = 1 if code is None else 2
    S = torch.zeros(B * K, H * up, W * up, dtype=torch.float64)
    for b in range(B):
        for k in range(K):
            f = int(idx[b, k])
            if f < 0 or f >= C:
                continue
            m = x[b, :, :, f].double()
            if mode:
                top = m.max() if mode == 1 else x[:, :, :, f].double().max()
                m = torch.where(m == top, m, torch.zeros_like(m))
            if code is not None:
                m = _unpool(m.view(1, H, W, 1), code[b, :, :, f].view(1, H, W, 1))[0, :, :, 0].clamp_min(0)
            S[b * K + k] = m
    return S


@functools.lru_cache(maxsize=None)
def _seedmap_case(B, H, W, C, K):
    g = _gen(B * H * W + C + K)
    HW = H * W
    x = _ints(g, (B, H, W, C), -2, 4)
    x[..., 0] = _ints(g, (B, H, W), -4, -1)  # channel 0: all negative
    x[..., 1] = _ints(g, (B, H, W), 0, 4)    # channel 1: a unique max per image, carried by the last wave
    x[..., 2] = _ints(g, (B, H, W), 0, 3)    # channel 2: the max tied at several pixels
    flat = x.view(B, HW, C)
    # pixel p is read by thread p % 256: the last of the four waves carries the pixels with p % 256 >= 192
    top = max((q for q in range(HW) if q % 256 >= 192), default=0)
    for b in range(B):
        flat[b, max(top - b, 0), 1] = 7.0 + b  # the batch's max (mode 2) lies in the last image
    for b in range(B):
        m1 = flat[b, :, 1]
        assert int((m1 == m1.max()).sum()) == 1
        if HW > 256:
            assert int(m1.argmax()) % 256 >= 192
        if HW > 1024:
            assert int(m1.argmax()) >= 768  # and on the loop's fourth trip
        if HW > 16:
            assert int((flat[b, :, 2] == flat[b, :, 2].max()).sum()) >= 2
    assert int(flat[:, :, 1].reshape(-1).argmax()) // HW == B - 1
    assert float(x[..., 0].max()) < 0
    code = torch.randint(0, 4, (B, H, W, C), generator=g, dtype=torch.uint8)
    pool = [1, -1, C, C + 5, 0, 2]
    tables = {}
    for mode in SEEDMAP_MODES:
        tabs = []
        for off in (0, 2):
            if mode == 2:  # batch-global top-k: every image shares the filters
                rows = [[pool[(off + k) % 6] for k in range(K)]] * B
            else:
                rows = [[pool[(off + b * K + k) % 6] for k in range(K)] for b in range(B)]
            tabs.append(torch.tensor(rows, dtype=torch.int32))
        flat_idx = torch.cat([t.flatten() for t in tabs]).tolist()
        assert {-1, C, C + 5} <= set(flat_idx)
        tables[mode] = tabs
    refs = {}
    for mode in SEEDMAP_MODES:
        for ti, idx in enumerate(tables[mode]):
            for pooled in (False, True):
                r = _seedmap_ref(x, idx, code if pooled else None, mode)
                bad = ((idx.flatten() < 0) | (idx.flatten() >= C))
                assert not bool(r[bad].any())
                _conditions(r, 16, where=~bad, dense=(mode == 0 and not pooled and HW > 16 and bool((~bad).any())))
                refs[mode, ti, pooled] = r
    _representable(x, "activation")
    assert float((x != 0).double().mean()) >= 0.25
    return _case(x=x, code=code, tables=tables, refs=refs)


@gpu
@dtypes
@pytest.mark.parametrize("pooled", [False, True], ids=["plain", "code"])
@pytest.mark.parametrize("mode", SEEDMAP_MODES)
@pytest.mark.parametrize("B,H,W,C,K", SEEDMAP_SHAPES)
def test_exact_seed_map(native_lib, B, H, W, C, K, mode, pooled, dt):
    """seed_map_kernel: second and fifth trips of the 256-strided loops, a max carried by the last wave,
    tied maxima (all kept), an all-negative map (max mode with ``code`` clamps it to 0), the batch max in
    the last image (mode 2), and idx in {-1, C, C + 5} (zero maps)."""
    c = _seedmap_case(B, H, W, C, K)
    up = 2 if pooled else 1
    for ti, idx in enumerate(c.tables[mode]):
        S = torch.full((B * K, H * up, W * up), SENTINEL, dtype=torch.float32, device=DEV)
        native_lib.seed_map(_dev(c.x, dt), idx.to(DEV), c.code.to(DEV) if pooled else None, S, mode)
        _same(S, c.refs[mode, ti, pooled])


# ----------------------------------------------------------------------------------------
# 4. channel_sum
# ----------------------------------------------------------------------------------------

# (2, 85, 24) and (2, 86, 24) sit on either side of groups = 256 / (24 / 8) = 85 pixel groups
CSUM_SHAPES = [(1, 1, 8), (3, 3, 24), (2, 63, 64), (2, 196, 512), (2, 300, 2048), (2, 85, 24), (2, 86, 24)]


@functools.lru_cache(maxsize=None)
def _csum_case(N, HW, C):
    g = _gen(N + 3 * HW + C)
    x = _ints(g, (N, HW, 1, C), 0, 8)
    ref = x.double().sum(dim=(1, 2))
    assert float(ref.max()) <= 8 * HW < 2 ** 24 and torch.equal(ref.float().double(), ref)
    _representable(x, "input")
    assert float((ref != 0).double().mean()) >= 0.25
    return _case(x=x, ref=ref.float())


@gpu
@dtypes
@pytest.mark.parametrize("N,HW,C", CSUM_SHAPES)
def test_exact_channel_sum(native_lib, N, HW, C, dt):
    c = _csum_case(N, HW, C)
    out = torch.full((N, C), SENTINEL, dtype=torch.float32, device=DEV)
    native_lib.channel_sum(_dev(c.x, dt), out, N, HW, C)
    assert torch.equal(out.cpu(), c.ref)


@gpu
@dtypes
@pytest.mark.parametrize("C", [12, 2056])
def test_channel_sum_rejects(native_lib, C, dt):
    """C % 8 != 0 and C > 2048: the launcher returns -1, nothing runs, the output keeps the sentinel."""
    x = torch.ones(2, 3, 1, C, dtype=dt, device=DEV)
    out = torch.full((2, C), SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="code -1"):
        native_lib.channel_sum(x, out, 2, 3, C)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ----------------------------------------------------------------------------------------
# 5. topk_pos: the edges test_property.py does not draw
# ----------------------------------------------------------------------------------------

TOPK_CASES = [(7, 10), (70, 8), (130, 5), (1, 3), (63, 64), (200, 12)]  # (C, k): k > C, C < 64, lanes with 2 - 4 entries
INF, NAN = float("inf"), float("nan")


def _topk_ref(v, k):
    """Per row: the strictly positive entries (NaN is not), by value descending then index ascending."""
    N, C = v.shape
    idx = torch.full((N, k), -1, dtype=torch.int32)
    val = torch.zeros(N, k)
    for n in range(N):
        cand = sorted((-float(v[n, c]), c) for c in range(C) if float(v[n, c]) > 0)  # NaN > 0 is False
        for t, (nv, c) in enumerate(cand[:k]):
            idx[n, t], val[n, t] = c, -nv
    return idx, val


@functools.lru_cache(maxsize=None)
def _topk_case(C, k):
    g = _gen(C * 100 + k)
    levels = torch.tensor([-1.0, 0.0, 0.5, 1.0, 2.0])
    v = levels[torch.randint(0, 5, (5, C), generator=g)]

    def put(row, cols, value):
        for col in cols:
            if col < C:
                v[row, col] = value
    put(0, (3, 67, 10), INF)          # +inf three times, two of them in one lane (3 and 67)
    put(0, (0, 5, 69), NAN)
    put(1, (1, 65, 129), 3.0)         # the row's max tied at c, c + 64, c + 128: the same lane
    put(1, (2,), NAN)
    v[2] = NAN                        # nothing to select
    put(3, (C - 1, 0), INF)
    v[4] = -1.0                       # no positive entry
    put(4, (C // 2,), 0.5)
    idx, val = _topk_ref(v, k)
    assert bool((idx[2] == -1).all()) and int((idx[4] >= 0).sum()) == 1
    assert not bool(torch.isnan(val).any())
    if C >= 70:
        assert idx[0, :3].tolist() == [3, 10, 67] and idx[1, :2].tolist() == [1, 65]
    if k > C:
        assert bool((idx[:, C:] == -1).all())
    return _case(v=v, idx=idx, val=val)


@gpu
@pytest.mark.parametrize("C,k", TOPK_CASES)
def test_exact_topk_edges(native_lib, C, k):
    """topk_pos_kernel: +inf entries and ties between them, NaN never selected, k > C, C < 64, equal values
    at c and c + 64 (one lane's two candidates)."""
    c = _topk_case(C, k)
    idx = torch.full((5, k), 99, dtype=torch.int32, device=DEV)
    val = torch.full((5, k), SENTINEL, dtype=torch.float32, device=DEV)
    native_lib.topk_pos(c.v.to(DEV), idx, val, k)
    assert torch.equal(idx.cpu(), c.idx), (idx.cpu(), c.idx)
    assert torch.equal(val.cpu(), c.val)


# ----------------------------------------------------------------------------------------
# 6. zsum3x3, directly
# ----------------------------------------------------------------------------------------

ZSUM_SHAPES = [(1, 1, 1), (2, 16, 32), (2, 17, 33), (3, 5, 70), (2, 35, 31)]  # one px; one tile; +1 row / col; 3 tiles wide; 3 high
ZSUM_CASES = [(N, H, W, sd) for N, H, W in ZSUM_SHAPES for sd in sorted({0, 1, N})]  # 0: no statistics


def _zsum_ref(z27):
    """out[n, y, x, c] = relu(sum_{kh, kw} Z[n, y+kh-1, x+kw-1, (kh*3 + kw)*3 + c]), zero padding."""
    N, H, W, _ = z27.shape
    zp = F.pad(z27.double(), (0, 0, 1, 1, 1, 1))
    out = torch.zeros(N, H, W, 3, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            t = (kh * 3 + kw) * 3
            out += zp[:, kh:kh + H, kw:kw + W, t:t + 3]
    return out.clamp_min(0)


def _stats_ref(ref, div):
    r = ref.double().reshape(ref.shape[0] // div, -1)
    return torch.stack([r.sum(1), (r * r).sum(1)], 1)


@functools.lru_cache(maxsize=None)
def _zsum_case(N, H, W):
    g = _gen(5 * N + 3 * H + W)
    z27 = _ints(g, (N, H, W, 27), -8, 8)
    if H * W == 1:
        z27[0, 0, 0, 12:15] = torch.tensor([5.0, -3.0, 2.0])  # the centre tap is all this case has
    ref = _zsum_ref(z27)
    _representable(z27, "Z")
    assert float(ref.max()) <= 72 and torch.equal(ref.float().double(), ref)
    assert float((ref != 0).double().mean()) >= 0.25
    st = {sd: _stats_ref(ref, sd) for sd in {1, N}}
    assert all(float(s.max()) < 2 ** 53 for s in st.values())
    return _case(z27=z27, ref=ref.float(), stats=st)


@gpu
@pytest.mark.parametrize("N,H,W,sd", ZSUM_CASES)
def test_exact_zsum3x3(native_lib, N, H, W, sd):
    """zsum3x3_kernel on integer Z: every border tap and tile edge exact; channels 27..31 hold NaN, so a
    read of them poisons the output; the statistics equal the exact integer sums."""
    c = _zsum_case(N, H, W)
    z = torch.empty(N, H, W, 32, dtype=torch.int16)
    z[..., :27] = c.z27.to(BF).view(torch.int16)
    z[..., 27:] = 0x7FC0  # bf16 NaN
    out = torch.full((N, H, W, 3), SENTINEL, dtype=torch.float32, device=DEV)
    st = torch.full((N // sd, 2), SENTINEL, dtype=torch.float64, device=DEV) if sd else None
    native_lib.zsum3x3(z.view(BF).to(DEV), out, st, max(sd, 1))
    _same(out, c.ref)
    if sd:
        assert torch.equal(st.cpu(), c.stats[sd])


# ----------------------------------------------------------------------------------------
# 7. fused tail: conv_unpool_z + zsum3x3 through ops.deconv_tail
# ----------------------------------------------------------------------------------------

TAIL_TH, TAIL_TW = 8, 32  # csrc/conv_smalln.hip TH, TW: conv_unpool_z's output tile
# 2 x 2: all border; 18 x 34: one row / column past 2 x 1 tiles; 16 x 32: whole tiles; the last has 6 * 9 * 7
# = 378 tiles, more than the 256 CUs the persistent grid is capped at, so workgroups take a second tile
TAIL_CASES = [(2, 2, 2, 1), (4, 18, 34, 2), (3, 16, 32, 3), (6, 66, 194, 2)]


def _tail_tiles(N, H, W):
    return N * -(-H // TAIL_TH) * -(-W // TAIL_TW)


@functools.lru_cache(maxsize=None)
def _tail_case(N, H, W, div):
    g = _gen(N * H + W + div)
    p = _ints(g, (N, H // 2, W // 2, 64), -3, 3)
    code = torch.randint(0, 4, (N // div, H // 2, W // 2, 64), generator=g, dtype=torch.uint8)
    mid = _weights(g, 64, 64, bias=False, taps=96)
    last = _weights(g, 3, 64, bias=False, taps=96)
    u = _unpool(p, code, div).clamp_min(0).double()  # unpool, ReLU
    d = F.conv2d(u.permute(0, 3, 1, 2), mid.w_oihw.double(), padding=1).clamp_min(0)  # conv, ReLU: [N, 64, H, W]
    w2 = last.w_oihw.double().permute(2, 3, 0, 1).reshape(27, 64)  # row (kh*3 + kw)*3 + c
    z = torch.einsum("nchw,zc->nhwz", d, w2)
    for t, what in ((d, "d"), (z, "Z")):  # the kernel's two bf16 rounding points are exact
        assert float(t.abs().max()) <= 256 and torch.equal(t, t.round()), what
        _representable(t, what)
    ref = F.conv2d(d, last.w_oihw.double(), padding=1).clamp_min(0).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(ref, _zsum_ref(z))
    bound = F.conv2d(u.abs().permute(0, 3, 1, 2), mid.w_oihw.double().abs(), padding=1).max()
    bound2 = F.conv2d(d, last.w_oihw.double().abs(), padding=1).max()
    assert float(bound) < 2 ** 24 and float(bound2) < 2 ** 24 and torch.equal(ref.float().double(), ref)
    assert float((ref != 0).double().mean()) >= 0.25 and float((d != 0).double().mean()) >= 0.25
    return _case(p=p, code=code, mid=mid, last=last, ref=ref.float(), stats=_stats_ref(ref, div))


@gpu
@pytest.mark.parametrize("N,H,W,div", TAIL_CASES)
def test_exact_deconv_tail(native_lib, N, H, W, div):
    """ops.deconv_tail (conv3x3_unpool_c64_v2_kernel ZOUT + zsum3x3_kernel) on integer operands whose d and
    Z are bf16-exact: the result equals unpool -> ReLU -> conv -> ReLU -> conv -> ReLU bit for bit, the
    statistics exactly, and so do the DV_TAIL_V schedules 0, 1 and 2."""
    from gpu_helpers import cus

    c = _tail_case(N, H, W, div)
    if (N, H, W) == TAIL_CASES[-1][:3]:
        assert _tail_tiles(N, H, W) > cus()
    mid, last = c.mid.to_device(DEV), c.last.to_device(DEV)
    pd, cd = c.p.to(BF).to(DEV), c.code.to(DEV)
    st = torch.full((N // div, 2), SENTINEL, dtype=torch.float64, device=DEV)
    got = ops.deconv_tail(pd, cd, div, mid, last, stats=st, stats_div=div)
    assert got is not None and got.shape == (N, H, W, 3)
    _same(got, c.ref)
    assert torch.equal(st.cpu(), c.stats)
    for v in ("0", "1", "2"):
        os.environ["DV_TAIL_V"] = v
        try:
            alt = ops.deconv_tail(pd, cd, div, mid, last)
        finally:
            del os.environ["DV_TAIL_V"]
        _same(alt, c.ref)


# ----------------------------------------------------------------------------------------
# 8. deprocess: the one-block two-pass kernel (W % 4 != 0) and recon_stats + deprocess_apply (W % 4 == 0)
# ----------------------------------------------------------------------------------------

# The band. With m, s the fp64 mean and standard deviation, d = s + 1e-7, z = (x - m) / d and
# U = (0.1 z + 0.5) * 255, the kernels compute fl(x - fl(m)), / fl(d), * 0.1f, + 0.5f, clamp, * 255 in fp32
# (unit roundoff e = 2^-24; division correctly rounded: the build has no fast-math flag). Where the clamp
# does not already decide the byte, |z| <= 5 and, by the cases' condition, |m| <= 4 s <= 4 d. Errors in
# units of t = 0.1 z + 0.5 (|0.1 z| <= 0.5, 0 <= t <= 1), first order in e:
#   fl(m):            |m| e <= 4 d e                  -> 0.1 * 4 e          = 0.4 e
#   x - fl(m):        |x - m| e <= 5 d e              -> 0.1 * 5 e          = 0.5 e
#   fl(d):            s from fp64 sums of fp32 differences (<= e), rounded to fp32 (e), + 1e-7f (e), the
#                     two-pass kernel's squares of fp32-rounded differences (e): <= 4 e relative
#                                                     -> 0.5 * 4 e          = 2.0 e
#   the division:     relative e                      -> 0.5 e
#   0.1f (relative 0.25 e) and the product (e; none when contracted to an FMA)
#                                                     -> 0.5 * 1.25 e      <= 0.7 e
#   + 0.5f:           result <= 1                     -> 1.0 e
# 5.1 e in t, 255 * 5.1 e = 1301 e in U, and the last product's own rounding (255 e): 1556 e = 9.3e-5,
# rounded up to 1e-4 (the second-order terms are below 1e-10). The band is 4 x that.
DEPROCESS_BOUND = 1e-4
DEPROCESS_BAND = 4 * DEPROCESS_BOUND

DEPROCESS_TWO_PASS = [(2, 4, 5, 5), (2, 1, 5, 5), (3, 2, 7, 9), (2, 3, 6, 10), (1, 4, 33, 35)]
DEPROCESS_APPLY = [(2, 4, 4, 4), (3, 1, 6, 8), (2, 2, 5, 12), (2, 3, 9, 16)]


def _deprocess_route(W):
    return "deprocess two-pass" if W % 4 else "deprocess stats+apply"


@functools.lru_cache(maxsize=None)
def _deprocess_case(B, tiles, H, W, integer=False):
    """The fp64 oracle of one mosaic batch: per byte the interval [lo, hi] of floor(clip(U -+ band)); a
    byte is decided where lo == hi.

    Conditions: <= 1 % undecided bytes per image, |m| <= 4 s, >= 50 % interior values, and values that clip
    at each end. (No data set has 10 % of its values at each end: a value clips at |x - m| >= 5 s, and by
    Chebyshev's inequality at most 1 / 25 of any population lies that far from its mean. The cases put
    1 % - 1.4 % at each end, 12 interior standard deviations out, and assert >= 1 %.)"""
    g = _gen(1000 * B + 100 * tiles + 10 * H + W + (5 if integer else 0))
    total = tiles * H * W * 3
    nc = -(-total // 100)
    x = torch.randn(B, total, generator=g) * 6 + 12
    for b in range(B):
        perm = torch.randperm(total, generator=g)
        x[b, perm[:nc]] = 84.0 + torch.rand(nc, generator=g)
        x[b, perm[nc:2 * nc]] = -60.0 - torch.rand(nc, generator=g)
    if integer:
        x = x.round()
    recon = x.view(B * tiles, H, W, 3).contiguous()
    xd = x.double()
    m = xd.mean(1, keepdim=True)
    s = ((xd - m) ** 2).mean(1, keepdim=True).sqrt()
    U = (((xd - m) / (s + 1e-7)) * 0.1 + 0.5) * 255
    lo = (U - DEPROCESS_BAND).clamp(0, 255).floor().long()
    hi = (U + DEPROCESS_BAND).clamp(0, 255).floor().long()
    assert bool((hi - lo <= 1).all())
    assert float((lo != hi).double().mean(1).max()) <= 0.01, "too many undecided bytes"
    assert bool((m.abs() <= 4 * s).all())
    assert float((U <= 0).double().mean(1).min()) >= 0.01 and float((U >= 255).double().mean(1).min()) >= 0.01
    assert float(((U > 0) & (U < 255)).double().mean(1).min()) >= 0.5
    assert lo.unique().numel() >= 16
    stats = torch.stack([xd.sum(1), (xd * xd).sum(1)], 1).contiguous()
    return _case(recon=recon, lo=lo.view(B, tiles, H, W, 3), hi=hi.view(B, tiles, H, W, 3), stats=stats)


def _mosaic(t, tiles, reverse, fill):
    """[B, tiles, H, W, 3] -> [B, rows * H, 2 W, 3] with tile t at (t // 2, t % 2); unused cells = fill."""
    B, _, H, W, _ = t.shape
    out = torch.full((B, (tiles + 1) // 2 * H, 2 * W, 3), fill, dtype=t.dtype)
    for k in range(tiles):
        out[:, (k // 2) * H:(k // 2 + 1) * H, (k % 2) * W:(k % 2 + 1) * W] = t[:, k].flip(-1) if reverse else t[:, k]
    return out


def _deprocess_check(native_lib, c, tiles, reverse, stats, recon=None):
    B, _, H, W, _ = c.lo.shape
    out = torch.full((B, (tiles + 1) // 2 * H, 2 * W, 3), SENT_U8, dtype=torch.uint8, device=DEV)
    native_lib.deprocess_mosaic(c.recon.to(DEV) if recon is None else recon, out, tiles, reverse, stats)
    assert _misc_route() == _deprocess_route(W)
    got = out.cpu().long()
    lo, hi = _mosaic(c.lo, tiles, reverse, -1), _mosaic(c.hi, tiles, reverse, -1)
    used = lo >= 0
    assert bool((used.double().mean() == tiles / (2 * ((tiles + 1) // 2))))
    assert bool((got[~used] == SENT_U8).all()), "a byte outside the tiles was written"
    bad = used & ((got < lo) | (got > hi))
    assert not bool(bad.any()), (f"{int(bad.sum())} bytes off, first at {bad.nonzero()[0].tolist()}: got "
                                 f"{int(got[bad][0])}, want {int(lo[bad][0])}..{int(hi[bad][0])}")
    return out


@gpu
@pytest.mark.parametrize("reverse", [False, True], ids=["rgb", "bgr"])
@pytest.mark.parametrize("B,tiles,H,W", DEPROCESS_TWO_PASS + DEPROCESS_APPLY)
def test_deprocess_oracle(native_lib, B, tiles, H, W, reverse):
    """Both deprocess paths against the banded fp64 oracle: every decided byte exact (statistics over the
    WHOLE mosaic for any tiles / H / W, tile placement, channel order), undecided ones one of two
    neighbours, nothing written outside the tiles (the fourth quadrant of a 3-tile mosaic, the right half
    of a 1-tile one)."""
    _deprocess_check(native_lib, _deprocess_case(B, tiles, H, W), tiles, reverse, None)


@gpu
def test_deprocess_two_pass_offset_view(native_lib):
    """The two-pass kernel on a view that starts one tile into its buffer (5 * 5 * 3 floats: 4-B aligned
    only), 1 tile per image: every image has a scalar head and tail."""
    B, tiles, H, W = 2, 1, 5, 5
    c = _deprocess_case(B, tiles, H, W)
    buf = torch.zeros(B * tiles + 1, H, W, 3, device=DEV)
    buf[1:] = c.recon.to(DEV)
    assert buf[1:].data_ptr() % 16 != 0 and buf[1:].is_contiguous()
    _deprocess_check(native_lib, c, tiles, True, None, recon=buf[1:])


@gpu
@pytest.mark.parametrize("B,tiles,H,W", DEPROCESS_APPLY)
def test_deprocess_stats_argument(native_lib, B, tiles, H, W):
    """``stats=`` (fp64 {sum, sum of squares} per mosaic, here the CPU's) goes through the same oracle; on
    integer-valued recon the sums are exact in any order, so stats=None gives the same bytes."""
    c = _deprocess_case(B, tiles, H, W)
    _deprocess_check(native_lib, c, tiles, True, c.stats.to(DEV))
    ci = _deprocess_case(B, tiles, H, W, integer=True)
    assert torch.equal(ci.recon, ci.recon.round()) and float(ci.stats.max()) < 2 ** 53
    a = _deprocess_check(native_lib, ci, tiles, True, ci.stats.to(DEV))
    b = _deprocess_check(native_lib, ci, tiles, True, None)
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------
# 9. resize / preprocess
# ----------------------------------------------------------------------------------------

# source -> output: upscale, one-pixel axes, exact 2x (the area path), copy
RESIZE_CASES = [((5, 3), (7, 9)), ((1, 9), (4, 4)), ((9, 1), (7, 9)), ((14, 18), (7, 9)), ((3, 3), (3, 3))]
CPADS = [3, 4, 8, 16]
# 70000 px is 274 blocks; the grid is capped at 256 * 32 blocks of 256 threads, so only the last size makes
# the stride loop take a second trip
PRE_P = [1, 255, 70000, 256 * 32 * 256 + 300]


def _pre_ref(u8, cpad, dt):
    """[..., 3] u8 RGB -> [..., cpad] 16-bit: slot c < 3 = rgb[c] - CAFFE_MEAN[c] (one rounding), else 0."""
    out = torch.zeros(*u8.shape[:-1], cpad)
    out[..., :3] = torch.from_numpy(u8.astype(np.float32)) - torch.tensor(ops.CAFFE_MEAN)
    return out.to(dt)


@functools.lru_cache(maxsize=None)
def _resize_case(src, dst):
    rng = np.random.default_rng(src[0] * 100 + src[1])
    imgs = rng.integers(0, 256, size=(3, *src, 3), dtype=np.uint8)
    ref = np.stack([ops.resize_u8_ref(im, *dst) for im in imgs])
    assert ref.shape == (3, *dst, 3) and ref.dtype == np.uint8
    assert ops.resize_mode(*src, *dst) == {(14, 18): 1, (3, 3): 2}.get(src, 0)
    if src == dst:
        assert np.array_equal(ref, imgs)
    return _case(imgs=imgs, ref=ref)


def _check_pre(out, ref_u8, cpad, dt):
    assert torch.equal(_bits(out), _bits(_pre_ref(ref_u8, cpad, dt)))
    assert not bool(_bits(out)[..., 3:].any()), "padding slots must be exactly zero"


@gpu
@dtypes
@pytest.mark.parametrize("cpad", CPADS)
@pytest.mark.parametrize("src,dst", RESIZE_CASES)
def test_resize_preprocess_shapes(native_lib, src, dst, cpad, dt):
    """resize_preprocess_kernel at outputs other than 224 x 224 (OH != OW), every mode, every store form."""
    c = _resize_case(src, dst)
    out = torch.full((3, *dst, cpad), SENTINEL, dtype=dt, device=DEV)
    native_lib.resize_preprocess(torch.from_numpy(c.imgs).to(DEV), out, ops.resize_mode(*src, *dst))
    _check_pre(out, c.ref, cpad, dt)


@functools.lru_cache(maxsize=None)
def _batch_case():
    """One table with all three modes, the images back to back in one blob, to 7 x 9."""
    rng = np.random.default_rng(77)
    imgs = [rng.integers(0, 256, size=(*s, 3), dtype=np.uint8) for s in [(5, 3), (14, 18), (7, 9), (1, 9)]]
    blob, rows = [np.zeros(5, np.uint8)], []  # (the first image does not start at offset 0)
    for im in imgs:
        rows.append([sum(b.size for b in blob), im.shape[0], im.shape[1], ops.resize_mode(*im.shape[:2], 7, 9)])
        blob.append(im.reshape(-1))
    assert [r[3] for r in rows] == [0, 1, 2, 0]
    ref = np.stack([ops.resize_u8_ref(im, 7, 9) for im in imgs])
    return _case(blob=torch.from_numpy(np.concatenate(blob)), table=torch.tensor(rows, dtype=torch.int64), ref=ref)


@gpu
@pytest.mark.parametrize("fmt,cpad", [("u8", 3), ("bf16", 3), ("bf16", 8), ("fp16", 3), ("fp16", 8)])
def test_resize_batch_modes(native_lib, fmt, cpad):
    """resize_batch_kernel: linear, exact-2x area and copy rows in one table, to u8, bf16 and fp16."""
    c = _batch_case()
    B = c.table.shape[0]
    if fmt == "u8":
        out = torch.full((B, 7, 9, 3), SENT_U8, dtype=torch.uint8, device=DEV)
    else:
        out = torch.full((B, 7, 9, cpad), SENTINEL, dtype=BF if fmt == "bf16" else HF, device=DEV)
    native_lib.resize_batch(c.blob.to(DEV), c.table.to(DEV), out, c.blob.numel())
    if fmt == "u8":
        assert np.array_equal(out.cpu().numpy(), c.ref)
    else:
        _check_pre(out, c.ref, cpad, out.dtype)


@functools.lru_cache(maxsize=None)
def _pre_case(P):
    return np.random.default_rng(P).integers(0, 256, size=(1, 1, P, 3), dtype=np.uint8)


@gpu
@dtypes
@pytest.mark.parametrize("cpad", [3, 8])
@pytest.mark.parametrize("P", PRE_P)
def test_preprocess_u8_sizes(native_lib, P, cpad, dt):
    u8 = _pre_case(P)
    out = torch.full((1, 1, P, cpad), SENTINEL, dtype=dt, device=DEV)
    native_lib.preprocess_u8(torch.from_numpy(u8).to(DEV), out)
    _check_pre(out, u8, cpad, dt)


# ----------------------------------------------------------------------------------------
# 10. maxpool2x2 / unpool2x2 / softmax_rows edges
# ----------------------------------------------------------------------------------------

POOL_EDGE = [(2, 6, 10, 8), (2, 6, 10, 12), (3, 2, 2, 8), (3, 4, 2, 12)]


@functools.lru_cache(maxsize=None)
def _pool_case(N, H, W, C):
    g = _gen(N + H + W + C)
    x = _ints(g, (N, H, W, C), -4, 4)
    win = x.view(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)
    val = win.max(dim=3).values
    code = torch.where(win == val.unsqueeze(3), torch.arange(4).view(1, 1, 1, 4, 1), 4).min(dim=3).values  # first max
    assert int(code.max()) <= 3
    assert float(((win == val.unsqueeze(3)).sum(3) >= 2).double().mean()) >= 0.05, "too few tied windows"
    _conditions(val, 4)
    return _case(x=x, val=val, code=code.to(torch.uint8))


@gpu
@dtypes
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("N,H,W,C", POOL_EDGE)
def test_exact_maxpool2x2(native_lib, N, H, W, C, aligned, dt):
    """maxpool2x2: C = 8 takes the vectorized kernel, C = 12 and a view that is only 2-B aligned the scalar
    one; values and first-max codes (0..3) exact in both dtypes."""
    c = _pool_case(N, H, W, C)
    n = c.x.numel()
    buf = torch.zeros(n + 8, dtype=dt, device=DEV)
    off = 0 if aligned else 1
    buf[off:off + n] = c.x.to(dt).flatten().to(DEV)
    x = buf[off:off + n].view(N, H, W, C)
    assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == aligned
    out = torch.full((N, H // 2, W // 2, C), SENTINEL, dtype=dt, device=DEV)
    code = torch.full((N, H // 2, W // 2, C), 255, dtype=torch.uint8, device=DEV)
    native_lib.maxpool2x2(x, out, code)
    assert _misc_route() == ("maxpool2x2 vec" if C % 8 == 0 and aligned else "maxpool2x2 scalar")
    _same(out, c.val)
    assert torch.equal(code.cpu(), c.code) and int(code.max()) <= 3


UNPOOL_EDGE = [(4, 3, 5, C, div, relu) for C in (8, 12) for div in (1, 2, 4) for relu in (False, True)]


@functools.lru_cache(maxsize=None)
def _unpool_case(N, PH, PW, C, div, relu, dt):
    """Expected 16-bit patterns: the pooled value's own bits at its switch position (-0.0 stays -0.0), +0
    elsewhere; with ``relu`` every value with the sign bit set (negatives, -0.0) becomes +0."""
    g = _gen(N + PH + PW + C + div)
    vals = torch.tensor([-3.0, -1.0, -0.0, 0.0, 1.0, 2.0, 5.0])
    p = vals[torch.randint(0, 7, (N, PH, PW, C), generator=g)].to(dt)
    code = torch.randint(0, 4, (N // div, PH, PW, C), generator=g, dtype=torch.uint8)
    pb = p.view(torch.int16)
    assert int((pb == -32768).sum()) > 0  # -0.0 is in the input
    want = _unpool(pb, code, div)
    if relu:
        want = torch.where(want < 0, torch.zeros_like(want), want)
        assert float((want == 0).double().mean()) > 0.75
    else:
        assert int((want == -32768).sum()) > 0
    assert float((want != 0).double().mean()) >= (0.08 if relu else 0.15)  # a quarter of the cells is the most
    return _case(p=p, code=code, want=want)


@gpu
@dtypes
@pytest.mark.parametrize("N,PH,PW,C,div,relu", UNPOOL_EDGE)
def test_exact_unpool2x2(native_lib, N, PH, PW, C, div, relu, dt):
    """unpool2x2 (vectorized at C = 8, scalar at C = 12): codes shared by ``div`` signals, bit patterns."""
    c = _unpool_case(N, PH, PW, C, div, relu, dt)
    out = torch.full((N, 2 * PH, 2 * PW, C), SENTINEL, dtype=dt, device=DEV)
    native_lib.unpool2x2(c.p.to(DEV), c.code.to(DEV), out, div, relu)
    assert _misc_route() == ("unpool2x2 vec" if C % 8 == 0 else "unpool2x2 scalar")
    assert torch.equal(_bits(out), c.want)


SOFTMAX_N = [1, 3, 255, 257, 1000]


@functools.lru_cache(maxsize=None)
def _softmax_case(N):
    g = _gen(N)
    x = torch.randn(7, N, generator=g) * 3
    x[1] = 2.5                                                        # a constant row
    x[2] = torch.where(torch.rand(N, generator=g) < 0.5, 80.0, -80.0)  # magnitudes of +-80
    x[2, 0] = 80.0
    x[3] = x[3] * 20
    x[4] = -80.0 + torch.randn(N, generator=g)
    x[5] = 80.0 + torch.randn(N, generator=g)
    if N > 1:
        x[6, 1::2] = -INF                                             # -inf entries (never a whole row)
        x[0, N - 1] = -INF
    ref = torch.softmax(x.double(), dim=1)
    assert bool(torch.isfinite(ref).all()) and torch.allclose(ref.sum(1), torch.ones(7, dtype=torch.float64))
    return _case(x=x, ref=ref)


@gpu
@pytest.mark.parametrize("N", SOFTMAX_N)
def test_softmax_rows_edges(native_lib, N):
    """softmax_rows_kernel against an fp64 softmax (rtol 1e-5, atol 1e-7): one element, fewer than / one more
    than a block's 256 threads, 1000 classes; -inf entries, a constant row, magnitudes of +-80."""
    c = _softmax_case(N)
    y = torch.full((7, N), SENTINEL, dtype=torch.float32, device=DEV)
    native_lib.softmax_rows(c.x.to(DEV), y)
    torch.testing.assert_close(y.cpu().double(), c.ref, rtol=1e-5, atol=1e-7)
    assert float((y.cpu().double().sum(1) - 1).abs().max()) <= 1e-5
    if N > 1:
        assert not bool(y.cpu()[6, 1::2].any())


# ----------------------------------------------------------------------------------------
# conditions (no GPU)
# ----------------------------------------------------------------------------------------

def test_conditions():
    """Every case of every table satisfies the method's conditions on its CPU reference."""
    for shape in SEED_SMALL + SEED_GRID:
        _seed_case(*shape)
    for shape in SEEDMAP_SHAPES:
        _seedmap_case(*shape)
    for shape in CSUM_SHAPES:
        _csum_case(*shape)
    for case in TOPK_CASES:
        _topk_case(*case)
    for shape in ZSUM_SHAPES:
        _zsum_case(*shape)
    for case in TAIL_CASES:
        _tail_case(*case)
    assert _tail_tiles(*TAIL_CASES[-1][:3]) > 256
    for case in DEPROCESS_TWO_PASS:
        assert case[3] % 4 != 0
        _deprocess_case(*case)
    assert any((t * H * W * 3) % 4 for _, t, H, W in DEPROCESS_TWO_PASS)  # totals the 16-B loads do not cover
    for case in DEPROCESS_APPLY:
        assert case[3] % 4 == 0
        _deprocess_case(*case)
        _deprocess_case(*case, integer=True)
    for src, dst in RESIZE_CASES:
        _resize_case(src, dst)
    _batch_case()
    for P in PRE_P:
        _pre_case(P)
    for shape in POOL_EDGE:
        _pool_case(*shape)
    for case in UNPOOL_EDGE:
        for dt in (BF, HF):
            _unpool_case(*case, dt)
    for N in SOFTMAX_N:
        _softmax_case(N)
