"""GPU: the conv kernels against an EXACT oracle.

Operands are small integers (x in [-3, 3], weights in [-2, 2] thinned to about 96 non-zero taps per
output, bias / residual / accumulate base in [-4, 4]), so every product and every partial sum is an
integer below 2^24: exact in fp32 under ANY summation order (split-K, stream-K hand-offs, MFMA
accumulation order), and the results are integers of at most 256 in magnitude: exact in bf16 and fp16.
A correct kernel therefore reproduces the fp32 CPU reference bit for bit, ``torch.equal``: a wrong border
element, a double rounding, a switch code on a tie (ties are the rule here: about half of the outputs
are 0 after the ReLU) or a mask applied in the wrong order all show, whatever K is.

Each case asserts, on the CPU reference and before it looks at the GPU result, that these conditions
hold (``_check_exact``): they are conditions of the method, not tolerances. Each case also asserts the
kernel that ran (``conv_route``), so it cannot turn into a test of that kernel's fallback.
"""
import pytest
import torch
import torch.nn.functional as F

from deconv_api_amd import ops
from deconv_api_amd.ops import autograd as AG
from exact_helpers import BF, DEV, HF, _check_exact, _dev, _gen, _geom, _ints, _pool_case, _same, _signs, _weights
from gpu_helpers import cus as _cus, route as _route, tune as _tune

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------
# KW3 family
# ----------------------------------------------------------------------------------------

KW3_SHAPES = [(3, 10, 9, 32, 256, BF), (2, 11, 13, 96, 256, HF), (2, 9, 12, 128, 512, BF), (3, 36, 35, 32, 128, HF)]


def _kw3_tile(OC):
    return "256x256" if OC % 256 == 0 else "512x128"


@pytest.mark.parametrize("mode", ["16bit", "f32", "accumulate", "res_emask", "unpool"])
@pytest.mark.parametrize("N,H,W,C,OC,dt", KW3_SHAPES)
def test_exact_kw3_epilogues(native_lib, monkeypatch, N, H, W, C, OC, dt, mode):
    """The non-persistent shared-tap kernel (conv_dma_kw3_kernel, DV_KW3=2 + DV_KW3_VAR=0) with every
    epilogue it has, on shapes of one to eight tiles with an M tail whose tiles cross image rows and
    images (W = 9 is the narrowest map the 256 x 256 tile takes, 35 the 512 x 128 tile's)."""
    monkeypatch.setenv("DV_KW3", "2")
    monkeypatch.setenv("DV_KW3_VAR", "0")
    g = _gen(N * H + C + len(mode))
    x = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C)
    cwd = cw.to_device(DEV, dt)
    kw, dkw, extra = dict(relu=True), dict(relu=True), 4.0
    if mode == "f32":
        kw = dkw = dict(relu=False, epilogue="f32")
    elif mode == "accumulate":
        base = _ints(g, (N, H, W, OC), -4, 4)
        kw = dict(relu=False, out=base.clone(), accumulate=True)
        dkw = dict(relu=False, out=_dev(base, dt), accumulate=True)
        extra = 8.0
    elif mode == "res_emask":
        res, em = _ints(g, (N, H, W, OC), -4, 4), _signs(g, (N, H, W, OC))
        kw = dict(relu=True, res=res, emask=em)
        dkw = dict(relu=True, res=_dev(res, dt), emask=_dev(em, dt))
        extra = 8.0
    elif mode == "unpool":
        code = torch.randint(0, 4, (N, H, W, OC), generator=g, dtype=torch.uint8)
        kw = dict(relu=True, unpool_out=code)
        dkw = dict(relu=True, unpool_out=code.to(DEV))
    ref = ops.conv2d(x, cw, **kw)
    # (res + emask: three quarters masked on top of the ReLU; unpool: three quarters structural zeros)
    _check_exact(ref, torch.float32 if mode == "f32" else dt, x, cw, extra, dense=mode not in ("res_emask", "unpool"))
    with _tune(0, 1):
        got = ops.conv2d(_dev(x, dt), cwd, **dkw)
        assert _route() == f"kw3 {_kw3_tile(OC)}", _route()
    _same(got, ref)


@pytest.mark.parametrize("epi", ["lds", "reg"])
@pytest.mark.parametrize("H,W,C,OC,dt", [(11, 13, 32, 256, BF), (36, 35, 32, 128, HF)])
def test_exact_kw3p_persistent(native_lib, monkeypatch, H, W, C, OC, dt, epi):
    """The persistent shared-tap kernel (conv_dma_kw3p_kernel) at 256 x 256 and 512 x 128 with its LDS-sliced
    16-B and register-transposed 8-B stores: one workgroup per CU and about 1.2 tiles per workgroup (the
    batch follows the CU count), so some workgroups walk two tiles; tiles cross image rows and images."""
    monkeypatch.setenv("DV_KW3", "2")
    monkeypatch.setenv("DV_NO_KW3_SK", "1")
    if epi == "reg":
        monkeypatch.setenv("DV_KW3P_EPI", "reg")
    bm = 256 if OC % 256 == 0 else 512
    N = -(-(6 * _cus() // 5) * bm // (H * W)) + 1
    g = _gen(H + OC)
    x = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C)
    ref = ops.conv2d(x, cw, relu=True)
    _check_exact(ref, dt, x, cw, 4.0)
    with _tune(0, 1):
        got = ops.conv2d(_dev(x, dt), cw.to_device(DEV, dt), relu=True)
        assert _route() == f"kw3p {_kw3_tile(OC)} {epi}", _route()
    _same(got, ref)


@pytest.mark.parametrize("div", [1, 2, 3, 4])
def test_exact_kw3p_unpool_out(native_lib, monkeypatch, div):
    """KW3P's max-unpool-out epilogue with the switch codes shared by 1 .. 4 images (code_div)."""
    monkeypatch.setenv("DV_KW3", "2")
    monkeypatch.setenv("DV_NO_KW3_SK", "1")
    N, H, W, C, OC = 12, 10, 9, 32, 256
    dt = BF if div % 2 else HF
    g = _gen(70 + div)
    x = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C, bias=False)
    code = torch.randint(0, 4, (N // div, H, W, OC), generator=g, dtype=torch.uint8)
    ref = ops.conv2d(x, cw, relu=True, use_bias=False, unpool_out=code, unpool_div=div)
    _check_exact(ops.conv2d(x, cw, relu=True, use_bias=False), dt, x, cw)
    with _tune(0, 1):
        got = ops.conv2d(_dev(x, dt), cw.to_device(DEV, dt), relu=True, use_bias=False, unpool_out=code.to(DEV),
                         unpool_div=div)
        assert _route() == "kw3p 256x256 unpool", _route()
    _same(got, ref)


@pytest.mark.parametrize("H,W,C,OC,div,dt", [(14, 14, 32, 256, 0, BF), (12, 11, 32, 512, 2, HF)])
def test_exact_kw3p_stream_k(native_lib, monkeypatch, H, W, C, OC, div, dt):
    """Stream-K KW3P on a grid of about 1.5 rounds of one workgroup per CU (the batch follows the CU count):
    bit-equal to the whole-tile kernel over the full tensor (integer partial sums: the extra fp32 add of
    a split tile is exact), equal to the CPU reference on the first and last 2 div images and 8 images
    from the middle, and no hand-off timed out."""
    monkeypatch.setenv("DV_KW3", "2")
    G = _cus()
    tiles_n, d = OC // 256, max(div, 1)
    if G % tiles_n:
        pytest.skip(f"stream-K needs the {tiles_n} column groups to divide the device's {G} CUs")
    sk = " sk"
    N = -(-(3 * G // (2 * tiles_n)) * 256 // (H * W * d)) * d
    tiles = -(-N * H * W // 256) * tiles_n
    assert G < tiles < 2 * G, (tiles, G)
    g = _gen(H + OC + div)
    x = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C, bias=not div)
    kw = dict(relu=True, use_bias=not div)
    code = None
    if div:
        code = torch.randint(0, 4, (N // div, H, W, OC), generator=g, dtype=torch.uint8)
        kw.update(unpool_out=code.to(DEV), unpool_div=div)
    epi = "unpool" if div else "lds"
    xd, cwd = _dev(x, dt), cw.to_device(DEV, dt)
    native_lib.sk_errors(True)
    with _tune(0, 1):
        got = ops.conv2d(xd, cwd, **kw)
        assert _route() == f"kw3p 256x256 {epi}{sk}", _route()
        monkeypatch.setenv("DV_NO_KW3_SK", "1")
        whole = ops.conv2d(xd, cwd, **kw)
        assert _route() == f"kw3p 256x256 {epi}", _route()
    torch.cuda.synchronize()
    assert native_lib.sk_errors(True) == 0
    assert torch.equal(got, whole)
    n = 2 * d
    mid = [(N // (9 * d)) * d * k for k in range(1, 9)]  # 8 images from the middle (whole code groups)
    for lo, hi in [(0, n), (N - n, N)] + [(m, m + d) for m in mid if n <= m <= N - n - d]:
        rkw = dict(relu=True, use_bias=not div)
        if div:
            rkw.update(unpool_out=code[lo // div: hi // div], unpool_div=div)
        ref = ops.conv2d(x[lo:hi], cw, **rkw)
        _check_exact(ops.conv2d(x[lo:hi], cw, relu=True, use_bias=not div), dt, x[lo:hi], cw, 4.0)
        _same(got[lo:hi], ref)


def test_exact_kw3_tail_split(native_lib, monkeypatch):
    """A grid of 1.05 rounds (the batch follows the CU count) without stream-K: the full round on KW3P, the
    rest as a 128 x 128 LDS-DMA tail launch from row m_base (kw3_split). Checked on the images on both
    sides of m_base, the first ones and the last ones (the M tail). (K = 9 x 512 is what it takes to pass the
    measured small-problem tile choice and reach kw3_split by the natural route: about 160 GFLOP on the GPU,
    under a second; the CPU reference covers seven images only.)"""
    monkeypatch.setenv("DV_NO_KW3_SK", "1")
    G = _cus()
    H, W, C, OC, dt = 14, 14, 512, 256, BF
    N = -(-(21 * G // 20 + 1) * 256 // (H * W))
    g = _gen(5)
    x = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C)
    got = ops.conv2d(_dev(x, dt), cw.to_device(DEV, dt), relu=True)
    m_base = G * 256
    assert _route() == f"kw3p 256x256 lds + dma 128x128 tail m_base={m_base}", _route()
    nb = m_base // (H * W)
    assert 1 <= nb < N - 2
    for lo, hi in [(0, 2), (nb - 1, nb + 2), (N - 2, N)]:
        ref = ops.conv2d(x[lo:hi], cw, relu=True)
        _check_exact(ref, dt, x[lo:hi], cw, 4.0)
        _same(got[lo:hi], ref)


# ----------------------------------------------------------------------------------------
# LDS-DMA tile matrix
# ----------------------------------------------------------------------------------------

# tile config (csrc/conv_dma_plan.h kDmaTiles) -> (BM, BN, stages)
DMA_CFGS = {1: (256, 256, 2), 2: (128, 256, 3), 3: (128, 128, 2), 4: (256, 128, 3), 5: (256, 64, 2), 6: (512, 64, 2),
            7: (128, 64, 3), 8: (64, 64, 3), 9: (128, 128, 2), 10: (64, 128, 3), 11: (256, 64, 2), 12: (64, 64, 6),
            13: (64, 64, 8), 14: (128, 64, 6), 15: (64, 128, 6), 16: (64, 64, 3), 17: (64, 64, 4)}
# per tile width: (C, OC, input / output as channel slices of wider buffers): OC < OCpad on the 64-wide
# tiles, C = 24 (K tiles straddle taps: the unaligned-K gather) on the 128-wide, slices on the 256-wide
DMA_WIDTH = {64: (32, 40, False), 128: (24, 128, False), 256: (32, 256, True)}


@pytest.mark.parametrize("dt", [BF, HF])
@pytest.mark.parametrize("cfg", sorted(DMA_CFGS))
def test_exact_dma_tile_matrix(native_lib, cfg, dt):
    """Every tile config the LDS-DMA kernel is instantiated with, forced (dma_tune), with and without a
    3-way split-K: forward with the 16-bit, fp32 and fused-pool epilogues and the stride-2 transposed
    gather, at M = BM - 1, BM + 1 and 3 BM + 7 rows (the pool epilogue, whose rows come in fours, at the
    multiples of 4 next to them: BM - 4, BM + 4, 3 BM + 8)."""
    BM, BN, ST = DMA_CFGS[cfg]
    C, OC, sliced = DMA_WIDTH[BN]
    g = _gen(cfg)
    cw = _weights(g, OC, C)
    ct = _weights(g, OC, C, kind="transpose", bias=False, taps=96 * 4)  # (a stride-2 gather meets 1/4 of the taps)
    cwd, ctd = cw.to_device(DEV, dt), ct.to_device(DEV, dt)
    ld_x, ld_o = (C + 8, OC + 8) if sliced else (C, OC)

    def xdev(x):  # a channel-slice view of a wider buffer (x_ld > C)
        buf = torch.full(x.shape[:3] + (ld_x,), 3.0, dtype=dt, device=DEV)
        buf[..., :C] = _dev(x, dt)
        return buf[..., :C]

    for mode in ("bf16", "f32", "pool", "transpose"):
        for M in ((BM - 4, BM + 4, 3 * BM + 8) if mode == "pool" else (BM - 1, BM + 1, 3 * BM + 7)):
            N, OH, OW, crop = _geom(M, even=mode == "pool")
            assert N * OH * OW == M
            if mode == "transpose":
                # (one output row: the stride-2 gather's row 0 meets the middle kernel row of input row 0 only)
                x = _ints(g, (N, (OH + 1) // 2, (OW + 1) // 2, C), -3, 3)
                kw = dict(relu=False, in_mode="transpose", stride=2, pad=(1, 1), out_hw=(OH, OW), use_bias=False)
                ref = ops.conv2d(x, ct, **kw)
                _check_exact(ref, dt, x, ct, stride=2)
            else:
                x = _ints(g, (N, OH + 2 if crop else OH, OW, C), -3, 3)
                kw = dict(relu=mode != "f32", epilogue=mode, pad=(0, 1) if crop else (1, 1))
                ref = ops.conv2d(x, cw, **kw)
                _check_exact(ops.conv2d(x, cw, relu=mode != "f32", pad=kw["pad"]) if mode == "pool" else ref,
                             torch.float32 if mode == "f32" else dt, x, cw, 4.0)
                if mode == "pool":
                    _check_exact(ref[0], dt, x, cw, 4.0)
            for ks in (1, 3):
                if mode == "pool" and ks > 1:
                    continue  # (no split-K under the pooled epilogue)
                odt = torch.float32 if mode == "f32" else dt
                oshape = (N, OH // 2, OW // 2, ld_o) if mode == "pool" else (N, OH, OW, ld_o)
                obuf = torch.full(oshape, 7.0, dtype=odt, device=DEV)
                with _tune(cfg, ks):
                    got = ops.conv2d(xdev(x), ctd if mode == "transpose" else cwd, out=obuf[..., :OC], **kw)
                    r = _route()
                assert r.startswith(f"dma {BM}x{BN} st{ST} ks{ks}"), (r, mode, M, ks)
                if mode == "pool":
                    _same(got[0], ref[0])
                    assert torch.equal(got[1].cpu(), ref[1]), (mode, M)
                else:
                    _same(got, ref)
                assert bool((obuf[..., OC:] == 7.0).all()), "wrote past the channel slice"


@pytest.mark.parametrize("cfg", [c for c, t in sorted(DMA_CFGS.items()) if t[1] > 64])
def test_exact_dma_tile_misfit_raises(native_lib, cfg):
    """A forced tile wider than the padded output (OCpad 64) does not fit: the launch raises."""
    g = _gen(cfg)
    x = _ints(g, (1, 8, 8, 32), -3, 3)
    cw = _weights(g, 40, 32)
    with _tune(cfg, 1):
        with pytest.raises(RuntimeError, match="launch failed"):
            ops.conv2d(_dev(x, BF), cw.to_device(DEV), relu=True)


# ----------------------------------------------------------------------------------------
# fused pool epilogues on ties
# ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi", ["pool_t", "pool_lds", "pool"])
@pytest.mark.parametrize("N,H,W,C,OC,cfg,tile", [(2, 16, 14, 64, 128, 4, "256x128 st3"), (3, 10, 14, 64, 192, 6, "512x64 st2"),
                                                 (1, 12, 12, 32, 48, 11, "256x64 st2")])
def test_exact_pool_ties_dma(native_lib, monkeypatch, N, H, W, C, OC, cfg, tile, epi):
    """The LDS-DMA kernel's three pooled-max epilogues (DPP-transposed 8-B stores, LDS-staged 16-B stores,
    per element) on windows full of ties: values and first-max switch codes equal the reference's."""
    if epi == "pool_lds":
        monkeypatch.setenv("DV_POOL_EPI", "lds")
    if epi == "pool":
        monkeypatch.setenv("DV_NO_POOL_T", "1")
    x, cw, rp, rc = _pool_case(_gen(OC), N, H, W, C, OC)
    with _tune(cfg, 0):
        gp, gc = ops.conv2d(_dev(x, BF), cw.to_device(DEV), relu=True, epilogue="pool")
        assert _route() == f"dma {tile} ks1 {epi}", _route()
    _same(gp, rp)
    assert torch.equal(gc.cpu(), rc)


@pytest.mark.parametrize("N,H,W,C,OC,route", [(1, 64, 64, 32, 64, "hs16 oc64 pool"), (1, 64, 80, 64, 128, "hs16 oc128 pool"),
                                              (1, 70, 66, 32, 128, "hs32 oc128 pool"), (1, 112, 120, 64, 64, "pool_v3")])
def test_exact_pool_ties_halo(native_lib, N, H, W, C, OC, route):
    """The halo-stream kernels' (16 x 16 and 16 x 32 tiles) and the weight-resident 64 -> 64 kernel's fused
    pool on windows full of ties."""
    x, cw, rp, rc = _pool_case(_gen(H + OC), N, H, W, C, OC)
    gp, gc = ops.conv2d(_dev(x, BF), cw.to_device(DEV), relu=True, epilogue="pool")
    assert _route() == route, _route()
    _same(gp, rp)
    assert torch.equal(gc.cpu(), rc)


def test_exact_pool_ties_stem(native_lib):
    """The fused stem (conv 8 -> 64, ReLU, conv 64 -> 64, ReLU, pool; the 64-channel map between the convs
    lives in LDS only): the intermediate map is integer too, so the whole chain is exact."""
    g = _gen(3)
    N, H, W = 2, 32, 48
    x = _ints(g, (N, H, W, 8), -3, 3)
    x[..., 3:] = 0
    # (two convs in a chain: thinner weights keep the second one's sums of first-conv outputs below 256)
    c1 = _weights(g, 64, 8, taps=24)
    c2 = _weights(g, 64, 64, taps=12)
    y1 = ops.conv2d(x, c1, relu=True)
    _check_exact(y1, BF, x, c1, 4.0)
    full = ops.conv2d(y1, c2, relu=True)
    _check_exact(full, BF, y1, c2, 4.0)
    rp, rc = ops.conv2d(y1, c2, relu=True, epilogue="pool")
    got = ops.stem_pool(_dev(x, BF), c1.to_device(DEV), c2.to_device(DEV))
    assert got is not None and _route() == "hs16 oc64 pool stem", _route()
    _same(got[0], rp)
    assert torch.equal(got[1].cpu(), rc)


# ----------------------------------------------------------------------------------------
# mask semantics: zeros of both signs, accumulate then mask
# ----------------------------------------------------------------------------------------

MASK_CASES = [
    # name, (N, H, W, C, OC, k), forced (cfg, ks), route prefix
    ("dma", (2, 9, 7, 64, 128, 3), (3, 1), "dma 128x128 st2 ks1"),
    ("dma_tail_chunk", (2, 9, 7, 32, 44, 3), (8, 1), "dma 64x64 st3 ks1"),  # OC % 8 != 0: per-element row tails
    ("splitk", (2, 9, 7, 64, 96, 3), (8, 3), "dma 64x64 st3 ks3"),
    ("pw", (2, 181, 183, 64, 128, 1), (0, 0), "pw 128x128"),
    ("hs16", (1, 64, 64, 32, 64, 3), (0, 0), "hs16 oc64 lds"),
    ("hs32", (1, 70, 66, 32, 128, 3), (0, 0), "hs32 oc128 lds"),
]


@pytest.mark.parametrize("dt", [BF, HF])
@pytest.mark.parametrize("name,shape,tune,route", MASK_CASES, ids=[c[0] for c in MASK_CASES])
def test_exact_emask_zeros(native_lib, name, shape, tune, route, dt):
    """emask drawn from {-1, -0.0, 0, 1}: the output is zero exactly where emask <= 0, both zeros included
    (the kernels test the bit pattern: zero magnitude or sign bit)."""
    N, H, W, C, OC, k = shape
    g = _gen(len(name) + OC)
    x = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C, k, k)
    em = _signs(g, (N, H, W, OC))
    kw = dict(relu=False, pad=k // 2)
    ref = ops.conv2d(x, cw, emask=em, **kw)
    _check_exact(ops.conv2d(x, cw, **kw), dt, x, cw, 4.0, pad=k // 2)
    assert bool((ref[em <= 0] == 0).all()) and float((ref != 0).float().mean()) > 0.15
    with _tune(*tune):
        got = ops.conv2d(_dev(x, dt), cw.to_device(DEV, dt), emask=_dev(em, dt), **kw)
        assert _route().startswith(route), _route()
    _same(got, ref)


@pytest.mark.parametrize("dt", [BF, HF])
@pytest.mark.parametrize("name,shape,tune,route", MASK_CASES[:4], ids=[c[0] for c in MASK_CASES[:4]])
def test_exact_accumulate_then_emask(native_lib, name, shape, tune, route, dt):
    """accumulate with emask and a base that is non-zero where emask <= 0: the kernels accumulate, then
    mask (out = (out + conv) * (emask > 0), conv2d's documented order), so the old output is zeroed there
    too: the input gradient of a ReLU output summed over its consumers."""
    N, H, W, C, OC, k = shape
    g = _gen(len(name) + OC + 1)
    x = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C, k, k)
    em = _signs(g, (N, H, W, OC))
    base = _ints(g, (N, H, W, OC), 1, 4) * torch.where(torch.rand(N, H, W, OC, generator=g) < 0.5, -1.0, 1.0)
    kw = dict(relu=False, pad=k // 2, accumulate=True)
    ref = ops.conv2d(x, cw, emask=em, out=base.clone(), **kw)
    _check_exact(ops.conv2d(x, cw, out=base.clone(), **kw), dt, x, cw, 8.0, pad=k // 2)
    assert bool((ref[em <= 0] == 0).all()) and bool((base != 0).all())
    out = _dev(base, dt)
    with _tune(*tune):
        got = ops.conv2d(_dev(x, dt), cw.to_device(DEV, dt), emask=_dev(em, dt), out=out, **kw)
        assert _route().startswith(route), _route()
    _same(got, ref)


@pytest.mark.parametrize("dt", [BF, HF])
def test_exact_res_accumulate_relu_order(native_lib, dt):
    """res + accumulate + ReLU (+ emask) on integer operands: the documented order is += res, += out, THEN the
    ReLU, then the mask. The CPU path follows it (a negative base under a positive conv + res tells
    relu(conv + res) + out from relu(conv + res + out)); the GPU binding takes res only without accumulate and
    must refuse the combination, not run it in some other order."""
    N, H, W, C, OC = 2, 9, 7, 64, 128
    g = _gen(41)
    x = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C)
    res, em = _ints(g, (N, H, W, OC), -4, 4), _signs(g, (N, H, W, OC))
    base = _ints(g, (N, H, W, OC), 1, 4) * torch.where(torch.rand(N, H, W, OC, generator=g) < 0.5, -1.0, 1.0)
    conv = ops.conv2d(x, cw, relu=False)
    _check_exact(conv, dt, x, cw, 12.0)
    want = (conv + res + base).clamp_min(0)
    other = (conv + res).clamp_min(0) + base
    _check_exact(want, dt, x, cw, 12.0)
    assert float((want != other).float().mean()) > 0.10, "the two orders do not differ on this case"
    want = want * (em > 0)
    for t in (torch.float32, dt):
        ref = ops.conv2d(x.to(t), cw, relu=True, res=res.to(t), emask=em.to(t), out=base.to(t).clone(), accumulate=True)
        _same(ref, want)
    with pytest.raises(RuntimeError, match="res: forward conv"):
        ops.conv2d(_dev(x, dt), cw.to_device(DEV, dt), relu=True, res=_dev(res, dt), emask=_dev(em, dt),
                   out=_dev(base, dt), accumulate=True)


@pytest.mark.parametrize("dt", [BF, HF])
@pytest.mark.parametrize("C,OC,stride", [(64, 128, 1), (32, 64, 2), (128, 256, 1)])
def test_exact_a_mask_zeros(native_lib, dt, C, OC, stride):
    """The A-operand ReLU mask (dgrad through a ReLU) drawn from {-1, -0.0, 0, 1}, forward and stride-2
    transposed gather, on the LDS-DMA kernel's masked tiles."""
    g = _gen(C + OC + stride)
    N, H, W = 2, 9, 11
    x = _ints(g, (N, H, W, C), -3, 3)
    m = _signs(g, (N, H, W, C))
    if stride == 1:
        cw = _weights(g, OC, C, bias=False)
        kw = dict(relu=False, use_bias=False)
    else:
        cw = _weights(g, OC, C, kind="transpose", bias=False, taps=96 * 4)
        kw = dict(relu=False, in_mode="transpose", stride=2, pad=(1, 1), out_hw=(2 * H, 2 * W), use_bias=False)
    ref = ops.conv2d(x, cw, mask=m, **kw)
    _check_exact(ref, dt, x, cw, stride=stride)
    with _tune(0, 1):
        got = ops.conv2d(_dev(x, dt), cw.to_device(DEV, dt), mask=_dev(m, dt), **kw)
        assert _route().startswith("dma ") and _route().endswith(" mask"), _route()
    _same(got, ref)


@pytest.mark.parametrize("dt", [BF, HF])
def test_exact_subpixel_merge_accumulate_then_emask(native_lib, dt):
    """The stride-2 input gradient merged from its parity classes INTO an existing gradient, masked by a
    ReLU output with zeros of both signs (csrc/pool.hip subpixel_merge_kernel): the sum is masked, so the
    old gradient is zeroed where emask <= 0 as well."""
    g = _gen(17)
    k, s, p, H, C, OC, N = 3, 2, 0, 17, 64, 96, 2
    w = _ints(g, (OC, C, k, k), -2, 2) * (torch.rand(OC, C, k, k, generator=g) < 0.4)
    u = AG.ConvUnit("u", w, None, s, (p, p)).build(DEV, dt)
    OH = (H + 2 * p - k) // s + 1
    gy = _ints(g, (N, OH, OH, OC), -3, 3)
    base = _ints(g, (N, H, H, C), 1, 4) * torch.where(torch.rand(N, H, H, C, generator=g) < 0.5, -1.0, 1.0)
    em = _signs(g, (N, H, H, C))
    grad = F.conv_transpose2d(gy.permute(0, 3, 1, 2), w, None, stride=s, padding=p).permute(0, 2, 3, 1)
    assert grad.shape == base.shape
    ref = (base + grad) * (em > 0)
    assert torch.equal(ref.to(dt).float(), ref) and float((ref != 0).float().mean()) > 0.15
    out = _dev(base, dt)
    assert AG._subpixel_ok(u, out), "class layout not taken by the native merge"
    AG._subpixel_dgrad(_dev(gy, dt), None, u, (H, H), out=out, accumulate=True, emask=_dev(em, dt))
    _same(out, ref)
    assert bool((out.float().cpu()[em <= 0] == 0).all())
    # the same gradient as ONE transposed conv written into its destination (small problems: strided_direct)
    assert AG.strided_direct(u, gy, (H, H))
    out = _dev(base, dt)
    AG.dgrad_strided_into(u, _dev(gy, dt), (H, H), out, accumulate=True, emask=_dev(em, dt))
    assert _route().startswith("dma "), _route()
    _same(out, ref)
