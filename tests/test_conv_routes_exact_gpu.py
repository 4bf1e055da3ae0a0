"""GPU: the conv kernels test_conv_exact_gpu.py leaves out, against the same EXACT oracle: the register-staged
implicit GEMM (csrc/conv_igemm.hip), the 64-channel halo / row-streaming kernels (csrc/conv_smalln.hip), the
halo-stream kernels' plain epilogues (csrc/conv_halo_stream.hip), the persistent 1x1 kernel (csrc/conv_pw.hip),
the LDS-DMA kernel's 16-wide tiles, the grouped launches (csrc/conv_dma_group.hip) and the classifier head's
[M, 1, 1, K] GEMMs on the planner's automatic tile and split-K (section 9).

The method is test_conv_exact_gpu.py's: operands are small integers (x in [-3, 3], weights in [-2, 2] thinned
to about 96 taps, bias / residual / base in [-4, 4], masks from {-1, -0.0, 0, 1}), so every partial sum is an
integer below 2^24 and every result an integer a 16-bit float holds: the fp32 CPU path of ``ops.conv2d`` is
exact and a correct kernel reproduces it bit for bit (``torch.equal``, no tolerance anywhere in this file).

Every case comes from a cached plain builder (``_case`` / ``_pool``) that draws the operands, computes the CPU
reference and asserts the method's conditions on it before any GPU result exists; ``test_conditions`` (no GPU)
builds every case of every table. Every launch writes through a view of a sentinel-filled buffer (neighbour
channels and one image past the end) that must stay untouched, and every test asserts ``conv_route()`` (and
``bits_flags()`` where 1-bit masks ride along), so no case can turn into a test of its fallback. Kernels are
chosen by shape, by ``ops.conv.set_policy`` and by the per-launch ``DV_*`` switches.

Switches latched in a static at first use (DV_STREAM_P, DV_NO_PW, DV_PW_MIN_TILES, DV_PW_WG_PER_CU, DV_HS_MIN_W,
DV_HS_RING, DV_NO_SPLITK) cannot be changed inside the test process: their DEFAULTS are what is tested here
(strip variant P = 1, two persistent 1x1 workgroups per CU, halo-stream from 64 x 64 maps with a 3-slot ring,
automatic split-K on).

Cases whose grid must exceed the CU count take the count as a parameter: ``gpu_helpers.cus()`` on the GPU,
``G_NOMINAL`` in ``test_conditions``.
"""
import functools
import types

import numpy as np
import pytest
import torch

from deconv_api_amd import ops
from deconv_api_amd.ops import conv as Cm
from exact_helpers import (BF, DEV, HF, SENT, _check_exact, _check_ties, _dev, _expect, _gen, _geom, _ints, _launch,
                           _out_view, _policy, _pool_case, _pw_m, PW_H, _same, _signs, _untouched, _weights)
from gpu_helpers import cus as _cus, route as _route, tune as _tune

gpu = pytest.mark.gpu
G_NOMINAL = 256  # the CU count test_conditions builds the CU-following cases for
F32 = torch.float32


# ----------------------------------------------------------------------------------------
# case builder (CPU only) and launcher
# ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)  # (tests that share a case are neighbours; the large cases are not kept alive)
def _case(seed, N, H, W, C, OC, k=(3, 3), stride=1, pad=None, dt=BF, epi="bf16", relu=True, relu_in=False,
          amode="plain", div=1, mask=False, acc=False, out_hw=None, bias=True, emask=False, res=False, relu_cols=0,
          taps=96):
    """One conv problem on integer operands with its CPU reference and the method's conditions asserted.
    H, W: the conv's input map (for ``amode='unpool'`` the UNPOOLED map: x is [N, H/2, W/2, C])."""
    g = _gen(seed)
    kh, kw_ = k
    pad = (kh // 2, kw_ // 2) if pad is None else pad
    tr = amode == "transpose"
    kw = dict(stride=stride, pad=pad, relu=relu, relu_in=relu_in, in_mode=amode, epilogue=epi,
              use_bias=bias and not tr)
    if amode == "unpool":
        x = _ints(g, (N, H // 2, W // 2, C), -3, 3)
        code = torch.randint(0, 4, (N // div, H // 2, W // 2, C), generator=g, dtype=torch.uint8)
        kw.update(code=code, code_div=div)
        x_eff = Cm.unpool_ref(x, code, div)
    else:
        x = x_eff = _ints(g, (N, H, W, C), -3, 3)
    # (a stride-s transposed gather meets 1 / s^2 of the taps)
    cw = _weights(g, OC, C, kh, kw_, kind="transpose" if tr else "fwd", bias=bias and not tr,
                  taps=taps * stride * stride if tr else taps)
    if out_hw is not None:
        kw["out_hw"] = out_hw
    if mask:
        kw["mask"] = _signs(g, tuple(x.shape))
    if relu_cols:
        kw["relu_cols"] = relu_cols
    odt = F32 if epi == "f32" else dt
    plain = ops.conv2d(x, cw, **{**kw, "epilogue": "bf16" if epi == "pool" else epi})
    base = None
    extra = 4.0
    more = {}
    if res:
        more["res"] = _ints(g, tuple(plain.shape), -4, 4)
        extra += 4.0
    if acc:
        base = _ints(g, tuple(plain.shape), 1, 4) * torch.where(torch.rand(plain.shape, generator=g) < 0.5, -1.0, 1.0)
        extra += 4.0
    if res or acc:  # the unmasked result carries the conditions
        plain = ops.conv2d(x, cw, **kw, **more, **(dict(out=base.clone(), accumulate=True) if acc else {}))
    _check_exact(plain, odt, x_eff, cw, extra, stride=stride, pad=pad)
    if emask:
        more["emask"] = _signs(g, tuple(plain.shape))
    if epi == "pool":
        _check_ties(plain)
        ref = ops.conv2d(x, cw, **kw)
        _check_exact(ref[0], dt, x_eff, cw, extra, stride=stride, pad=pad)
    elif emask:
        ref = ops.conv2d(x, cw, **kw, **more, **(dict(out=base.clone(), accumulate=True) if acc else {}))
        assert bool((ref[more["emask"] <= 0] == 0).all()) and float((ref != 0).float().mean()) > 0.15
    else:
        ref = plain
    return types.SimpleNamespace(x=x, cw=cw, kw=kw, more=more, base=base, ref=ref, dt=dt, odt=odt, OC=OC, C=C, N=N,
                                 epi=epi)


def _bits_of(t):
    """packbits(t > 0): bit c % 8 of byte c / 8, rows = pixels."""
    return np.packbits((t.float() > 0).cpu().numpy().reshape(-1, t.shape[-1]), axis=1, bitorder="little")


# ----------------------------------------------------------------------------------------
# 1. conv_igemm (policy 'reg')
# ----------------------------------------------------------------------------------------

IG = {128: (128, 128), 64: (256, 40), 16: (256, 5)}  # tile width BN -> (BM, OC)
IG_C = {128: 24, 64: 8, 16: 64}                       # the input width each tile's M matrix runs at


def _ig_tile_args(bn, which, epi):
    BM, OC = IG[bn]
    M = ((BM - 4, BM + 4, 2 * BM + 8) if epi == "pool" else (BM - 1, BM + 1, 2 * BM + 7))[which]
    N, OH, OW, crop = _geom(M, even=epi == "pool")
    assert N * OH * OW == M
    return dict(seed=bn + which, N=N, H=OH + 2 if crop else OH, W=OW, C=IG_C[bn], OC=OC, pad=(0, 1) if crop else (1, 1),
                epi=epi, relu=epi != "f32")


IG_TILES = [(bn, which, epi) for bn in IG for which in range(3) for epi in ("bf16", "f32", "pool")]


@gpu
@pytest.mark.parametrize("bn,which,epi", IG_TILES)
def test_igemm_tiles(native_lib, bn, which, epi):
    """All three tile shapes (128x128, 256x64 with columns past OC = 40, 256x16 with OC = 5) at M = BM - 1,
    BM + 1 and 2 BM + 7 rows (the pool epilogue at the multiples of 4 next to them), with the 16-bit, fp32 and
    fused-pool epilogues (windows full of ties, switch codes exact), C = 24 / 8 / 64."""
    c = _case(**_ig_tile_args(bn, which, epi))
    got, r, _ = _launch(c, "reg")
    assert r == f"igemm {IG[bn][0]}x{bn}", r
    _expect(c, got)


IG_KERNELS = [((3, 3), 1, (1, 1)), ((1, 1), 1, (0, 0)), ((1, 7), 1, (0, 3)), ((5, 5), 2, (2, 2))]
IG_K = [(C, ki, (128, 64, 16)[(ci + ki) % 3]) for ci, C in enumerate((8, 24, 64)) for ki in range(4)]


def _ig_k_args(C, ki, bn):
    k, stride, pad = IG_KERNELS[ki]
    return dict(seed=100 + C + ki, N=3, H=13, W=15, C=C, OC=IG[bn][1], k=k, stride=stride, pad=pad)


@gpu
@pytest.mark.parametrize("C,ki,bn", IG_K)
def test_igemm_k_gather(native_lib, C, ki, bn):
    """The K gather at C = 8 (eight taps per K tile; 3x3: K = 72 padded to 128, the kh < KH guard live), C = 24
    (K tiles straddle taps) and C = 64, for 3x3 pad 1, 1x1, 1x7 pad (0, 3) and 5x5 stride 2."""
    c = _case(**_ig_k_args(C, ki, bn))
    got, r, _ = _launch(c, "reg")
    assert r == f"igemm {IG[bn][0]}x{bn}", r
    _expect(c, got)


# name -> (case arguments, launch arguments, policies, tile width)
IG_MODES = {
    "fp16_fwd": (dict(seed=201, N=3, H=13, W=15, C=24, OC=128, dt=HF), {}, ("reg",), 128),
    "fp16_transpose": (dict(seed=202, N=2, H=8, W=9, C=64, OC=40, dt=HF, amode="transpose", stride=2, pad=(1, 1),
                            out_hw=(16, 18), relu=False), {}, ("reg",), 64),
    "acc_16bit": (dict(seed=203, N=3, H=13, W=15, C=64, OC=40, acc=True), {}, ("reg",), 64),
    "acc_f32": (dict(seed=204, N=3, H=13, W=15, C=8, OC=5, acc=True, epi="f32", relu=False), {}, ("reg",), 16),
    "acc_fp16": (dict(seed=205, N=3, H=13, W=15, C=24, OC=128, acc=True, dt=HF, relu=False), {}, ("reg",), 128),
    "relu_in": (dict(seed=206, N=3, H=13, W=15, C=64, OC=128, relu_in=True), {}, ("reg",), 128),
    "relu_in_f32": (dict(seed=207, N=3, H=13, W=15, C=24, OC=16, relu_in=True, epi="f32"), {}, ("reg",), 16),
    # MASK_IN: the mask a channel slice of a wider buffer (mask_ld != x_ld: igemm under 'auto' too)
    "mask_fwd_bf16": (dict(seed=210, N=3, H=13, W=15, C=64, OC=128, mask=True, relu=False, bias=False),
                      dict(mask_extra=8), ("reg", "auto"), 128),
    "mask_fwd_fp16": (dict(seed=211, N=3, H=13, W=15, C=24, OC=40, mask=True, relu=False, bias=False, dt=HF),
                      dict(mask_extra=16, x_extra=8), ("reg", "auto"), 64),
    "mask_tr_bf16": (dict(seed=212, N=2, H=8, W=9, C=64, OC=16, mask=True, amode="transpose", stride=2, pad=(1, 1),
                          out_hw=(16, 18), relu=False), dict(mask_extra=8), ("reg", "auto"), 16),
    "mask_tr_fp16": (dict(seed=213, N=2, H=8, W=9, C=64, OC=128, mask=True, amode="transpose", stride=2, pad=(1, 1),
                          out_hw=(16, 18), relu=False, dt=HF), dict(mask_extra=8), ("reg", "auto"), 128),
    # f32 epilogue + mask: no LDS-DMA kernel has it, whatever the mask's stride
    "mask_f32": (dict(seed=214, N=3, H=13, W=15, C=64, OC=40, mask=True, relu=False, epi="f32"), {}, ("reg", "auto"), 64),
    # CONV_A_UNPOOL: code_div 1 / 2 / 3 (N a multiple), relu_in on / off, x_ld > C
    "unpool_div1": (dict(seed=220, N=6, H=10, W=12, C=64, OC=40, amode="unpool", relu_in=True, bias=False), {},
                    ("reg",), 64),
    "unpool_div2_f32": (dict(seed=221, N=6, H=10, W=12, C=64, OC=16, amode="unpool", div=2, epi="f32", bias=False), {},
                        ("reg",), 16),
    "unpool_div3_wide": (dict(seed=222, N=6, H=10, W=12, C=24, OC=128, amode="unpool", div=3, relu_in=True, bias=False),
                         dict(x_extra=8), ("reg",), 128),
    "unpool_f32_wide": (dict(seed=223, N=6, H=10, W=12, C=64, OC=40, amode="unpool", div=2, relu_in=True, epi="f32"),
                        dict(x_extra=16), ("reg",), 64),
    # CONV_A_TRANSPOSE: stride 2 with pad (1, 1), and with pad 0 and an odd out_hw
    "transpose_p1": (dict(seed=230, N=2, H=8, W=9, C=64, OC=128, amode="transpose", stride=2, pad=(1, 1),
                          out_hw=(16, 18), relu=False), {}, ("reg",), 128),
    "transpose_p0_odd": (dict(seed=231, N=2, H=8, W=9, C=24, OC=16, amode="transpose", stride=2, pad=(0, 0),
                              out_hw=(17, 19), relu=False), {}, ("reg",), 16),
}


@gpu
@pytest.mark.parametrize("name", sorted(IG_MODES))
def test_igemm_modes(native_lib, name):
    """fp16 forward and transposed, accumulate into 16-bit and fp32 outputs, relu_in on signed inputs, MASK_IN
    (mask from {-1, -0.0, 0, 1} with its own pixel stride, forward and stride-2 transposed, both dtypes, one fp32
    epilogue; these reach igemm under policy 'auto' as well), the fused unpool gather (code_div 1 / 2 / 3,
    relu_in on and off, x_ld > C) and the stride-2 transposed gather (pad (1, 1); pad 0 with an odd out_hw)."""
    args, largs, policies, bn = IG_MODES[name]
    c = _case(**args)
    for policy in policies:
        got, r, _ = _launch(c, policy, **largs)
        assert r == f"igemm {IG[bn][0]}x{bn}", (policy, r)
        _expect(c, got)


# ----------------------------------------------------------------------------------------
# 2. halo-tile kernels (csrc/conv_smalln.hip)
# ----------------------------------------------------------------------------------------

STRIPS = [
    # N, H, W, OC, epilogue, relu_in, channels right of the view (0: dense rows)
    (2, 3, 34, 3, "f32", True, 0),     # W & 3 != 0: scalar stores on a dense fp32 / OC 3 row
    (2, 9, 36, 5, "bf16", False, 8),   # one full strip + a 4-px strip
    (2, 16, 64, 16, "f32", False, 8),
    (3, 9, 100, 3, "bf16", True, 8),
    (2, 16, 64, 3, "f32", True, 0),    # fp32 / OC 3 / dense: the staged vector-store path
    (2, 16, 64, 3, "f32", True, 5),    # the same through a wider row
    (2, 3, 36, 16, "bf16", True, 8),
    (2, 16, 100, 5, "f32", False, 0),
]


def _strips_args(N, H, W, OC, epi, relu_in, right):
    return dict(seed=300 + H + W + OC, N=N, H=H, W=W, C=64, OC=OC, epi=epi, relu_in=relu_in)


@gpu
@pytest.mark.parametrize("N,H,W,OC,epi,relu_in,right", STRIPS)
def test_halo_strips(native_lib, N, H, W, OC, epi, relu_in, right):
    """conv3x3_c64_stream_kernel (row strips of 32 px; DV_STREAM_P's default variant): OC 3 / 5 / 16, 16-bit and
    fp32 epilogues, relu_in on and off, W = 34 / 36 / 64 / 100, H = 3 / 9 / 16, N >= 2."""
    c = _case(**_strips_args(N, H, W, OC, epi, relu_in, right))
    got, r, _ = _launch(c, "halo", right=right)
    assert r == "halo_v1 strips", r
    _expect(c, got)


def _stats_args(div):
    return dict(seed=340 + div, N=4, H=9, W=64, C=64, OC=3, epi="f32")


def _stats_ref(c, div):
    y = c.ref.double().reshape(c.N // div, -1)
    return torch.stack([y.sum(1), (y * y).sum(1)], dim=1)


@gpu
@pytest.mark.parametrize("policy,route", [("halo", "halo_v1 strips"), ("dma", "dma 256x16 st2 ks")])
@pytest.mark.parametrize("div", [1, 2, 4])
def test_conv_stats(native_lib, div, policy, route):
    """{sum, sum of squares} of each group of stats_div output images, from the strip kernel's own fp64
    accumulation and from the generic recon_stats pass behind the LDS-DMA kernel: the outputs are integers, so
    both sums are exact in fp64 in any order; the buffer's initial garbage is overwritten."""
    c = _case(**_stats_args(div))
    stats = torch.full((c.N // div, 2), 12345.0, dtype=torch.float64, device=DEV)
    got, r, _ = _launch(c, policy, right=0, stats=stats, stats_div=div)
    assert r.startswith(route), r
    _expect(c, got)
    assert torch.equal(stats.cpu(), _stats_ref(c, div)), (stats.cpu(), _stats_ref(c, div))


PERSIST = {
    # name -> (case arguments, channels right of the view): <FN, EPI, UNPOOL> of conv3x3_c64_persist_kernel
    "narrow16_unpool_bf16": (dict(seed=401, N=2, H=18, W=34, C=64, OC=16, amode="unpool", relu_in=True, bias=False), 8),
    "narrow3_unpool_f32": (dict(seed=402, N=2, H=8, W=30, C=64, OC=3, amode="unpool", div=2, epi="f32", bias=False), 8),
    "oc48_plain_bf16": (dict(seed=403, N=2, H=7, W=30, C=64, OC=48), 8),
    "oc48_unpool_bf16": (dict(seed=404, N=2, H=10, W=66, C=64, OC=48, amode="unpool", relu_in=True, bias=False), 8),
    "oc64_plain_f32": (dict(seed=405, N=2, H=9, W=34, C=64, OC=64, epi="f32", relu_in=True), 8),
    "oc64_plain_bf16": (dict(seed=406, N=1, H=17, W=66, C=64, OC=64), 8),
    "oc64_unpool_f32": (dict(seed=407, N=2, H=18, W=30, C=64, OC=64, amode="unpool", epi="f32", bias=False), 8),
    # out_ld % 8 != 0 (a 64-channel slice of a 68-channel buffer): v1 instead of v2
    "oc64_unpool_ld68": (dict(seed=408, N=2, H=10, W=34, C=64, OC=64, amode="unpool", relu_in=True, bias=False), 4),
}


@gpu
@pytest.mark.parametrize("name", sorted(PERSIST))
def test_halo_persist(native_lib, name):
    """conv3x3_c64_persist_kernel (8 x 32 tiles, weights in LDS) in every reachable <FN, EPI, UNPOOL>: narrow +
    unpool (OC 16, OC 3), OC 48 plain and unpool, OC 64 fp32, and OC 64 unpool through a row with out_ld % 8 != 0;
    ragged tiles in H and W."""
    args, right = PERSIST[name]
    c = _case(**args)
    got, r, _ = _launch(c, "halo", right=right)
    assert r == "halo_v1 persist", r
    _expect(c, got)


def _persist_walk_args(G):
    return dict(seed=410, N=(6 * G // 5) // 54 + 1, H=66, W=190, C=64, OC=64)  # 9 x 6 tiles per image


@gpu
def test_halo_persist_two_tiles(native_lib):
    """More tiles than CUs (the batch follows the CU count): some workgroups walk two tiles."""
    G = _cus()
    args = _persist_walk_args(G)
    assert G < args["N"] * 54 < 2 * G
    c = _case(**args)
    got, r, _ = _launch(c, "halo")
    assert r == "halo_v1 persist", r
    _expect(c, got)


HALO_V2 = [
    # N, H, W, code_div, relu_in, channels left / right of the view (row stride % 8 == 0)
    (1, 18, 34, 1, True, 0, 8),
    (4, 10, 6, 2, False, 0, 0),
    (4, 10, 6, 4, True, 8, 8),
    (2, 18, 34, 2, False, 8, 16),
]


def _v2_args(N, H, W, div, relu_in):
    return dict(seed=420 + N + H + div, N=N, H=H, W=W, C=64, OC=64, amode="unpool", div=div, relu_in=relu_in, bias=False)


@gpu
@pytest.mark.parametrize("N,H,W,div,relu_in,left,right", HALO_V2)
def test_halo_v2(native_lib, N, H, W, div, relu_in, left, right):
    """conv3x3_unpool_c64_v2_kernel<false>: even maps with ragged tiles (18 x 34, 10 x 6), code_div 1 / 2 / 4,
    relu_in on and off, channel-slice outputs with 16-B aligned rows."""
    c = _case(**_v2_args(N, H, W, div, relu_in))
    got, r, _ = _launch(c, "halo", left=left, right=right)
    assert r == "halo_v2", r
    _expect(c, got)


def _v2_walk_args(G):
    return dict(seed=430, N=2 * ((G // 6 + 8) // 2), H=18, W=34, C=64, OC=64, amode="unpool", div=2, relu_in=True,
                bias=False)  # 3 x 2 tiles per image


@gpu
def test_halo_v2_two_tiles(native_lib):
    """halo_v2 on a grid larger than the CU count (the batch follows it)."""
    G = _cus()
    args = _v2_walk_args(G)
    assert G < args["N"] * 6 < 2 * G
    c = _case(**args)
    got, r, _ = _launch(c, "halo")
    assert r == "halo_v2", r
    _expect(c, got)


C8 = [(2, 56, 64, 64, 0, 0), (2, 57, 58, 64, 0, 8), (2, 57, 58, 24, 8, 8)]  # N, H, W, OC, left, right


def _c8_args(N, H, W, OC):
    return dict(seed=440 + H + OC, N=N, H=H, W=W, C=8, OC=OC)


@gpu
@pytest.mark.parametrize("N,H,W,OC,left,right", C8)
def test_c8_stream(native_lib, N, H, W, OC, left, right):
    """conv3x3_c8_stream_kernel (the first layer, maps >= 56 x 56): the FULL instantiation (56 x 64, OC 64) and the
    ragged one (57 x 58, OC 64 and 24), all eight input channels non-zero, N = 2, channel-slice outputs."""
    c = _case(**_c8_args(N, H, W, OC))
    assert bool((c.x.abs().sum(dim=(0, 1, 2)) > 0).all())
    got, r, _ = _launch(c, "auto", left=left, right=right)
    assert r == "c8_stream", r
    _expect(c, got)


@functools.lru_cache(maxsize=4)
def _pool(seed, N, H, W, C, OC):
    x, cw, rp, rc = _pool_case(_gen(seed), N, H, W, C, OC)
    return types.SimpleNamespace(x=x, cw=cw, kw=dict(relu=True, epilogue="pool"), more={}, base=None, ref=(rp, rc), dt=BF,
                                 odt=BF, OC=OC, C=C, N=N, epi="pool")


def _pool_v3_n(G):
    return G // 60 + 1  # 15 x 4 tiles per 114 x 116 image


@gpu
@pytest.mark.parametrize("walk", [False, True], ids=["ragged", "two_tiles"])
def test_pool_v3(native_lib, walk):
    """conv3x3_c64_pool_v3_kernel on a ragged map (114 x 116: a 2-row and a 20-px tile edge), one image and a
    batch with more tiles than CUs, on tie-rich windows: values and first-max switch codes exact."""
    G = _cus()
    N = _pool_v3_n(G) if walk else 1
    assert not walk or G < N * 60 < 2 * G
    c = _pool(450, N, 114, 116, 64, 64)
    got, r, _ = _launch(c, "auto")
    assert r == "pool_v3", r
    _expect(c, got)


# ----------------------------------------------------------------------------------------
# 3. halo-stream kernels (csrc/conv_halo_stream.hip), policy 'auto'
# ----------------------------------------------------------------------------------------

HS = [
    # N, H, W, C, OC, dtype, pad, DV_HS16_EPI=reg, route
    (2, 64, 64, 32, 64, BF, 1, False, "hs16 oc64 lds"),
    (2, 64, 80, 64, 128, HF, 1, False, "hs16 oc128 lds"),
    (2, 64, 64, 96, 64, HF, 1, True, "hs16 oc64 reg"),
    (2, 64, 80, 96, 128, BF, 1, True, "hs16 oc128 reg"),
    (2, 64, 64, 32, 36, HF, 1, False, "hs16 oc64 reg"),    # OC % 8 != 0: the register epilogue by itself
    (2, 64, 80, 64, 100, BF, 1, False, "hs16 oc128 reg"),
    (2, 70, 66, 32, 64, BF, 1, False, "hs32 oc64 lds"),    # C == 32, OCpad == 64: the single-halo-buffer variant
    (2, 70, 66, 32, 64, HF, 1, True, "hs32 oc64 reg"),
    (2, 65, 97, 64, 128, HF, 1, False, "hs32 oc128 lds"),
    (2, 70, 66, 96, 64, HF, 1, False, "hs32 oc64 lds"),
    (2, 70, 66, 96, 128, BF, 1, True, "hs32 oc128 reg"),
    (2, 70, 66, 32, 36, HF, 1, False, "hs32 oc64 reg"),
    (2, 65, 97, 64, 100, BF, 1, False, "hs32 oc128 reg"),
    # pad 0 and pad 2: 66 x 66 -> 64 x 64, 62 x 78 -> 64 x 80 (hs16); 72 x 68 -> 70 x 66, 63 x 95 -> 65 x 97 (hs32).
    # (The dispatch tests the INPUT map against DV_HS_MIN_W: a 62 x 62 input stays on the LDS-DMA kernel.)
    (2, 66, 66, 32, 64, BF, 0, False, "hs16 oc64 lds"),
    (2, 62, 78, 64, 128, HF, 2, False, "hs16 oc128 lds"),
    (2, 72, 68, 64, 64, HF, 0, False, "hs32 oc64 lds"),
    (2, 63, 95, 32, 128, BF, 2, False, "hs32 oc128 lds"),
]


def _hs_args(N, H, W, C, OC, dt, pad):
    return dict(seed=500 + H + C + OC + pad, N=N, H=H, W=W, C=C, OC=OC, dt=dt, pad=(pad, pad))


@gpu
@pytest.mark.parametrize("N,H,W,C,OC,dt,pad,reg,route", HS)
def test_halo_stream_plain(native_lib, monkeypatch, N, H, W, C, OC, dt, pad, reg, route):
    """hs16 (outputs % 16) and hs32 with the plain 16-bit epilogues: LDS-staged, register (forced by
    DV_HS16_EPI=reg and reached by OC % 8 != 0), bf16 and fp16, OCpad 64 and 128, C = 32 / 64 / 96, pad 0 / 1 / 2
    (DV_HS_MIN_W and DV_HS_RING at their defaults)."""
    if reg:
        monkeypatch.setenv("DV_HS16_EPI", "reg")
    c = _case(**_hs_args(N, H, W, C, OC, dt, pad))
    got, r, bits = _launch(c, "auto")
    assert r == route and bits == 0, (r, bits)
    _expect(c, got)


HS_SPLIT = [
    # N, H, W, C, OC, dtype, emask, x_extra, left, right, route
    (1, 64, 64, 96, 192, BF, False, 0, 0, 8, "hs16 oc64 lds ocsplit"),
    (1, 64, 64, 96, 192, BF, True, 8, 8, 8, "hs16 oc64 lds ocsplit"),
    (1, 64, 64, 32, 160, HF, False, 8, 8, 16, "hs16 oc64 lds ocsplit"),   # second half 32 wide
    (1, 64, 64, 32, 160, HF, True, 0, 0, 0, "hs16 oc64 lds ocsplit"),
    (1, 70, 66, 32, 256, BF, False, 8, 0, 8, "hs32 oc128 lds ocsplit"),
    (1, 70, 66, 32, 256, HF, True, 0, 8, 8, "hs32 oc128 lds ocsplit"),
]


def _hs_split_args(N, H, W, C, OC, dt, emask):
    return dict(seed=540 + H + OC + emask, N=N, H=H, W=W, C=C, OC=OC, dt=dt, emask=emask, relu=not emask)


@gpu
@pytest.mark.parametrize("N,H,W,C,OC,dt,emask,x_extra,left,right,route", HS_SPLIT)
def test_halo_stream_ocsplit(native_lib, N, H, W, C, OC, dt, emask, x_extra, left, right, route):
    """192 / 256 padded output channels as two launches over the channel halves: OC 192, 160 (second half 32
    wide) and 256, with and without emask, channel-slice input and output; no 1-bit masks on this form."""
    c = _case(**_hs_split_args(N, H, W, C, OC, dt, emask))
    extra = {}
    if emask:  # offered, and ignored by the channel-split form: the 16-bit emask applies
        extra["ebits"] = torch.from_numpy(_bits_of(c.more["emask"])).to(DEV) if left == right == 0 else None
    got, r, bits = _launch(c, "auto", x_extra=x_extra, left=left, right=right, **extra)
    assert r == route and bits == 0, (r, bits)
    _expect(c, got)


HS_BITS = [(1, 64, 64, 32, 64, BF, "hs16 oc64"), (1, 64, 80, 64, 128, HF, "hs16 oc128"),
           (1, 70, 66, 32, 64, HF, "hs32 oc64"), (1, 65, 97, 64, 128, BF, "hs32 oc128")]


def _bits_args(N, H, W, C, OC, dt, k=(3, 3)):
    fwd = dict(seed=560 + H + OC, N=N, H=H, W=W, C=C, OC=OC, dt=dt, k=k)
    return fwd, dict(fwd, seed=561 + H + OC, emask=True, relu=False)


def _check_bits(c, cm, route, reg_route, monkeypatch):
    """obits of the forward case ``c``, ebits in place of the emask of ``cm``; with ``reg_route`` also the
    register epilogue, which takes neither."""
    M = c.ref.numel() // c.OC
    ob = torch.full((M, c.OC // 8), 0xA5, dtype=torch.uint8, device=DEV)
    got, r, bits = _launch(c, "auto", right=0, obits=ob)
    assert r == route and bits == 1, (r, bits)
    _expect(c, got)
    assert np.array_equal(ob.cpu().numpy(), _bits_of(c.ref)), "obits != packbits(reference > 0)"
    eb = torch.from_numpy(_bits_of(cm.more["emask"])).to(DEV)
    got, r, bits = _launch(cm, "auto", right=0, ebits=eb)
    assert r == route and bits == 2, (r, bits)
    _expect(cm, got)
    if reg_route:
        monkeypatch.setenv("DV_HS16_EPI", "reg")
        ob.fill_(0xA5)
        got, r, bits = _launch(cm, "auto", right=0, ebits=eb, obits=ob)
        assert r == reg_route and bits == 0, (r, bits)
        _expect(cm, got)
        assert bool((ob == 0xA5).all())


@gpu
@pytest.mark.parametrize("N,H,W,C,OC,dt,route", HS_BITS)
def test_halo_stream_bits(native_lib, monkeypatch, N, H, W, C, OC, dt, route):
    """1-bit masks on the LDS-staged epilogues: obits == packbits(reference > 0) (bit c % 8 of byte c / 8),
    the result under ebits == the CPU reference under the 16-bit emask, bits_flags() 1 and 2; 0 on the register
    epilogue, with emask still applied and obits unwritten."""
    fwd, msk = _bits_args(N, H, W, C, OC, dt)
    _check_bits(_case(**fwd), _case(**msk), route + " lds", route + " reg", monkeypatch)


# ----------------------------------------------------------------------------------------
# 4. persistent 1x1 (csrc/conv_pw.hip)
# ----------------------------------------------------------------------------------------

PW = {
    # name -> (C, OC, dtype, case options, x_extra)
    "relu_bias_oc128": (64, 128, BF, {}, 0),
    "relu_bias_oc192_k3": (192, 192, HF, {}, 8),          # 256x64 tile, three column tiles, three K tiles
    "res_oc256": (64, 256, HF, dict(res=True), 0),        # ReLU after the add
    "accumulate_oc64": (64, 64, BF, dict(acc=True, relu=False), 8),
    "accumulate_emask_oc128": (64, 128, HF, dict(acc=True, emask=True, relu=False), 0),
    "relu_cols_oc128_k3": (192, 128, BF, dict(relu_cols=40), 0),
    "relu_cols_oc64": (64, 64, HF, dict(relu_cols=24), 0),
}


def _pw_args(name, G):
    C, OC, dt, opts, _ = PW[name]
    return dict(seed=600 + len(name) + OC, N=1, H=PW_H, W=_pw_m(G, OC)[0] // PW_H, C=C, OC=OC, dt=dt, k=(1, 1), **opts)


@gpu
@pytest.mark.parametrize("name", sorted(PW))
def test_pw_epilogues(native_lib, name):
    """The persistent 1x1 kernel on both tiles (128x128: OC 128 / 256; 256x64: OC 64 / 192) with about 2.25
    tiles per CU and an M tail (M follows the CU count; DV_PW_WG_PER_CU's default of two workgroups per CU), C = 64
    (one K tile) and 192 (the two-stage ring crosses tile boundaries), both dtypes, x as a channel slice: ReLU +
    bias, res (ReLU after the add), accumulate, accumulate + emask, relu_cols (columns below the boundary
    clamped, the others signed)."""
    G = _cus()
    c = _case(**_pw_args(name, G))
    _, BM, BN = _pw_m(G, PW[name][1])
    if "relu_cols" in c.kw:
        rc = c.kw["relu_cols"]
        assert bool((c.ref[..., :rc] >= 0).all()) and bool((c.ref[..., rc:] < 0).any())
    got, r, _ = _launch(c, "auto", x_extra=PW[name][4])
    assert r == f"pw {BM}x{BN}", r
    _expect(c, got)


PW_OUT2 = [(256, 128, BF), (192, 64, HF), (128, 40, BF)]  # OC, split_col, dtype


def _pw_out2_args(G, OC, dt):
    return dict(seed=630 + OC, N=1, H=PW_H, W=_pw_m(G, OC)[0] // PW_H, C=64, OC=OC, dt=dt, k=(1, 1))


@gpu
@pytest.mark.parametrize("OC,split,dt", PW_OUT2)
def test_pw_out2(native_lib, OC, split, dt):
    """out2 / split_col: channels >= split_col to a second tensor, both destinations channel slices between
    sentinels (split on a tile boundary, on a 64-column tile boundary, and inside a tile)."""
    G = _cus()
    M, BM, BN = _pw_m(G, OC)
    c = _case(**_pw_out2_args(G, OC, dt))
    b1 = torch.full((1, PW_H, M // PW_H, split + 16), SENT, dtype=dt, device=DEV)
    b2 = torch.full((1, PW_H, M // PW_H, OC - split + 16), SENT, dtype=dt, device=DEV)
    ops.conv2d(_dev(c.x, dt), c.cw.to_device(DEV, dt), out=b1[..., 8: 8 + split], out2=b2[..., 8: 8 + OC - split],
               split_col=split, **c.kw)
    assert _route() == f"pw {BM}x{BN}", _route()
    _same(b1[..., 8: 8 + split], c.ref[..., :split])
    _same(b2[..., 8: 8 + OC - split], c.ref[..., split:])
    for b, w in ((b1, split), (b2, OC - split)):
        assert bool((b[..., :8] == SENT).all()) and bool((b[..., 8 + w:] == SENT).all()), "wrote outside the views"


@gpu
@pytest.mark.parametrize("OC,dt", [(128, BF), (64, HF)])
def test_pw_bits(native_lib, monkeypatch, OC, dt):
    """obits / ebits on the persistent 1x1 kernel, as on the halo-stream kernels."""
    G = _cus()
    M, BM, BN = _pw_m(G, OC)
    fwd, msk = _bits_args(1, PW_H, M // PW_H, 64, OC, dt, k=(1, 1))
    _check_bits(_case(**fwd), _case(**msk), f"pw {BM}x{BN}", None, monkeypatch)


# ----------------------------------------------------------------------------------------
# 5. LDS-DMA leftovers: the 16-wide tiles, grouped launches
# ----------------------------------------------------------------------------------------

DMA16 = [
    # name, case arguments: few rows -> dma 256x16 (K = 576: nine K tiles, the automatic split-K takes 2)
    ("oc3_bf16", dict(seed=701, N=2, H=9, W=11, C=64, OC=3)),
    ("oc16_f32", dict(seed=702, N=2, H=9, W=11, C=64, OC=16, epi="f32", relu=False)),
    ("oc16_fp16", dict(seed=703, N=3, H=11, W=9, C=64, OC=16, dt=HF)),
    ("oc5_mask", dict(seed=704, N=2, H=9, W=11, C=64, OC=5, mask=True, relu=False, bias=False)),
    ("oc16_mask_fp16", dict(seed=705, N=2, H=9, W=11, C=64, OC=16, mask=True, relu=False, bias=False, dt=HF)),
]


@gpu
@pytest.mark.parametrize("auto_ks", [False, True], ids=["ks1", "auto"])
@pytest.mark.parametrize("name,args", DMA16, ids=[d[0] for d in DMA16])
def test_dma_256x16(native_lib, name, args, auto_ks):
    """The 256 x 16 tile by its natural route (OC 3 / 5 / 16, few rows), plain and masked, 16-bit and fp32
    epilogues, without split-K and with the automatic one (2 for K = 576 on an idle device; DV_NO_SPLITK unset)."""
    c = _case(**args)
    with _tune(0, 0 if auto_ks else 1):
        got, r, _ = _launch(c, "dma")
    assert r == f"dma 256x16 st2 ks{2 if auto_ks else 1}" + (" mask" if "mask" in c.kw else ""), r
    _expect(c, got)


def _dma512_args(G, epi):
    return dict(seed=710, N=-(-512 * G // 400) + 1, H=20, W=20, C=64, OC=16, epi=epi, relu=epi != "f32")


@gpu
@pytest.mark.parametrize("epi", ["bf16", "f32"])
def test_dma_512x16(native_lib, epi):
    """The 512 x 16 tile: M >= 512 CUs rows (the batch follows the CU count), K = 576, with an M tail."""
    c = _case(**_dma512_args(_cus(), epi))
    got, r, _ = _launch(c, "dma")
    assert r == "dma 512x16 st2 ks1", r
    _expect(c, got)


GROUPS = {
    # name -> (cfg, problems: case arguments without the dtype)
    "cfg3": (3, [dict(seed=801, N=15, H=40, W=40, C=32, OC=128),
                 dict(seed=802, N=15, H=40, W=40, C=64, OC=128, k=(1, 1), relu=False),
                 dict(seed=803, N=8, H=40, W=40, C=64, OC=256, k=(1, 7), pad=(0, 3)),
                 dict(seed=804, N=15, H=40, W=40, C=32, OC=128, emask=True, relu=False)]),
    "transpose": (8, [dict(seed=811, N=2, H=8, W=9, C=64, OC=32, amode="transpose", stride=2, pad=(1, 1), out_hw=(16, 18),
                           relu=False),
                      dict(seed=812, N=2, H=8, W=9, C=32, OC=64, amode="transpose", stride=2, pad=(0, 0), out_hw=(17, 19),
                           relu=False),
                      dict(seed=813, N=3, H=7, W=7, C=64, OC=96, amode="transpose", stride=2, pad=(1, 1), out_hw=(14, 14),
                           relu=False),
                      dict(seed=814, N=1, H=9, W=8, C=128, OC=40, amode="transpose", stride=2, pad=(1, 1), out_hw=(18, 16),
                           relu=False)]),
    "unaligned": (8, [dict(seed=821, N=2, H=9, W=11, C=24, OC=40),   # C % 64 != 0: the aligned == false instantiation
                      dict(seed=822, N=2, H=9, W=11, C=64, OC=96),
                      dict(seed=823, N=2, H=11, W=9, C=64, OC=64, k=(1, 1)),
                      dict(seed=824, N=3, H=9, W=9, C=128, OC=128, acc=True, relu=False)]),
}


@gpu
@pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("name", sorted(GROUPS))
def test_dma_groups(native_lib, name, n, dt):
    """Grouped launches against the CPU oracle: a cfg 3 group (128-wide problems with M OCpad > 3e6, K < 1024),
    a transposed-gather group and a group with one C % 64 != 0 problem, 1 and 4 problems per group, both
    dtypes: 'group cfgN' at record time, outputs checked after conv_group_end()."""
    cfg, probs = GROUPS[name]
    cases = [_case(**p, dt=dt) for p in probs[:n]]
    lib = ops.native.lib()
    held = []
    with _policy("auto"):
        lib.conv_group_begin()
        try:
            for c in cases:
                kw = dict(c.kw)
                for key, v in c.more.items():
                    kw[key] = _dev(v, dt)
                buf, view = _out_view(tuple(c.ref.shape), dt, 8, 8)
                if c.base is not None:
                    view.copy_(_dev(c.base, dt))
                    kw["accumulate"] = True
                xd, cwd = _dev(c.x, dt), c.cw.to_device(DEV, dt)
                ops.conv2d(xd, cwd, out=view, **kw)
                assert _route() == f"group cfg{cfg}", _route()
                held.append((buf, view, xd, cwd, kw))
        finally:
            launches = lib.conv_group_end()
    assert launches == 1, launches
    for c, (buf, view, *_rest) in zip(cases, held):
        _same(view, c.ref)
        assert _untouched(buf, tuple(c.ref.shape), 8), "wrote outside the output view"


# ----------------------------------------------------------------------------------------
# 9. the classifier head's GEMMs: [M, 1, 1, K] rows on the LDS-DMA kernel, automatic tile and split-K
# ----------------------------------------------------------------------------------------
# VGG16Runtime packs fc1 / fc2 / predictions as 1x1 ConvWeights (models/vgg16.py); the engine runs them with
# M = B rows going up and M = B K_filters rows coming down (engine/deconvnet.py _dense_up, backward). The planner
# (csrc/conv_dma_plan.h auto_cfg, splitk) gives M OCpad <= 3e6 the 64 x 64 st3 tile and, up to small_splitk_mn =
# 300 000, split-K 2 (16..19 K tiles) or 4 (>= 20); neither rule reads the CU count. Nothing is forced here.

def _dn(seed, M, K, OC, **kw):
    return dict(seed=seed, N=M, H=1, W=1, C=K, OC=OC, k=(1, 1), **kw)


_DOWN = dict(bias=False, epi="f32")
DENSE = {
    # name: (case arguments without the dtype, route)
    # fc1 / fc2 up: bias + ReLU, 16-bit. K = 1344 is 21 K tiles: split-K 4 with parts of 6, 5, 5, 5
    **{f"up_m{M}_k{K}": (_dn(900 + M + K, M, K, 192), "dma 64x64 st3 ks4") for M in (1, 3, 4) for K in (1344, 4096)},
    # predictions up: fp32 logits, no ReLU, OC 1000 < OCpad 1024: bias and columns past 1000 untouched
    **{f"pred_up_m{M}": (_dn(910 + M, M, 4096, 1000, epi="f32", relu=False), "dma 64x64 st3 ks4") for M in (1, 5)},
    # predictions down: K = 1000 -> Kpad 1024, 16 K tiles: split-K 2, the K tail inside every row
    **{f"pred_down_m{M}_relu{int(r)}": (_dn(920 + M + r, M, 1000, 4096, relu=r, **_DOWN), "dma 64x64 st3 ks2")
       for M in (4, 12) for r in (True, False)},
    "fc_down_m12": (_dn(930, 12, 4096, 256, **_DOWN), "dma 64x64 st3 ks4"),
    # the batch-size flips: M OCpad either side of small_splitk_mn (split-K 4 -> none) ...
    "flip_splitk_below": (_dn(940, 73, 1344, 4096, **_DOWN), "dma 64x64 st3 ks4"),
    "flip_splitk_above": (_dn(941, 74, 1344, 4096, **_DOWN), "dma 64x64 st3 ks1"),
    # ... and of auto_cfg's 3 000 000 (the 64 x 64 tile -> 128 x 128; K = 256 is 4 K tiles: no split-K)
    "flip_tile_below": (_dn(942, 119, 256, 25088, **_DOWN), "dma 64x64 st3 ks1"),
    "flip_tile_above": (_dn(943, 128, 256, 25088, **_DOWN), "dma 128x128 st2 ks1"),
}
# the real fc1 shapes, bf16 only: name -> (M, K, OC, keep 1 weight in ``thin``, route). fc1.down's 102 760 448
# weights put B's row offsets past 2^27 elements; its M OCpad = 401 408 is past small_splitk_mn: no split-K
DENSE_REAL = {"fc1_up": (4, 25088, 4096, 256, "dma 64x64 st3 ks4"), "fc1_down": (16, 4096, 25088, 42, "dma 64x64 st3 ks1")}


def _dense_plan(M, K, OC):
    """(tile id, split-K) of csrc/conv_dma_plan.h auto_cfg / splitk for an unmasked 1x1 problem with K < 4096 or
    M OCpad <= 3e6 (the cases of this section), independent of the CU count."""
    ocp, kpad = Cm.oc_pad(OC), -(-K // 64) * 64
    mn, nk = M * ocp, kpad // 64
    if ocp % 64 == 0 and OC > 16 and mn <= 3_000_000:
        return 8, (1 if mn > 300_000 else (4 if nk >= 20 else (2 if nk >= 16 else 1)))
    assert ocp % 128 == 0 and OC > 64 and kpad < 1024 and nk < 8
    return 3, 1


@gpu
@pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", sorted(DENSE))
def test_dense_head_gemm(native_lib, name, dt):
    """The dense head's GEMM shapes, bit for bit against the fp32 CPU conv, on the planner's own route: 1 to 128
    rows on a 64-row tile, split-K 4 with unequal parts, OC < OCpad, a K tail inside each row (the padded k read
    as zero although NaNs follow each row), both sides of the two batch-size route flips."""
    args, want = DENSE[name]
    c = _case(**args, dt=dt)
    tail = args["C"] % 64 != 0
    got, r, _ = _launch(c, "auto", x_extra=24 if tail else 0, x_fill=float("nan"))
    assert r == want, r
    _expect(c, got)
    if tail:  # and with the rows ending where the allocation ends
        got, r, _ = _launch(c, "auto", x_tail=True)
        assert r == want, r
        _expect(c, got)


def _dense_real(name):
    """A real fc1 shape on integer operands: weights in [-2, 2] drawn with one call (a table lookup of one
    randint: 1 value in ``thin`` is non-zero, about 96 taps per output), its fp32 CPU reference and conditions."""
    M, K, OC, thin, _ = DENSE_REAL[name]
    g = _gen(950 + M)
    x = _ints(g, (M, 1, 1, K), -3, 3)
    lut = torch.zeros(4 * thin)
    lut[:4] = torch.tensor([-2.0, -1.0, 1.0, 2.0])
    w = lut[torch.randint(0, 4 * thin, (OC, K, 1, 1), generator=g, dtype=torch.int16).long()]
    up = name == "fc1_up"
    cw = Cm.ConvWeights(w, _ints(g, (OC,), -4, 4) if up else None, "fwd")
    kw = dict(pad=(0, 0), relu=True, epilogue="bf16" if up else "f32", use_bias=up)
    ref = ops.conv2d(x, cw, **kw)
    _check_exact(ref, BF if up else F32, x, cw, 4.0, pad=(0, 0))
    return types.SimpleNamespace(x=x, cw=cw, kw=kw, more={}, base=None, ref=ref, dt=BF, odt=BF if up else F32, OC=OC,
                                 C=K, N=M, epi=kw["epilogue"])


@gpu
@pytest.mark.parametrize("name", sorted(DENSE_REAL))
def test_dense_head_real_shapes(native_lib, name):
    """fc1.up (M 4, K 25088, OC 4096: 392 K tiles in four parts) and fc1.down (M 16, K 4096, OC 25088: a 205 MB
    B matrix) once each in bf16."""
    c = _dense_real(name)
    got, r, _ = _launch(c, "auto")
    assert r == DENSE_REAL[name][4], r
    _expect(c, got)


# ----------------------------------------------------------------------------------------
# the method's conditions for every case above, without a GPU
# ----------------------------------------------------------------------------------------

def _all_case_args(G):
    yield from (_ig_tile_args(*t) for t in IG_TILES)
    yield from (_ig_k_args(*t) for t in IG_K)
    yield from (v[0] for v in IG_MODES.values())
    yield from (_strips_args(*t) for t in STRIPS)
    yield from (_stats_args(d) for d in (1, 2, 4))
    yield from (v[0] for v in PERSIST.values())
    yield _persist_walk_args(G)
    yield from (_v2_args(*t[:5]) for t in HALO_V2)
    yield _v2_walk_args(G)
    yield from (_c8_args(*t[:4]) for t in C8)
    yield from (_hs_args(*t[:7]) for t in HS)
    yield from (_hs_split_args(*t[:7]) for t in HS_SPLIT)
    for t in HS_BITS:
        yield from _bits_args(*t[:6])
    yield from (_pw_args(name, G) for name in PW)
    yield from (_pw_out2_args(G, OC, dt) for OC, _, dt in PW_OUT2)
    for OC, dt in [(128, BF), (64, HF)]:
        yield from _bits_args(1, PW_H, _pw_m(G, OC)[0] // PW_H, 64, OC, dt, k=(1, 1))
    yield from (d[1] for d in DMA16)
    yield from (_dma512_args(G, e) for e in ("bf16", "f32"))
    for _, probs in GROUPS.values():
        for p in probs:
            yield from (dict(p, dt=dt) for dt in (BF, HF))
    for args, _ in DENSE.values():
        yield from (dict(args, dt=dt) for dt in (BF, HF))


def test_conditions():
    """Every case of every table: generator, CPU reference and the method's conditions (asserted inside the
    builders), without a GPU; the CU-following cases at G_NOMINAL CUs."""
    n = 0
    for args in _all_case_args(G_NOMINAL):
        try:
            _case.__wrapped__(**args)
        except AssertionError as e:
            raise AssertionError(f"case {args}: {e}") from e
        n += 1
    assert n > 150
    _pool.__wrapped__(450, 1, 114, 116, 64, 64)
    _pool.__wrapped__(450, _pool_v3_n(G_NOMINAL), 114, 116, 64, 64)
    for G in (G_NOMINAL, 304, 128):  # the grids that must exceed the CU count do so at other counts too
        assert G < _persist_walk_args(G)["N"] * 54 < 2 * G
        assert G < _v2_walk_args(G)["N"] * 6 < 2 * G
        assert G < _pool_v3_n(G) * 60 < 2 * G
        for OC in (64, 128, 192, 256):
            _pw_m(G, OC)
    # cfg 3 groups: M OCpad > 3e6 and Kpad < 1024 (csrc/conv_dma_plan.h auto_cfg)
    for p in GROUPS["cfg3"][1]:
        kh, kw_ = p.get("k", (3, 3))
        assert p["N"] * p["H"] * p["W"] * Cm.oc_pad(p["OC"]) > 3_000_000 and kh * kw_ * p["C"] < 1024
    for name in ("transpose", "unaligned"):
        for p in GROUPS[name][1]:
            oh, ow = p.get("out_hw", (p["H"], p["W"]))
            assert p["N"] * oh * ow * Cm.oc_pad(p["OC"]) <= 3_000_000 and p["OC"] > 16
    assert any(p["C"] % 64 for p in GROUPS["unaligned"][1])
    # the dense head: every asserted route is the planner's rule for the shape, the two flips really flip, and the
    # real shapes' partial sums are exact whatever the draw (|x| <= 3, |w| <= 2, |bias| <= 4)
    for name, (args, want) in DENSE.items():
        tile, ks = _dense_plan(args["N"], args["C"], args["OC"])
        assert want == f"dma {'64x64 st3' if tile == 8 else '128x128 st2'} ks{ks}", name
    assert DENSE["flip_splitk_below"][1] != DENSE["flip_splitk_above"][1]
    assert DENSE["flip_tile_below"][1] != DENSE["flip_tile_above"][1]
    assert 73 * 4096 <= 300_000 < 74 * 4096 and 119 * 25088 <= 3_000_000 < 128 * 25088
    for name, (M, K, OC, thin, want) in DENSE_REAL.items():
        assert 6 * K + 4 < 2 ** 24 and 80 <= K / thin <= 112
        assert want == f"dma 64x64 st3 ks{_dense_plan(M, K, OC)[1]}" and _dense_plan(M, K, OC)[0] == 8
