"""GPU: WHERE the conv epilogues round, against a float64 oracle that rounds at stated points.

The sibling exact-oracle files (test_conv_exact_gpu.py, test_conv_routes_exact_gpu.py) run on results that are
integers of at most 256 in magnitude: those pass through the fp32 -> bf16 / fp16 conversion unchanged, so no bit
of theirs depends on how or where an epilogue rounds. Here the results are INEXACT in 16 bits yet exact in fp32
under any summation order:

  * fractional operands: x integer in [-3, 3] (``xl``), weights integer in [-2, 2] thinned to about 96 taps, so
    the K sum is an exact integer; the fp32 bias is an integer in [-4, 4] plus a multiple of 2^-q, ``res`` and the
    accumulate base are 16-bit multiples of 2^-q' below 16 (exact_helpers.FRAC_Q);
  * dense integers for the bias-free transposed gather: |x| <= 15 / 63, |w| <= 7 / 31 (bf16 / fp16), so the sums
    themselves pass 2^8 / 2^11;
  * lifted operands for the pool epilogues: three channels in four carry an integer bias inside a binade whose
    spacing is 2 to 8 (exact_helpers.LIFT), so distinct fp32 window values often round to ONE stored value and
    only round-then-compare gives the unfused conv -> store -> maxpool2x2 switch codes.

The oracle (rounding_oracle.py) is float64 ``F.conv2d`` / ``conv_transpose2d`` in the operation order of the
``conv2d`` docstring with two rounding models, 'single' (one conversion at the end) and 'staged' (the 16-bit C
tile of the LDS-staged epilogues: round after the first ReLU, add res / out in fp32, round again). Every case
names the model its route must match (docs/KERNELS.md "Rounding points"); bit equality, no tolerance anywhere in
this file. Every builder asserts the method's conditions on the CPU before a GPU result exists (fp32-exactness,
rounding density, model separation, pool separation: exact_helpers._check_*), and that ``ops.conv2d`` on the CPU
equals the 'single' oracle; ``test_conditions`` (no GPU) builds every case of every table. Every launch asserts
``conv_route()`` and writes through a sentinel-framed view (the ``unpool_out`` epilogue allocates its own output).
The LDS-DMA route string does not name the epilogue: which one runs is decided by the 16-byte alignment of the
out / res / emask rows (csrc/bindings.cpp ``vec_epi``), which each such case asserts on the view it launched with.
"""
import functools
import types

import pytest
import torch

import rounding_oracle as RO
from deconv_api_amd import ops
from deconv_api_amd.ops import conv as Cm
from exact_helpers import (BF, DENSE_INT, DEV, FRAC_Q, HF, PW_H, _check_fp32_exact, _check_pool_separation,
                           _check_rounding, _check_separation, _check_ties, _dev, _expect, _frac16, _frac_bias, _gen,
                           _ints, _launch, _lift_bias, _out_view, _policy, _pw_m, _same, _signs, _untouched, _weights)
from gpu_helpers import cus as _cus, route as _route, tune as _tune

gpu = pytest.mark.gpu
G_NOMINAL = 256  # the CU count test_conditions builds the CU-following cases for
DTS = {"bf16": BF, "fp16": HF}


# ----------------------------------------------------------------------------------------
# case builders (CPU only)
# ----------------------------------------------------------------------------------------

def _out_hw(H, W, cw, stride, pad, tr, out_hw):
    if out_hw is not None:
        return out_hw
    if tr:
        return (H - 1) * stride - 2 * pad[0] + cw.KH, (W - 1) * stride - 2 * pad[1] + cw.KW
    return (H + 2 * pad[0] - cw.KH) // stride + 1, (W + 2 * pad[1] - cw.KW) // stride + 1


@functools.lru_cache(maxsize=8)  # (tests that share a case are neighbours)
def _rcase(seed, N, H, W, C, OC, k=(3, 3), stride=1, pad=None, dt=BF, relu=True, relu_in=False, amode="plain", div=1,
           out_hw=None, kind="frac", res=False, acc=False, emask=False, relu_cols=0, taps=96, xl=3, model="single",
           q=None, overflow=False):
    """One conv problem whose results are inexact in ``dt`` and exact in fp32, with both rounding models of the
    float64 oracle, the method's conditions and the CPU path's equality with 'single' asserted. ``kind``: 'frac'
    (fractional bias) or 'dense' (no bias, large integers). H, W: the conv's input map (``amode='unpool'``: the
    UNPOOLED map). ``overflow``: channel 0's bias puts fp16 results past 65504, channel 1's below -65504."""
    g = _gen(seed)
    kh, kw_ = k
    pad = (kh // 2, kw_ // 2) if pad is None else pad
    tr = amode == "transpose"
    frac = kind == "frac"
    q = FRAC_Q[dt][0] if q is None else q
    xlim, wlim = (xl, 2) if frac else DENSE_INT[dt]
    kw = dict(stride=stride, pad=pad, relu=relu, relu_in=relu_in, in_mode=amode, use_bias=frac)
    if amode == "unpool":
        x = _ints(g, (N, H // 2, W // 2, C), -xlim, xlim)
        code = torch.randint(0, 4, (N // div, H // 2, W // 2, C), generator=g, dtype=torch.uint8)
        kw.update(code=code, code_div=div)
        x_eff = RO.unpool(x, code, div)
    else:
        x = x_eff = _ints(g, (N, H, W, C), -xlim, xlim)
    if relu_in:
        x_eff = x_eff.clamp_min(0)
    cw = _weights(g, OC, C, kh, kw_, kind="transpose" if tr else "fwd", bias=False, taps=taps * stride * stride if tr else taps)
    if not frac:
        cw.w_oihw = cw.w_oihw.sign() * _ints(g, tuple(cw.w_oihw.shape), 1, wlim)
    bias = None
    if frac:
        bias = (_ints(g, (OC,), -4, 4) + _ints(g, (OC,), 0, 2 ** q - 1) * 2.0 ** -q) if q != FRAC_Q[dt][0] else \
            _frac_bias(g, OC, dt)
        if overflow:
            bias[0] += 70000.0
            bias[1] -= 70000.0
        cw.bias = bias
    ohw = _out_hw(x_eff.shape[1], x_eff.shape[2], cw, stride, pad, tr, out_hw)
    if out_hw is not None:
        kw["out_hw"] = out_hw
    if relu_cols:
        kw["relu_cols"] = relu_cols
    acc64 = RO.conv_acc(x_eff, cw.w_oihw, cw.kind, stride, pad, ohw)
    shape = tuple(acc64.shape)
    more, base = {}, None
    if res:
        more["res"] = _frac16(g, shape, dt)
    if acc:
        base = _frac16(g, shape, dt)
    em = _signs(g, shape) if emask else None
    okw = dict(res=more.get("res"), base=base, relu_cols=relu_cols)
    # the conditions, on the unmasked result
    y = RO.exact(acc64, bias, relu, **okw)
    gbits = max(q if frac else 0, FRAC_Q[dt][1] if (res or acc) else 0)
    _check_fp32_exact(y, x_eff, cw, gbits, stride, pad, (bias, more.get("res"), base))
    _check_rounding(y[..., 2:] if overflow else y, dt)
    one, two = RO.single(acc64, bias, relu, dt, **okw), RO.staged(acc64, bias, relu, dt, **okw)
    if res or acc:
        _check_separation(one, two, OC)
    else:
        assert torch.equal(one, two)
    if overflow:
        assert bool((y[..., 0] > 65504 + 16).all()) and bool((y[..., 1] == 0).all() if relu else (y[..., 1] < -65520).all())
        assert bool(torch.isfinite(one).all()) == (dt == BF)
    refs = dict(single=RO.single(acc64, bias, relu, dt, emask=em, **okw),
                staged=RO.staged(acc64, bias, relu, dt, emask=em, **okw))
    if em is not None:
        more["emask"] = em
        # (a quarter of the mask values is positive; under a ReLU about half of those outputs are zero already)
        assert bool((refs[model][em <= 0] == 0).all()) and float((refs[model] != 0).float().mean()) > 0.08
    # the CPU path rounds once, in the documented order
    ckw = {key: v.to(dt) for key, v in more.items()}
    if base is not None:
        ckw.update(out=base.to(dt).clone(), accumulate=True)
    cpu = ops.conv2d(x.to(dt), cw, **kw, **ckw)
    assert cpu.dtype == dt and torch.equal(cpu.float().double(), refs["single"]), "CPU path != single-rounding oracle"
    return types.SimpleNamespace(x=x, cw=cw, kw=kw, more=more, base=base, ref=refs[model], refs=refs, dt=dt, odt=dt,
                                 OC=OC, C=C, N=N, epi="bf16", model=model, differ=int((one != two).sum()))


@functools.lru_cache(maxsize=4)
def _pcase(seed, N, H, W, C, OC, dt=BF, pad=(1, 1), taps=96):
    """A ReLU conv with the fused max-pool on LIFTED operands: values and first-max codes of round-then-pool."""
    g = _gen(seed)
    x = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C, taps=taps, bias=False)
    cw.bias = _lift_bias(g, OC, dt)
    ohw = _out_hw(H, W, cw, 1, pad, False, None)
    full = RO.exact(RO.conv_acc(x, cw.w_oihw, "fwd", 1, pad, ohw), cw.bias, True)
    _check_fp32_exact(full, x, cw, 0, 1, pad, (cw.bias,))
    assert float((full != 0).float().mean()) >= 0.25 and full.flatten()[:65536].unique().numel() >= 16
    rv, rc = _check_pool_separation(full, dt)
    kw = dict(relu=True, epilogue="pool", pad=pad)
    cv, cc = ops.conv2d(x.to(dt), cw, **kw)
    assert torch.equal(cv.float().double(), rv) and torch.equal(cc, rc), "CPU path != round-then-pool oracle"
    return types.SimpleNamespace(x=x, cw=cw, kw=kw, more={}, base=None, ref=(rv, rc), dt=dt, odt=dt, OC=OC, C=C, N=N,
                                 epi="pool")


def R(route, policy="auto", tune=(0, 0), env=(), vec=None, **largs):
    """A launch recipe: the route to assert, the policy, the forced (tile config, split-K), per-launch DV_*
    switches, whether the rows must (True) / must not (False) satisfy the LDS-staged epilogue's alignment rule,
    and _launch's layout arguments."""
    return types.SimpleNamespace(route=route, policy=policy, tune=tune, env=dict(env), vec=vec, largs=largs)


def _vec_rows(got, kw):
    """csrc/bindings.cpp vec_epi on the tensors of a launch: 16-bit out / res / emask rows 16-B aligned."""
    ts = [got] + [kw[key] for key in ("res", "emask") if key in kw]
    return all(t.data_ptr() % 16 == 0 and t.stride(-2) % 8 == 0 for t in ts)


def _run(c, rec, monkeypatch):
    for key, v in rec.env.items():
        monkeypatch.setenv(key, v)
    seen = {}
    if rec.vec is not None:  # look at the tensors the launch really got
        real = ops.conv2d

        def spy(x, cw, **kw):
            seen.update(kw)
            return real(x, cw, **kw)

        monkeypatch.setattr(ops, "conv2d", spy)
    with _tune(*rec.tune):
        got, r, _ = _launch(c, rec.policy, **rec.largs)
    assert r == rec.route, r
    if rec.vec is not None:
        assert _vec_rows(seen["out"], seen) == rec.vec, "the rows' alignment does not select the epilogue under test"
    _expect(c, got)


# ----------------------------------------------------------------------------------------
# 1. plain 16-bit stores on every route: round to nearest, ties to even (the two models coincide)
# ----------------------------------------------------------------------------------------

KW3 = (("DV_KW3", "2"), ("DV_KW3_VAR", "0"))
KW3P = (("DV_KW3", "2"), ("DV_NO_KW3_SK", "1"))
NOVEC = (("DV_NO_VEC_EPI", "1"),)
TR = dict(amode="transpose", stride=2, pad=(1, 1), out_hw=(16, 18), relu=False, kind="dense")

# name -> (case arguments without dtype, recipe, dtypes)
PLAIN = {
    # conv_igemm: 128x128 at M = 263 (one cropped row), 256x64 / 256x16 at M = 519
    "igemm128": (dict(seed=1, N=1, H=3, W=263, C=24, OC=128, pad=(0, 1)), R("igemm 128x128", "reg"), "bf16 fp16"),
    "igemm64": (dict(seed=2, N=1, H=3, W=173, C=8, OC=40), R("igemm 256x64", "reg"), "bf16 fp16"),
    "igemm16": (dict(seed=3, N=1, H=3, W=173, C=64, OC=5), R("igemm 256x16", "reg"), "bf16 fp16"),
    "igemm_transpose": (dict(seed=4, N=2, H=8, W=9, C=64, OC=40, **TR), R("igemm 256x64", "reg"), "bf16 fp16"),
    # csrc/conv_smalln.hip (bf16 only)
    "halo_strips": (dict(seed=10, N=2, H=9, W=36, C=64, OC=16), R("halo_v1 strips", "halo"), "bf16"),
    "halo_persist": (dict(seed=11, N=2, H=7, W=30, C=64, OC=48), R("halo_v1 persist", "halo"), "bf16"),
    "halo_v2": (dict(seed=12, N=2, H=18, W=34, C=64, OC=64, amode="unpool", div=2, relu_in=True, xl=15),
                R("halo_v2", "halo"), "bf16"),
    "c8_stream": (dict(seed=13, N=2, H=57, W=58, C=8, OC=24), R("c8_stream", left=8), "bf16"),
    # csrc/conv_halo_stream.hip: LDS-staged and register epilogues, the channel-split form, emask
    "hs16_oc64_lds": (dict(seed=20, N=1, H=64, W=64, C=32, OC=64), R("hs16 oc64 lds"), "bf16 fp16"),
    "hs16_oc128_lds": (dict(seed=21, N=1, H=64, W=80, C=64, OC=128), R("hs16 oc128 lds"), "bf16 fp16"),
    "hs16_oc64_reg": (dict(seed=22, N=1, H=64, W=64, C=96, OC=64), R("hs16 oc64 reg", env=(("DV_HS16_EPI", "reg"),)),
                      "bf16 fp16"),
    "hs16_oc128_tail": (dict(seed=23, N=1, H=64, W=80, C=64, OC=100), R("hs16 oc128 reg"), "bf16 fp16"),
    "hs32_oc64_lds": (dict(seed=24, N=1, H=70, W=66, C=32, OC=64), R("hs32 oc64 lds"), "bf16 fp16"),
    "hs32_oc128_lds": (dict(seed=25, N=1, H=65, W=97, C=64, OC=128), R("hs32 oc128 lds"), "bf16 fp16"),
    "hs32_oc64_reg": (dict(seed=26, N=1, H=70, W=66, C=32, OC=64), R("hs32 oc64 reg", env=(("DV_HS16_EPI", "reg"),)),
                      "bf16 fp16"),
    "hs16_ocsplit": (dict(seed=27, N=1, H=64, W=64, C=96, OC=192), R("hs16 oc64 lds ocsplit"), "bf16 fp16"),
    "hs32_ocsplit_emask": (dict(seed=28, N=1, H=70, W=66, C=32, OC=256, emask=True, relu=False),
                           R("hs32 oc128 lds ocsplit", left=8, x_extra=8), "bf16 fp16"),
    "hs16_emask": (dict(seed=29, N=1, H=64, W=64, C=32, OC=64, emask=True, relu=False), R("hs16 oc64 lds"), "bf16 fp16"),
    "hs16_emask_reg": (dict(seed=30, N=1, H=64, W=64, C=32, OC=64, emask=True, relu=False),
                       R("hs16 oc64 reg", env=(("DV_HS16_EPI", "reg"),)), "bf16 fp16"),
    # LDS-DMA: register epilogue (rows not 16-B aligned; DV_NO_VEC_EPI), LDS epilogue (8 chunks per thread on
    # 128x128, 16 on 256x256), split-K reduce, OC % 8 != 0 (the in-loop element tail; epi_tail under emask)
    "dma_reg": (dict(seed=40, N=2, H=9, W=7, C=64, OC=128), R("dma 128x128 st2 ks1", "dma", (3, 1), vec=False, right=4),
                "bf16 fp16"),
    "dma_novec": (dict(seed=40, N=2, H=9, W=7, C=64, OC=128), R("dma 128x128 st2 ks1", "dma", (3, 1), NOVEC), "bf16 fp16"),
    "dma_lds": (dict(seed=40, N=2, H=9, W=7, C=64, OC=128), R("dma 128x128 st2 ks1", "dma", (3, 1), vec=True), "bf16 fp16"),
    "dma_lds_256": (dict(seed=41, N=2, H=9, W=15, C=32, OC=256), R("dma 256x256 st2 ks1", "dma", (1, 1), vec=True),
                    "bf16 fp16"),
    "dma_splitk": (dict(seed=42, N=2, H=9, W=7, C=64, OC=96), R("dma 64x64 st3 ks3", "dma", (8, 3)), "bf16 fp16"),
    "dma_tail_lds": (dict(seed=43, N=2, H=9, W=7, C=32, OC=44), R("dma 64x64 st3 ks1", "dma", (8, 1), vec=True, right=4),
                     "bf16 fp16"),
    "dma_tail_emask": (dict(seed=44, N=2, H=9, W=7, C=32, OC=44, emask=True, relu=False),
                       R("dma 64x64 st3 ks1", "dma", (8, 1), vec=True, right=4, more_extra=4), "bf16 fp16"),
    "dma_tail_reg": (dict(seed=43, N=2, H=9, W=7, C=32, OC=44), R("dma 64x64 st3 ks1", "dma", (8, 1), vec=False, right=3),
                     "bf16 fp16"),
    "dma_relu_cols": (dict(seed=45, N=2, H=9, W=7, C=64, OC=128, relu_cols=40), R("dma 128x128 st2 ks1", "dma", (3, 1), vec=True),
                      "bf16 fp16"),
    "dma_relu_cols_reg": (dict(seed=45, N=2, H=9, W=7, C=64, OC=128, relu_cols=40),
                          R("dma 128x128 st2 ks1", "dma", (3, 1), vec=False, right=4), "bf16 fp16"),
    "dma_transpose": (dict(seed=46, N=2, H=8, W=9, C=64, OC=40, **TR), R("dma 64x64 st3 ks1", "dma", (8, 1)), "bf16 fp16"),
    "dma_transpose_splitk": (dict(seed=46, N=2, H=8, W=9, C=64, OC=40, **TR), R("dma 64x64 st3 ks3", "dma", (8, 3)),
                             "bf16 fp16"),
    # KW3 / KW3P (csrc/conv_dma_impl.h conv_dma_kw3_kernel / conv_dma_kw3p_kernel)
    "kw3_256": (dict(seed=50, N=3, H=10, W=9, C=32, OC=256), R("kw3 256x256", "auto", (0, 1), KW3, vec=True), "bf16 fp16"),
    "kw3_512": (dict(seed=51, N=3, H=36, W=35, C=32, OC=128), R("kw3 512x128", "auto", (0, 1), KW3, vec=True), "bf16 fp16"),
    "kw3_reg": (dict(seed=50, N=3, H=10, W=9, C=32, OC=256), R("kw3 256x256", "auto", (0, 1), KW3, vec=False, right=4),
                "bf16 fp16"),
    "kw3p_lds": (dict(seed=52, N=3, H=11, W=13, C=32, OC=256), R("kw3p 256x256 lds", "auto", (0, 1), KW3P), "bf16 fp16"),
    "kw3p_reg": (dict(seed=52, N=3, H=11, W=13, C=32, OC=256),
                 R("kw3p 256x256 reg", "auto", (0, 1), KW3P + (("DV_KW3P_EPI", "reg"),)), "bf16 fp16"),
    "kw3p_512_lds": (dict(seed=53, N=3, H=36, W=35, C=32, OC=128), R("kw3p 512x128 lds", "auto", (0, 1), KW3P), "bf16 fp16"),
}


def _cases(table):
    return [(name, d) for name, v in table.items() for d in v[2].split()]


@gpu
@pytest.mark.parametrize("name,d", _cases(PLAIN))
def test_plain_store_rounds_to_nearest_even(native_lib, monkeypatch, name, d):
    """Every route's plain 16-bit store (packed, scalar, per-element tail and LDS-staged converts) on inexact
    results with exact ties in both directions: bit-equal to one round-to-nearest-even conversion."""
    args, rec, _ = PLAIN[name]
    _run(_rcase(**args, dt=DTS[d]), rec, monkeypatch)


PW_PLAIN = {"oc128": (64, 128, {}), "oc192_k3": (192, 192, {}), "relu_cols_oc128": (64, 128, dict(relu_cols=40))}


def _pw_args(G, C, OC, seed, **opts):
    return dict(seed=seed, N=1, H=PW_H, W=_pw_m(G, OC)[0] // PW_H, C=C, OC=OC, k=(1, 1), **opts)


@gpu
@pytest.mark.parametrize("d", sorted(DTS))
@pytest.mark.parametrize("name", sorted(PW_PLAIN))
def test_plain_pw(native_lib, monkeypatch, name, d):
    """The persistent 1x1 kernel's plain store (the shared LDS-staged epilogue), rows following the CU count."""
    C, OC, opts = PW_PLAIN[name]
    G = _cus()
    _, BM, BN = _pw_m(G, OC)
    _run(_rcase(**_pw_args(G, C, OC, 60 + OC, **opts), dt=DTS[d]), R(f"pw {BM}x{BN}", x_extra=8), monkeypatch)


# KW3P routes that need a grid longer than the CU count. The oracle is built for LONG_SUB images; the batch repeats
# them (an image's outputs do not depend on its neighbours), so the WHOLE output is compared at four images' cost
# on the CPU, and the tiles (256 rows, images of 196) meet the images at every phase.
LONG_SUB = 4
LONG = {
    # name -> (case arguments, env, forced (tile, split-K), images for G CUs, route for G CUs)
    # stream-K: about 1.5 rounds of one workgroup per CU; split tiles add two fp32 partials: exact here
    "stream_k": (dict(seed=54, N=LONG_SUB, H=14, W=14, C=32, OC=256), (("DV_KW3", "2"),), (0, 1),
                 lambda G: -(-(3 * G // 2) * 256 // 196), lambda G: "kw3p 256x256 lds sk"),
    # 1.05 rounds without stream-K: the full round on KW3P, the rest as a 128 x 128 LDS-DMA tail launch (K = 9 x 512
    # is what it takes to reach kw3_split by the natural route, as in test_conv_exact_gpu.py)
    "tail_split": (dict(seed=55, N=LONG_SUB, H=14, W=14, C=512, OC=256), (("DV_NO_KW3_SK", "1"),), (0, 0),
                   lambda G: -(-(21 * G // 20 + 1) * 256 // 196),
                   lambda G: f"kw3p 256x256 lds + dma 128x128 tail m_base={G * 256}"),
}


@gpu
@pytest.mark.parametrize("d", sorted(DTS))
@pytest.mark.parametrize("name", sorted(LONG))
def test_plain_kw3p_long_grids(native_lib, monkeypatch, name, d):
    """KW3P stream-K and the KW3P + LDS-DMA tail split (the batch follows the CU count): every output of the
    whole batch is the one round-to-nearest-even conversion, and no stream-K hand-off timed out."""
    args, env, tune, n_of, route_of = LONG[name]
    for key, v in env:
        monkeypatch.setenv(key, v)
    G = _cus()
    N = n_of(G)
    tiles = -(-N * 196 // 256)
    assert G < tiles < 2 * G, (tiles, G)
    c = _rcase(**args, dt=DTS[d])
    xd = _dev(c.x, c.dt).repeat(-(-N // LONG_SUB), 1, 1, 1)[:N].contiguous()
    shape = (N,) + tuple(c.ref.shape[1:])
    buf, view = _out_view(shape, c.dt, 0, 8)
    native_lib.sk_errors(True)
    with _tune(*tune):
        got = ops.conv2d(xd, c.cw.to_device(DEV, c.dt), out=view, **c.kw)
        assert _route() == route_of(G), _route()
    torch.cuda.synchronize()
    assert native_lib.sk_errors(True) == 0
    assert _untouched(buf, shape, 0), "wrote outside the output view"
    want = c.ref.float().to(DEV)[torch.arange(N, device=DEV) % LONG_SUB]
    bad = got.float() != want
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} values differ, first at {bad.nonzero()[0].tolist()}"


UNPOOL_OUT = {
    # name -> (case arguments, route, tune, env): the LDS-staged epilogue's max-unpool-out branch and KW3P's
    "dma": (dict(seed=70, N=4, H=9, W=7, C=64, OC=128), "dma 128x128 st2 ks1", (3, 1), ()),
    "kw3p": (dict(seed=71, N=4, H=10, W=9, C=32, OC=256), "kw3p 256x256 unpool", (0, 1), KW3P),
}


def _unpool_codes(c, div):
    return torch.randint(0, 4, (c.N // div,) + tuple(c.ref.shape[1:]), generator=_gen(72 + div), dtype=torch.uint8)


@gpu
@pytest.mark.parametrize("d", sorted(DTS))
@pytest.mark.parametrize("name", sorted(UNPOOL_OUT))
def test_plain_unpool_out(native_lib, monkeypatch, name, d):
    """The max-unpool-out epilogues: the rounded value at the window position its switch code names (codes
    shared by two images), zeros elsewhere. (conv2d allocates this output itself: no sentinel frame.)"""
    args, route, tune, env = UNPOOL_OUT[name]
    for key, v in env:
        monkeypatch.setenv(key, v)
    c = _rcase(**args, dt=DTS[d])
    code = _unpool_codes(c, 2)
    with _tune(*tune), _policy("dma" if name == "dma" else "auto"):
        got = ops.conv2d(_dev(c.x, c.dt), c.cw.to_device(DEV, c.dt), unpool_out=code.to(DEV), unpool_div=2, **c.kw)
        assert _route() == route, _route()
    _same(got, RO.unpool(c.ref, code, 2))


def _out2_args():
    return dict(seed=73, N=2, H=9, W=7, C=64, OC=128)


@gpu
@pytest.mark.parametrize("d", sorted(DTS))
@pytest.mark.parametrize("split", [64, 40])
def test_plain_out2(native_lib, d, split):
    """out2 / split_col on the LDS-DMA kernel (the LDS-staged epilogue's two-destination branch): both halves
    through sentinel-framed channel slices, split on and off a 64-column boundary."""
    c = _rcase(**_out2_args(), dt=DTS[d])
    shape = tuple(c.ref.shape)
    b1, v1 = _out_view(shape[:-1] + (split,), c.dt, 8, 8)
    b2, v2 = _out_view(shape[:-1] + (c.OC - split,), c.dt, 8, 16)
    with _tune(3, 1):
        ops.conv2d(_dev(c.x, c.dt), c.cw.to_device(DEV, c.dt), out=v1, out2=v2, split_col=split, **c.kw)
        assert _route() == "dma 128x128 st2 ks1", _route()
    _same(v1, c.ref[..., :split])
    _same(v2, c.ref[..., split:])
    assert _untouched(b1, shape[:-1] + (split,), 8) and _untouched(b2, shape[:-1] + (c.OC - split,), 8), \
        "wrote outside the views"


GROUP = [dict(seed=74, N=2, H=9, W=11, C=24, OC=40), dict(seed=75, N=2, H=9, W=11, C=64, OC=96),
         dict(seed=76, N=3, H=9, W=9, C=128, OC=128, acc=True, relu=False, model="staged")]


@gpu
@pytest.mark.parametrize("d", sorted(DTS))
def test_grouped_launch(native_lib, d):
    """A grouped launch (csrc/conv_dma_group.hip: the same tile program and LDS-staged epilogue): two plain
    problems and one that accumulates, which must match the 'staged' model."""
    dt = DTS[d]
    cases = [_rcase(**p, dt=dt) for p in GROUP]
    lib = ops.native.lib()
    held = []
    with _policy("auto"):
        lib.conv_group_begin()
        try:
            for c in cases:
                buf, view = _out_view(tuple(c.ref.shape), dt, 8, 8)
                kw = dict(c.kw)
                if c.base is not None:
                    view.copy_(_dev(c.base, dt))
                    kw["accumulate"] = True
                xd, cwd = _dev(c.x, dt), c.cw.to_device(DEV, dt)
                ops.conv2d(xd, cwd, out=view, **kw)
                assert _route() == "group cfg8", _route()
                held.append((buf, view, xd, cwd))
        finally:
            launches = lib.conv_group_end()
    assert launches == 1, launches
    for c, (buf, view, *_rest) in zip(cases, held):
        _same(view, c.ref)
        assert _untouched(buf, tuple(c.ref.shape), 8), "wrote outside the output view"


# ----------------------------------------------------------------------------------------
# 2. res / accumulate (+ ReLU, + emask): each route against the model it is documented to follow
# ----------------------------------------------------------------------------------------

VARIANTS = {
    "res": dict(res=True, relu=False), "res_relu": dict(res=True, relu=True),
    "acc": dict(acc=True, relu=False), "acc_relu": dict(acc=True, relu=True),
    "res_relu_emask": dict(res=True, relu=True, emask=True), "acc_emask": dict(acc=True, relu=False, emask=True),
}
ALL, ACC = tuple(VARIANTS), ("acc", "acc_relu")
_D128 = dict(seed=80, N=2, H=9, W=7, C=64, OC=128)
_D44 = dict(seed=81, N=2, H=9, W=7, C=32, OC=44)
_K256 = dict(seed=82, N=3, H=10, W=9, C=32, OC=256)

# name -> (case arguments, recipe, model, variants)
POST = {
    # single: conv_igemm.hip's epilogue (one conversion, lines 270-281); accumulate is all it takes
    "igemm": (dict(seed=83, N=1, H=3, W=173, C=64, OC=40), R("igemm 256x64", "reg"), "single", ACC),
    # single: csrc/conv_dma_impl.h epilogue (accumulate) / epilogue_res (res, emask), reached when a row is not
    # 16-B aligned or under DV_NO_VEC_EPI; per element, so OC % 8 != 0 takes no other path
    "dma_reg": (_D128, R("dma 128x128 st2 ks1", "dma", (3, 1), vec=False, right=4), "single", ALL),
    "dma_novec": (_D128, R("dma 128x128 st2 ks1", "dma", (3, 1), NOVEC), "single", ALL),
    "dma_reg_oc44": (_D44, R("dma 64x64 st3 ks1", "dma", (8, 1), vec=False, right=3), "single", ALL),
    # single: csrc/conv_dma.hip splitk_reduce_kernel sums the fp32 planes and converts once, aligned or not
    "dma_splitk": (dict(seed=84, N=2, H=9, W=7, C=64, OC=96), R("dma 64x64 st3 ks3", "dma", (8, 3), vec=True), "single", ALL),
    # staged: epilogue_lds, batched form (<= 8 chunks per thread: epi_combine) on 128x128 and 64x64 ...
    "dma_lds": (_D128, R("dma 128x128 st2 ks1", "dma", (3, 1), vec=True), "staged", ALL),
    # ... its rows' last partial chunk (OC = 44: epi_tail) ...
    "dma_lds_oc44": (_D44, R("dma 64x64 st3 ks1", "dma", (8, 1), vec=True, right=4, more_extra=4), "staged", ALL),
    # ... and the per-chunk loop (256x256: 16 chunks per thread)
    "dma_lds_loop": (dict(seed=85, N=2, H=9, W=15, C=32, OC=256), R("dma 256x256 st2 ks1", "dma", (1, 1), vec=True),
                     "staged", ALL),
    # KW3 (conv_dma_impl.h conv_dma_kw3_kernel's epilogue dispatch, "if (a.vec_epi) epilogue_lds ... epilogue_res ...
    # epilogue"): aligned rows take epilogue_lds' per-chunk loop (16 chunks per thread) -> staged; other rows
    # epilogue_res / epilogue -> single. KW3P takes no res / accumulate / emask (its header comment).
    "kw3_lds": (_K256, R("kw3 256x256", "auto", (0, 1), KW3, vec=True), "staged", ALL),
    "kw3_reg": (_K256, R("kw3 256x256", "auto", (0, 1), KW3, vec=False, right=4), "single", ALL),
}


def _post_cases():
    return [(name, v, d) for name, t in POST.items() for v in t[3] for d in sorted(DTS)]


def _post_case(name, variant, d):
    args, _, model, _ = POST[name]
    return _rcase(**args, **VARIANTS[variant], model=model, dt=DTS[d])


@gpu
@pytest.mark.parametrize("name,variant,d", _post_cases())
def test_post_ops_rounding_model(native_lib, monkeypatch, name, variant, d):
    """res / accumulate, with and without ReLU and emask, on operands where rounding once and rounding the staged
    tile first differ on more than 5 % of the outputs: every route equals ITS model bit for bit."""
    c = _post_case(name, variant, d)
    assert c.differ > 0
    _run(c, POST[name][1], monkeypatch)


PW_POST = {"res_relu_oc256": (64, 256, "res_relu"), "res_oc128": (64, 128, "res"), "acc_oc64": (64, 64, "acc"),
           "acc_relu_oc192_k3": (192, 192, "acc_relu"), "acc_emask_oc128": (64, 128, "acc_emask"),
           "res_relu_emask_oc64": (64, 64, "res_relu_emask")}


@gpu
@pytest.mark.parametrize("d", sorted(DTS))
@pytest.mark.parametrize("name", sorted(PW_POST))
def test_post_ops_pw(native_lib, monkeypatch, name, d):
    """The persistent 1x1 kernel runs epilogue_lds (csrc/conv_pw.hip): 'staged'."""
    C, OC, variant = PW_POST[name]
    G = _cus()
    _, BM, BN = _pw_m(G, OC)
    c = _rcase(**_pw_args(G, C, OC, 90 + OC, **VARIANTS[variant], model="staged"), dt=DTS[d])
    _run(c, R(f"pw {BM}x{BN}", vec=True, x_extra=8), monkeypatch)


def _res_acc_args():
    return dict(_D128, res=True, acc=True, relu=True, emask=True)


@gpu
def test_res_with_accumulate_is_refused(native_lib):
    """res together with accumulate: the CPU path computes it in the documented order (asserted against the
    'single' oracle by the builder), the binding refuses it, so no GPU route has a model to pin for it yet."""
    c = _rcase(**_res_acc_args())
    with pytest.raises(RuntimeError, match="res: forward conv"):
        _launch(c, "dma")


# ----------------------------------------------------------------------------------------
# 3. fused pool epilogues on lifted operands: values and switch codes of round-then-pool
# ----------------------------------------------------------------------------------------

POOL_DMA = [(2, 16, 14, 64, 128, 4, "256x128 st3"), (3, 10, 14, 64, 192, 6, "512x64 st2"), (1, 12, 12, 32, 48, 11, "256x64 st2")]
POOL_EPI = {"pool_t": (), "pool_lds": (("DV_POOL_EPI", "lds"),), "pool": (("DV_NO_POOL_T", "1"),)}


@gpu
@pytest.mark.parametrize("d", sorted(DTS))
@pytest.mark.parametrize("epi", sorted(POOL_EPI))
@pytest.mark.parametrize("N,H,W,C,OC,cfg,tile", POOL_DMA)
def test_pool_dma(native_lib, monkeypatch, N, H, W, C, OC, cfg, tile, epi, d):
    """The LDS-DMA kernel's three pooled-max epilogues compare STORED-precision values."""
    c = _pcase(100 + OC, N, H, W, C, OC, DTS[d])
    _run(c, R(f"dma {tile} ks1 {epi}", "auto", (cfg, 0), POOL_EPI[epi]), monkeypatch)


POOL_IG = {128: (1, 6, 44, 24, 128), 64: (1, 10, 52, 8, 40), 16: (1, 10, 52, 64, 7)}  # M = BM + 4 / 2 BM + 8


@gpu
@pytest.mark.parametrize("bn", sorted(POOL_IG))
def test_pool_igemm(native_lib, monkeypatch, bn):
    """conv_igemm's pool epilogue on its three tiles (bf16: its only pooled instantiation)."""
    c = _pcase(110 + bn, *POOL_IG[bn], BF)
    _run(c, R(f"igemm {128 if bn == 128 else 256}x{bn}", "reg"), monkeypatch)


POOL_HALO = {
    # (the fused-pool instantiations of these kernels and of conv_igemm are bf16 only)
    "hs16_oc64": ((1, 64, 64, 32, 64), "hs16 oc64 pool", "bf16"),
    "hs16_oc128": ((1, 64, 80, 64, 128), "hs16 oc128 pool", "bf16"),
    "hs32_oc128": ((1, 70, 66, 32, 128), "hs32 oc128 pool", "bf16"),
    "hs32_oc64": ((1, 70, 66, 32, 64), "hs32 oc64 pool", "bf16"),
    "pool_v3": ((1, 112, 120, 64, 64), "pool_v3", "bf16"),
}


@gpu
@pytest.mark.parametrize("name,d", _cases(POOL_HALO))
def test_pool_halo(native_lib, monkeypatch, name, d):
    """The halo-stream kernels' and the weight-resident 64 -> 64 kernel's fused pool."""
    shape, route, _ = POOL_HALO[name]
    _run(_pcase(120 + shape[1] + shape[4], *shape, DTS[d]), R(route), monkeypatch)


@functools.lru_cache(maxsize=2)
def _stem_case(chain):
    """The fused stem conv 8 -> 64, ReLU, conv 64 -> 64, ReLU, pool. ``chain`` False: integer conv1 output, LIFTED
    conv2 bias (the pool compares stored values). True: a FRACTIONAL conv1 bias, so the 64-channel map the kernel
    keeps in LDS is inexact in bf16 and must be rounded there exactly as the unfused conv2d would store it; the
    second conv then sums 8-bit fractions (multiples of 2^-5), whose fp32-exactness is asserted as well."""
    g = _gen(130 + chain)
    N, H, W = 2, 32, 48
    xl = 15 if chain else 3  # (a wider image range lifts conv1's outputs into binades coarser than 2^-5)
    x = _ints(g, (N, H, W, 8), -xl, xl)
    x[..., 3:] = 0
    c1 = _weights(g, 64, 8, taps=24, bias=False)
    c2 = _weights(g, 64, 64, taps=12, bias=False)
    c1.bias = _frac_bias(g, 64, BF) if chain else _ints(g, (64,), -4, 4)
    c2.bias = _ints(g, (64,), -4, 4) if chain else _lift_bias(g, 64, BF)
    q = FRAC_Q[BF][0] if chain else 0
    y1x = RO.exact(RO.conv_acc(x, c1.w_oihw, "fwd", 1, (1, 1), (H, W)), c1.bias, True)
    _check_fp32_exact(y1x, x, c1, q, 1, (1, 1), (c1.bias,))
    if chain:
        _check_rounding(y1x, BF)
    y1 = RO.round16(y1x, BF)  # rounding point 1: the stored (here: LDS-resident) conv1 map
    full = RO.exact(RO.conv_acc(y1, c2.w_oihw, "fwd", 1, (1, 1), (H, W)), c2.bias, True)
    _check_fp32_exact(full, y1, c2, q, 1, (1, 1), (c2.bias,))  # second stage: sums of 2^-q fractions
    if chain:
        assert float((~RO.representable(full, BF)).float().mean()) >= 0.20
        rv, rc = RO.pool_first_max(RO.round16(full, BF))  # rounding point 2, then the pool
        _check_ties(RO.round16(full, BF))
    else:
        rv, rc = _check_pool_separation(full, BF)
    cv, cc = ops.conv2d(ops.conv2d(x.to(BF), c1, relu=True), c2, relu=True, epilogue="pool")
    assert torch.equal(cv.float().double(), rv) and torch.equal(cc, rc), "CPU chain != oracle"
    return types.SimpleNamespace(x=x, c1=c1, c2=c2, ref=(rv, rc))


@gpu
@pytest.mark.parametrize("chain", [False, True], ids=["lifted", "fractional_conv1"])
def test_stem_pool(native_lib, chain):
    """ops.conv.stem_pool == conv2d(conv2d(x, c1), c2, epilogue='pool') with both of its 16-bit rounding points."""
    c = _stem_case(chain)
    got = ops.stem_pool(_dev(c.x, BF), c.c1.to_device(DEV), c.c2.to_device(DEV))
    assert got is not None and _route() == "hs16 oc64 pool stem", _route()
    _same(got[0], c.ref[0])
    assert torch.equal(got[1].cpu(), c.ref[1]), "switch codes differ"


# ----------------------------------------------------------------------------------------
# 4. the fused deconvnet tail: 16-bit d, 16-bit Z (ops.conv.deconv_tail_ref's rounding points)
# ----------------------------------------------------------------------------------------

TAIL = [(2, 18, 34, 2), (3, 16, 32, 1)]


def _zsum(z):
    """out[n, h, w, c] = sum over taps t = kh*3 + kw of Z[n, h + kh - 1, w + kw - 1, 3 t + c] (zero outside)."""
    N, H, W, _ = z.shape
    zp = torch.nn.functional.pad(z, (0, 0, 1, 1, 1, 1))
    out = z.new_zeros(N, H, W, 3)
    for kh in range(3):
        for kw in range(3):
            t = kh * 3 + kw
            out += zp[:, kh:kh + H, kw:kw + W, 3 * t:3 * t + 3]
    return out


@functools.lru_cache(maxsize=2)
def _tail_case(N, H, W, div):
    g = _gen(140 + N + H)
    q = FRAC_Q[BF][0]
    p = _ints(g, (N, H // 2, W // 2, 64), -255, 255) * 2.0 ** -q  # bf16 values below 8, multiples of 2^-5
    assert torch.equal(p.to(BF).float(), p)
    code = torch.randint(0, 4, (N // div, H // 2, W // 2, 64), generator=g, dtype=torch.uint8)
    mid = _weights(g, 64, 64, bias=False, taps=288)  # (ReLU and unpool leave one input in eight non-zero)
    last = _weights(g, 3, 64, bias=False, taps=96)
    u = RO.unpool(p.double(), code, div).clamp_min(0)
    dx = RO.conv_acc(u, mid.w_oihw, "fwd", 1, (1, 1), (H, W)).clamp_min(0)
    _check_fp32_exact(dx, u, mid, q)
    _check_rounding(dx, BF)
    d = RO.round16(dx, BF)  # rounding point 1: the 16-bit tile of d the MFMA epilogue multiplies
    w2 = last.w_oihw.double().permute(2, 3, 0, 1).reshape(27, 64)  # row (kh*3 + kw)*3 + c
    zx = torch.einsum("nhwc,zc->nhwz", d, w2)
    bound = torch.einsum("nhwc,zc->nhwz", d, w2.abs()).max()
    assert float(bound) * 2.0 ** q < 2 ** 24, "Z's partial sums not exact in fp32"
    assert float((~RO.representable(zx, BF)).float().mean()) >= 0.20, "too few inexact Z values"
    z = RO.round16(zx, BF)      # rounding point 2: the stored Z
    assert 9 * float(z.abs().max()) * 2.0 ** q < 2 ** 24
    ref = _zsum(z).clamp_min(0)  # fp32 shift-add: exact
    assert torch.equal(ref.float().double(), ref) and float((ref != 0).float().mean()) >= 0.25
    cpu = Cm.deconv_tail_ref(p.to(BF), code, div, mid, last)
    assert torch.equal(cpu.double(), ref), "deconv_tail_ref != oracle"
    return types.SimpleNamespace(p=p, code=code, mid=mid, last=last, ref=ref)


@gpu
@pytest.mark.parametrize("N,H,W,div", TAIL)
def test_deconv_tail_rounding_points(native_lib, N, H, W, div):
    """ops.deconv_tail on a fractional pooled map: d and Z are inexact in bf16, and the fp32 result equals the
    float64 model that rounds d and Z to bf16 (and nothing else) bit for bit."""
    c = _tail_case(N, H, W, div)
    got = ops.deconv_tail(c.p.to(BF).to(DEV), c.code.to(DEV), div, c.mid.to_device(DEV), c.last.to_device(DEV))
    assert got is not None and got.shape == (N, H, W, 3) and got.dtype == torch.float32
    _same(got, c.ref)


# ----------------------------------------------------------------------------------------
# 5. overflow: past +-65504 fp16 stores +inf (0 under the ReLU), bf16 stays finite
# ----------------------------------------------------------------------------------------

OVERFLOW = {"reg": R("dma 128x128 st2 ks1", "dma", (3, 1), vec=False, right=4),
            "lds": R("dma 128x128 st2 ks1", "dma", (3, 1), vec=True)}


OVERFLOW_Q = {BF: 5, HF: 7}  # bias fractions 2^-q: (70000 + sum |x| |w| + 4) 2^q stays below 2^24


def _overflow_args():
    return dict(seed=150, N=2, H=9, W=7, C=64, OC=128, overflow=True, xl=15)


@gpu
@pytest.mark.parametrize("d", sorted(DTS))
@pytest.mark.parametrize("epi", sorted(OVERFLOW))
def test_overflow(native_lib, monkeypatch, epi, d):
    """Channel 0's bias puts the results past 65504 (fp16: +inf, bf16: finite and rounded), channel 1's below
    -65504 under the ReLU (0), on the LDS-DMA kernel's register and LDS-staged epilogues (no emask: the
    reference's inf * 0 is not the kernels' zeroing)."""
    _run(_rcase(**_overflow_args(), dt=DTS[d], q=OVERFLOW_Q[DTS[d]]), OVERFLOW[epi], monkeypatch)


# ----------------------------------------------------------------------------------------
# the method's conditions for every case above, without a GPU
# ----------------------------------------------------------------------------------------

def _all_rcases(G):
    for name, d in _cases(PLAIN):
        yield dict(PLAIN[name][0], dt=DTS[d])
    for d in DTS.values():
        for C, OC, opts in PW_PLAIN.values():
            yield dict(_pw_args(G, C, OC, 60 + OC, **opts), dt=d)
        for v in list(UNPOOL_OUT.values()) + list(LONG.values()):
            yield dict(v[0], dt=d)
        yield dict(_out2_args(), dt=d)
        for p in GROUP:
            yield dict(p, dt=d)
        for C, OC, variant in PW_POST.values():
            yield dict(_pw_args(G, C, OC, 90 + OC, **VARIANTS[variant], model="staged"), dt=d)
        yield dict(_overflow_args(), dt=d, q=OVERFLOW_Q[d])
    for name, variant, d in _post_cases():
        yield dict(POST[name][0], **VARIANTS[variant], model=POST[name][2], dt=DTS[d])
    yield _res_acc_args()


def _all_pcases():
    for d in DTS.values():
        for N, H, W, C, OC, _, _ in POOL_DMA:
            yield (100 + OC, N, H, W, C, OC, d)
    for bn, shape in POOL_IG.items():
        yield (110 + bn,) + shape + (BF,)
    for name, d in _cases(POOL_HALO):
        shape = POOL_HALO[name][0]
        yield (120 + shape[1] + shape[4],) + shape + (DTS[d],)


def test_conditions():
    """Every case of every table: generator, both oracles, the method's conditions and the CPU path's equality
    with the single-rounding oracle (asserted inside the builders), without a GPU."""
    n = 0
    for args in _all_rcases(G_NOMINAL):
        try:
            _rcase.__wrapped__(**args)
        except AssertionError as e:
            raise AssertionError(f"case {args}: {e}") from e
        n += 1
    for args in _all_pcases():
        try:
            _pcase.__wrapped__(*args)
        except AssertionError as e:
            raise AssertionError(f"pool case {args}: {e}") from e
        n += 1
    assert n > 200, n
    for chain in (False, True):
        _stem_case.__wrapped__(chain)
    for t in TAIL:
        _tail_case.__wrapped__(*t)
    # the epilogue a POST route's alignment selects is the one its model is documented for
    for name, (_, rec, model, _) in POST.items():
        if name.startswith("dma_") and name != "dma_splitk" and rec.vec is not None:
            assert (model == "staged") == rec.vec, name
    for G in (G_NOMINAL, 304, 128):
        for OC in (64, 128, 192, 256):
            _pw_m(G, OC)
