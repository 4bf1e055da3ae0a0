"""GPU: the conv kernels below the smallest normal 16-bit value, the ReLU-mask predicate on tiny stored values and
NaN in the slack next to the operands, against float64 oracles (rounding_oracle.py; ``torch.where`` for the masks).

The sibling exact-oracle files pin what is summed, where it is written and where a value is rounded on results of
ordinary magnitude. Three regimes they exclude by construction are run here:

  A. small magnitudes. The integer method of test_conv_rounding_exact_gpu.py scaled by powers of two (``FAM``), so
     every partial sum stays exact in fp32 under any order and the only freedom left is how a kernel treats fp16 /
     bf16 / fp32 SUBNORMALS: operands reaching the MFMA unchanged, a subnormal 16-bit C tile read back from LDS,
     round-to-nearest-even on the fixed grid (2^-24 fp16, 2^-133 bf16), |v| <= 2^-25 -> 0, round-then-compare in
     the fused pool. The builders assert, on the float64 reference alone, the density of subnormal results, ties
     and underflows, and that the reference differs from three mutants (outputs flushed, operands flushed, round
     toward zero) on a stated share of the outputs.
  B. the mask predicate. A mask element is positive iff its value is > 0 as a real number: of the stored values
     +-1, +-0.0, +-(smallest subnormal) and +-(smallest normal) (exact_helpers._signs_tiny) the three positive ones
     keep and the five others zero, whether a kernel tests bits or compares floats. 2 x 2 windows drawn from
     {-0.0, +0.0, +-smallest subnormal, +-twice that}: the first maximum wins, the zeros tie, a negative
     subnormal loses to either zero.
  C. slack. x's / mask's / res' / emask's extra channels and the rows before x hold NaN instead of a finite fill:
     a kernel that reads past the logical K or a row and meets a zero weight there is no longer invisible.

Bit equality, no tolerance anywhere. The SIGN of a zero is not pinned: ``_same`` compares as fp32 (-0.0 == 0.0),
and -0 and +0 are the same mask value everywhere downstream (that is rule B). Every launch asserts
``conv_route()`` and writes through a sentinel-framed view (the recipes ``R`` / ``_run`` and the route tables are
test_conv_rounding_exact_gpu.py's own, imported, not re-derived); every builder asserts its conditions on the CPU
before a GPU result exists, and that ``ops.conv2d`` on the CPU equals the single-rounding oracle;
``test_conditions`` (no GPU) builds every case of every table and records the minimum of every fraction.
"""
import functools
import types

import numpy as np
import pytest
import torch

import rounding_oracle as RO
import test_conv_rounding_exact_gpu as RT  # the recipe tables, R and _run (no test function is taken from it)
import test_conv_routes_exact_gpu as RR    # the mask / bits recipes and their integer cases
import test_deconv_exact_gpu as TDC        # the pool / unpool shapes and the misc route report
from deconv_api_amd import ops
from deconv_api_amd.ops import autograd as AG, conv as Cm
from exact_helpers import (BF, DEV, HF, SENT, TINY_BITS, _check_fp32_exact, _check_pool_separation,
                           _check_separation, _dev, _gen, _ints, _launch, _out_view, _policy, _pw_m, _same,
                           _signs_tiny, _untouched, _weights)
from gpu_helpers import cus as _cus, route as _route, tune as _tune

gpu = pytest.mark.gpu
G_NOMINAL = RT.G_NOMINAL
F32 = torch.float32
R, _run = RT.R, RT._run

# ----------------------------------------------------------------------------------------
# A. operand families: integers k, j, b times powers of two
# ----------------------------------------------------------------------------------------
# name -> dtype, exponents of x / weights / bias (None: no bias), |b| limit, taps, and the result's granularity
FAM = {
    "sub": types.SimpleNamespace(dt=HF, xe=-24, we=-3, be=-27, blim=32, taps=96),
    "edge": types.SimpleNamespace(dt=HF, xe=-24, we=-5, be=-29, blim=8, taps=24),
    "straddle": types.SimpleNamespace(dt=HF, xe=-14, we=-14, be=None, blim=0, taps=96),
    "bsub": types.SimpleNamespace(dt=BF, xe=-60, we=-70, be=-136, blim=32, taps=96),
}
RES_LIM = 127  # res / accumulate base: n 2^-24, |n| <= 127 (below 2^-17)
MINS = {}      # (family, fraction) -> minimum over the cases built so far (test_conditions prints it)


def _frac(name, fam, m, least):
    v = float(m.sum()) / m.numel()
    MINS[fam, name] = min(MINS.get((fam, name), 1.0), v)
    assert v >= least, f"{fam}: {name} on {v:.3f} of the outputs only (need {least})"
    return v


def _trunc16(y, dt):
    """Round-toward-zero to ``dt`` (the mutant): where round16(y) overshot |y|, one step back on the bits (the
    magnitude code of a 16-bit float minus one is its neighbour toward zero)."""
    r16 = y.float().to(dt)
    over = r16.double().abs() > y.abs()
    bits = r16.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(dt).double()


def _conditions(fam, y, r, x, dt):
    """The family's conditions on the float64 result ``y`` (unmasked), its rounding ``r`` and the stored ``x``."""
    small = 2.0 ** RO.MIN_NORMAL_EXP[dt]
    inexact = ~RO.representable(y, dt)
    assert torch.equal(inexact, r != y), "representability test disagrees with the conversion"
    tie = RO.ties(y, dt)
    nzsub = (r != 0) & (r.abs() < small)
    if fam == "sub":
        _frac("non-zero subnormal outputs", fam, nzsub, 0.35)
        _frac("ties", fam, tie, 0.05)
        _frac("ties toward zero", fam, tie & (r.abs() < y.abs()), 0.02)
        _frac("ties away from zero", fam, tie & (r.abs() > y.abs()), 0.02)
        _frac("non-zero results that round to zero", fam, (y != 0) & (r == 0), 0.04)
        _frac("non-zero subnormal x", fam, (x != 0) & (x.abs() < small), 0.80)
    elif fam == "edge":
        _frac("non-zero results that round to zero", fam, (y != 0) & (r == 0), 0.30)
        _frac("ties to the even neighbour below", fam, tie & (r.abs() < y.abs()), 0.01)
        _frac("non-zero subnormal outputs", fam, nzsub, 0.08)
    elif fam == "straddle":
        assert bool(((x == 0) | (x.abs() >= small)).all()), "straddle: subnormal operand"
        _frac("non-zero outputs below the smallest normal", fam, nzsub, 0.10)
        _frac("outputs from the smallest normal up", fam, r.abs() >= small, 0.10)
        _frac("inexact", fam, inexact, 0.30)
    else:
        _frac("non-zero outputs below 2^-126", fam, nzsub, 0.10)
        _frac("outputs from 2^-126 up", fam, r.abs() >= small, 0.10)
        _frac("inexact", fam, inexact, 0.30)
        _frac("ties", fam, tie, 0.02)


def _mutants(fam, y, r, y_flushed_x, dt):
    """Mutant separation (asserted on 'sub'): the reference differs from a kernel that flushes subnormal outputs,
    one that flushes subnormal operands (``y_flushed_x``: the result with every subnormal x read as 0) and one
    that rounds toward zero."""
    small = 2.0 ** RO.MIN_NORMAL_EXP[dt]
    _frac("differs from flushed outputs", fam, torch.where(r.abs() < small, torch.zeros_like(r), r) != r, 0.30)
    _frac("differs from flushed operands", fam, RO.round16(y_flushed_x, dt) != r, 0.40)
    _frac("differs from round-toward-zero", fam, _trunc16(y, dt) != r, 0.15)


@functools.lru_cache(maxsize=8)
def _scase(fam, seed, N, H, W, C, OC, k=(3, 3), stride=1, pad=None, dt=None, relu=True, relu_in=False, amode="plain",
           div=1, out_hw=None, kind=None, res=False, acc=False, relu_cols=0, taps=None, xl=None,
           model="single", epi="bf16"):
    """RT._rcase's argument list (``kind`` / ``xl`` are that builder's draws and ignored) on the operands of family
    ``fam``: x = k 2^xe with k in [-3, 3], weights j 2^we with j in [-2, 2] thinned to the family's taps, fp32 bias
    b 2^be. 'straddle' multiplies the weights by one odd integer a <= 1023 chosen per case from the integer sums,
    so that the results lie on both sides of the smallest normal. Both rounding models, the family's conditions,
    fp32-exactness at the family's granularity and the CPU path's equality with 'single' are asserted."""
    F = FAM[fam]
    assert dt in (None, F.dt)
    dt = F.dt
    g = _gen(seed)
    kh, kw_ = k
    pad = (kh // 2, kw_ // 2) if pad is None else pad
    tr = amode == "transpose"
    use_bias = F.be is not None and not tr
    kw = dict(stride=stride, pad=pad, relu=relu, relu_in=relu_in, in_mode=amode, use_bias=use_bias)
    if epi != "bf16":
        kw["epilogue"] = epi
    # 'bsub' without a bias (the transposed gather): products k j 2^-130 would all sit on the 2^-133 grid, so the
    # sums themselves carry the low bits: |k| <= 15, |j| <= 31 at 2^-136
    xlim, wlim, we = (15, 31, F.be - F.xe) if fam == "bsub" and not use_bias else (3, 2, F.we)
    if amode == "unpool":
        xi = _ints(g, (N, H // 2, W // 2, C), -xlim, xlim)
        code = torch.randint(0, 4, (N // div, H // 2, W // 2, C), generator=g, dtype=torch.uint8)
        kw.update(code=code, code_div=div)
        xi_eff = RO.unpool(xi, code, div)
    else:
        xi = xi_eff = _ints(g, (N, H, W, C), -xlim, xlim)
    if relu_in:
        xi_eff = xi_eff.clamp_min(0)
    # (a stride-s transposed gather meets 1 / s^2 of the taps, an unpooled map is 3 / 4 zeros, relu_in halves it)
    taps = (F.taps if taps is None else taps) * (stride * stride if tr else 1) * (4 if amode == "unpool" else 1) * \
        (2 if relu_in else 1)
    cw = _weights(g, OC, C, kh, kw_, kind="transpose" if tr else "fwd", bias=False, taps=taps)
    if wlim != 2:
        cw.w_oihw = cw.w_oihw.sign() * _ints(g, tuple(cw.w_oihw.shape), 1, wlim)
    wi = cw.w_oihw
    ohw = RT._out_hw(xi_eff.shape[1], xi_eff.shape[2], cw, stride, pad, tr, out_hw)
    if out_hw is not None:
        kw["out_hw"] = out_hw
    if relu_cols:
        kw["relu_cols"] = relu_cols
    S = RO.conv_acc(xi_eff, wi, cw.kind, stride, pad, ohw)  # the integer sums
    a = 1
    if fam == "straddle":  # the median non-zero |sum| lands on the smallest normal: 2^(xe + we) a |S| ~ 2^-14
        med = float(S.abs()[S != 0].median())
        a = min(1023, max(1, int(2.0 ** (RO.MIN_NORMAL_EXP[dt] - F.xe - we) / med))) | 1
    x = xi * 2.0 ** F.xe
    cw.w_oihw = (wi.double() * a * 2.0 ** we).float()
    assert torch.equal(cw.w_oihw.to(dt).double(), wi.double() * a * 2.0 ** we), "weights not 16-bit values"
    assert torch.equal(x.to(dt).double(), xi.double() * 2.0 ** F.xe), "x not a 16-bit value"
    acc64 = S * (a * 2.0 ** (F.xe + we))
    bias = None
    if use_bias:
        bias = (_ints(g, (OC,), -F.blim, F.blim).double() * 2.0 ** F.be).float()
        cw.bias = bias
    shape = tuple(acc64.shape)
    more, base = {}, None
    ge = F.xe + we if F.be is None else min(F.xe + we, F.be)  # the result's granularity 2^ge
    if res or acc:
        assert fam == "sub"
        ge = min(ge, -24)
    if res:
        more["res"] = _ints(g, shape, -RES_LIM, RES_LIM) * 2.0 ** -24
    if acc:
        base = _ints(g, shape, -RES_LIM, RES_LIM) * 2.0 ** -24
    okw = dict(res=more.get("res"), base=base, relu_cols=relu_cols)
    y = RO.exact(acc64, bias, relu, **okw)
    # fp32-exactness: every partial sum of every order is a multiple of 2^ge below 2^(ge + 24), at least 2^-149
    x_eff = xi_eff * 2.0 ** F.xe
    _check_fp32_exact(y, x_eff, cw, -ge, stride, pad, (bias, more.get("res"), base))
    bound = float(RO.conv_acc(xi_eff.abs(), wi.abs(), cw.kind, stride, pad, ohw).max()) * a * 2.0 ** (F.xe + we) + \
        sum(float(t.abs().max()) for t in (bias, more.get("res"), base) if t is not None)
    assert bound < 2.0 ** (ge + 24) and ge >= -149, "partial sums not exact in fp32"
    one, two = RO.single(acc64, bias, relu, dt, **okw), RO.staged(acc64, bias, relu, dt, **okw)
    differ = int((one != two).sum())
    if res or acc:
        _check_separation(one, two, OC)
    else:
        assert differ == 0
        _conditions(fam, y, one, x, dt)
        if fam == "sub":
            assert float(x.abs().max()) < 2.0 ** RO.MIN_NORMAL_EXP[dt]  # every x is subnormal or zero
            _mutants(fam, y, one, RO.exact(torch.zeros_like(acc64), bias, relu, **okw), dt)
    refs = dict(single=one, staged=two)
    ckw = {key: v.to(dt) for key, v in more.items()}
    if base is not None:
        ckw.update(out=base.to(dt).clone(), accumulate=True)
    cpu = ops.conv2d(x.to(dt), cw, **kw, **ckw)
    ref = refs[model]
    if epi == "f32":  # no rounding: the fp32 result IS the float64 one
        assert cpu.dtype == F32 and torch.equal(cpu.double(), y), "CPU path != exact result"
        ref = y
    else:
        assert cpu.dtype == dt and torch.equal(cpu.float().double(), refs["single"]), \
            "CPU path != single-rounding oracle"
    return types.SimpleNamespace(x=x, cw=cw, kw=kw, more=more, base=base, ref=ref, refs=refs, dt=dt,
                                 odt=F32 if epi == "f32" else dt, OC=OC, C=C, N=N, epi=epi, model=model, differ=differ)


@functools.lru_cache(maxsize=4)
def _spcase(seed, N, H, W, C, OC, pad=(1, 1)):
    """A ReLU conv with the fused max-pool on 'sub' operands: many distinct fp32 window values round to ONE
    subnormal, so only round-then-compare gives the unfused switch codes (RT._pcase at a new place)."""
    F = FAM["sub"]
    dt = F.dt
    g = _gen(seed)
    xi = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C, taps=F.taps, bias=False)
    wi = cw.w_oihw
    cw.w_oihw = wi * 2.0 ** F.we
    cw.bias = _ints(g, (OC,), -F.blim, F.blim) * 2.0 ** F.be
    x = xi * 2.0 ** F.xe
    ohw = RT._out_hw(H, W, cw, 1, pad, False, None)
    full = RO.exact(RO.conv_acc(xi, wi, "fwd", 1, pad, ohw) * 2.0 ** (F.xe + F.we), cw.bias, True)
    _check_fp32_exact(full, x, cw, -F.be, 1, pad, (cw.bias,))
    r = RO.round16(full, dt)
    assert float(((r != 0) & (r < 2.0 ** -14)).float().mean()) >= 0.35 and bool((r < 2.0 ** -14).all())
    rv, rc = _check_pool_separation(full, dt)
    kw = dict(relu=True, epilogue="pool", pad=pad)
    cv, cc = ops.conv2d(x.to(dt), cw, **kw)
    assert torch.equal(cv.float().double(), rv) and torch.equal(cc, rc), "CPU path != round-then-pool oracle"
    return types.SimpleNamespace(x=x, cw=cw, kw=kw, more={}, base=None, ref=(rv, rc), dt=dt, odt=dt, OC=OC, C=C, N=N,
                                 epi="pool")


def _of(table, d):
    return [name for name, v in table.items() if d in v[2].split()]


SMALL = [(fam, relu) for fam in ("sub", "edge") for relu in (True, False)]
_ID = lambda v: "relu" if v is True else ("signed" if v is False else None)


REDRAW = {("sub", "igemm16"): 1003}  # OC = 5: five bias values decide the densities; a draw that meets them


def _plain_args(name, relu=True, fam=None):
    args = dict(RT.PLAIN[name][0], relu=relu)
    args["seed"] = REDRAW.get((fam, name), args["seed"])
    args.pop("emask", None)  # (the tiny-valued emask has its own section)
    return args


@gpu
@pytest.mark.parametrize("fam,relu", SMALL, ids=[f"{f}-{_ID(r)}" for f, r in SMALL])
@pytest.mark.parametrize("name", _of(RT.PLAIN, "fp16"))
def test_small_plain(native_lib, monkeypatch, name, fam, relu):
    """Every fp16 route's plain store (packed, scalar, element-tail, LDS-staged; split-K reduce; transposed gather;
    relu_cols) on subnormal operands and results: one round-to-nearest-even conversion on the 2^-24 grid, 2^-25
    and below to zero."""
    _run(_scase(fam, **_plain_args(name, relu, fam)), RT.PLAIN[name][1], monkeypatch)


@gpu
@pytest.mark.parametrize("fam,relu", SMALL, ids=[f"{f}-{_ID(r)}" for f, r in SMALL])
@pytest.mark.parametrize("name", sorted(RT.PW_PLAIN))
def test_small_pw(native_lib, monkeypatch, name, fam, relu):
    """The persistent 1x1 kernel's plain store on 'sub' / 'edge' (rows follow the CU count)."""
    C, OC, opts = RT.PW_PLAIN[name]
    G = _cus()
    _, BM, BN = _pw_m(G, OC)
    _run(_scase(fam, **RT._pw_args(G, C, OC, 60 + OC, **opts), relu=relu), R(f"pw {BM}x{BN}", x_extra=8), monkeypatch)


@gpu
@pytest.mark.parametrize("fam,relu", SMALL, ids=[f"{f}-{_ID(r)}" for f, r in SMALL])
@pytest.mark.parametrize("name", sorted(RT.LONG))
def test_small_kw3p_long_grids(native_lib, monkeypatch, name, fam, relu):
    """KW3P stream-K (two fp32 partials of subnormal magnitude handed over) and the KW3P + LDS-DMA tail split on
    'sub' / 'edge': the whole batch, as RT.test_plain_kw3p_long_grids compares it."""
    args, env, tune, n_of, route_of = RT.LONG[name]
    for key, v in env:
        monkeypatch.setenv(key, v)
    G = _cus()
    N = n_of(G)
    tiles = -(-N * 196 // 256)
    assert G < tiles < 2 * G, (tiles, G)
    c = _scase(fam, **dict(args, relu=relu))
    sub = RT.LONG_SUB
    xd = _dev(c.x, c.dt).repeat(-(-N // sub), 1, 1, 1)[:N].contiguous()
    shape = (N,) + tuple(c.ref.shape[1:])
    buf, view = _out_view(shape, c.dt, 0, 8)
    native_lib.sk_errors(True)
    with _tune(*tune):
        got = ops.conv2d(xd, c.cw.to_device(DEV, c.dt), out=view, **c.kw)
        assert _route() == route_of(G), _route()
    torch.cuda.synchronize()
    assert native_lib.sk_errors(True) == 0
    assert _untouched(buf, shape, 0), "wrote outside the output view"
    want = c.ref.float().to(DEV)[torch.arange(N, device=DEV) % sub]
    bad = got.float() != want
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} values differ, first at {bad.nonzero()[0].tolist()}"


@gpu
@pytest.mark.parametrize("fam", ["sub", "edge"])
@pytest.mark.parametrize("name", sorted(RT.UNPOOL_OUT))
def test_small_unpool_out(native_lib, monkeypatch, name, fam):
    """The max-unpool-out epilogues on subnormal results."""
    args, route, tune, env = RT.UNPOOL_OUT[name]
    for key, v in env:
        monkeypatch.setenv(key, v)
    c = _scase(fam, **args)
    code = RT._unpool_codes(c, 2)
    with _tune(*tune), _policy("dma" if name == "dma" else "auto"):
        got = ops.conv2d(_dev(c.x, c.dt), c.cw.to_device(DEV, c.dt), unpool_out=code.to(DEV), unpool_div=2, **c.kw)
        assert _route() == route, _route()
    _same(got, RO.unpool(c.ref, code, 2))


@gpu
@pytest.mark.parametrize("fam", ["sub", "edge"])
def test_small_out2(native_lib, fam):
    """out2 / split_col (the LDS-staged epilogue's two-destination branch), split inside a 64-column tile."""
    c = _scase(fam, **RT._out2_args())
    split, shape = 40, tuple(c.ref.shape)
    b1, v1 = _out_view(shape[:-1] + (split,), c.dt, 8, 8)
    b2, v2 = _out_view(shape[:-1] + (c.OC - split,), c.dt, 8, 16)
    with _tune(3, 1):
        ops.conv2d(_dev(c.x, c.dt), c.cw.to_device(DEV, c.dt), out=v1, out2=v2, split_col=split, **c.kw)
        assert _route() == "dma 128x128 st2 ks1", _route()
    _same(v1, c.ref[..., :split])
    _same(v2, c.ref[..., split:])
    assert _untouched(b1, shape[:-1] + (split,), 8) and _untouched(b2, shape[:-1] + (c.OC - split,), 8), \
        "wrote outside the views"


def _group_cases():
    return [_scase("sub", **dict(p, **({"model": "staged"} if p.get("acc") else {}))) for p in RT.GROUP]


@gpu
def test_small_grouped_launch(native_lib):
    """One grouped launch (csrc/conv_dma_group.hip) on 'sub': two plain problems and one that accumulates a
    subnormal base ('staged')."""
    cases = _group_cases()
    lib = ops.native.lib()
    held = []
    with _policy("auto"):
        lib.conv_group_begin()
        try:
            for c in cases:
                buf, view = _out_view(tuple(c.ref.shape), c.dt, 8, 8)
                kw = dict(c.kw)
                if c.base is not None:
                    view.copy_(_dev(c.base, c.dt))
                    kw["accumulate"] = True
                xd, cwd = _dev(c.x, c.dt), c.cw.to_device(DEV, c.dt)
                ops.conv2d(xd, cwd, out=view, **kw)
                assert _route() == "group cfg8", _route()
                held.append((buf, view, xd, cwd))
        finally:
            launches = lib.conv_group_end()
    assert launches == 1, launches
    for c, (buf, view, *_rest) in zip(cases, held):
        _same(view, c.ref)
        assert _untouched(buf, tuple(c.ref.shape), 8), "wrote outside the output view"


# conv_igemm's relu_in (relu_bf2 on the bits of subnormal x), which no fp16 recipe of RT.PLAIN carries: RR.IG_MODES'
# "relu_in" shape in fp16. (The fused unpool gather has no fp16 instantiation: conv_igemm_launch refuses it.)
IG_SMALL = {"relu_in": (dict(seed=206, N=3, H=13, W=15, C=64, OC=128, relu_in=True), 128)}


@gpu
@pytest.mark.parametrize("fam", ["sub", "edge"])
@pytest.mark.parametrize("name", sorted(IG_SMALL))
def test_small_igemm_relu_in(native_lib, name, fam):
    """relu_in on signed subnormal fp16 inputs (policy 'reg'): the negative ones become 0, the positive ones pass."""
    args, bn = IG_SMALL[name]
    c = _scase(fam, **args)
    got, r, _ = _launch(c, "reg")
    assert r == f"igemm {RR.IG[bn][0]}x{bn}", r
    _same(got, c.ref)


# one recipe per kernel file with an fp16 instantiation (conv_igemm, conv_halo_stream, conv_dma, its split-K
# reduce, conv_dma_impl.h's KW3 and KW3P kernels); the persistent 1x1 kernel has its own test below
STRADDLE = ["igemm64", "igemm_transpose", "hs16_oc64_lds", "hs32_oc64_reg", "dma_lds", "dma_reg", "dma_splitk",
            "kw3_256", "kw3p_lds"]


@gpu
@pytest.mark.parametrize("name", STRADDLE)
def test_straddle(native_lib, monkeypatch, name):
    """Normal fp16 operands, results on both sides of 2^-14: where the grid stops following the exponent."""
    _run(_scase("straddle", **_plain_args(name, RT.PLAIN[name][0].get("relu", True))), RT.PLAIN[name][1], monkeypatch)


def _straddle_pw_args(G):
    return RT._pw_args(G, 64, 128, 188)


@gpu
def test_straddle_pw(native_lib, monkeypatch):
    G = _cus()
    _, BM, BN = _pw_m(G, 128)
    _run(_scase("straddle", **_straddle_pw_args(G)), R(f"pw {BM}x{BN}", x_extra=8), monkeypatch)


@gpu
@pytest.mark.parametrize("name", _of(RT.PLAIN, "bf16"))
def test_bsub(native_lib, monkeypatch, name):
    """Every bf16 route with fp32-SUBNORMAL accumulators (products k j 2^-130, bias b 2^-136): bf16 results on
    both sides of 2^-126, rounded to nearest even on the 2^-133 grid below it."""
    _run(_scase("bsub", **_plain_args(name, True)), RT.PLAIN[name][1], monkeypatch)


# res / accumulate on 'sub': the routes of RT.POST against the model the Round 15 table assigns them. (On the fixed
# grid the models part on ties with an odd res / base only, 6 % of signed results; a ReLU halves that: not a case.)
POST_SMALL = ["dma_lds", "dma_reg", "dma_splitk", "kw3_lds", "kw3_reg"]
POST_VARIANTS = ("res", "acc")


def _post_args(name, variant):
    return dict(RT.POST[name][0], **RT.VARIANTS[variant], model=RT.POST[name][2])


@gpu
@pytest.mark.parametrize("variant", POST_VARIANTS)
@pytest.mark.parametrize("name", POST_SMALL)
def test_small_post_ops(native_lib, monkeypatch, name, variant):
    """res / accumulate of fp16 multiples of 2^-24 below 2^-17 onto 'sub' results: on the fixed grid the two
    models part exactly where v is a tie and res / base is odd (>= 5 % of the outputs)."""
    c = _scase("sub", **_post_args(name, variant))
    assert c.differ > 0
    _run(c, RT.POST[name][1], monkeypatch)


PW_POST_SMALL = {"res_oc128": (64, 128, "res"), "acc_oc64": (64, 64, "acc"), "res_oc256": (64, 256, "res")}


def _pw_post_args(G, name):
    C, OC, variant = PW_POST_SMALL[name]
    return RT._pw_args(G, C, OC, 90 + OC, **RT.VARIANTS[variant], model="staged")


@gpu
@pytest.mark.parametrize("name", sorted(PW_POST_SMALL))
def test_small_post_ops_pw(native_lib, monkeypatch, name):
    """The persistent 1x1 kernel (epilogue_lds: 'staged') with a subnormal res / base."""
    G = _cus()
    _, BM, BN = _pw_m(G, PW_POST_SMALL[name][1])
    _run(_scase("sub", **_pw_post_args(G, name)), R(f"pw {BM}x{BN}", vec=True, x_extra=8), monkeypatch)


@gpu
@pytest.mark.parametrize("epi", sorted(RT.POOL_EPI))
@pytest.mark.parametrize("N,H,W,C,OC,cfg,tile", RT.POOL_DMA)
def test_small_pool_dma(native_lib, monkeypatch, N, H, W, C, OC, cfg, tile, epi):
    """The LDS-DMA kernel's three pooled-max epilogues (the fused pool's only fp16 instantiations) compare
    STORED subnormals: values and first-max switch codes of round-then-pool."""
    c = _spcase(100 + OC, N, H, W, C, OC)
    _run(c, R(f"dma {tile} ks1 {epi}", "auto", (cfg, 0), RT.POOL_EPI[epi]), monkeypatch)


def _f32_args():
    return dict(RR.DENSE["pred_up_m5"][0], epi="f32", relu=False)


@gpu
def test_small_f32_dense_head(native_lib):
    """epilogue='f32' on subnormal fp16 operands (the dense head's logits, M = 5, K = 4096, split-K 4): the fp32
    result needs no rounding and equals the float64 one."""
    args = _f32_args()
    args.pop("bias", None)
    c = _scase("sub", **args)
    got, r, _ = _launch(c, "auto")
    assert r == RR.DENSE["pred_up_m5"][1], r
    _same(got, c.ref)


# ----------------------------------------------------------------------------------------
# B. the mask predicate on tiny values: conv2d's mask / emask / ebits / obits
# ----------------------------------------------------------------------------------------

def _bits_of(t):
    """packbits(t > 0) over channels: bit c % 8 of byte c / 8, rows = pixels."""
    return np.packbits((t.double() > 0).numpy().reshape(-1, t.shape[-1]), axis=1, bitorder="little")


@functools.lru_cache(maxsize=8)
def _mcase(dt, seed, N, H, W, C, OC, k=(3, 3), stride=1, pad=None, relu=True, amode="plain", out_hw=None, bias=True,
           mask=False, emask=False, res=False, acc=False, epi="bf16", taps=96, relu_in=False, **_ignored):
    """RR._case's integer operands with the masks drawn by ``_signs_tiny``, against float64 F.conv2d and
    ``torch.where(mask > 0, ...)`` (rounding_oracle.conv_acc / exact: nothing of the code under test). Results are
    integers a 16-bit float holds: no rounding model is involved."""
    g = _gen(seed)
    kh, kw_ = k
    pad = (kh // 2, kw_ // 2) if pad is None else pad
    tr = amode == "transpose"
    use_bias = bias and not tr
    kw = dict(stride=stride, pad=pad, relu=relu, relu_in=relu_in, in_mode=amode, use_bias=use_bias)
    if epi != "bf16":
        kw["epilogue"] = epi
    x = _ints(g, (N, H, W, C), -3, 3)
    cw = _weights(g, OC, C, kh, kw_, kind="transpose" if tr else "fwd", bias=use_bias,
                  taps=taps * (stride * stride if tr else 1) * (3 if mask else 1))
    x_eff = x.double()
    if mask:
        kw["mask"] = m = _signs_tiny(g, tuple(x.shape), dt)
        x_eff = torch.where(m.double() > 0, x_eff, torch.zeros_like(x_eff))
        assert abs(float((m.double() > 0).float().mean()) - 0.375) < 0.05
    if relu_in:
        x_eff = x_eff.clamp_min(0)
    ohw = RT._out_hw(H, W, cw, stride, pad, tr, out_hw)
    if out_hw is not None:
        kw["out_hw"] = out_hw
    acc64 = RO.conv_acc(x_eff, cw.w_oihw, cw.kind, stride, pad, ohw)
    shape = tuple(acc64.shape)
    more, base = {}, None
    if res:
        more["res"] = _ints(g, shape, -4, 4)
    if acc:
        base = _ints(g, shape, -4, 4)
    em = _signs_tiny(g, shape, dt) if emask else None
    plain = RO.exact(acc64, cw.bias if use_bias else None, relu, res=more.get("res"), base=base)
    ref = RO.exact(acc64, cw.bias if use_bias else None, relu, res=more.get("res"), base=base, emask=em)
    assert torch.equal(plain.float().to(dt).double(), plain) and float(plain.abs().max()) < 2 ** 11
    assert float((ref != 0).float().mean()) >= 0.10 and ref.flatten()[:65536].unique().numel() >= 16
    if em is not None:
        more["emask"] = em
        # the six non-positive mask values zero results that are not zero by themselves, the tiny positive ones keep
        for i, bits in enumerate(_tiny_codes(dt)):
            sel = em.view(torch.int16) == bits
            assert bool(sel.any())
            kept = bool((ref[sel] != 0).any())
            assert kept == (float(em[sel][0]) > 0) and bool((plain[sel] != 0).any()), (i, bits)
    ckw = {key: v.to(dt) for key, v in more.items()}
    if base is not None:
        ckw.update(out=base.to(dt).clone(), accumulate=True)
    cpu = ops.conv2d(x.to(dt), cw, **kw, **ckw)
    assert torch.equal(cpu.double(), ref), "CPU path != oracle"
    return types.SimpleNamespace(x=x, cw=cw, kw=kw, more=more, base=base, ref=ref, dt=dt,
                                 odt=F32 if epi == "f32" else dt, OC=OC, C=C, N=N, epi=epi)


def _tiny_codes(dt):
    sub, nrm = TINY_BITS[dt]
    one = int(torch.ones((), dtype=dt).view(torch.int16))
    pos = [one, 0, sub, nrm]
    return [b if b < 0x8000 else b - 0x10000 for b in pos + [b | 0x8000 for b in pos]]


def _margs(args):
    a = dict(args)
    dt = a.pop("dt", BF)
    return dt, a


# A side: conv_igemm with the mask at its own pixel stride (forward, transposed, fp32 epilogue), the LDS-DMA
# kernel's staged mask (256 x 16 tile, with and without split-K)
MASK_IG = ["mask_fwd_bf16", "mask_fwd_fp16", "mask_tr_bf16", "mask_tr_fp16", "mask_f32"]
MASK_DMA = ["oc5_mask", "oc16_mask_fp16"]


@gpu
@pytest.mark.parametrize("name", MASK_IG)
def test_tiny_mask_igemm(native_lib, name):
    args, largs, policies, bn = RR.IG_MODES[name]
    dt, a = _margs(args)
    c = _mcase(dt, **a)
    for policy in policies:
        got, r, _ = _launch(c, policy, **largs)
        assert r == f"igemm {RR.IG[bn][0]}x{bn}", (policy, r)
        _same(got, c.ref)


@gpu
@pytest.mark.parametrize("auto_ks", [False, True], ids=["ks1", "auto"])
@pytest.mark.parametrize("name", MASK_DMA)
def test_tiny_mask_dma(native_lib, name, auto_ks):
    dt, a = _margs(dict(RR.DMA16)[name])
    c = _mcase(dt, **a)
    with _tune(0, 0 if auto_ks else 1):
        got, r, _ = _launch(c, "dma")
    assert r == f"dma 256x16 st2 ks{2 if auto_ks else 1} mask", r
    _same(got, c.ref)


# emask: the recipes of RT.PLAIN / RT.POST that carry one (hs16 / hs32 LDS and register forms, the channel-split
# form, the LDS-DMA register / LDS epilogues and epi_tail, KW3, the split-K reduce), both dtypes
EMASK_PLAIN = ["hs16_emask", "hs16_emask_reg", "hs32_ocsplit_emask", "dma_tail_emask"]
EMASK_POST = [("dma_reg", "res_relu_emask"), ("dma_lds", "acc_emask"), ("dma_lds_oc44", "res_relu_emask"),
              ("dma_splitk", "acc_emask"), ("kw3_lds", "res_relu_emask"), ("kw3_reg", "acc_emask")]


def _emask_args(name, variant):
    if variant is None:
        return dict(RT.PLAIN[name][0])
    return dict(RT.POST[name][0], **RT.VARIANTS[variant])


def _emask_cases():
    return [(n, None) for n in EMASK_PLAIN] + EMASK_POST


@gpu
@pytest.mark.parametrize("d", sorted(RT.DTS))
@pytest.mark.parametrize("name,variant", _emask_cases())
def test_tiny_emask(native_lib, monkeypatch, name, variant, d):
    """emask drawn from the eight tiny / unit values on integer payloads: kept iff > 0 as a real number."""
    rec = (RT.PLAIN[name] if variant is None else RT.POST[name])[1]
    _run(_mcase(RT.DTS[d], **_emask_args(name, variant)), rec, monkeypatch)


PW_EMASK = {"acc_emask_oc128": (64, 128, "acc_emask"), "res_relu_emask_oc64": (64, 64, "res_relu_emask")}


@gpu
@pytest.mark.parametrize("d", sorted(RT.DTS))
@pytest.mark.parametrize("name", sorted(PW_EMASK))
def test_tiny_emask_pw(native_lib, monkeypatch, name, d):
    C, OC, variant = PW_EMASK[name]
    G = _cus()
    _, BM, BN = _pw_m(G, OC)
    c = _mcase(RT.DTS[d], **RT._pw_args(G, C, OC, 90 + OC, **RT.VARIANTS[variant]))
    _run(c, R(f"pw {BM}x{BN}", vec=True, x_extra=8), monkeypatch)


def _bits_cases(G):
    out = [(t[:6], t[6] + " lds") for t in RR.HS_BITS]
    for OC, dt in [(128, BF), (64, HF)]:
        M, BM, BN = _pw_m(G, OC)
        out.append(((1, RT.PW_H, M // RT.PW_H, 64, OC, dt, (1, 1)), f"pw {BM}x{BN}"))
    return out


def _check_tiny_bits(shape, route):
    """ebits = packbits(emask > 0 as a real number) with the tiny emask alongside; obits of 'sub' outputs (fp16):
    set for a positive subnormal result, clear for one that rounded to zero."""
    fwd, msk = RR._bits_args(*shape)
    dt, a = _margs(msk)
    cm = _mcase(dt, **a)
    eb = torch.from_numpy(_bits_of(cm.more["emask"])).to(DEV)
    got, r, bits = _launch(cm, "auto", right=0, ebits=eb)
    assert r == route and bits == 2, (r, bits)
    _same(got, cm.ref)
    if dt == HF:
        dt, a = _margs(fwd)
        c = _scase("sub", **a)
        tiny_pos = (c.ref > 0) & (c.ref < 2.0 ** -14)
        assert float(tiny_pos.float().mean()) >= 0.35  # (and >= 4 % positive results rounded to zero: 'sub')
        ob = torch.full((c.ref.numel() // c.OC, c.OC // 8), 0xA5, dtype=torch.uint8, device=DEV)
        got, r, bits = _launch(c, "auto", right=0, obits=ob)
        assert r == route and bits == 1, (r, bits)
        _same(got, c.ref)
        assert np.array_equal(ob.cpu().numpy(), _bits_of(c.ref)), "obits != packbits(reference > 0)"


@gpu
@pytest.mark.parametrize("i", range(6))
def test_tiny_bits(native_lib, i):
    """1-bit masks on the halo-stream LDS-staged epilogues and the persistent 1x1 kernel: bits_flags() asserted."""
    shape, route = _bits_cases(_cus())[i]
    _check_tiny_bits(shape, route)


# ----------------------------------------------------------------------------------------
# B. the other kernels that evaluate the predicate, and the max-pool on tiny windows
# ----------------------------------------------------------------------------------------

def _tiny_windows(g, shape, dt):
    """Values from {-0.0, +0.0, +-smallest subnormal, +-twice that} as a ``dt`` tensor."""
    codes = torch.tensor([0x0000, 0x0001, 0x0002], dtype=torch.int32)
    codes = torch.cat([codes, codes | 0x8000])
    codes = torch.where(codes >= 0x8000, codes - 0x10000, codes).to(torch.int16)
    return codes.view(dt)[torch.randint(0, 6, shape, generator=g)]


@functools.lru_cache(maxsize=None)
def _pool_tiny_case(dt, N, H, W, C):
    x = _tiny_windows(_gen(900 + C), (N, H, W, C), dt)
    val, code = RO.pool_first_max(x.double())
    win = RO.windows(x.double())
    top2 = win.topk(2, dim=3).values
    assert float((top2[..., 0, :] == top2[..., 1, :]).float().mean()) >= 0.25, "too few tied windows"
    # (a window's maximum is a zero in about 19 % of the draws; a third of those hold zeros of both signs)
    neg0, pos0 = (win == 0) & torch.signbit(win), (win == 0) & ~torch.signbit(win)
    both = (val == 0) & neg0.any(3) & pos0.any(3)
    assert float(both.float().mean()) >= 0.02, "too few windows whose maximum is tied between -0.0 and +0.0"
    assert bool((both & (neg0.to(torch.int8).argmax(3) < pos0.to(torch.int8).argmax(3))).any()), "-0.0 never first"
    assert bool(((val == 0) & (win < 0).any(3)).any()), "no negative subnormal losing to a zero"
    return types.SimpleNamespace(x=x, val=val, code=code)


POOL_TINY = TDC.POOL_EDGE[:2]  # (2, 6, 10, 8): the vectorized kernel; (2, 6, 10, 12): the scalar one


@gpu
@pytest.mark.parametrize("d", sorted(RT.DTS))
@pytest.mark.parametrize("N,H,W,C", POOL_TINY)
def test_maxpool_tiny_windows(native_lib, N, H, W, C, d):
    """maxpool2x2 on windows of zeros of both signs and the four smallest subnormals: the first maximum wins,
    -0.0 and +0.0 tie, a negative subnormal loses to either zero."""
    dt = RT.DTS[d]
    c = _pool_tiny_case(dt, N, H, W, C)
    out = torch.full((N, H // 2, W // 2, C), SENT, dtype=dt, device=DEV)
    code = torch.full((N, H // 2, W // 2, C), 255, dtype=torch.uint8, device=DEV)
    native_lib.maxpool2x2(c.x.to(DEV), out, code)
    assert TDC._misc_route() == ("maxpool2x2 vec" if C % 8 == 0 else "maxpool2x2 scalar")
    _same(out, c.val)
    assert torch.equal(code.cpu(), c.code), "switch codes differ"


@functools.lru_cache(maxsize=2)
def _pool_fused_tiny_case(dt):
    """One fused-pool recipe (the LDS-DMA kernel's pool_t epilogue, RT.POOL_DMA[2]) on windows of tiny values: a
    1-tap conv (weight 1 on the centre tap of channel oc % C, no bias, no ReLU) copies x's tiny windows to the
    output, so the stored values compared are zeros of both signs and the smallest subnormals."""
    N, H, W, C, OC, cfg, tile = RT.POOL_DMA[2]
    x = _tiny_windows(_gen(905), (N, H, W, C), dt)
    w = torch.zeros(OC, C, 3, 3)
    w[torch.arange(OC), torch.arange(OC) % C, 1, 1] = 1.0
    cw = Cm.ConvWeights(w, None, "fwd")
    full = x.double()[..., torch.arange(OC) % C]
    rv, rc = RO.pool_first_max(full)
    kw = dict(relu=False, epilogue="pool", use_bias=False)
    cv, cc = ops.conv2d(x, cw, **kw)
    assert torch.equal(cv.double(), rv) and torch.equal(cc, rc), "CPU path != oracle"
    neg0 = (RO.windows(full) == 0) & torch.signbit(RO.windows(full))
    assert bool(((rv == 0) & neg0[..., 0, :]).any())  # a -0.0 first in a window whose maximum is a zero
    return types.SimpleNamespace(x=x, cw=cw, kw=kw, more={}, base=None, ref=(rv, rc), dt=dt, odt=dt, OC=OC, C=C, N=N,
                                 epi="pool")


@gpu
@pytest.mark.parametrize("d", sorted(RT.DTS))
def test_fused_pool_tiny_windows(native_lib, monkeypatch, d):
    """The same windows through a conv's fused pool epilogue (products x * 1 are exact, -0.0 + 0.0 sums aside:
    the sign of a zero is not compared, its tie with the other zero is)."""
    N, H, W, C, OC, cfg, tile = RT.POOL_DMA[2]
    _run(_pool_fused_tiny_case(RT.DTS[d]), R(f"dma {tile} ks1 pool_t", "auto", (cfg, 0)), monkeypatch)


UNPOOL_TINY = [(4, 3, 5, C, div) for C in (8, 12) for div in (1, 2)]  # TDC.UNPOOL_EDGE's shapes, relu on


@functools.lru_cache(maxsize=None)
def _unpool_tiny_case(dt, N, PH, PW, C, div):
    g = _gen(910 + C + div)
    p = _signs_tiny(g, (N, PH, PW, C), dt)
    code = torch.randint(0, 4, (N // div, PH, PW, C), generator=g, dtype=torch.uint8)
    ref = RO.unpool(torch.where(p.double() > 0, p.double(), torch.zeros(())), code, div)
    assert float((ref != 0).float().mean()) >= 0.06
    assert bool(((ref > 0) & (ref < 2.0 ** RO.SUB_GRID_EXP[dt] * 1.5)).any())
    return types.SimpleNamespace(p=p, code=code, ref=ref)


@gpu
@pytest.mark.parametrize("d", sorted(RT.DTS))
@pytest.mark.parametrize("N,PH,PW,C,div", UNPOOL_TINY)
def test_unpool_relu_tiny(native_lib, N, PH, PW, C, div, d):
    """unpool2x2 with its ReLU (a bit test): the tiny positive values pass unchanged, the five others give 0."""
    dt = RT.DTS[d]
    c = _unpool_tiny_case(dt, N, PH, PW, C, div)
    out = torch.full((N, 2 * PH, 2 * PW, C), SENT, dtype=dt, device=DEV)
    native_lib.unpool2x2(c.p.to(DEV), c.code.to(DEV), out, div, True)
    assert TDC._misc_route() == ("unpool2x2 vec" if C % 8 == 0 else "unpool2x2 scalar")
    _same(out, c.ref)


SCATTER_TINY = [(C, s, 7, 9) for C in (8, 24) for s in (1, 2)]  # TD.SCATTER_CASES' shapes, masked


@functools.lru_cache(maxsize=None)
def _scatter_tiny_case(dt, C, s, H, W):
    g = _gen(920 + C + s)
    N = 2
    E = _ints(g, (N, -(-H // s), -(-W // s), C), 1, 4) * (2 * torch.randint(0, 2, (N, -(-H // s), -(-W // s), C),
                                                                              generator=g) - 1)
    em = _signs_tiny(g, (N, H, W, C), dt)
    gx = torch.zeros(N, H, W, C, dtype=torch.float64)
    gx[:, ::s, ::s] = E.double()
    gx = torch.where(em.double() > 0, gx, torch.zeros(()))
    _each_code_decides(em, gx, dt)
    return types.SimpleNamespace(N=N, E=E, em=em, gx=gx)


def _each_code_decides(em, ref, dt, live=None):
    """Each of the eight mask codes meets a non-zero payload, and the result there is non-zero iff the code is > 0."""
    for bits in _tiny_codes(dt):
        sel = em.view(torch.int16) == bits
        if live is not None:
            sel = sel & live
        assert bool(sel.any()), bits
        assert bool((ref[sel] != 0).any()) == (float(em[em.view(torch.int16) == bits][0]) > 0), bits


@gpu
@pytest.mark.parametrize("d", sorted(RT.DTS))
@pytest.mark.parametrize("C,s,H,W", SCATTER_TINY)
def test_subpixel_scatter_tiny_mask(native_lib, C, s, H, W, d):
    """subpixel_scatter_kernel's float compare on the tiny mask values."""
    dt = RT.DTS[d]
    c = _scatter_tiny_case(dt, C, s, H, W)
    gx = torch.full((c.N, H, W, C), SENT, dtype=dt, device=DEV)
    native_lib.subpixel_scatter(_dev(c.E, dt), c.em.to(DEV), gx, s)
    _same(gx, c.gx)


@functools.lru_cache(maxsize=None)
def _merge_tiny_case(dt, acc):
    """test_conv_exact_gpu.py's stride-2 sub-pixel merge (3x3 / 2, 17 x 17, 96 -> 64) with the tiny emask."""
    g = _gen(930 + acc)
    k, s, p, H, C, OC, N = 3, 2, 0, 17, 64, 96, 2
    w = _ints(g, (OC, C, k, k), -2, 2) * (torch.rand(OC, C, k, k, generator=g) < 0.4)
    OH = (H + 2 * p - k) // s + 1
    gy = _ints(g, (N, OH, OH, OC), -3, 3)
    base = _ints(g, (N, H, H, C), 1, 4) * torch.where(torch.rand(N, H, H, C, generator=g) < 0.5, -1.0, 1.0)
    em = _signs_tiny(g, (N, H, H, C), dt)
    grad = torch.nn.functional.conv_transpose2d(gy.double().permute(0, 3, 1, 2), w.double(), None, stride=s,
                                                padding=p).permute(0, 2, 3, 1)
    assert grad.shape == base.shape
    ref = torch.where(em.double() > 0, grad + base.double() if acc else grad, torch.zeros(()))
    assert torch.equal(ref.float().to(dt).double(), ref) and float((ref != 0).float().mean()) > 0.15
    _each_code_decides(em, ref, dt)
    return types.SimpleNamespace(w=w, gy=gy, base=base, em=em, ref=ref, s=s, p=p, H=H, N=N, C=C)


@gpu
@pytest.mark.parametrize("d", sorted(RT.DTS))
@pytest.mark.parametrize("acc", [False, True], ids=["fresh", "acc"])
def test_subpixel_merge_tiny_mask(native_lib, acc, d):
    """subpixel_merge_kernel (float compare), into a fresh gradient and accumulating into an old one."""
    dt = RT.DTS[d]
    c = _merge_tiny_case(dt, acc)
    u = AG.ConvUnit("u", c.w, None, c.s, (c.p, c.p)).build(DEV, dt)
    out = _dev(c.base, dt) if acc else torch.full((c.N, c.H, c.H, c.C), SENT, dtype=dt, device=DEV)
    assert AG._subpixel_ok(u, out), "class layout not taken by the native merge"
    AG._subpixel_dgrad(_dev(c.gy, dt), None, u, (c.H, c.H), out=out, accumulate=acc, emask=c.em.to(DEV))
    _same(out, c.ref)


STEM_TINY = (17, 33)  # TD.STEM_FUSED_CASES: 2 x 2 tiles with tails


@functools.lru_cache(maxsize=None)
def _stem_tiny_case(dt):
    H, W = STEM_TINY
    g = _gen(940)
    N, k, pad = 2, 7, 3
    cw = _weights(g, 64, 3, k, k, bias=False, taps=14 * 3)  # (3 mask values in 8 keep)
    OH, OW = (H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1
    gy = _ints(g, (N, OH, OW, 64), -3, 3)
    mask = _signs_tiny(g, (N, OH, OW, 64), dt)
    gym = torch.where(mask.double() > 0, gy.double(), torch.zeros(()))
    opad = (H - ((OH - 1) * 2 - 2 * pad + k), W - ((OW - 1) * 2 - 2 * pad + k))
    gx = torch.nn.functional.conv_transpose2d(gym.permute(0, 3, 1, 2), cw.w_oihw.double(), None, stride=2, padding=pad,
                                              output_padding=opad).permute(0, 2, 3, 1)
    cols = torch.einsum("nhwo,ocyx->nhwyxc", gym, cw.w_oihw.double())  # the 16-bit intermediate of both paths
    for t in (cols, gx):
        assert torch.equal(t.float().to(dt).double(), t)
    assert float((gx != 0).float().mean()) >= 0.25
    # the mask decides: dropping the tiny positive values, or keeping the tiny negative ones, changes gx
    for wrong in (mask.double() >= 2.0 ** -10, mask.double() != 0):
        alt = torch.nn.functional.conv_transpose2d(torch.where(wrong, gy.double(), torch.zeros(())).permute(0, 3, 1, 2),
                                                   cw.w_oihw.double(), None, stride=2, padding=pad, output_padding=opad)
        assert float((alt.permute(0, 2, 3, 1) != gx).float().mean()) >= 0.25
    return types.SimpleNamespace(N=N, w=cw.w_oihw, gy=gy, mask=mask, gx=gx)


@gpu
@pytest.mark.parametrize("d", sorted(RT.DTS))
def test_stem_dgrad_fused_tiny_mask(native_lib, d):
    """ResNet-50 conv1's fused input gradient (mask_pos_pk on the bits) with the tiny ReLU mask."""
    dt = RT.DTS[d]
    H, W = STEM_TINY
    c = _stem_tiny_case(dt)
    unit = AG.ConvUnit("u", c.w, None, 2, (3, 3), relu=True).build(DEV, dt)
    assert unit.stem_w is None and unit.col_w is not None
    gx = torch.full((c.N, H, W, 8), SENT, dtype=dt, device=DEV)
    assert native_lib.stem_dgrad_fused(_dev(c.gy, dt), c.mask.to(DEV), unit.col_w.w_gemm, gx, [7, 7, 2, 3, 3])
    _same(gx[..., :3], c.gx)
    assert not bool(gx[..., 3:].float().any()), "padding channels must get a zero gradient"


PREMASKED_GEOM = (5, 1, 2, 48, 64)  # test_blocks_exact_gpu.CONV_GEOMS' stride-1 unit on its 2 x 9 x 11 map


@functools.lru_cache(maxsize=None)
def _premasked_tiny_case(dt):
    k, s, p, cin, cout = PREMASKED_GEOM
    g = _gen(950)
    w = _ints(g, (cout, cin, k, k), -2, 2) * (torch.rand(cout, cin, k, k, generator=g) < 96 / (cout * k * k))
    x = _signs_tiny(g, (2, 9, 11, cin), dt)  # the unit's input, tagged a ReLU output: its gradient's emask
    gy = _ints(g, (2, 9, 11, cout), -3, 3)
    grad = torch.nn.functional.conv_transpose2d(gy.double().permute(0, 3, 1, 2), w.double(), None, padding=p)
    gx = torch.where(x.double() > 0, grad.permute(0, 2, 3, 1), torch.zeros(()))
    assert torch.equal(gx.float().to(dt).double(), gx)
    _each_code_decides(x, gx, dt)
    return types.SimpleNamespace(w=w, x=x, gy=gy, gx=gx, k=k, s=s, p=p)


@gpu
@pytest.mark.parametrize("d", sorted(RT.DTS))
def test_premasked_gradient_tiny_input(native_lib, d):
    """ops/autograd.py's premasked contract: the gradient a conv unit returns is masked by its (ReLU-tagged)
    input > 0 in the dgrad's emask epilogue; the input holds the tiny values. (The forward result, which sums them,
    is not compared.)"""
    dt = RT.DTS[d]
    c = _premasked_tiny_case(dt)
    u = AG.ConvUnit("u", c.w, None, c.s, (c.p, c.p), relu=False).build(DEV, dt)
    xd = c.x.to(DEV).requires_grad_(True)
    with AG.premasked_grads():
        y = u(AG.tag_relu_output(xd))
    (gx,) = torch.autograd.grad(y, xd, _dev(c.gy, dt))
    assert _route().startswith("dma "), _route()
    _same(gx, c.gx)


GUIDE_TINY = (2, 9, 11, 64, 16, 2)  # test_dream_guide_exact_gpu.CASES[1]


@functools.lru_cache(maxsize=None)
def _guide_tiny_case(dt):
    """guide_match's masked form with an activation made of tiny values only: +-0.0, +-smallest subnormal,
    +-smallest normal (no +-1: scores k 2^e with integer k < 2^24 stay exact in fp32, for bf16 as fp32 subnormals),
    guide rows integers in [0, 3]. The gradient term scale y[q*] passes where a > 0 as a real number."""
    N, H, W, C, Q, b = GUIDE_TINY
    g = _gen(960)
    sub, nrm = TINY_BITS[dt]
    codes = torch.tensor([0, sub, nrm, 0x8000 - 0x10000, (sub | 0x8000) - 0x10000, (nrm | 0x8000) - 0x10000],
                         dtype=torch.int16)
    a = codes.view(dt)[torch.randint(0, 6, (N, H, W, C), generator=g)]
    y = _ints(g, (N, Q, C), 0, 3) * (torch.rand(N, Q, C, generator=g) < 0.5)
    gidx = [(n + 1) % N for n in range(N)]
    scale = torch.tensor([0.5, 0.25])
    addend = _ints(g, (N, H, W, C), -4, 4)
    Hc, Wc = H - 2 * b, W - 2 * b
    s = np.einsum("npc,nqc->npq", a[:, b:H - b, b:W - b].reshape(N, Hc * Wc, C).double().numpy(),
                  y[gidx].double().numpy())
    unit = 2.0 ** RO.SUB_GRID_EXP[dt]
    assert np.array_equal(np.round(s / unit), s / unit)
    assert float(np.abs(a.double().numpy()).sum(-1).max()) * 3 / unit < 2 ** 24
    win = s.argmax(axis=2)
    best = np.take_along_axis(s, win[..., None], axis=2)[..., 0]
    loss = torch.from_numpy(best.sum(axis=1))
    assert float(np.abs(best).sum(axis=1).max()) / unit < 2 ** 24 and len(np.unique(win)) >= 8
    rows = torch.stack([y[gidx[n]][torch.from_numpy(win[n])] for n in range(N)])
    term = torch.zeros(N, H, W, C, dtype=torch.float64)
    term[:, b:H - b, b:W - b] = (scale.view(N, 1, 1) * rows).view(N, Hc, Wc, C).double()
    grad = torch.where(a.double() > 0, term, torch.zeros(()))
    core = torch.zeros(N, H, W, C, dtype=torch.bool)
    core[:, b:H - b, b:W - b] = True
    _each_code_decides_guide(a, grad, codes, core)
    return types.SimpleNamespace(a=a, y=y, gidx=gidx, scale=scale, addend=addend, loss=loss,
                                 ref=addend.double() + grad, b=b)


def _each_code_decides_guide(a, grad, codes, core):
    for bits in codes.tolist():
        sel = (a.view(torch.int16) == bits) & core
        assert bool(sel.any()) and bool((grad[sel] != 0).any()) == (float(a[sel][0]) > 0), bits


@gpu
@pytest.mark.parametrize("d", sorted(RT.DTS))
def test_guide_match_tiny_mask(native_lib, d):
    """csrc/dream_guide.hip: the masked gradient (a float compare on a) and the loss on tiny activations."""
    dt = RT.DTS[d]
    c = _guide_tiny_case(dt)
    N = c.a.shape[0]
    gx = torch.full(tuple(c.a.shape), SENT, dtype=dt, device=DEV)
    part = torch.full((N, 1), SENT, dtype=torch.float32, device=DEV)
    native_lib.guide_match(c.a.to(DEV), _dev(c.y, dt), AG.guide_index(c.gidx, N, DEV), c.scale.to(DEV), gx, c.b,
                           _dev(c.addend, dt), part, True)
    _same(gx, c.ref)
    assert torch.equal(part.double().sum(1).cpu(), c.loss), (part.tolist(), c.loss.tolist())


# ----------------------------------------------------------------------------------------
# C. NaN in the slack
# ----------------------------------------------------------------------------------------
NAN = float("nan")
# c8_stream takes dense 8-channel rows only (conv3x3_c8_stream_launch refuses x_ld != 8): it has no slack to poison
SLACK_DENSE_X = ("c8_stream",)
SLACK_TAIL = ["igemm64", "halo_persist", "hs16_oc64_lds", "dma_lds", "kw3_256", "kw3p_lds"]  # one per kernel file


def _slack_largs(name):
    args, rec, _ = RT.PLAIN[name]
    largs = dict(rec.largs, x_fill=NAN, more_fill=NAN, mask_fill=NAN)
    largs["x_extra"] = 24 if args["C"] % 64 else 8
    if args.get("emask"):
        largs["more_extra"] = largs.get("more_extra", 0) or 8
    return largs


def _run_slack(c, rec, largs, monkeypatch):
    for key, v in rec.env.items():
        monkeypatch.setenv(key, v)
    with _tune(*rec.tune):
        got, r, _ = _launch(c, rec.policy, **largs)
    assert r == rec.route, r
    assert bool(torch.isfinite(got.float()).all()), "NaN from the slack reached a result"
    _same(got, c.ref)


@gpu
@pytest.mark.parametrize("name,d", [t for t in RT._cases(RT.PLAIN) if t[0] not in SLACK_DENSE_X])
def test_nan_slack(native_lib, monkeypatch, name, d):
    """x as a channel slice of a buffer 8 (C % 64 != 0: 24) channels wider whose extra channels hold NaN, emask
    likewise: bit-equal to the reference and finite on every route."""
    args, rec, _ = RT.PLAIN[name]
    _run_slack(RT._rcase(**args, dt=RT.DTS[d]), rec, _slack_largs(name), monkeypatch)


@gpu
@pytest.mark.parametrize("name", SLACK_TAIL)
def test_nan_before_x(native_lib, monkeypatch, name):
    """x as the last rows of a longer buffer whose leading rows are NaN (and which ends where x ends)."""
    args, rec, dts = RT.PLAIN[name]
    c = RT._rcase(**args, dt=RT.DTS[dts.split()[-1]])
    _run_slack(c, rec, dict(rec.largs, x_tail=True, x_fill=NAN), monkeypatch)


@gpu
@pytest.mark.parametrize("name", MASK_IG[:4] + MASK_DMA)
def test_nan_mask_slack(native_lib, name):
    """The A-side mask's (and x's) extra channels hold NaN."""
    if name in RR.IG_MODES:
        args, largs, policies, bn = RR.IG_MODES[name]
        route = f"igemm {RR.IG[bn][0]}x{bn}"
    else:
        args, largs, policies, route = dict(RR.DMA16)[name], dict(x_extra=8, mask_extra=8), ("dma",), None
    # (conv_igemm is reached by a mask whose pixel stride differs from x's: the extras differ by 8)
    largs = dict(largs, x_extra=largs.get("x_extra") or largs["mask_extra"] + 8 * (route is not None))
    c = RR._case(**args)
    for policy in policies:
        got, r, _ = _launch(c, policy, **dict(largs, x_fill=NAN, mask_fill=NAN))
        assert (r == route) if route else r.startswith("dma 256x16 st2 ks") and r.endswith("mask"), (policy, r)
        assert bool(torch.isfinite(got.float()).all())
        _same(got, c.ref)


# ----------------------------------------------------------------------------------------
# the conditions of every case above, without a GPU
# ----------------------------------------------------------------------------------------

def _all_scases(G):
    for fam, relu in SMALL:
        for name in _of(RT.PLAIN, "fp16"):
            yield (fam, _plain_args(name, relu, fam))
        for C, OC, opts in RT.PW_PLAIN.values():
            yield (fam, dict(RT._pw_args(G, C, OC, 60 + OC, **opts), relu=relu))
        for v in RT.LONG.values():
            yield (fam, dict(v[0], relu=relu))
    for fam in ("sub", "edge"):
        for v in RT.UNPOOL_OUT.values():
            yield (fam, v[0])
        yield (fam, RT._out2_args())
    for p in RT.GROUP:
        yield ("sub", dict(p, **({"model": "staged"} if p.get("acc") else {})))
    for fam in ("sub", "edge"):
        for args, _ in IG_SMALL.values():
            yield (fam, args)
    for name in STRADDLE:
        yield ("straddle", _plain_args(name, RT.PLAIN[name][0].get("relu", True)))
    yield ("straddle", _straddle_pw_args(G))
    for name in _of(RT.PLAIN, "bf16"):
        yield ("bsub", _plain_args(name, True))
    for name in POST_SMALL:
        for v in POST_VARIANTS:
            yield ("sub", _post_args(name, v))
    for name in PW_POST_SMALL:
        yield ("sub", _pw_post_args(G, name))
    a = _f32_args()
    a.pop("bias", None)
    yield ("sub", a)
    for shape, _ in _bits_cases(G):
        dt, a = _margs(RR._bits_args(*shape)[0])
        if dt == HF:
            yield ("sub", a)


def _all_mcases(G):
    for name in MASK_IG:
        yield _margs(RR.IG_MODES[name][0])
    for name in MASK_DMA:
        yield _margs(dict(RR.DMA16)[name])
    for d in RT.DTS.values():
        for name, variant in _emask_cases():
            yield d, _emask_args(name, variant)
        for C, OC, variant in PW_EMASK.values():
            yield d, RT._pw_args(G, C, OC, 90 + OC, **RT.VARIANTS[variant])
    for shape, _ in _bits_cases(G):
        yield _margs(RR._bits_args(*shape)[1])


def test_conditions(capsys):
    """Every case of every table of this file: operands, both oracles, the families' conditions, the mutant
    separation and the CPU path's equality with the oracle (asserted inside the builders), without a GPU; and the
    extended ``representable`` / ``ties`` leave the normal range as it was."""
    n = 0
    for fam, args in _all_scases(G_NOMINAL):
        try:
            _scase.__wrapped__(fam, **args)
        except AssertionError as e:
            raise AssertionError(f"case {fam} {args}: {e}") from e
        n += 1
    for N, H, W, C, OC, _, _ in RT.POOL_DMA:
        _spcase.__wrapped__(100 + OC, N, H, W, C, OC)
        n += 1
    for dt, args in _all_mcases(G_NOMINAL):
        try:
            _mcase.__wrapped__(dt, **args)
        except AssertionError as e:
            raise AssertionError(f"mask case {dt} {args}: {e}") from e
        n += 1
    for d in RT.DTS.values():
        for shape in POOL_TINY:
            _pool_tiny_case.__wrapped__(d, *shape)
        _pool_fused_tiny_case.__wrapped__(d)
        for shape in UNPOOL_TINY:
            _unpool_tiny_case.__wrapped__(d, *shape)
        for shape in SCATTER_TINY:
            _scatter_tiny_case.__wrapped__(d, *shape)
        for acc in (False, True):
            _merge_tiny_case.__wrapped__(d, acc)
        _stem_tiny_case.__wrapped__(d)
        _premasked_tiny_case.__wrapped__(d)
        _guide_tiny_case.__wrapped__(d)
    assert n > 250, n
    with capsys.disabled():
        for (fam, name), v in sorted(MINS.items()):
            print(f"\n  {fam:9s} min {name}: {v:.3f}", end="")
        print()
    # the normal range: the old definitions (frexp significand on SIG bits) on cases of the rounding file
    for name in ("dma_lds", "igemm_transpose"):
        for d in RT.DTS.values():
            c = RT._rcase.__wrapped__(**RT.PLAIN[name][0], dt=d)
            y = RO.exact(RO.conv_acc(c.x, c.cw.w_oihw, c.cw.kind, c.kw["stride"], c.kw["pad"], c.ref.shape[1:3]),
                         c.cw.bias if c.kw["use_bias"] else None, c.kw["relu"])
            m, _ = torch.frexp(y)
            s1, s2 = m * float(2 ** RO.SIG[d]), m * float(2 ** (RO.SIG[d] + 1))
            old_rep = s1 == s1.round()
            assert torch.equal(RO.representable(y, d), old_rep)
            assert torch.equal(RO.ties(y, d), (s2 == s2.round()) & ~old_rep) and bool(RO.ties(y, d).any())
    # and below it: the grid is fixed
    for d, e in RO.SUB_GRID_EXP.items():
        v = torch.tensor([0.0, 1.0, 1.5, 2.5, 3.0, 0.5, 0.25, 2.0 ** (RO.SIG[d] - 1) + 0.5]).double() * 2.0 ** e
        assert RO.representable(v, d).tolist() == [True, True, False, False, True, False, False, False]
        assert RO.ties(v, d).tolist() == [False, False, True, True, False, True, False, True]
        want = torch.tensor([0, 1, 2, 2, 3, 0, 0, 2.0 ** (RO.SIG[d] - 1)]).double() * 2.0 ** e
        assert torch.equal(RO.round16(v, d), want)
