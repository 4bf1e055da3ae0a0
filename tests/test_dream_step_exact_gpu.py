"""GPU: the kernels that finish every DeepDream step (csrc/dream.hip: dream_update with its absmean_part
pre-pass, tile_gather, tile_pack, tile_update, octave_resize) against an EXACT oracle.

These kernels carry state across steps: the fp32 master image, the max_loss early-stop flag, the
rank / world / chunk pack layout of the multi-GPU tiled dream and the image roll. The oracle is written here
from the layouts documented in csrc/dream.hip and csrc/kernels.h (plain indexing, Python loops over units,
``torch.roll`` for the shift); no engine path is called. How each result is made exact:

* 16-bit conversions equal the CPU's ``.to(dt)`` (round to nearest even) bit for bit; one case per converting
  kernel carries a table of edge values (ties at both parities, just above a tie, 65504, 65520, negatives,
  -0.0).
* Sums: gradients are small integers times a per-image power of two, loss partials integers in [0, 64],
  coefficients from {0.25, 0.5, 2}: every partial sum is a multiple of a power of two below 2^24, so the
  loss and sum |g| are exact in fp32 under any order, with or without FMA contraction.
* The update x += sc g, sc = step / max(sum|g| / (3 H W), 1e-7): the two correctly rounded fp32 divisions
  are reproduced in numpy.float32. Power-of-two cases (mean |g| and step powers of two) round once either
  way and must be bit-equal; general cases (integer g, x on a 2^-10 grid, step 0.01) must equal, element by
  element, either candidate A = fl32(x + fl32(sc g)) or candidate B = the FMA result (computed exactly in
  fp64).
* octave_resize: dyadic size ratios and integer operands make every weight and intermediate a multiple of
  2^-14 below 2^6: the result equals the fp64 F.interpolate(align_corners=True) bit for bit.

Every output buffer starts filled with a sentinel (7.0, or NaN for fp32 scratch), so what must be written is
seen to be written and what must be left alone is compared bit for bit. Every case is built by a cached
``_*_case`` function that asserts the method's conditions on the reference alone; ``test_conditions`` (no
GPU) builds them all, so a condition failure is never mistaken for a kernel failure.
"""
import functools
import types
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from deconv_api_amd.engine.deepdream import TiledDeepDream
from exact_helpers import BF, DEV, HF, _gen, _ints

gpu = pytest.mark.gpu
dtypes = pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
SENTINEL = 7.0
NAN = float("nan")
JUNK = 5.0  # channels 3 .. 7 of a gradient: never part of a sum or an update
STEP_POW2, STEP_GENERAL = 2.0 ** -6, 0.01
# csrc/dream.hip: plan row length, pack blocks per unit, fp32 tail entries per unit
TPLAN, TP, TAILF = 7, 31, 32
LCOEFS = torch.tensor([0.25, 0.5, 2.0])


def _case(**kw):
    return types.SimpleNamespace(**kw)


def _bits(t):
    """The bit patterns of a 16-bit or fp32 tensor (on the CPU)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} != {tuple(w.shape)}"
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(bad[0].tolist())
        pytest.fail(f"{what}: {bad.shape[0]} of {g.numel()} values differ bitwise, first at {list(i)}: "
                    f"got {float(got.detach().cpu()[i])}, want {float(want.detach().cpu()[i])}")


def _representable(t, what):
    for dt in (BF, HF):
        assert torch.equal(t.to(dt).double(), t.double()), f"{what} not representable in {dt}"


# ----------------------------------------------------------------------------------------
# 16-bit conversion edge values
# ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _edge_values():
    """fp32 sources whose rounding to bf16 / fp16 is an edge: ties at both parities, a value just above a
    tie, the largest finite fp16 (65504), 65520 (inf in fp16, finite in bf16), ordinary values, all with
    both signs, and the two zeros. No fp16-subnormal result, no NaN / inf source."""
    pos = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20,
           1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20,
           65504.0, 65520.0, 0.1, 3.1415927, 1.5]
    t = torch.tensor(pos + [-v for v in pos] + [-0.0, 0.0], dtype=torch.float32)
    assert t[:8].double().tolist() == pos[:8], "the edge values are not exact in fp32"
    assert bool(torch.isfinite(t).all())
    b, h = t.to(BF).double(), t.to(HF).double()
    # the CPU conversion is round to nearest, ties to even
    assert b[:3].tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]
    assert h[3:6].tolist() == [1.0, 1 + 2.0 ** -9, 1 + 2.0 ** -10]
    assert float(h[6]) == 65504.0 and float(h[7]) == float("inf") and float(b[7]) == 65536.0
    assert float(h[len(pos) + 7]) == float("-inf")
    for r in (b, h):
        nz = r[r != 0].abs()
        assert float(nz.min()) >= 2.0 ** -14, "an fp16-subnormal result"
    assert _bits(t.to(HF))[-2].item() == -0x8000 and _bits(t.to(BF))[-2].item() == -0x8000  # -0.0 keeps its sign
    return t


def _tile_edges(shape):
    """An fp32 tensor of ``shape`` filled with the edge table, repeated."""
    t = _edge_values()
    n = int(np.prod(shape))
    return t.repeat(-(-n // t.numel()))[:n].reshape(shape).clone()


# ----------------------------------------------------------------------------------------
# the update x += sc * g
# ----------------------------------------------------------------------------------------

def _magnitudes(g, count, total):
    """A seeded permutation of ``count`` values from {1, 2, 3} that sum to ``total`` exactly: 1s and 3s and at
    most one 2 (total = 2 count: half 1s, half 3s, one 2 if count is odd - the mean is exactly 2)."""
    extra = total - count
    assert 0 <= extra <= 2 * count, "no multiset of {1, 2, 3} has this sum"
    n3, n2 = divmod(extra, 2)
    v = torch.ones(count)
    v[:n3] = 3.0
    if n2:
        v[n3] = 2.0
    v = v[torch.randperm(count, generator=g)]
    assert float(v.double().sum()) == total
    return v


def _rand_signs(g, shape):
    return torch.randint(0, 2, shape, generator=g).float() * 2 - 1


def _scale(step, asum, H, W):
    """sc = step / max(sum|g| / (3 H W), 1e-7) as the kernels compute it: -O3 without fast-math, so two
    correctly rounded fp32 divisions (3.f * (float)(H W) is exact below 2^24)."""
    f = np.float32
    assert 3 * H * W < 2 ** 24
    assert float(f(asum)) == asum, "sum |g| not exact in fp32"
    mean = f(asum) / f(3 * H * W)
    return f(step) / max(mean, f(1e-7))


def _update_candidates(x, g, sc):
    """x + sc g per element in fp32: A rounds the product and then the sum (no contraction), B is the FMA
    (one rounding of the exact value; the fp64 arithmetic is exact under the builders' range conditions)."""
    xn, gn = x.numpy().astype(np.float32), g.numpy().astype(np.float32)
    sc = np.broadcast_to(np.asarray(sc, dtype=np.float32), xn.shape)
    A = xn + sc * gn
    assert A.dtype == np.float32
    B = (xn.astype(np.float64) + sc.astype(np.float64) * gn.astype(np.float64)).astype(np.float32)
    return torch.from_numpy(A.copy()), torch.from_numpy(B.copy())


def _check_pow2(x, g, sc, live, step, mean):
    """Power-of-two case conditions: sc of every live image is a power of two, so sc g is exact, A == B
    bitwise, and both equal the fp64 value of x + step g / mean|g| rounded once."""
    A, B = _update_candidates(x, g, sc)
    scv = np.asarray(sc, dtype=np.float32).reshape(-1)
    for n in range(scv.size):
        if live[n]:
            assert np.frexp(scv[n])[0] == 0.5 and float(scv[n]) == step / mean[n], "sc is not the exact power of two"
        else:
            assert scv[n] == 0
    assert torch.equal(_bits(A), _bits(B)), "a power-of-two case must round once either way"
    m = torch.tensor([step / mean[n] if live[n] else 0.0 for n in range(scv.size)], dtype=torch.float64)
    ref = (x.double() + m.view(-1, *[1] * (x.dim() - 1)) * g.double()).float()
    assert torch.equal(A, ref)
    return A, B


def _check_general(x, g, sc, gq=0):
    """General case conditions: x on the grid m 2^-10 with |m| < 2^11, g multiples of 2^-gq with |g| < 16;
    then sc g and the sum are exact in fp64 (asserted from the bit budget, and against fractions.Fraction on
    a sample that includes every element where the candidates differ, up to 64), so B is the true FMA
    result. Returns (A, B, number of elements with A != B)."""
    xm = x.double() * 2 ** 10
    assert torch.equal(xm, xm.round()) and float(xm.abs().max()) < 2 ** 11, "x off the 2^-10 grid"
    gm = g.double() * 2 ** gq
    assert torch.equal(gm, gm.round()) and float(g.abs().max()) < 16, "g off its grid"
    scv = np.asarray(sc, dtype=np.float32).reshape(-1)
    for s in scv:
        if s != 0:
            _, e = np.frexp(s)  # s = m 2^e, 0.5 <= m < 1: a multiple of 2^(e - 24)
            assert s < 1 and 5 - min(-10, int(e) - 24 - gq) <= 53, "x + sc g not exact in fp64"
    A, B = _update_candidates(x, g, sc)
    diff = (A != B).reshape(-1).nonzero().reshape(-1)
    scb = np.broadcast_to(np.asarray(sc, dtype=np.float32), tuple(x.shape)).reshape(-1)
    xf, gf = x.reshape(-1), g.reshape(-1)
    sample = diff[:64].tolist() + list(range(0, x.numel(), max(1, x.numel() // 64)))
    for i in sample:
        exact = Fraction(float(xf[i])) + Fraction(float(scb[i])) * Fraction(float(gf[i]))
        f64 = float(xf[i]) + float(scb[i]) * float(gf[i])
        assert Fraction(f64) == exact, "the fp64 value of x + sc g is not exact"
        assert float(B.reshape(-1)[i]) == float(np.float32(f64))
    return A, B, int(diff.numel())


def _assert_update(got, c, where=None):
    """The device's fp32 image against the case's candidates: bitwise A (== B) for a power-of-two case,
    element-wise A or B for a general one (the split is printed). ``where``: the elements updated."""
    got = got.detach().cpu()
    ga, A, B = _bits(got), _bits(c.A), _bits(c.B)
    if where is None:
        where = torch.ones_like(ga, dtype=torch.bool)
    isA, isB = (ga == A) & where, (ga == B) & where
    bad = where & ~isA & ~isB
    if c.kind == "general":
        n = int((A != B)[where].sum())
        print(f"general update: {n} elements with A != B: {int((isA & ~isB).sum())} match A only, "
              f"{int((isB & ~isA).sum())} match B only")
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        pytest.fail(f"x: {int(bad.sum())} of {int(where.sum())} updated elements are neither candidate, first at "
                    f"{list(i)}: got {float(got[i])!r}, A {float(c.A[i])!r}, B {float(c.B[i])!r}")


# ----------------------------------------------------------------------------------------
# 1. dream_update (+ absmean_part)
# ----------------------------------------------------------------------------------------

# (N, H, W, gparts, L, lparts, mode, kind). (3, 5, 7): one update block, most absmean blocks empty;
# (2, 129, 130): H W = 16 770 > 64 * 256, the 64-block cap's stride loop. gparts / lparts 70 / 130: the
# partial loops over more than 64 entries. mode: "off" max_loss = -1; "strict" max_loss == loss[0] < loss[1];
# "preset" the last image arrives done, with a loss below max_loss; "edge" = "preset" with the conversion edge
# table as the done image.
DU_CASES = [
    (3, 5, 7, 1, 1, 1, "off", "pow2"),
    (3, 5, 7, 32, 3, 5, "strict", "pow2"),
    (3, 5, 7, 70, 1, 64, "preset", "pow2"),
    (3, 5, 7, 70, 3, 130, "off", "general"),
    (3, 5, 7, 1, 3, 130, "strict", "general"),
    (3, 5, 7, 32, 1, 5, "preset", "general"),
    (3, 5, 7, 32, 3, 5, "edge", "pow2"),
    (2, 129, 130, 1, 3, 64, "off", "general"),
    (2, 129, 130, 70, 3, 130, "strict", "pow2"),
    (2, 129, 130, 32, 1, 1, "preset", "general"),
    (2, 129, 130, 70, 1, 5, "off", "pow2"),
]
SEEDS = 64  # a general case takes the first of this many seeds whose candidates A and B differ somewhere


def _draw_losses(g, L, N, lparts, mode):
    """lpart [L, N, lparts] integers in [0, 64], lcoef [L] from {0.25, 0.5, 2} and the exact per-image loss.
    "strict": image 0 draws from [0, 32] and image 1 from [33, 64], so loss[1] > loss[0]."""
    lpart = _ints(g, (L, N, lparts), 0, 64)
    if mode == "strict":
        lpart[:, 0] = _ints(g, (L, lparts), 0, 32)
        lpart[:, 1] = _ints(g, (L, lparts), 33, 64)
    lcoef = LCOEFS[torch.randint(0, 3, (L,), generator=g)]
    loss = torch.einsum("l,lnp->n", lcoef.double(), lpart.double())
    assert float(2.0 * lpart.double().sum(dim=(0, 2)).max()) * 4 < 2 ** 24, "loss partial sums not exact in fp32"
    assert torch.equal(loss.float().double(), loss)
    return lpart, lcoef, loss


def _stop_rule(mode, loss, N):
    """(max_loss, done before, done after) of a mode: done |= max_loss >= 0 and loss > max_loss, strictly."""
    done_in = torch.zeros(N, dtype=torch.uint8)
    if mode == "off":
        max_loss = -1.0
    elif mode == "strict":
        max_loss = float(loss[0])
        assert N >= 2 and float(loss[1]) > max_loss >= 0
    else:
        done_in[N - 1] = 1
        max_loss = float(loss.max()) + 1.0
    done = done_in.bool() | ((loss > max_loss) if max_loss >= 0 else torch.zeros(N, dtype=torch.bool))
    if mode == "strict":
        assert not done[0] and done[1], "the comparison is strict: image 0 goes on, image 1 stops"
    elif mode != "off":
        assert float(loss[N - 1]) < max_loss and done.tolist() == [0] * (N - 1) + [1]
    else:
        assert not done.any()
    return max_loss, done_in, done.to(torch.uint8)


def _du_draw(seed, N, H, W, gparts, L, lparts, mode, kind):
    g = _gen(seed)
    n3 = 3 * H * W
    if kind == "pow2":
        j = torch.randint(-2, 3, (N,), generator=g)
        mag = torch.stack([_magnitudes(g, n3, 2 * n3) for _ in range(N)]).view(N, H, W, 3)
        g3 = _rand_signs(g, (N, H, W, 3)) * mag * (2.0 ** j).view(N, 1, 1, 1)
        x = torch.randn(N, H, W, 3, generator=g)
        step = STEP_POW2
    else:
        g3 = _ints(g, (N, H, W, 3), -15, 15)
        x = _ints(g, (N, H, W, 3), -(2 ** 11 - 1), 2 ** 11 - 1) * 2.0 ** -10
        step = STEP_GENERAL
    if mode == "edge":
        x[N - 1] = _tile_edges((H, W, 3))
    _representable(g3, "g")
    asum = g3.double().abs().sum(dim=(1, 2, 3))
    assert float(asum.max()) * (4 if kind == "pow2" else 1) < 2 ** 24, "sum |g| not exact in fp32"
    lpart, lcoef, loss = _draw_losses(g, L, N, lparts, mode)
    max_loss, done_in, done = _stop_rule(mode, loss, N)
    sc = np.array([0.0 if done[n] else _scale(step, float(asum[n]), H, W) for n in range(N)], dtype=np.float32)
    scb = sc.reshape(N, 1, 1, 1)
    if kind == "pow2":
        mean = [2.0 ** (int(j[n]) + 1) for n in range(N)]
        assert [float(a) / n3 for a in asum] == mean
        A, B = _check_pow2(x, g3, scb, [not d for d in done.tolist()], step, mean)
        ndiff = 0
    else:
        A, B, ndiff = _check_general(x, g3, scb)
    g8 = torch.cat([g3, torch.full((N, H, W, 5), JUNK)], dim=-1)
    return _case(kind=kind, mode=mode, g8=g8, x=x, lpart=lpart, lcoef=lcoef, loss=loss, asum=asum, step=step,
                 max_loss=max_loss, done_in=done_in, done=done, A=A, B=B, ndiff=ndiff)


def _first_nonvacuous(draw, seed, kind):
    for s in range(seed, seed + SEEDS):
        c = draw(s)
        if kind != "general" or c.ndiff > 0:
            return c
    raise AssertionError("no seed gives a general case whose candidates A and B differ: the acceptance is vacuous")


@functools.lru_cache(maxsize=None)
def _du_case(N, H, W, gparts, L, lparts, mode, kind):
    seed = 1000 * (N * H * W + gparts + L + lparts) + len(mode)
    return _first_nonvacuous(lambda s: _du_draw(s, N, H, W, gparts, L, lparts, mode, kind), seed, kind)


@gpu
@dtypes
@pytest.mark.parametrize("N,H,W,gparts,L,lparts,mode,kind", DU_CASES)
def test_exact_dream_update(native_lib, N, H, W, gparts, L, lparts, mode, kind, dt):
    """absmean_part_kernel + dream_update_kernel: every gpart entry written and their sum the exact sum |g| of
    channels 0..2; loss[n] exact and published for done images too; the early stop strict; x of a live image
    the exact update (bitwise, or one of the two roundings), x of a done image unchanged by value; xin the
    16-bit rounding of the new x bit for bit, channels 3..7 zero."""
    c = _du_case(N, H, W, gparts, L, lparts, mode, kind)
    g = c.g8.to(dt).to(DEV)
    x = c.x.clone().to(DEV)
    xin = torch.full((N, H, W, 8), SENTINEL, dtype=dt, device=DEV)
    gpart = torch.full((N, gparts), NAN, device=DEV)
    loss = torch.full((N,), NAN, device=DEV)
    done = c.done_in.clone().to(DEV)
    native_lib.dream_update(g, x, xin, gpart, c.lpart.to(DEV), c.lcoef.to(DEV), done, loss, c.step, c.max_loss)
    gp = gpart.cpu().double()
    assert not bool(torch.isnan(gp).any()), "a gpart entry was not written"
    assert torch.equal(gp.sum(1), c.asum), (gp.sum(1).tolist(), c.asum.tolist())
    assert torch.equal(loss.cpu().double(), c.loss), (loss.tolist(), c.loss.tolist())
    assert torch.equal(done.cpu(), c.done), (done.tolist(), c.done.tolist())
    _assert_update(x, c)
    xc = x.cpu()
    for n in range(N):
        if c.done[n]:
            assert torch.equal(xc[n], c.x[n]), f"image {n} is done: its x must not change"
    _same_bits(xin[..., :3], xc.to(dt), "xin channels 0..2 vs the rounded x")
    assert not bool(_bits(xin[..., 3:]).any()), "xin channels 3..7 must be zero"
    if mode == "edge":
        assert bool(torch.isinf(xc[N - 1].to(HF)).any()), "the edge table did not reach the conversion"


# ----------------------------------------------------------------------------------------
# 2. tiled step: plans and the pack layout
# ----------------------------------------------------------------------------------------

def _gplan(B, H, W, tile):
    """The engine's plan builder (TiledDeepDream._gplan) without an engine: it needs ``tile`` only."""
    eng = object.__new__(TiledDeepDream)
    eng.tile = tile
    Th, Tw, plan, _ = eng._gplan(B, H, W)
    return Th, Tw, plan


@functools.lru_cache(maxsize=None)
def _plan(name):
    """(B, H, W, Th, Tw, plan int32 [units, 7]); rows {image, tile origin y, x, owned y0, y1, x0, x1 (tile-local,
    half-open)}. Validated here as the kernels index with them unchecked.
    tiles8: 2 x 2 overlapping 6 x 7 tiles of two 11 x 13 images, owned rectangles at non-zero local offsets;
    one256: one unit of 65 536 owned pixels (hand-built; the second round of tile_pack's 8-deep unroll needs
            more than 31 * 256 * 8 = 63 488);
    one384: one unit of 135 168 pixels, above the 512-block cap of tile_gather / tile_update;
    hand:   hand-built, 5 units on two 9 x 10 images: a 1 x 1 owned rectangle at its tile's last corner,
            owned rectangles inside their tiles, and most image pixels owned by no unit."""
    if name == "tiles8":
        B, H, W = 2, 11, 13
        Th, Tw, plan = _gplan(B, H, W, 7)
        assert (Th, Tw, plan.shape[0]) == (6, 7, 8)
        assert int(plan[:, 3].max()) > 0 and int(plan[:, 5].max()) > 0, "no owned rectangle at a local offset"
    elif name == "one256":
        B, H, W, Th, Tw = 1, 256, 256, 256, 256
        plan = torch.tensor([[0, 0, 0, 0, 256, 0, 256]], dtype=torch.int32)
        assert 256 * 256 > TP * 256 * 8
    elif name == "one384":
        B, H, W = 1, 384, 352
        Th, Tw, plan = _gplan(B, H, W, 512)
        assert (Th, Tw, plan.shape[0]) == (384, 352, 1) and (Th * Tw + 255) // 256 > 512
    else:
        B, H, W, Th, Tw = 2, 9, 10, 4, 5
        plan = torch.tensor([[0, 0, 0, 0, 4, 0, 5],
                             [0, 5, 5, 3, 4, 4, 5],
                             [1, 2, 3, 1, 3, 0, 2],
                             [1, 5, 0, 0, 4, 2, 5],
                             [0, 0, 5, 0, 2, 1, 5]], dtype=torch.int32)
    assert plan.dtype == torch.int32 and plan.shape[1] == TPLAN
    p = plan.long()
    assert bool(((p[:, 0] >= 0) & (p[:, 0] < B)).all())
    assert bool(((p[:, 1] >= 0) & (p[:, 1] + Th <= H) & (p[:, 2] >= 0) & (p[:, 2] + Tw <= W)).all())
    assert bool(((p[:, 3] >= 0) & (p[:, 3] < p[:, 4]) & (p[:, 4] <= Th)).all())
    assert bool(((p[:, 5] >= 0) & (p[:, 5] < p[:, 6]) & (p[:, 6] <= Tw)).all())
    cover = torch.zeros(B, H, W, dtype=torch.int64)
    for b, oy, ox, y0, y1, x0, x1 in p.tolist():
        cover[b, oy + y0:oy + y1, ox + x0:ox + x1] += 1
    assert int(cover.max()) == 1, "every pixel is owned by at most one unit"
    if name == "hand":
        assert int((cover == 0).sum()) > 0 and p[1].tolist()[3:] == [Th - 1, Th, Tw - 1, Tw]
    else:
        assert int(cover.min()) == 1
    return B, H, W, Th, Tw, plan


def _shifts(H, W, tile):
    return [(0, 0), (1, -1), (-(H + 3), W + 5), (H, W), (tile // 2, -(tile // 2))]


def _ustride(Th, Tw):
    """16-bit elements per unit in a pack: 3 channels x tile, rounded up to 16 B."""
    return (Th * Tw * 3 + 7) & ~7


def _pack_elems(ucc, Th, Tw):
    """16-bit elements of one rank's pack of ``ucc`` units: the units, then TAILF fp32 per unit (+ padding),
    rounded to 16 B (csrc/dream.hip:tile_pack_elems)."""
    return (ucc * (_ustride(Th, Tw) + 2 * TAILF + 4) + 7) & ~7


def _layout(nunits, world, chunks):
    """(chunk count C, units per rank and chunk ucc) for ``chunks`` in {1, 2, "ucap"}. Unit v lives on rank
    v % world as local unit j = v // world, in chunk j // ucc at slot j % ucc; packs are [C][world][pack]."""
    ucap = -(-nunits // world)
    C = ucap if chunks == "ucap" else min(chunks, ucap)
    return C, -(-ucap // C)


def _chunk_options(nunits, world):
    return sorted({_layout(nunits, world, ch) for ch in (1, 2, "ucap")})


def _rank_chunks(nunits, world, C, ucc, rank):
    """[(chunk, k0, [global units])] of a rank's non-empty chunks."""
    mine = list(range(rank, nunits, world))
    out = []
    for c in range(C):
        units = mine[c * ucc:(c + 1) * ucc]
        if units:
            assert units[0] == rank + c * ucc * world
            out.append((c, c * ucc, units))
    return out


def _owned(plan, u):
    b, oy, ox, y0, y1, x0, x1 = plan[u].tolist()
    return b, oy, ox, y0, y1, x0, x1


def _rolled_to_image(t, sy, sx):
    """A [B, H, W, ...] tensor in the rolled frame (rolled[Y][X] = x[(Y - sy) mod H][(X - sx) mod W]) back in
    the image frame."""
    return torch.roll(t, shifts=(-sy, -sx), dims=(1, 2))


# ----------------------------------------------------------------------------------------
# 3. tile_gather
# ----------------------------------------------------------------------------------------

# (plan, world, edge): every rank of the world, with 1, 2 and ucap chunks, at five shifts. world = 3 on 8 units
# leaves rank 2 one unit short (U < ucap, k0 > 0).
TG_CASES = [("tiles8", 1, False), ("tiles8", 2, False), ("tiles8", 3, False), ("hand", 1, True), ("hand", 2, False),
            ("hand", 3, False), ("one256", 1, False), ("one384", 1, False)]


@functools.lru_cache(maxsize=None)
def _tg_case(name, world, edge):
    B, H, W, Th, Tw, plan = _plan(name)
    g = _gen(7 * len(name) + world)
    x = torch.randn(B, H, W, 3, generator=g)
    if edge:
        x[0] = _tile_edges((H, W, 3))
    ref = {}
    for sy, sx in _shifts(H, W, min(Th, Tw)):
        rolled = torch.roll(x, shifts=(sy, sx), dims=(1, 2))
        assert float(rolled[0, sy % H, sx % W, 0]) == float(x[0, 0, 0, 0])
        tiles = torch.stack([rolled[b, oy:oy + Th, ox:ox + Tw] for b, oy, ox, *_ in plan.tolist()])
        if edge:
            assert bool(torch.isinf(tiles.to(HF)).any()), "the edge table is not in a tile"
        ref[(sy, sx)] = tiles
    return _case(B=B, H=H, W=W, Th=Th, Tw=Tw, plan=plan, x=x, ref=ref)


@gpu
@dtypes
@pytest.mark.parametrize("name,world,edge", TG_CASES)
def test_exact_tile_gather(native_lib, name, world, edge, dt):
    """tile_gather_kernel: xin[k] is the tile of the rolled image of unit rank + (k0 + k) world, rounded to
    16 bits bit for bit, channels 3..7 zero; x itself is not changed."""
    c = _tg_case(name, world, edge)
    x, plan = c.x.to(DEV), c.plan.to(DEV)
    nunits = c.plan.shape[0]
    for C, ucc in _chunk_options(nunits, world):
        for shift in c.ref:
            sh = torch.tensor(shift, dtype=torch.int32, device=DEV)
            for rank in range(world):
                for _, k0, units in _rank_chunks(nunits, world, C, ucc, rank):
                    xin = torch.full((len(units), c.Th, c.Tw, 8), SENTINEL, dtype=dt, device=DEV)
                    native_lib.tile_gather(x, xin, plan, sh, rank, world, k0)
                    want = torch.zeros(len(units), c.Th, c.Tw, 8, dtype=dt)
                    want[..., :3] = c.ref[shift][units].to(dt)
                    _same_bits(xin, want, f"xin (chunks {C}, shift {shift}, rank {rank}, k0 {k0})")
    _same_bits(x, c.x, "x")


# ----------------------------------------------------------------------------------------
# 4. tile_pack
# ----------------------------------------------------------------------------------------

# (plan, world, L, lparts)
TPK_CASES = [("tiles8", 1, 1, 1), ("tiles8", 2, 3, 5), ("tiles8", 3, 1, 64), ("hand", 1, 3, 5), ("hand", 2, 3, 130),
             ("hand", 3, 1, 5), ("one256", 1, 3, 64), ("one384", 1, 1, 130)]


@functools.lru_cache(maxsize=None)
def _tpk_case(name, world, L, lparts):
    B, H, W, Th, Tw, plan = _plan(name)
    U = plan.shape[0]
    g = _gen(11 * len(name) + world + L + lparts)
    g3 = _ints(g, (U, Th, Tw, 3), -3, 3)
    g3[(g3 == 0) & (torch.rand(U, Th, Tw, 3, generator=g) < 0.5)] = -0.0
    g3 = g3 * (2.0 ** torch.randint(-2, 3, (U,), generator=g)).view(U, 1, 1, 1)
    _representable(g3, "g")
    g8 = torch.cat([g3, torch.full((U, Th, Tw, 5), JUNK)], dim=-1)
    lpart, lcoef, loss = _draw_losses(g, L, U, lparts, "off")
    owned, asum = [], []
    for u in range(U):
        _, _, _, y0, y1, x0, x1 = _owned(plan, u)
        o = g3[u, y0:y1, x0:x1].reshape(-1)
        owned.append(o)
        asum.append(float(o.double().abs().sum()))
    assert max(asum) * 4 < 2 ** 24, "sum |g| not exact in fp32"
    allo = torch.cat(owned)
    assert bool(((allo == 0) & torch.signbit(allo)).any()), "no -0.0 among the owned pixels"
    return _case(Th=Th, Tw=Tw, plan=plan, g8=g8, lpart=lpart, lcoef=lcoef, loss=loss, owned=owned, asum=asum)


def _new_pack(ucc, Th, Tw, dt, device):
    """A pack whose unit region holds the 16-bit sentinel and whose fp32 tail region holds NaN."""
    us, pe = _ustride(Th, Tw), _pack_elems(ucc, Th, Tw)
    pack = torch.full((pe,), SENTINEL, dtype=dt, device=device)
    pack[ucc * us:].view(torch.float32).fill_(NAN)
    return pack


@gpu
@dtypes
@pytest.mark.parametrize("name,world,L,lparts", TPK_CASES)
def test_exact_tile_pack(native_lib, name, world, L, lparts, dt):
    """tile_pack_kernel, for every rank and chunk of 1, 2 and ucap chunks: the owned pixels of each unit are
    bit copies of channels 0..2 of g (-0.0 included) in tile-local row-major order; the rest of the unit's
    stride, the slots of units not packed, their tails and the padding keep the sentinel; tail[0] is the exact
    loss; the 31 per-block |g| entries are all written and sum (fp64) to the exact sum |g| of the unit."""
    c = _tpk_case(name, world, L, lparts)
    nunits, us = c.plan.shape[0], _ustride(c.Th, c.Tw)
    plan, lcoef = c.plan.to(DEV), c.lcoef.to(DEV)
    for C, ucc in _chunk_options(nunits, world):
        assert native_lib.tile_pack_elems(ucc, c.Th, c.Tw) == _pack_elems(ucc, c.Th, c.Tw)
        for rank in range(world):
            for _, k0, units in _rank_chunks(nunits, world, C, ucc, rank):
                pack = _new_pack(ucc, c.Th, c.Tw, dt, DEV)
                native_lib.tile_pack(c.g8[units].to(dt).to(DEV), pack, plan, c.lpart[:, units].contiguous().to(DEV),
                                     lcoef, ucc, rank, world, k0)
                got = pack.cpu()
                want = torch.full((ucc * us,), SENTINEL, dtype=dt)
                for k, u in enumerate(units):
                    want[k * us:k * us + c.owned[u].numel()] = c.owned[u].to(dt)
                where = f"(chunks {C}, rank {rank}, k0 {k0})"
                _same_bits(got[:ucc * us], want, f"pack units {where}")
                tail = got[ucc * us:].clone().view(torch.float32).double()
                for k, u in enumerate(units):
                    t = tail[k * TAILF:(k + 1) * TAILF]
                    got0, sumg = float(t[0]), float(t[1:].sum())
                    assert got0 == float(c.loss[u]), f"unit {u} loss {where}: {got0}, want {float(c.loss[u])}"
                    assert not bool(torch.isnan(t[1:]).any()), f"unit {u}: a |g| tail entry was not written {where}"
                    assert sumg == c.asum[u], f"unit {u} sum |g| {where}: {sumg}, want {c.asum[u]}"
                assert bool(torch.isnan(tail[len(units) * TAILF:]).all()), f"wrote a tail past its units {where}"


# ----------------------------------------------------------------------------------------
# 5. tile_update
# ----------------------------------------------------------------------------------------

# (plan, world, chunks, mode, kind, shift index)
TU_CASES = [
    ("tiles8", 1, 1, "off", "pow2", 0), ("tiles8", 1, 2, "strict", "general", 1),
    ("tiles8", 1, "ucap", "preset", "pow2", 2), ("tiles8", 2, 1, "strict", "pow2", 3),
    ("tiles8", 2, 2, "preset", "general", 4), ("tiles8", 2, "ucap", "off", "general", 2),
    ("tiles8", 3, 1, "preset", "general", 1), ("tiles8", 3, 2, "off", "pow2", 4),
    ("tiles8", 3, "ucap", "strict", "pow2", 2), ("tiles8", 3, "ucap", "strict", "general", 3),
    ("hand", 1, 1, "off", "general", 2), ("hand", 2, 2, "strict", "pow2", 1),
    ("hand", 3, "ucap", "preset", "general", 4), ("hand", 3, 1, "off", "pow2", 3),
    ("hand", 2, "ucap", "strict", "general", 0),
    ("one256", 1, 1, "off", "pow2", 2), ("one384", 1, 1, "off", "general", 4), ("one384", 1, 1, "preset", "pow2", 1),
]
TAIL_JUNK = 4096.0  # tails of slots that hold no unit: reading one moves a loss or a sum |g|


def _tu_draw(seed, name, world, chunks, mode, kind, si):
    B, H, W, Th, Tw, plan = _plan(name)
    U = plan.shape[0]
    g = _gen(seed)
    sy, sx = _shifts(H, W, min(Th, Tw))[si]
    units_of = [[u for u in range(U) if int(plan[u, 0]) == b] for b in range(B)]
    npix = [(int(plan[u, 4]) - int(plan[u, 3])) * (int(plan[u, 6]) - int(plan[u, 5])) for u in range(U)]
    owned = [None] * U
    asum, mean = [], []
    for b in range(B):
        n = 3 * sum(npix[u] for u in units_of[b])
        if kind == "pow2":
            # sum |g| = 3 H W 2^k with n <= sum <= 3 n (k < 0 where few pixels are owned), times 2^j
            k = 1
            while 3 * H * W * 2.0 ** k > 3 * n:
                k -= 1
            total = 3 * H * W * 2.0 ** k
            assert total == int(total) and n <= total <= 3 * n
            j = int(torch.randint(-2, 3, (1,), generator=g))
            vals = _rand_signs(g, (n,)) * _magnitudes(g, n, int(total)) * 2.0 ** j
            mean.append(2.0 ** (k + j))
        else:
            vals = _ints(g, (n,), -15, 15)
        asum.append(float(vals.double().abs().sum()))
        o = 0
        for u in units_of[b]:
            owned[u] = vals[o:o + 3 * npix[u]]
            o += 3 * npix[u]
    assert max(asum) * (4 if kind == "pow2" else 1) < 2 ** 24, "sum |g| not exact in fp32"
    _representable(torch.cat(owned), "g")
    uloss = _ints(g, (U,), 0, 200) * 0.25
    loss = torch.tensor([float(uloss[units_of[b]].double().sum()) for b in range(B)], dtype=torch.float64)
    if mode == "strict" and float(loss[1]) <= float(loss[0]):
        uloss[units_of[1][0]] += float(loss[0] - loss[1]) + 1.0
        loss[1] = float(uloss[units_of[1]].double().sum())
    assert float(loss.max()) * 4 < 2 ** 24
    max_loss, done_in, done = _stop_rule(mode, loss, B)
    if kind == "pow2":
        x, step = torch.randn(B, H, W, 3, generator=g), STEP_POW2
    else:
        x, step = _ints(g, (B, H, W, 3), -(2 ** 11 - 1), 2 ** 11 - 1) * 2.0 ** -10, STEP_GENERAL
    sc = np.array([0.0 if done[b] else _scale(step, asum[b], H, W) for b in range(B)], dtype=np.float32)
    # the gradient and the owned mask in the rolled frame, then back in the image frame
    G, mask = torch.zeros(B, H, W, 3), torch.zeros(B, H, W, 3, dtype=torch.bool)
    for u in range(U):
        b, oy, ox, y0, y1, x0, x1 = _owned(plan, u)
        G[b, oy + y0:oy + y1, ox + x0:ox + x1] = owned[u].view(y1 - y0, x1 - x0, 3)
        mask[b, oy + y0:oy + y1, ox + x0:ox + x1] = True
    G, mask = _rolled_to_image(G, sy, sx), _rolled_to_image(mask, sy, sx)
    scb = sc.reshape(B, 1, 1, 1)
    if kind == "pow2":
        assert [asum[b] / (3 * H * W) for b in range(B)] == mean
        A, Bc = _check_pow2(x, G, scb, [not d for d in done.tolist()], step, mean)
        ndiff = 0
    else:
        A, Bc, ndiff = _check_general(x, G, scb)
    C, ucc = _layout(U, world, chunks)
    return _case(kind=kind, Th=Th, Tw=Tw, plan=plan, world=world, C=C, ucc=ucc, shift=(sy, sx), x=x,
                 owned=owned, uloss=uloss, loss=loss, step=step, max_loss=max_loss, done_in=done_in, done=done,
                 mask=mask, A=A, B=Bc, ndiff=ndiff)


@functools.lru_cache(maxsize=None)
def _tu_case(name, world, chunks, mode, kind, si):
    seed = 1000 * (len(name) + world + si) + len(mode) + (7 if chunks == "ucap" else chunks)
    return _first_nonvacuous(lambda s: _tu_draw(s, name, world, chunks, mode, kind, si), seed, kind)


def _tu_packs(c, dt):
    """The packs [C][world][pack_elems] a correct tile_pack + all-gather would leave, written from the
    documented layout: unit v on rank v % world, local j = v // world, chunk j // ucc, slot j % ucc; its owned
    pixels, then in the tail {loss, 31 partial sums of |g|}. Everything else is junk that must not be read."""
    us, pe = _ustride(c.Th, c.Tw), _pack_elems(c.ucc, c.Th, c.Tw)
    packs = torch.full((c.C, c.world, pe), SENTINEL, dtype=dt)
    packs[:, :, c.ucc * us:].view(torch.float32).fill_(TAIL_JUNK)
    seen = set()
    for v in range(c.plan.shape[0]):
        r, j = v % c.world, v // c.world
        ch, slot = j // c.ucc, j % c.ucc
        assert ch < c.C and (ch, r, slot) not in seen
        seen.add((ch, r, slot))
        o = c.owned[v]
        packs[ch, r, slot * us:slot * us + o.numel()] = o.to(dt)
        tail = packs[ch, r, c.ucc * us:].view(torch.float32)[slot * TAILF:(slot + 1) * TAILF]
        tail[0] = float(c.uloss[v])
        bins = torch.zeros(TP, dtype=torch.float64)
        bins.index_add_(0, torch.arange(o.numel()) % TP, o.double().abs())
        tail[1:] = bins.float()
        assert float(tail[1:].double().sum()) == float(o.double().abs().sum())
    return packs


@gpu
@dtypes
@pytest.mark.parametrize("name,world,chunks,mode,kind,si", TU_CASES)
def test_exact_tile_update(native_lib, name, world, chunks, mode, kind, si, dt):
    """tile_update_kernel on synthetic packs of every rank and chunk: per-image loss and sum |g| over the
    units of that image, the strict max_loss rule, the exact update at the owned pixels through the roll, and
    pixels owned by no unit (or of a done image) left bit-identical (unchanged by value)."""
    c = _tu_case(name, world, chunks, mode, kind, si)
    nb = c.x.shape[0]
    packs = _tu_packs(c, dt).to(DEV)
    x = c.x.clone().to(DEV)
    done = c.done_in.clone().to(DEV)
    loss = torch.full((nb,), NAN, device=DEV)
    native_lib.tile_update(packs, c.ucc, c.plan.to(DEV), torch.tensor(c.shift, dtype=torch.int32, device=DEV), x, done,
                           loss, c.step, c.max_loss, world, c.Th, c.Tw)
    assert torch.equal(loss.cpu().double(), c.loss), (loss.tolist(), c.loss.tolist())
    assert torch.equal(done.cpu(), c.done), (done.tolist(), c.done.tolist())
    _assert_update(x, c, where=c.mask)
    xc = x.cpu()
    assert torch.equal(_bits(xc)[~c.mask], _bits(c.x)[~c.mask]), "a pixel owned by no unit changed"
    for b in range(nb):
        if c.done[b]:
            assert torch.equal(xc[b], c.x[b]), f"image {b} is done: its x must not change"


# ----------------------------------------------------------------------------------------
# 6. gather -> (g = xin) -> pack -> update
# ----------------------------------------------------------------------------------------

# (plan, world, chunks, mode, shift index)
CHAIN_CASES = [("tiles8", 1, 1, "off", 1), ("tiles8", 2, 2, "strict", 2), ("tiles8", 3, "ucap", "off", 4),
               ("tiles8", 3, 2, "preset", 3), ("hand", 2, 1, "off", 2), ("hand", 3, "ucap", "strict", 1),
               ("one256", 1, 1, "off", 4)]
CHAIN_L, CHAIN_LPARTS = 3, 5


def _chain_draw(seed, name, world, chunks, mode, si):
    """x on the grid k / 8, |x| < 2 (exact in both 16-bit types), the network replaced by g = xin: the owned
    pixels of every unit map back to their own image pixels whatever the shift, so the update is
    x += sc x at the owned pixels, sc from sum |x| over them."""
    B, H, W, Th, Tw, plan = _plan(name)
    U = plan.shape[0]
    g = _gen(seed)
    sy, sx = _shifts(H, W, min(Th, Tw))[si]
    x = _ints(g, (B, H, W, 3), -15, 15) / 8.0
    _representable(x, "x")
    lpart, lcoef, uloss = _draw_losses(g, CHAIN_L, U, CHAIN_LPARTS, "off")
    units_of = [[u for u in range(U) if int(plan[u, 0]) == b] for b in range(B)]
    loss = torch.tensor([float(uloss[units_of[b]].sum()) for b in range(B)], dtype=torch.float64)
    if mode == "strict" and float(loss[1]) <= float(loss[0]):
        # image 0 takes the units' smaller partials: swap the two images' roles by zeroing image 0's
        lpart[:, units_of[0]] = 0.0
        uloss = torch.einsum("l,lup->u", lcoef.double(), lpart.double())
        loss = torch.tensor([float(uloss[units_of[b]].sum()) for b in range(B)], dtype=torch.float64)
    max_loss, done_in, done = _stop_rule(mode, loss, B)
    mask = torch.zeros(B, H, W, 3, dtype=torch.bool)
    for u in range(U):
        b, oy, ox, y0, y1, x0, x1 = _owned(plan, u)
        mask[b, oy + y0:oy + y1, ox + x0:ox + x1] = True
    mask = _rolled_to_image(mask, sy, sx)
    G = x * mask
    asum = [float(G[b].double().abs().sum()) for b in range(B)]
    assert max(asum) * 8 < 2 ** 24
    sc = np.array([0.0 if done[b] else _scale(STEP_GENERAL, asum[b], H, W) for b in range(B)], dtype=np.float32)
    A, Bc, ndiff = _check_general(x, G, sc.reshape(B, 1, 1, 1), gq=3)
    C, ucc = _layout(U, world, chunks)
    return _case(kind="general", Th=Th, Tw=Tw, plan=plan, world=world, C=C, ucc=ucc, shift=(sy, sx), x=x, lpart=lpart,
                 lcoef=lcoef, loss=loss, max_loss=max_loss, done_in=done_in, done=done, mask=mask, A=A, B=Bc,
                 ndiff=ndiff)


@functools.lru_cache(maxsize=None)
def _chain_case(name, world, chunks, mode, si):
    seed = 5000 + 100 * (len(name) + world + si) + len(mode)
    return _first_nonvacuous(lambda s: _chain_draw(s, name, world, chunks, mode, si), seed, "general")


@gpu
@dtypes
@pytest.mark.parametrize("name,world,chunks,mode,si", CHAIN_CASES)
def test_exact_tile_chain(native_lib, name, world, chunks, mode, si, dt):
    """The three tiled kernels chained as a step chains them, every rank and chunk packing into its slot of
    one packs buffer, with g = xin as a stand-in network: whatever the shift, x += sc x at the owned pixels
    (one of the two roundings), every other pixel bit-identical, loss and done exact."""
    c = _chain_case(name, world, chunks, mode, si)
    nunits, nb = c.plan.shape[0], c.x.shape[0]
    pe = _pack_elems(c.ucc, c.Th, c.Tw)
    packs = torch.full((c.C, world, pe), SENTINEL, dtype=dt, device=DEV)
    plan, lcoef = c.plan.to(DEV), c.lcoef.to(DEV)
    sh = torch.tensor(c.shift, dtype=torch.int32, device=DEV)
    x = c.x.clone().to(DEV)
    for rank in range(world):
        for ch, k0, units in _rank_chunks(nunits, world, c.C, c.ucc, rank):
            xin = torch.full((len(units), c.Th, c.Tw, 8), SENTINEL, dtype=dt, device=DEV)
            native_lib.tile_gather(x, xin, plan, sh, rank, world, k0)
            native_lib.tile_pack(xin, packs[ch, rank], plan, c.lpart[:, units].contiguous().to(DEV), lcoef, c.ucc, rank,
                                 world, k0)
    done = c.done_in.clone().to(DEV)
    loss = torch.full((nb,), NAN, device=DEV)
    native_lib.tile_update(packs, c.ucc, plan, sh, x, done, loss, STEP_GENERAL, c.max_loss, world, c.Th, c.Tw)
    assert torch.equal(loss.cpu().double(), c.loss), (loss.tolist(), c.loss.tolist())
    assert torch.equal(done.cpu(), c.done), (done.tolist(), c.done.tolist())
    _assert_update(x, c, where=c.mask)
    assert torch.equal(_bits(x)[~c.mask], _bits(c.x)[~c.mask]), "a pixel owned by no unit changed"


# ----------------------------------------------------------------------------------------
# 7. octave_resize
# ----------------------------------------------------------------------------------------

# (N, (Hs, Ws), (Hd, Wd)): dyadic ratios (1/2, 2, 3/4, 1, 0, 2^-7); the last has 1 051 650 output pixels, more
# than the 4096 x 256 threads of the capped grid: the grid-stride loop
OCT_SIZES = [(2, (5, 9), (9, 17)), (2, (9, 17), (5, 9)), (2, (4, 7), (5, 9)), (2, (5, 5), (5, 5)), (2, (1, 5), (3, 1)),
             (2, (3, 2), (1, 1)), (2, (5, 9), (513, 1025))]
OCT_OPS = ["a", "ab", "ac", "abc"]


@functools.lru_cache(maxsize=None)
def _oct_case(N, src, dst, ops):
    g = _gen(N + 31 * src[0] + 7 * src[1] + 3 * dst[0] + dst[1])
    a, b, c = (_ints(g, (N, *src, 3), -8, 8) for _ in range(3))
    total = a.double() + (b.double() if "b" in ops else 0) - (c.double() if "c" in ops else 0)
    for i, o in zip(src, dst):
        r = Fraction(i - 1, o - 1) if o > 1 else Fraction(0)
        assert (r * 2 ** 7).denominator == 1, "the size ratio is not a multiple of 2^-7"
    ref64 = F.interpolate(total.permute(0, 3, 1, 2), size=dst, mode="bilinear", align_corners=True)
    ref64 = ref64.permute(0, 2, 3, 1).contiguous()
    # weights are multiples of 2^-7, operands integers below 2^5: every product and sum a multiple of 2^-14
    q = ref64 * 2 ** 14
    assert torch.equal(q, q.round()) and float(ref64.abs().max()) < 2 ** 6 and float(total.abs().max()) <= 24
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64)
    assert ref.unique().numel() >= 3, "degenerate reference"
    if "c" in ops:
        assert not torch.equal(total, a.double() + (b.double() if "b" in ops else 0) + c.double())
    return _case(a=a, b=b if "b" in ops else None, c=c if "c" in ops else None, ref=ref)


@functools.lru_cache(maxsize=None)
def _oct_edge_case():
    a = _tile_edges((2, 5, 5, 3))
    return _case(a=a, b=None, c=None, ref=a)


def _run_resize(native_lib, c, dst, dt, with_yin):
    N = c.a.shape[0]
    y = torch.full((N, *dst, 3), NAN, device=DEV)
    yin = torch.full((N, *dst, 8), SENTINEL, dtype=dt, device=DEV) if with_yin else None
    native_lib.octave_resize(c.a.to(DEV), None if c.b is None else c.b.to(DEV), None if c.c is None else c.c.to(DEV), y,
                             yin)
    return y.cpu(), yin


@gpu
@dtypes
@pytest.mark.parametrize("N,src,dst", OCT_SIZES, ids=[f"{n}-{s[0]}x{s[1]}-{d[0]}x{d[1]}" for n, s, d in OCT_SIZES])
def test_exact_octave_resize(native_lib, N, src, dst, dt):
    """octave_resize_kernel with a alone, a + b, a - c and a + b - c, with and without the 16-bit copy: y
    equals the fp64 F.interpolate(bilinear, align_corners=True) exactly; yin channels 0..2 are its rounding
    bit for bit and channels 3..7 zero."""
    for ops in OCT_OPS:
        c = _oct_case(N, src, dst, ops)
        for with_yin in (True, False):
            y, yin = _run_resize(native_lib, c, dst, dt, with_yin)
            assert torch.equal(y, c.ref), (f"operands {ops}, yin {with_yin}: {int((y != c.ref).sum())} of {y.numel()} "
                                           f"values differ")
            if with_yin:
                _same_bits(yin[..., :3], c.ref.to(dt), f"yin channels 0..2 (operands {ops})")
                assert not bool(_bits(yin[..., 3:]).any()), "yin channels 3..7 must be zero"


@gpu
@dtypes
def test_exact_octave_resize_conversion_edges(native_lib, dt):
    """An identity resize of the conversion edge table with b = c = None: y equals a by value (the weights
    are 1 and 0; a -0.0 may come back as 0.0) and yin is the rounding of y bit for bit."""
    c = _oct_edge_case()
    y, yin = _run_resize(native_lib, c, (5, 5), dt, True)
    assert torch.equal(y, c.ref)
    _same_bits(yin[..., :3], y.to(dt), "yin channels 0..2 vs the rounded y")
    nz = c.ref != 0
    assert torch.equal(_bits(yin[..., :3])[nz], _bits(c.ref.to(dt))[nz])
    assert not bool(_bits(yin[..., 3:]).any()), "yin channels 3..7 must be zero"


# ----------------------------------------------------------------------------------------
# 8. what the bindings refuse (csrc/bindings.cpp), before any launch
# ----------------------------------------------------------------------------------------

GPU_TENSOR = "must be a GPU tensor"


def _strided(t):
    """``t`` as every second element of a buffer twice its size filled with 9: same values, not contiguous."""
    buf = torch.full((2 * t.numel(),), 9, dtype=t.dtype, device=t.device)
    buf[::2] = t
    v = buf[::2]
    assert not v.is_contiguous() or t.numel() < 2
    return buf, v


def _refusal_setup(dt):
    """Valid operands of the three tiled kernels on the hand-built plan (one rank, one chunk)."""
    B, H, W, Th, Tw, plan = _plan("hand")
    U = plan.shape[0]
    s = _case(B=B, U=U, Th=Th, Tw=Tw, plan=plan.to(DEV), shift=torch.zeros(2, dtype=torch.int32, device=DEV))
    s.x = torch.full((B, H, W, 3), SENTINEL, device=DEV)
    s.xin = torch.full((U, Th, Tw, 8), SENTINEL, dtype=dt, device=DEV)
    s.g = torch.ones(U, Th, Tw, 8, dtype=dt, device=DEV)
    s.pack = _new_pack(U, Th, Tw, dt, DEV)
    s.lpart = torch.ones(2, U, 3, device=DEV)
    s.lcoef = torch.ones(2, device=DEV)
    s.done = torch.full((B,), 9, dtype=torch.uint8, device=DEV)
    s.loss = torch.full((B,), SENTINEL, device=DEV)
    return s


def _untouched(s, dt):
    torch.cuda.synchronize()
    B, H, W, Th, Tw, _ = _plan("hand")
    assert bool((s.x.cpu() == SENTINEL).all()) and bool((s.xin.float().cpu() == SENTINEL).all())
    _same_bits(s.pack, _new_pack(s.U, Th, Tw, dt, "cpu"), "pack")
    assert bool((s.done.cpu() == 9).all()) and bool((s.loss.cpu() == SENTINEL).all())


@gpu
@dtypes
def test_tile_gather_refuses_host_xin(native_lib, dt):
    """A CPU ``xin`` would hand the kernel a host pointer: refused."""
    s = _refusal_setup(dt)
    xin = s.xin.cpu()
    with pytest.raises(RuntimeError, match=GPU_TENSOR):
        native_lib.tile_gather(s.x, xin, s.plan, s.shift, 0, 1, 0)
    assert bool((xin.float() == SENTINEL).all())
    _untouched(s, dt)


@gpu
@dtypes
@pytest.mark.parametrize("what", ["pack_host", "lpart_host", "lcoef_host", "lcoef_strided", "units_over_ucap",
                                  "pack_too_small"])
def test_tile_pack_refuses(native_lib, what, dt):
    """tile_pack refuses a CPU pack, lpart or lcoef, an lcoef that is not contiguous, more units than ucap
    and a pack smaller than tile_pack_elems(ucap), and writes nothing."""
    s = _refusal_setup(dt)
    pack, lpart, lcoef, ucap, match = s.pack, s.lpart, s.lcoef, s.U, GPU_TENSOR
    if what == "pack_host":
        pack = s.pack.cpu()
    elif what == "lpart_host":
        lpart = s.lpart.cpu()
    elif what == "lcoef_host":
        lcoef = s.lcoef.cpu()
    elif what == "lcoef_strided":
        _, lcoef = _strided(s.lcoef)
        match = "tile_pack: lcoef"
    elif what == "units_over_ucap":
        ucap, match = s.U - 1, "tile_pack: units"
    else:
        pack, match = s.pack[:_pack_elems(s.U, s.Th, s.Tw) - 8], "pack too small"
    before = pack.cpu().clone()
    with pytest.raises(RuntimeError, match=match):
        native_lib.tile_pack(s.g, pack, s.plan, lpart, lcoef, ucap, 0, 1, 0)
    _same_bits(pack, before, "the refused pack")
    _untouched(s, dt)


@gpu
@dtypes
@pytest.mark.parametrize("what", ["x_host", "done_host", "loss_host", "done_strided", "loss_strided",
                                  "packs_not_a_multiple"])
def test_tile_update_refuses(native_lib, what, dt):
    """tile_update refuses a CPU x, done or loss, a done or loss that is not contiguous, and packs whose size
    is no multiple of world * tile_pack_elems(ucap), and writes nothing."""
    s = _refusal_setup(dt)
    packs, x, done, loss, match = s.pack, s.x, s.done, s.loss, GPU_TENSOR
    bufs = []
    if what == "x_host":
        x = s.x.cpu()
    elif what == "done_host":
        done = s.done.cpu()
    elif what == "loss_host":
        loss = s.loss.cpu()
    elif what == "done_strided":
        buf, done = _strided(s.done)
        bufs, match = [(buf, 9)], "tile_update: done u8"
    elif what == "loss_strided":
        buf, loss = _strided(s.loss)
        bufs, match = [(buf, None)], "tile_update: done u8"
    else:
        packs, match = s.pack[:-8], "tile_update: packs"
    before = [t.cpu().clone() for t in (x, done, loss)] + [b.cpu().clone() for b, _ in bufs]
    with pytest.raises(RuntimeError, match=match):
        native_lib.tile_update(packs, s.U, s.plan, s.shift, x, done, loss, STEP_GENERAL, -1.0, 1, s.Th, s.Tw)
    torch.cuda.synchronize()
    for t, b in zip([x, done, loss] + [b for b, _ in bufs], before):
        assert torch.equal(t.cpu(), b), "a refused call wrote an output"
    _untouched(s, dt)


@gpu
@dtypes
def test_dream_update_refuses_empty_gpart(native_lib, dt):
    """gpart of shape [N, 0] leaves the absmean pass no block: the launcher returns -1 and nothing is
    written."""
    N, H, W = 2, 5, 7
    g = torch.ones(N, H, W, 8, dtype=dt, device=DEV)
    x = torch.full((N, H, W, 3), SENTINEL, device=DEV)
    xin = torch.full((N, H, W, 8), SENTINEL, dtype=dt, device=DEV)
    done = torch.full((N,), 9, dtype=torch.uint8, device=DEV)
    loss = torch.full((N,), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="launch failed with code -1"):
        native_lib.dream_update(g, x, xin, torch.empty(N, 0, device=DEV), torch.ones(1, N, 3, device=DEV),
                                torch.ones(1, device=DEV), done, loss, STEP_GENERAL, -1.0)
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all()) and bool((xin.float() == SENTINEL).all())
    assert bool((done == 9).all()) and bool((loss == SENTINEL).all())


# ----------------------------------------------------------------------------------------
# the conditions of every case, on the CPU alone
# ----------------------------------------------------------------------------------------

def _tu_with_packs(*case):
    c = _tu_case(*case)
    for dt in (BF, HF):
        _tu_packs(c, dt)
    return c


CASE_TABLES = {
    "edge_values": (_edge_values, [()]),
    "plans": (_plan, [("tiles8",), ("one256",), ("one384",), ("hand",)]),
    "dream_update": (_du_case, DU_CASES),
    "tile_gather": (_tg_case, TG_CASES),
    "tile_pack": (_tpk_case, TPK_CASES),
    "tile_update": (_tu_with_packs, TU_CASES),
    "tile_chain": (_chain_case, CHAIN_CASES),
    "octave_resize": (_oct_case, [(N, s, d, ops) for N, s, d in OCT_SIZES for ops in OCT_OPS]),
    "octave_resize_edges": (_oct_edge_case, [()]),
}


@pytest.mark.parametrize("table", sorted(CASE_TABLES))
def test_conditions(table):
    """Every case of every table: generator, CPU reference and the method's conditions (asserted inside
    the case builders, for bf16 and fp16), without a GPU."""
    build, cases = CASE_TABLES[table]
    assert cases
    for case in cases:
        try:
            build(*case)
        except AssertionError as e:
            raise AssertionError(f"{table} case {case}: {e}") from e
