"""Exact-oracle tests of the occlusion kernels (csrc/occlusion.hip: occlude_variants, occlusion_heat,
occlusion_overlay, through the binding and through ops.occlusion), in the style of test_dream_lap_exact_gpu.py.

The oracle is the naive float64 loop of occlusion_oracle.py. Variants are copies and zeros: bit for bit. Heat on
integer scores in [-8, 8]: every drop and every sum of at most 9 drops is a small integer, exact in fp32 in any order;
where all covering counts are powers of two the quotient is exact too, elsewhere it is ONE correctly rounded fp32
division of exact operands, within 1 ulp of the float64 quotient rounded to fp32. The overlay's condition (every
byte within one level, at most 0.5 % of the bytes different) is first asserted for the fp32 torch reference on the
same inputs."""
import numpy as np
import pytest
import torch

import occlusion_oracle as O
from deconv_api_amd import ops
from exact_helpers import BF, DEV, HF

gpu = pytest.mark.gpu
dtypes = pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
SENTINEL = -77.0
GUARD = 64  # elements of sentinel on either side of an output (keeps 16-B alignment for every dtype used)


def _guarded(shape, dtype=torch.float32, fill=SENTINEL):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(*shape), buf


def _guards_intact(bufs, fill=SENTINEL):
    return all(bool((b[:GUARD].float() == fill).all()) and bool((b[-GUARD:].float() == fill).all()) for b in bufs)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


# --------------------------------------------------------------------------- occlude_variants
def _variants(native_lib, B, S, p, s, dt):
    x0 = O.image_case(B, S, dt)
    V = len(O.grid(S, p, s)) ** 2 + 1
    want = torch.cat([torch.from_numpy(O.variants(x0[b].float().numpy(), p, s)) for b in range(B)]).to(dt)
    xg = x0.to(DEV)
    keep = xg.clone()
    xv, buf = _guarded((B * V, S, S, 8), dt)
    native_lib.occlude_variants(xg, xv, p, s)
    assert torch.equal(_bits(xv), _bits(want))
    assert _guards_intact([buf]) and torch.equal(xg, keep)
    assert torch.equal(_bits(ops.occlude_variants(xg, p, s)), _bits(want))


@gpu
@dtypes
@pytest.mark.parametrize("S,p,s", O.SMALL)
def test_exact_variants(native_lib, S, p, s, dt):
    """Bit for bit (so every element is written: none keeps the sentinel, and all 8 channels are copied outside a
    patch and zeroed inside), guards intact, input unchanged; the op surface gives the same bits."""
    _variants(native_lib, 2, S, p, s, dt)


@gpu
def test_exact_variants_default_grid(native_lib):
    """The production geometry once: 170 variants of one 224 x 224 image (196 x 11 blocks)."""
    _variants(native_lib, 1, 224, 32, 16, BF)


# --------------------------------------------------------------------------- occlusion_heat
@gpu
@pytest.mark.parametrize("S,p,s", O.SMALL)
@pytest.mark.parametrize("C", [64, 1000])
def test_exact_heat(native_lib, S, p, s, C):
    sc, idx = O.score_case(2, S, p, s, C)
    ref = O.heat_case(2, S, p, s, C)
    heat, hbuf = _guarded((2, 4, S, S))
    part, pbuf = _guarded((2, 4, native_lib.occlusion_parts(S)))
    scg, ig = sc.to(DEV), idx.to(DEV)
    native_lib.occlusion_heat(scg, ig, heat, part, p, s)
    got = heat.cpu().numpy()
    assert not bool((part == SENTINEL).any())
    if (S, p, s) in O.POW2:
        assert np.array_equal(got.astype(np.float64), ref)
    else:
        u = float(O.ulp_diff(got, ref).max())
        print(f"heat ({S}, {p}, {s}) C {C}: max {u:.3g} ulp")
        assert u <= 1
    assert not got[1, 1].any() and got[0].any()  # the idx = -1 row is zero
    # the partials reduce to exactly max |heat| of what the kernel wrote
    assert np.array_equal(part.amax(dim=2).cpu().numpy(), np.abs(got).max(axis=(2, 3)))
    assert _guards_intact([hbuf, pbuf]) and torch.equal(scg.cpu(), sc) and torch.equal(ig.cpu(), idx)
    h2, p2 = ops.occlusion_heat(scg, ig, S, p, s)
    assert torch.equal(h2, heat) and torch.equal(p2, part)


# --------------------------------------------------------------------------- occlusion_overlay
@gpu
@dtypes
@pytest.mark.parametrize("S,p,s", [(24, 8, 4), (27, 8, 6), (25, 12, 5)])
def test_overlay(native_lib, S, p, s, dt):
    heat, idx, x0 = O.overlay_case(S, p, s, dt)
    part1 = heat.abs().amax(dim=(2, 3)).unsqueeze(-1)
    # the condition, on the CPU: the fp32 torch reference stays inside the bound for these inputs
    O.overlay_within(ops.occlusion_overlay(heat, part1, idx, x0).numpy(), heat, idx, x0)
    hg, ig, xg = heat.to(DEV), idx.to(DEV), x0.to(DEV)
    part = torch.zeros(2, 4, native_lib.occlusion_parts(S), device=DEV)  # max |heat| in the first partial ...
    part[..., 0] = part1[..., 0]
    out, obuf = _guarded((2, 2 * S, 2 * S, 3), torch.uint8, fill=77)
    native_lib.occlusion_overlay(hg, part, ig, xg, out)
    got = out.cpu()
    O.overlay_within(got.numpy(), heat, idx, x0)
    assert _guards_intact([obuf], fill=77)
    assert not bool(got[1, :S, S:].any()), "the idx = -1 tile is not black"
    bg = (x0[0, ..., :3].float() + torch.tensor(O.MEAN)).clamp(0, 255)
    assert torch.equal(got[0, S:, :S], torch.floor(bg + 0.5).to(torch.uint8)), "an m = 0 tile is not the plain image"
    tiles = [got[0, :S, :S], got[0, :S, S:], got[0, S:, :S], got[0, S:, S:]]
    assert all(not torch.equal(tiles[i], tiles[j]) for i in range(4) for j in range(i))  # tile placement
    # ... or in the last: the maximum is the partials' maximum wherever it sits among them
    assert torch.equal(ops.occlusion_overlay(hg, part.flip(2).contiguous(), ig, xg).cpu(), got)


@gpu
def test_binding_refuses_bad_arguments(native_lib):
    x0 = O.image_case(1, 24).to(DEV)
    xv = torch.empty(10, 24, 24, 8, dtype=BF, device=DEV)
    native_lib.occlude_variants(x0, xv, 8, 8)
    for bad in (lambda: native_lib.occlude_variants(x0, xv[:9], 8, 8),  # extent
                lambda: native_lib.occlude_variants(x0, xv.half(), 8, 8),  # dtype
                lambda: native_lib.occlude_variants(x0.cpu(), xv, 8, 8),  # device
                lambda: native_lib.occlude_variants(x0.transpose(1, 2), xv, 8, 8),  # contiguity
                lambda: native_lib.occlude_variants(x0.float(), xv, 8, 8),
                lambda: native_lib.occlude_variants(x0, xv, 7, 4),  # p < 8
                lambda: native_lib.occlude_variants(x0, xv, 13, 4),  # p > S / 2
                lambda: native_lib.occlude_variants(x0, xv, 8, 9),  # s > p
                lambda: native_lib.occlude_variants(x0, xv, 8, 3)):  # s < 4
        with pytest.raises(RuntimeError):
            bad()
    big = torch.empty(1, 224, 224, 8, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):  # 16 x 16 = 256 patches
        native_lib.occlude_variants(big, torch.empty(257, 224, 224, 8, dtype=BF, device=DEV), 14, 14)
    sc, idx = [t.to(DEV) for t in O.score_case(1, 24, 8, 8, 64)]
    heat = torch.empty(1, 4, 24, 24, device=DEV)
    part = torch.empty(1, 4, native_lib.occlusion_parts(24), device=DEV)
    native_lib.occlusion_heat(sc, idx, heat, part, 8, 8)
    for bad in (lambda: native_lib.occlusion_heat(sc[:, :9], idx, heat, part, 8, 8),  # P + 1 rows
                lambda: native_lib.occlusion_heat(sc, idx.long(), heat, part, 8, 8),
                lambda: native_lib.occlusion_heat(sc, idx, heat, part[..., :1], 8, 8),
                lambda: native_lib.occlusion_heat(sc.cpu(), idx, heat, part, 8, 8),
                lambda: native_lib.occlusion_heat(sc, idx, heat, part, 8, 4)):  # another grid
        with pytest.raises(RuntimeError):
            bad()
    out = torch.empty(1, 48, 48, 3, dtype=torch.uint8, device=DEV)
    native_lib.occlusion_overlay(heat, part, idx, x0, out)
    for bad in (lambda: native_lib.occlusion_overlay(heat, part, idx, x0, out[:, :47]),
                lambda: native_lib.occlusion_overlay(heat[:, :3], part, idx, x0, out),
                lambda: native_lib.occlusion_overlay(heat, part, idx, x0.float(), out),
                lambda: native_lib.occlusion_overlay(heat, part, idx, x0, out.cpu())):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(ValueError):
        ops.occlude_variants(x0, 8, 3)
