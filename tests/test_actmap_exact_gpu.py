"""Exact-oracle tests of the activation-map kernel (csrc/actmap.hip: activation_heat, through the binding and through
ops.actmap), in the style of test_occlusion_exact_gpu.py.

The oracle is the naive float64 loop of actmap_oracle.py. On integer maps in [-64, 64] every intermediate of the
definition is a multiple of 2^-14 below 2^7, exact in fp32 in any order with or without FMA contraction: bit for bit,
the max |heat| partials included. On random 16-bit maps the bound is 8 x 2^-24 max |a| (at most five fp32 roundings of
values bounded by max |a|). The overlay's condition (every byte within one level of the float64 oracle on the float64
heat, at most 0.5 % of the bytes different) is first asserted for the fp32 torch reference on the same inputs."""
import numpy as np
import pytest
import torch

import actmap_oracle as A
import occlusion_oracle as O
from deconv_api_amd import ops
from exact_helpers import BF, DEV, HF

gpu = pytest.mark.gpu
dtypes = pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
SENTINEL = -77.0
GUARD = 64  # elements of sentinel on either side of an output


def _guarded(shape, dtype=torch.float32, fill=SENTINEL):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf[GUARD:GUARD + n].view(*shape), buf


def _guards_intact(bufs, fill=SENTINEL):
    return all(bool((b[:GUARD].float() == fill).all()) and bool((b[-GUARD:].float() == fill).all()) for b in bufs)


def _run(native_lib, act, idx, S):
    """The kernel through the binding into guarded sentinel-filled outputs; inputs unchanged, no sentinel left, the
    partials reduce to exactly max |heat| of what was written, and ops gives the same bits."""
    B = act.shape[0]
    ag, ig = act.to(DEV), idx.to(DEV)
    ka, ki = ag.clone(), ig.clone()
    heat, hbuf = _guarded((B, 4, S, S))
    part, pbuf = _guarded((B, 4, native_lib.occlusion_parts(S)))
    native_lib.activation_heat(ag, ig, heat, part)
    torch.cuda.synchronize()
    assert _guards_intact([hbuf, pbuf]) and torch.equal(ag, ka) and torch.equal(ig, ki)
    assert not bool((part == SENTINEL).any()) and not bool((heat == SENTINEL).any())
    assert torch.equal(part.amax(dim=2), heat.abs().amax(dim=(2, 3)))
    h2, p2 = ops.activation_heat(ag, ig, S)
    assert torch.equal(h2, heat) and torch.equal(p2, part)
    return heat.clone(), part.clone()


@gpu
@dtypes
@pytest.mark.parametrize("C", [8, 512])
@pytest.mark.parametrize("S,H", A.CASES)
def test_exact_heat_integer_maps(native_lib, S, H, C, dt):
    act, idx = A.int_case(S, H, C, dt)
    ref = A.heat_case("int", S, H, C, dt)
    heat, part = _run(native_lib, act, idx, S)
    got = heat.cpu().numpy()
    assert np.array_equal(got.astype(np.float64), ref)
    assert np.array_equal(part.amax(dim=2).cpu().numpy().astype(np.float64), np.abs(ref).max(axis=(2, 3)))
    assert not got[1, 1].any() and not got[1, 2].any() and got[0].any()  # idx = -1 and idx = C: zero maps
    assert not bool(part[1, 1].any()) and not bool(part[1, 2].any())


@gpu
@dtypes
@pytest.mark.parametrize("C", [8, 512])
@pytest.mark.parametrize("S,H", A.CASES)
def test_heat_random_maps(native_lib, S, H, C, dt):
    act, idx = A.rand_case(S, H, C, dt)
    heat, _ = _run(native_lib, act, idx, S)
    u = A.within_bound(heat.cpu().numpy(), A.heat_case("rand", S, H, C, dt), act, idx)
    print(f"heat ({S}, {H}) C {C} {dt}: {u:.3f} of the bound")


@gpu
@dtypes
def test_ratio_one_equals_the_seed_map(native_lib, dt):
    act, _ = A.rand_case(32, 32, 512, dt)
    idx = torch.tensor([[3, 0, 511, -1], [-1, 8, 8, 7]], dtype=torch.int32)
    heat, _ = _run(native_lib, act, idx, 32)
    assert torch.equal(heat, ops.seed_map(act.to(DEV), idx.to(DEV), "all").view(2, 4, 32, 32))


@gpu
def test_production_geometry(native_lib):
    """block5_conv3 at 224: (S, H) = (224, 14), C = 512, one image (196 blocks)."""
    act, idx = A.int_case(224, 14, 512, BF, 1)
    heat, _ = _run(native_lib, act, idx, 224)
    assert np.array_equal(heat.cpu().numpy().astype(np.float64), A.heat_case("int", 224, 14, 512, BF, 1))
    act, idx = A.rand_case(224, 14, 512, BF, 1)
    heat, _ = _run(native_lib, act, idx, 224)
    A.within_bound(heat.cpu().numpy(), A.heat_case("rand", 224, 14, 512, BF, 1), act, idx)


@gpu
@pytest.mark.parametrize("S,H", [(32, 4), (48, 6), (32, 16), (224, 14)])
def test_overlay_of_the_kernels_heat(native_lib, S, H):
    B = 1 if S == 224 else 2
    act, idx = A.rand_case(S, H, 8, BF, B)
    x0 = O.image_case(B, S)
    ref = A.heat_case("rand", S, H, 8, BF, B)
    fn = A.overlay_rows if S == 224 else O.overlay
    # the condition, on the CPU: the fp32 torch reference stays inside the bound for these inputs
    hc, pc = ops.activation_heat(act, idx, S)
    A.overlay_within(ops.occlusion_overlay(hc, pc, idx, x0).numpy(), ref, idx, x0, fn)
    heat, part = _run(native_lib, act, idx, S)
    got = ops.occlusion_overlay(heat, part, idx.to(DEV), x0.to(DEV)).cpu()
    frac = A.overlay_within(got.numpy(), ref, idx, x0, fn)
    print(f"overlay ({S}, {H}): {100 * frac:.4f} % of the bytes differ")
    assert not bool(got[-1, :S, S:].any()), "the idx = -1 tile is not black"
    bg = (x0[-1, ..., :3].float() + torch.tensor(O.MEAN)).clamp(0, 255)
    assert torch.equal(got[-1, S:, :S], torch.floor(bg + 0.5).to(torch.uint8)), "a zero map (idx = C) is not the plain image"


@gpu
def test_binding_refuses_bad_arguments(native_lib):
    act = A.int_case(24, 12, 8)[0].to(DEV)
    idx = A.filters(8).to(DEV)
    heat = torch.empty(2, 4, 24, 24, device=DEV)
    part = torch.empty(2, 4, native_lib.occlusion_parts(24), device=DEV)
    native_lib.activation_heat(act, idx, heat, part)

    def outs(B, S):
        return torch.empty(B, 4, S, S, device=DEV), torch.empty(B, 4, native_lib.occlusion_parts(S), device=DEV)

    z = lambda *s: torch.zeros(*s, dtype=BF, device=DEV)  # noqa: E731
    i1 = idx[:1].contiguous()
    for bad in (lambda: native_lib.activation_heat(z(1, 8, 8, 8), i1, *outs(1, 24)),  # r = 3
                lambda: native_lib.activation_heat(z(1, 8, 4, 8), i1, *outs(1, 16)),  # H != W
                lambda: native_lib.activation_heat(z(1, 8, 8, 12), i1, *outs(1, 16)),  # C = 12
                lambda: native_lib.activation_heat(z(1, 4, 4, 8), i1, *outs(1, 8)),  # S = 8
                lambda: native_lib.activation_heat(z(1, 1, 1, 8), i1, *outs(1, 128)),  # r = 128
                lambda: native_lib.activation_heat(z(1, 32, 32, 8), i1, *outs(1, 16)),  # r < 1
                lambda: native_lib.activation_heat(act.float(), idx, heat, part),  # dtype
                lambda: native_lib.activation_heat(act.cpu(), idx, heat, part),  # device
                lambda: native_lib.activation_heat(act.transpose(1, 2), idx, heat, part),  # contiguity
                lambda: native_lib.activation_heat(act, idx.long(), heat, part),
                lambda: native_lib.activation_heat(act, idx[:1], heat, part),  # idx rows
                lambda: native_lib.activation_heat(act, idx, heat[:1], part),  # heat batch
                lambda: native_lib.activation_heat(act, idx, heat[:, :3], part),
                lambda: native_lib.activation_heat(act, idx, heat.half(), part),
                lambda: native_lib.activation_heat(act, idx, heat, part[..., :2]),  # parts
                lambda: native_lib.activation_heat(act, idx, heat, part.cpu())):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(ValueError):
        ops.activation_heat(z(1, 8, 8, 8), i1, 24)
    with pytest.raises(ValueError):
        ops.activation_heat(z(1, 8, 8, 8).float(), i1, 16)  # the kernel takes the 16-bit layer output
