"""Activation maps on the CPU: the torch reference of ops/actmap.py against the naive float64 oracle
(actmap_oracle.py) and against F.interpolate, and engine/activations.py on the small CPU VGG16 (S = 32)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import actmap_oracle as A
import occlusion_oracle as O
from deconv_api_amd import ops
from deconv_api_amd.engine.activations import ActivationMaps, ActivationResult
from deconv_api_amd.engine.deconvnet import DeconvNet, UnknownLayerError
from deconv_api_amd.models.vgg16 import VGG16

BF, HF = torch.bfloat16, torch.float16
cases = pytest.mark.parametrize("S,H", A.CASES)


# --------------------------------------------------------------------------- the oracle's own two forms
@pytest.mark.parametrize("S,H", [(24, 12), (40, 5), (64, 2)])
def test_oracle_row_forms_equal_the_pixel_loops(S, H):
    act, idx = A.rand_case(S, H, 8)
    assert np.array_equal(A.heat(act, idx, S, A.heat_map_rows), A.heat_case("rand", S, H, 8))
    h = A.heat_case("rand", S, H, 8)
    x0 = O.image_case(2, S)
    for b in range(2):
        assert np.array_equal(A.overlay_rows(h[b], idx[b].numpy(), x0[b].float().numpy()),
                              O.overlay(h[b], idx[b].numpy(), x0[b].float().numpy()))


# --------------------------------------------------------------------------- torch reference against the oracle
@cases
@pytest.mark.parametrize("C", [8, 512])
def test_reference_is_bit_exact_on_integer_maps(S, H, C):
    """Integers in [-64, 64]: every intermediate is a multiple of 2^-14 below 2^7, exact in fp32 in any order."""
    act, idx = A.int_case(S, H, C)
    keep = act.clone()
    heat, part = ops.activation_heat(act, idx, S)
    ref = A.heat_case("int", S, H, C)
    assert heat.shape == (2, 4, S, S) and heat.dtype == torch.float32 and part.shape == (2, 4, 1)
    assert np.array_equal(heat.numpy().astype(np.float64), ref)
    assert np.array_equal(part[..., 0].numpy().astype(np.float64), np.abs(ref).max(axis=(2, 3)))
    assert torch.equal(act, keep)
    # a filter outside 0 .. C - 1: a zero map and a zero partial
    assert not bool(heat[1, 1].any()) and not bool(heat[1, 2].any()) and bool(heat[0].any())
    assert float(part[1, 1]) == 0 and float(part[1, 2]) == 0


@cases
@pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "fp16"])
def test_reference_on_random_maps(S, H, dt):
    act, idx = A.rand_case(S, H, 8, dt)
    heat, part = ops.activation_heat(act, idx, S)
    u = A.within_bound(heat.numpy(), A.heat_case("rand", S, H, 8, dt), act, idx)
    print(f"reference ({S}, {H}) {dt}: {u:.3f} of the bound")
    assert torch.equal(part[..., 0], heat.abs().amax(dim=(2, 3)))
    # fp32 input (the CPU engine's layer output) gives the same as the 16-bit bits
    assert torch.equal(ops.activation_heat(act.float(), idx, S)[0], heat)


@pytest.mark.parametrize("S,H", A.CASES + [(224, 14), (224, 7), (224, 224), (32, 4), (48, 6)])
def test_reference_equals_interpolate_on_integer_maps(S, H):
    act, idx = A.int_case(S, H, 8, BF, 1)
    heat, _ = ops.activation_heat(act, idx, S)
    want = F.interpolate(act.float().permute(0, 3, 1, 2), size=(S, S), mode="bilinear", align_corners=False)
    assert torch.equal(heat[0], want[0, idx[0].long().clamp(0, 7)] * ((idx[0] >= 0) & (idx[0] < 8)).view(4, 1, 1))


def test_ratio_one_equals_the_seed_map():
    act, _ = A.rand_case(32, 32, 8)
    idx = torch.tensor([[3, 0, 7, -1], [-1, 5, 5, 1]], dtype=torch.int32)
    heat, _ = ops.activation_heat(act, idx, 32)
    assert torch.equal(heat, ops.seed_map(act, idx, "all").view(2, 4, 32, 32))


def test_refusals():
    idx = torch.zeros(1, 4, dtype=torch.int32)
    for act, S in ((torch.zeros(8, 8, 8), 16),  # not 4-D
                   (torch.zeros(1, 8, 8, 8), 24),  # r = 3
                   (torch.zeros(1, 8, 4, 8), 16),  # H != W
                   (torch.zeros(1, 1, 1, 8), 128),  # r = 128
                   (torch.zeros(1, 5, 5, 8), 16),  # S / H not whole
                   (torch.zeros(1, 8, 8, 8), 8),  # S < 16
                   (torch.zeros(1, 16, 16, 8), 8)):  # r < 1
        with pytest.raises(ValueError):
            ops.activation_heat(act, idx, S)
    with pytest.raises(ValueError):
        ops.activation_heat(torch.zeros(2, 8, 8, 8), idx, 16)  # idx rows


# --------------------------------------------------------------------------- overlay of the reference's heat
@pytest.mark.parametrize("S,H", [(32, 4), (48, 6), (32, 16), (224, 14)])
def test_overlay_of_the_reference_heat(S, H):
    """The picture's condition (every byte within one level of the float64 oracle on the float64 heat, at most 0.5 % of
    the bytes different) for the fp32 torch reference."""
    B = 1 if S == 224 else 2
    act, idx = A.rand_case(S, H, 8, BF, B)
    x0 = O.image_case(B, S)
    heat, part = ops.activation_heat(act, idx, S)
    got = ops.occlusion_overlay(heat, part, idx, x0)
    frac = A.overlay_within(got.numpy(), A.heat_case("rand", S, H, 8, BF, B), idx, x0,
                            A.overlay_rows if S == 224 else O.overlay)
    print(f"overlay ({S}, {H}): {100 * frac:.4f} % of the bytes differ")
    assert not bool(got[-1, :S, S:].any()), "the idx = -1 tile is not black"
    bg = (x0[-1, ..., :3].float() + torch.tensor(O.MEAN)).clamp(0, 255)
    assert torch.equal(got[-1, S:, :S], torch.floor(bg + 0.5).to(torch.uint8)), "a zero map (idx = C) is not the plain image"


# --------------------------------------------------------------------------- engine on the small CPU VGG16
@pytest.fixture(scope="module")
def net(small_specs):
    return DeconvNet(VGG16.random(0, specs=small_specs).build("cpu", torch.float32))


@pytest.fixture(scope="module")
def x32():
    x = torch.zeros(3, 32, 32, 8)
    x[..., :3] = torch.randint(0, 256, (3, 32, 32, 3), generator=torch.Generator().manual_seed(5)).float() - \
        torch.tensor(O.MEAN)
    return x


@pytest.mark.parametrize("layer", ["block1_conv2", "block3_pool", "block5_conv3"])
def test_engine_equals_the_oracle_on_its_forward(net, x32, layer):
    res = ActivationMaps(net).run(x32, layer)
    assert isinstance(res, ActivationResult)
    assert res.filters.shape == (3, 4) and res.filters.dtype == torch.int32 and res.sums.shape == (3, 4)
    assert res.heat.shape == (3, 4, 32, 32) and res.heat.dtype == torch.float32
    assert res.mosaic.shape == (3, 64, 64, 3) and res.mosaic.dtype == torch.uint8
    out = net.forward(x32, layer).out
    idx, sums = net.select_filters(out, 4, "per_image")
    assert torch.equal(res.filters, idx) and torch.equal(res.sums, sums) and bool((idx >= 0).any())
    ref = A.heat(out, idx, 32)
    A.within_bound(res.heat.numpy(), ref, out, idx)
    A.overlay_within(res.mosaic.numpy(), ref, idx, x32)
    assert float(res.heat.abs().max()) > 0


def test_engine_refusals(net, x32):
    maps = ActivationMaps(net)
    for layer in ("flatten", "fc1", "predictions"):
        with pytest.raises(ValueError, match="has no feature map"):
            maps.run(x32, layer)
    with pytest.raises(UnknownLayerError):
        maps.run(x32, "nope")
    with pytest.raises(UnknownLayerError):
        maps.run(x32, "input_1")
    with pytest.raises(ValueError):
        maps.run(x32[0], "block1_conv2")
    assert maps.spatial_layers() == [s.name for s in net.specs[1:] if s.kind in ("conv", "pool")]
    assert "flatten" not in maps.spatial_layers() and "block5_pool" in maps.spatial_layers()
