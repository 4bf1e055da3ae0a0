"""Occlusion sensitivity on the CPU: the grid, the torch references of ops/occlusion.py against the naive float64
oracle (occlusion_oracle.py), and engine/occlusion.py on the CPU VGG16 (5 variants: patch = stride = 112)."""
import numpy as np
import pytest
import torch

import occlusion_oracle as O
from deconv_api_amd import ops
from deconv_api_amd.engine.deconvnet import DeconvNet, UnknownLayerError
from deconv_api_amd.engine.occlusion import Occlusion
from deconv_api_amd.models.vgg16 import VGG16

BF = torch.bfloat16


# --------------------------------------------------------------------------- grid
@pytest.mark.parametrize("S,p,s", O.GRID_CASES)
def test_grid_equals_the_oracle(S, p, s):
    o = ops.occlusion_grid(S, p, s)
    assert list(o) == O.grid(S, p, s)
    assert all(0 <= a and a + p <= S for a in o) and list(o) == sorted(set(o))  # inside, distinct, ascending
    assert O.counts(S, p, s).min() >= 1  # covered


def test_grid_properties_of_the_cases():
    assert len(ops.occlusion_grid(224, 32, 16)) == 13
    assert set(O.counts(24, 8, 8)) == {1}
    assert set(O.counts(24, 8, 4)) == {1, 2}  # per axis: 1, 2 and 4 patches per pixel
    assert ops.occlusion_grid(27, 8, 6)[-2:] == (18, 19) and 3 in set(O.counts(27, 8, 6))  # clamped last position
    assert len(ops.occlusion_grid(224, 112, 112)) ** 2 == 4


@pytest.mark.parametrize("S,p,s", [(224, 16, 12), (224, 7, 4), (224, 113, 16), (224, 32, 33), (224, 32, 3),
                                   (24, 13, 4), (224, 32, 16.0), (224, "32", 16), (224, True, 16)],
                         ids=["P>255", "p<8", "p>S/2", "s>p", "s<4", "p>S/2 small", "float", "str", "bool"])
def test_grid_refusals(S, p, s):
    with pytest.raises(ValueError):
        ops.occlusion_grid(S, p, s)
    if isinstance(p, int) and isinstance(s, int) and not isinstance(p, bool):
        with pytest.raises(ValueError):
            O.grid(S, p, s)
        with pytest.raises(ValueError):
            ops.occlude_variants(torch.zeros(1, S, S, 8), p, s)
        with pytest.raises(ValueError):
            ops.occlusion_heat(torch.zeros(1, 5, 4), torch.zeros(1, 4, dtype=torch.int32), S, p, s)


def test_grid_limit_is_255_patches():
    assert len(ops.occlusion_grid(224, 28, 14)) == 15  # 15 x 15 = 225 passes
    with pytest.raises(ValueError, match="at most 255"):
        ops.occlusion_grid(224, 14, 14)  # 16 x 16 = 256


# --------------------------------------------------------------------------- torch references against the oracle
@pytest.mark.parametrize("S,p,s", O.SMALL)
def test_variants_reference_is_bit_exact(S, p, s):
    x0 = O.image_case(2, S)
    keep = x0.clone()
    got = ops.occlude_variants(x0, p, s)
    V = len(O.grid(S, p, s)) ** 2 + 1
    assert got.shape == (2 * V, S, S, 8) and got.dtype == x0.dtype
    for b in range(2):
        want = O.variants(x0[b].float().numpy(), p, s)
        assert np.array_equal(got[b * V:(b + 1) * V].float().numpy(), want)
    assert bool((x0[..., 3:] != 0).all()) and torch.equal(x0, keep)


@pytest.mark.parametrize("S,p,s", O.SMALL)
def test_heat_reference(S, p, s):
    """Integer scores in [-8, 8]: every sum is a small integer in any order; where all covering counts are powers of
    two the quotient is exact, elsewhere it is one fp32 division of exact operands (<= 1 ulp of the float64 one)."""
    sc, idx = O.score_case(2, S, p, s, 64)
    heat, part = ops.occlusion_heat(sc, idx, S, p, s)
    ref = O.heat_case(2, S, p, s, 64)
    assert heat.shape == (2, 4, S, S) and heat.dtype == torch.float32
    if (S, p, s) in O.POW2:
        assert np.array_equal(heat.numpy().astype(np.float64), ref)
    else:
        assert float(O.ulp_diff(heat.numpy(), ref).max()) <= 1
    assert not bool(heat[1, 1].any()) and bool(heat[0].any())  # the idx = -1 row
    assert np.array_equal(part.amax(dim=2).numpy(), np.abs(heat.numpy()).max(axis=(2, 3)))


@pytest.mark.parametrize("S,p,s", [(24, 8, 4), (27, 8, 6)])
@pytest.mark.parametrize("dt", [BF, torch.float16], ids=["bf16", "fp16"])
def test_overlay_reference(S, p, s, dt):
    heat, idx, x0 = O.overlay_case(S, p, s, dt)
    part = heat.abs().amax(dim=(2, 3)).unsqueeze(-1)
    got = ops.occlusion_overlay(heat, part, idx, x0)
    assert got.shape == (2, 2 * S, 2 * S, 3) and got.dtype == torch.uint8
    O.overlay_within(got.numpy(), heat, idx, x0)
    assert not bool(got[1, :S, S:].any()), "the idx = -1 tile is not black"
    bg = (x0[0, ..., :3].float() + torch.tensor(O.MEAN)).clamp(0, 255)
    assert torch.equal(got[0, S:, :S], torch.floor(bg + 0.5).to(torch.uint8)), "a zero-heat tile is not the plain image"
    tiles = [got[0, :S, :S], got[0, :S, S:], got[0, S:, :S], got[0, S:, S:]]
    assert all(not torch.equal(tiles[i], tiles[j]) for i in range(4) for j in range(i))  # placement


# --------------------------------------------------------------------------- engine on the CPU VGG16
@pytest.fixture(scope="module")
def net():
    return DeconvNet(VGG16.random(0, include_top=False).build("cpu", torch.float32))


@pytest.fixture(scope="module")
def x224():
    rgb = torch.randint(0, 256, (1, 224, 224, 3), generator=torch.Generator().manual_seed(5)).float()
    x = torch.zeros(1, 224, 224, 8)
    x[..., :3] = rgb - torch.tensor(O.MEAN)
    return x


@pytest.mark.parametrize("layer", ["block1_conv2", "block2_pool"])
def test_engine_equals_the_oracle_on_its_scores(net, x224, layer):
    res = Occlusion(net).run(x224, layer, patch=112, stride=112)
    assert res.scores.shape == (1, 5, 4) and res.filters.shape == (1, 4) and res.heat.shape == (1, 4, 224, 224)
    assert res.mosaic.shape == (1, 448, 448, 3) and res.mosaic.dtype == torch.uint8
    xv = torch.from_numpy(O.variants(x224[0].numpy(), 112, 112))
    sums = ops.channel_sum(net.forward(xv, layer).out)  # one call on the oracle's variants
    f = res.filters[0].long()
    assert bool((f >= 0).all()) and torch.equal(res.filters, net.select_filters(net.forward(x224, layer).out, 4)[0])
    assert torch.equal(res.scores[0], sums[:, f])
    want = O.heat(sums.numpy(), res.filters[0].numpy(), 224, 112, 112)
    assert np.array_equal(res.heat[0].numpy().astype(np.float64), want.astype(np.float32).astype(np.float64))
    ref = O.overlay(res.heat[0].double().numpy(), res.filters[0].numpy(), x224[0].numpy())
    d = np.abs(res.mosaic[0].numpy().astype(int) - ref.astype(int))
    assert d.max() <= 1 and (d != 0).mean() <= 0.005
    assert float(res.heat.abs().max()) > 0


def test_engine_with_fewer_than_four_positive_filters():
    """A constant image on a model whose block1_conv2 weights are zero except two channels (positive bias there):
    two filters, two -1, black tiles."""
    model = VGG16.random(0, include_top=False)
    w, b = model.params["block1_conv2"]
    w = torch.zeros_like(w)
    b = torch.zeros_like(b)
    w[..., 5] = 0.01
    w[..., 9] = 0.02
    model.params["block1_conv2"] = (w, b)
    x = torch.zeros(1, 224, 224, 8)
    x[..., :3] = 40.0
    res = Occlusion(DeconvNet(model.build("cpu", torch.float32))).run(x, "block1_conv2", 112, 112)
    assert sorted(res.filters[0].tolist()) == [-1, -1, 5, 9]
    for k in range(4):
        tile = res.mosaic[0, (k // 2) * 224:(k // 2 + 1) * 224, (k % 2) * 224:(k % 2 + 1) * 224]
        if int(res.filters[0, k]) < 0:
            assert not bool(tile.any()) and not bool(res.heat[0, k].any()) and not bool(res.scores[0, :, k].any())
        else:
            assert bool(tile.any())


def test_engine_refusals(net, x224):
    occ = Occlusion(net)
    with pytest.raises(UnknownLayerError):
        occ.run(x224, "nope")
    with pytest.raises(UnknownLayerError):
        occ.run(x224, "input_1")
    with pytest.raises(ValueError):
        occ.run(x224, "block1_conv2", patch=16, stride=12)  # 19 x 19 patches
    with pytest.raises(ValueError):
        occ.run(x224[0], "block1_conv2")
