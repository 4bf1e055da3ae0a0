"""GPU: engine/activations.py on the HIP VGG16 (one forward of three images), its heat against the oracle on the
forward's own output bits, and against the fp32 CPU engine."""
import pytest
import torch

import actmap_oracle as A
import occlusion_oracle as O
from deconv_api_amd import ops
from deconv_api_amd.engine.activations import ActivationMaps
from deconv_api_amd.engine.deconvnet import DeconvNet
from deconv_api_amd.models.vgg16 import VGG16

pytestmark = pytest.mark.gpu
BF, HF = torch.bfloat16, torch.float16


@pytest.fixture(scope="module")
def model():
    return VGG16.random(0, include_top=False)


@pytest.fixture(scope="module")
def nets(model, native_lib):
    return {BF: DeconvNet(model.build("cuda", BF)), HF: DeconvNet(model.build("cuda", HF))}


@pytest.fixture(scope="module")
def x3():
    """Three distinct images as the fp32 network input [3, 224, 224, 8] (integer RGB minus the mean colour)."""
    x = torch.zeros(3, 224, 224, 8)
    x[..., :3] = torch.randint(0, 256, (3, 224, 224, 3), generator=torch.Generator().manual_seed(9)).float() - \
        torch.tensor(O.MEAN)
    return x


@pytest.mark.parametrize("layer,dt", [("block1_conv2", BF), ("block3_conv3", BF), ("block4_pool", BF),
                                      ("block5_conv3", BF), ("block3_conv3", HF)],
                         ids=["block1_conv2", "block3_conv3", "block4_pool", "block5_conv3", "fp16"])
def test_engine(nets, x3, layer, dt):
    """filters: those of ``select_filters`` on ONE ``forward`` call on the same input. heat: within 8 x 2^-24 max |a| of
    the oracle applied to that call's output bits. mosaic: every byte within one level of the float64 oracle on the
    float64 heat, at most 0.5 % of the bytes different."""
    net = nets[dt]
    x = x3.to(dt)
    res = ActivationMaps(net).run(x.cuda(), layer)
    torch.cuda.synchronize()
    assert res.filters.shape == (3, 4) and res.heat.shape == (3, 4, 224, 224) and res.mosaic.shape == (3, 448, 448, 3)
    out = net.forward(x.cuda(), layer).out
    idx, sums = net.select_filters(out, 4, "per_image")
    assert torch.equal(res.filters, idx) and torch.equal(res.sums, sums)
    assert bool((idx >= 0).all()), idx
    out, idx = out.cpu(), idx.cpu()
    ref = A.heat(out, idx, 224, A.heat_map_rows)
    u = A.within_bound(res.heat.cpu().numpy(), ref, out, idx)
    frac = A.overlay_within(res.mosaic.cpu().numpy(), ref, idx, x, A.overlay_rows)
    print(f"{layer} {dt}: heat {u:.3f} of the bound, {100 * frac:.4f} % of the mosaic's bytes differ")
    assert float(res.heat.abs().max()) > 0
    assert not torch.equal(res.mosaic[0], res.mosaic[1]) and not torch.equal(res.mosaic[1], res.mosaic[2])


def test_heat_against_the_cpu_engine(model, nets, x3):
    """GPU bf16 against the fp32 CPU engine on the same input, block3_conv1, the GPU's filters: heat is a convex
    combination of the layer output, so the forward bound of test_engine_gpu.py carries over:
    max |heat_gpu - heat_cpu| <= 5e-2 max |out_cpu|."""
    x = x3.to(BF)
    res = ActivationMaps(nets[BF]).run(x.cuda(), "block3_conv1")
    out = DeconvNet(model.build("cpu", torch.float32)).forward(x.float(), "block3_conv1").out
    heat, _ = ops.activation_heat(out, res.filters.cpu(), 224)
    err, amax = float((res.heat.cpu() - heat).abs().max()), float(out.abs().max())
    print(f"GPU bf16 against CPU fp32, block3_conv1: max |heat_gpu - heat_cpu| = {err:.4g} = {err / amax:.3g} max |out_cpu|")
    assert err <= 5e-2 * amax
