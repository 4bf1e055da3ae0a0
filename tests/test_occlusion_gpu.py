"""GPU: engine/occlusion.py on the HIP VGG16 (default grid, 170 variants as one forward), its drop maps against the
fp32 CPU engine, and POST /occlusion through a GPU DeconvService."""
import numpy as np
import pytest
import torch

import occlusion_oracle as O
from deconv_api_amd import ops
from deconv_api_amd.codec import make_data_url
from deconv_api_amd.config import Config
from deconv_api_amd.engine.deconvnet import DeconvNet
from deconv_api_amd.engine.occlusion import Occlusion
from deconv_api_amd.models.vgg16 import VGG16
from deconv_api_amd.serve.service import DeconvService

pytestmark = pytest.mark.gpu
BF, HF = torch.bfloat16, torch.float16


@pytest.fixture(scope="module")
def model():
    return VGG16.random(0)


@pytest.fixture(scope="module")
def nets(model, native_lib):
    return {BF: DeconvNet(model.build("cuda", BF)), HF: DeconvNet(model.build("cuda", HF))}


@pytest.mark.parametrize("layer,dt", [("block3_conv1", BF), ("block4_pool", BF), ("predictions", BF),
                                      ("block3_conv1", HF)], ids=["block3_conv1", "block4_pool", "predictions", "fp16"])
def test_engine_default_grid(nets, layer, dt):
    """scores: bit for bit the channel sums (unit values for a dense target) of ONE DeconvNet.forward call on the
    oracle's 170 variants, the same call on the same batch. heat against the oracle applied to the engine's own
    scores: the default grid's covering counts are 1, 2 and 4, so the division is exact and what remains is the fp32
    rounding of each drop (one) and of the running sum of n <= 4 drops d (n - 1): the sum is off by at most
    n 2^-24 sum|d|, so |heat - ref| <= 2^-24 sum|d| <= 4 x 2^-24 max|d| (first order; max over the filter's 169
    drops)."""
    net = nets[dt]
    x0, xv = O.default_variants(dt)
    res = Occlusion(net).run(x0.cuda(), layer)
    torch.cuda.synchronize()
    assert res.scores.shape == (1, 170, 4) and res.heat.shape == (1, 4, 224, 224) and res.mosaic.shape == (1, 448, 448, 3)
    out = net.forward(xv.cuda(), layer).out
    sums = ops.channel_sum(out) if out.dim() == 4 else out.float()
    assert torch.equal(res.filters, net.select_filters(out[:1], 4)[0])
    f = res.filters[0].long()
    assert bool((f >= 0).all()), res.filters
    assert torch.equal(res.scores[0], sums[:, f])
    sc = res.scores[0].cpu().numpy()
    want = O.heat(sc, np.arange(4), 224, 32, 16)
    dmax = np.abs(sc[:1].astype(np.float64) - sc[1:].astype(np.float64)).max(axis=0)  # [4]
    err = np.abs(res.heat[0].double().cpu().numpy() - want).max(axis=(1, 2))
    print(f"{layer} {dt}: heat err {err}, bound {4 * 2.0 ** -24 * dmax}, max|d| / score {dmax / np.abs(sc[0])}")
    assert np.all(err <= 4 * 2.0 ** -24 * dmax)
    ref = O.overlay(res.heat[0].double().cpu().numpy(), res.filters[0].cpu().numpy(), x0[0].float().numpy())
    d = np.abs(res.mosaic[0].cpu().numpy().astype(int) - ref.astype(int))
    assert d.max() <= 1 and (d != 0).mean() <= 0.005


def _cos(a, b):
    return float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


def test_drop_maps_against_the_cpu_engine(model, nets):
    """GPU (bf16) against the fp32 CPU forward on the same 17 variants (patch = stride = 56), block3_conv1, the GPU's
    filters: cosine of the drop maps d[k] >= 0.98 (the project's bound for each-runs-its-own-forward comparisons,
    test_engine_gpu.py) for every k whose CPU max |d| exceeds 1 % of score[0, f_k]."""
    x0, _ = O.default_variants(BF)
    res = Occlusion(nets[BF]).run(x0.cuda(), "block3_conv1", 56, 56)
    cpu = DeconvNet(model.build("cpu", torch.float32))
    xv = torch.from_numpy(O.variants(x0[0].float().numpy(), 56, 56))
    sums = ops.channel_sum(cpu.forward(xv, "block3_conv1").out).double().numpy()
    sg = res.scores[0].double().cpu().numpy()
    used = 0
    for k, f in enumerate(res.filters[0].tolist()):
        dc, dg = sums[0, f] - sums[1:, f], sg[0, k] - sg[1:, k]
        rel = np.abs(dc).max() / abs(sums[0, f])
        c = _cos(dc, dg)
        print(f"drop-map cosine k {k} filter {f}: {c:.5f} (CPU max|d| / score {rel:.4f})")
        if rel > 0.01:
            used += 1
            assert c >= 0.98, (k, f, c)
    assert used >= 1


def test_service_occlusion_then_deconv(model, nets):
    """POST /occlusion through a GPU DeconvService (queue, worker, staging ring, copy-back, encoder), then POST /: the
    POST / bytes equal those of a fresh service."""
    from fastapi.testclient import TestClient

    from deconv_api_amd.api.app import create_app
    from deconv_api_amd.codec import parse_result_data_url

    img = np.random.default_rng(3).integers(0, 256, (240, 300, 3), dtype=np.uint8)
    form = {"file": make_data_url(img, "PNG"), "layer": "block5_conv3"}
    cfg = Config.from_env(device="cuda")

    def serve(with_occlusion):
        svc = DeconvService(cfg, engine=nets[BF])
        try:
            with TestClient(create_app(svc, cfg)) as c:
                if with_occlusion:
                    first = c.post("/occlusion", data=form)
                    assert first.status_code == 200, first.text[:300]
                    first = first.json()
                else:  # the engine's mosaic for the same image
                    first = Occlusion(nets[BF]).run(svc.preprocess([img]), "block5_conv3").mosaic[0].cpu().numpy()
                r = c.post("/", data=form)
                assert r.status_code == 200
                return first, r.content
        finally:
            svc.close()

    occ, after = serve(True)
    want, fresh = serve(False)
    assert after == fresh and occ.encode() not in after
    rgb = parse_result_data_url(occ).astype(int)
    assert rgb.shape == (448, 448, 3) and rgb.std() > 1.0
    # it is the engine's mosaic, in true RGB
    assert np.abs(rgb - want.astype(int)).mean() < np.abs(rgb - want[..., ::-1].astype(int)).mean()
