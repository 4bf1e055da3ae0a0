"""GPU: the KW3 / KW3P kernels staging their weights from the packed, line-contiguous image (ConvWeights.w_kw3,
ops/conv.py kw3_pack) against the same kernels reading the strided w_gemm (DV_KW3_BPACK=0). LDS receives the
same bytes either way, so every output is equal BIT FOR BIT. Each case asserts the kernel route and, through
conv_bpack(), that the first call did stage from the image and the second did not. The shapes are the smallest
that reach each way the piece offset can go wrong: a second column group (n0 != 0), odd K-step counts, both
tile shapes, the step-1 DMA issued ahead of the epilogue, stream-K ranges that start inside a tile."""
import pytest
import torch

from deconv_api_amd import ops
from deconv_api_amd.ops.conv import ConvWeights
from gpu_helpers import cus as _cus, route as _route, tune as _tune

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, HF = torch.bfloat16, torch.float16


def _cw(oc, c, bias=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(oc, c, 3, 3, generator=g) / (3 * c ** 0.5)).to(BF).float()
    b = (torch.randn(oc, generator=g) * 0.1).to(BF).float() if bias else None
    return ConvWeights(w, b, "fwd")


def _tile(OC):
    return "256x256" if OC % 256 == 0 else "512x128"


def _ab(lib, monkeypatch, run, route, packed=True):
    """run() with the packed image (default) and with DV_KW3_BPACK=0: same route, bit-equal outputs, and the
    binding's report of which B source the launch used."""
    got = run()
    assert _route() == route, _route()
    assert lib.conv_bpack() is packed
    monkeypatch.setenv("DV_KW3_BPACK", "0")
    base = run()
    assert _route() == route, _route()
    assert lib.conv_bpack() is False
    monkeypatch.delenv("DV_KW3_BPACK")
    outs = got if isinstance(got, tuple) else (got,)
    bases = base if isinstance(base, tuple) else (base,)
    for o, b in zip(outs, bases):
        assert o.shape == b.shape and torch.equal(o, b)
    return outs[0]


@pytest.mark.parametrize("epi", ["lds", "reg"])
@pytest.mark.parametrize("N,H,W,C,OC,dt", [(90, 14, 13, 96, 512, BF), (200, 28, 28, 32, 256, BF), (300, 20, 20, 64, 256, HF),
                                           (120, 36, 36, 64, 128, BF)])
def test_bpack_kw3p_plain(native_lib, monkeypatch, N, H, W, C, OC, dt, epi):
    """Persistent KW3P, whole tiles: the LDS-sliced epilogue and DV_KW3P_EPI=reg; both issue the next tile's
    step 1 ahead of their stores (PRE). Two column groups at OC = 512, 9 / 3 K steps (odd), the 512 x 128 tile."""
    monkeypatch.setenv("DV_KW3", "2")
    monkeypatch.setenv("DV_NO_KW3_SK", "1")
    if epi == "reg":
        monkeypatch.setenv("DV_KW3P_EPI", "reg")
    g = torch.Generator().manual_seed(N + C)
    xd = torch.randn(N, H, W, C, generator=g).to(dt).to(DEV)
    cw = _cw(OC, C)
    cwd = cw.to_device(DEV, dt)
    assert cwd.w_kw3 is not None and cwd.w_kw3.dtype == dt and cwd.w_kw3.numel() == cwd.OCpad * 9 * C
    with _tune(0, 1):
        got = _ab(native_lib, monkeypatch, lambda: ops.conv2d(xd, cwd, relu=True), f"kw3p {_tile(OC)} {epi}")
    ref = ops.conv2d(xd[:2].cpu().float(), cw, relu=True)
    assert float((got[:2].float().cpu() - ref).abs().max()) < 1e-2 * float(ref.abs().max())


def test_bpack_kw3p_512x128_second_column_group(native_lib, monkeypatch):
    """OC = 256 on the 512 x 128 tile (DV_KW3_TILE): n0 = 128 indexes the image by 16-row blocks, whatever BN.
    (K = 4608 and M x N > 3e6 keep the shape off the small-problem tiles without forcing DV_KW3.)"""
    monkeypatch.setenv("DV_KW3_TILE", "512x128")
    monkeypatch.setenv("DV_NO_KW3_SK", "1")
    N, H, W, C, OC = 10, 36, 36, 512, 256
    g = torch.Generator().manual_seed(5)
    xd = torch.randn(N, H, W, C, generator=g).to(BF).to(DEV)
    cw = _cw(OC, C)
    cwd = cw.to_device(DEV)
    with _tune(0, 1):
        got = _ab(native_lib, monkeypatch, lambda: ops.conv2d(xd, cwd, relu=True), "kw3p 512x128 lds")
    ref = ops.conv2d(xd[:1].cpu().float(), cw, relu=True)
    assert float((got[:1].float().cpu() - ref).abs().max()) < 1e-2 * float(ref.abs().max())


@pytest.mark.parametrize("N,H,W,C,OC,div", [(131, 10, 12, 32, 512, 1), (90, 28, 28, 96, 256, 2)])
def test_bpack_kw3p_unpool_out(native_lib, monkeypatch, N, H, W, C, OC, div):
    monkeypatch.setenv("DV_KW3", "2")
    monkeypatch.setenv("DV_NO_KW3_SK", "1")
    g = torch.Generator().manual_seed(N + W)
    xd = torch.relu(torch.randn(N, H, W, C, generator=g)).to(BF).to(DEV)
    cd = torch.randint(0, 4, (N // div, H, W, OC), generator=g, dtype=torch.uint8).to(DEV)
    cwd = _cw(OC, C, bias=False).to_device(DEV)
    kw = dict(relu=True, use_bias=False, unpool_out=cd, unpool_div=div)
    with _tune(0, 1):
        got = _ab(native_lib, monkeypatch, lambda: ops.conv2d(xd, cwd, **kw), f"kw3p {_tile(OC)} unpool")
    assert got.shape == (N, 2 * H, 2 * W, OC) and bool((got != 0).any())


@pytest.mark.parametrize("N,H,W,C,OC,div", [(300, 14, 14, 96, 512, 4), (600, 14, 14, 64, 256, 0)])
def test_bpack_kw3p_stream_k(native_lib, monkeypatch, N, H, W, C, OC, div):
    """Stream-K: a workgroup's range starts at K step k0 > 0 of a tile. Packed and strided split the same
    tiles at the same steps, so here too the outputs are equal bit for bit. N scales with the CU count as in
    test_kernels_gpu.py::test_conv_kw3p_stream_k."""
    G = _cus()
    N = -(-N * G // (256 * max(div, 1))) * max(div, 1)
    bm, bn = (256, 256) if OC % 256 == 0 else (512, 128)
    tiles = -(-N * H * W // bm) * (OC // bn)
    assert G < tiles < 4 * G, (tiles, G)
    if G % (OC // bn):
        pytest.skip(f"stream-K needs the {OC // bn} column groups to divide the device's {G} CUs")
    monkeypatch.setenv("DV_KW3", "2")
    g = torch.Generator().manual_seed(N + C + OC)
    xd = torch.relu(torch.randn(N, H, W, C, generator=g)).to(BF).to(DEV)
    cwd = _cw(OC, C, bias=div == 0).to_device(DEV)
    kw = dict(relu=True, use_bias=div == 0)
    if div:
        code = torch.randint(0, 4, (N // div, H, W, OC), generator=g, dtype=torch.uint8)
        kw.update(unpool_out=code.to(DEV), unpool_div=div)
    native_lib.sk_errors(True)
    with _tune(0, 1):
        got = _ab(native_lib, monkeypatch, lambda: ops.conv2d(xd, cwd, **kw),
                  f"kw3p {bm}x{bn} {'unpool' if div else 'lds'} sk")
    torch.cuda.synchronize()
    assert native_lib.sk_errors(True) == 0
    assert bool((got != 0).any())


@pytest.mark.parametrize("N,H,W,C,OC", [(2, 28, 28, 256, 256), (3, 14, 13, 96, 512)])
def test_bpack_kw3_nonpersistent(native_lib, monkeypatch, N, H, W, C, OC):
    """conv_dma_kw3_kernel (DV_KW3_VAR=0) with the fp32 epilogue and with accumulate."""
    monkeypatch.setenv("DV_KW3", "2")
    monkeypatch.setenv("DV_KW3_VAR", "0")
    g = torch.Generator().manual_seed(N + C)
    xd = torch.randn(N, H, W, C, generator=g).to(BF).to(DEV)
    cw = _cw(OC, C)
    cwd = cw.to_device(DEV)
    base = torch.randn(N, H, W, OC, generator=g).to(BF).to(DEV)
    with _tune(0, 1):
        f32 = _ab(native_lib, monkeypatch, lambda: ops.conv2d(xd, cwd, relu=False, epilogue="f32"), "kw3 256x256")
        _ab(native_lib, monkeypatch, lambda: ops.conv2d(xd, cwd, relu=False, out=base.clone(), accumulate=True),
            "kw3 256x256")
    ref = ops.conv2d(xd.cpu().float(), cw, relu=False, epilogue="f32")
    assert f32.dtype == torch.float32 and float((f32.cpu() - ref).abs().max()) < 1e-3 * float(ref.abs().max())


@pytest.mark.parametrize("N,H,W,C,OC", [(2, 16, 16, 8, 128), (2, 16, 16, 64, 64)])
def test_bpack_uncovered_conv(native_lib, monkeypatch, N, H, W, C, OC):
    """C = 8 / OC = 64: no image is built, the conv runs as before and reports 'not packed'."""
    monkeypatch.setenv("DV_KW3", "2")
    g = torch.Generator().manual_seed(C + OC)
    xd = torch.randn(N, H, W, C, generator=g).to(BF).to(DEV)
    cw = _cw(OC, C)
    cwd = cw.to_device(DEV)
    assert cwd.w_kw3 is None
    with _tune(0, 1):
        got = _ab(native_lib, monkeypatch, lambda: ops.conv2d(xd, cwd, relu=True), _route_of(xd, cwd), packed=False)
    ref = ops.conv2d(xd.cpu().float(), cw, relu=True)
    assert float((got.float().cpu() - ref).abs().max()) < 1e-2 * float(ref.abs().max())


def _route_of(xd, cwd):
    ops.conv2d(xd, cwd, relu=True)
    r = _route()
    assert not r.startswith("kw3"), r
    return r


def test_bpack_engine_block5_conv3(native_lib, monkeypatch):
    """Real-width VGG16 deconvnet: filters and mosaic are identical with and without the packed images."""
    from deconv_api_amd.engine.deconvnet import DeconvNet
    from deconv_api_amd.models.vgg16 import VGG16

    eng = DeconvNet(VGG16.random(0, include_top=False).build("cuda", BF))
    g = torch.Generator().manual_seed(3)
    x = torch.zeros(2, 224, 224, 8)
    x[..., :3] = torch.randint(0, 256, (2, 224, 224, 3), generator=g).float() - torch.tensor(ops.CAFFE_MEAN)
    x = x.to(BF).cuda()
    packed = eng.run(x, "block5_conv3", k=4)
    monkeypatch.setenv("DV_KW3_BPACK", "0")
    strided = eng.run(x, "block5_conv3", k=4)
    assert torch.equal(packed.filters, strided.filters)
    assert torch.equal(packed.mosaic, strided.mosaic)
