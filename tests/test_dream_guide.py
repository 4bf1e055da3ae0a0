"""Guided DeepDream in the engine (engine/deepdream.py: DeepDream.run(x, guide), loss_and_grad(x, guide_feats)):
the torch form on the CPU, and on the GPU the fused step with the guide_match kernel against the torch-tail
step, graph replay against eager, and no guide leaking through the graph cache."""
import pytest
import torch

import deconv_api_amd.engine.deepdream as deepdream_mod
from deconv_api_amd.engine.deepdream import (RESNET_LAYERS, DeepDream, DreamSettings, GuideFeatures,
                                              TiledDeepDream)
from deconv_api_amd.models.inception_v3 import InceptionV3
from deconv_api_amd.models.resnet50 import ResNet50
from deconv_api_amd.ops import autograd as AG


@pytest.fixture(scope="module")
def inc_cpu():
    return InceptionV3(0).build("cpu")


def _rand(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm()))


# --------------------------------------------------------------------------- CPU
def test_guide_core_gradient_is_the_argmax_row():
    """guide_core's gradient by autograd equals y[argmax] gathered by a naive loop (lowest q on ties, which the
    {0, 1, 2} operands produce), zero on the border; the loss is the sum of the winning scores."""
    g = torch.Generator().manual_seed(1)
    N, H, W, C, Q, b = 2, 6, 7, 8, 9, 1
    a = torch.randint(0, 3, (N, H, W, C), generator=g).float().requires_grad_(True)
    y = torch.randint(0, 3, (2, Q, C), generator=g).float()
    gidx = AG.guide_index([1, 0], 2, "cpu")
    loss = AG.guide_core(a, y, gidx, b)
    (ga,) = torch.autograd.grad(loss.sum(), a)
    want, wloss, ties = torch.zeros(N, H, W, C), torch.zeros(N), 0
    for n in range(N):
        yy = y[int(gidx[n])]
        for h in range(b, H - b):
            for w in range(b, W - b):
                s = [float(a[n, h, w].detach() @ yy[q]) for q in range(Q)]
                q = s.index(max(s))  # the first maximum
                ties += s.count(max(s)) > 1
                want[n, h, w] = yy[q]
                wloss[n] += s[q]
    assert ties > 0
    assert torch.equal(ga, want) and torch.equal(loss.detach(), wloss)


def test_guided_run_changes_the_image_and_differs_from_unguided(inc_cpu):
    s = DreamSettings(octaves=2, iterations=2, guide_size=96)
    x, guide = _rand((2, 110, 110, 3), 2), _rand((2, 80, 120, 3), 3)
    plain = DeepDream(inc_cpu, s).run(x)
    guided = DeepDream(inc_cpu, s).run(x, guide)
    assert guided.shape == x.shape and torch.isfinite(guided).all()
    assert (guided - x).abs().max() > 1e-3 and (guided - plain).abs().max() > 1e-3
    other = DeepDream(inc_cpu, s).run(x, _rand((2, 80, 120, 3), 4))
    assert (guided - other).abs().max() > 1e-3  # the guide matters, not only the objective
    with pytest.raises(ValueError):
        DeepDream(inc_cpu, s).run(x, _rand((3, 80, 80, 3), 5))  # G must be 1 or B


def test_shared_guide_equals_the_guide_repeated(inc_cpu):
    s = DreamSettings(octaves=1, iterations=2, guide_size=96)
    x, guide = _rand((3, 100, 100, 3), 6), _rand((1, 90, 70, 3), 7)
    dd = DeepDream(inc_cpu, s)
    one = dd.run(x, guide)
    rep = dd.run(x, guide.expand(3, -1, -1, -1))
    assert (one - rep).abs().max() < 1e-4  # (the guide's forward at batch 1 and 3 rounds differently on the CPU)
    f1 = dd.guide_features(guide, 3)
    # the same features as three guides, one per row: the same loss and gradient, exactly
    f3 = GuideFeatures({n: f.repeat(3, 1, 1) for n, f in f1.feats.items()}, AG.guide_index(range(3), 3, "cpu"))
    (l1, g1), (l3, g3) = dd.loss_and_grad(x, f1), dd.loss_and_grad(x, f3)
    assert torch.equal(l1, l3) and torch.equal(g1, g3)
    assert f1.gidx.tolist() == [0, 0, 0] and all(f.shape[0] == 1 for f in f1.feats.values())
    # the features cover the WHOLE guide map (no border crop), at guide_size
    acts = inc_cpu.forward(torch.zeros(1, 96, 96, 8), list(s.layers))
    assert {n: f.shape[1] for n, f in f1.feats.items()} == {n: a.shape[1] * a.shape[2] for n, a in acts.items()}


def test_dream_u8_takes_a_guide(inc_cpu):
    s = DreamSettings(octaves=1, iterations=1, guide_size=96)
    g = torch.Generator().manual_seed(8)
    img = torch.randint(0, 256, (1, 100, 100, 3), generator=g, dtype=torch.uint8)
    guide = torch.randint(0, 256, (1, 64, 64, 3), generator=g, dtype=torch.uint8)
    dd = DeepDream(inc_cpu, s)
    a, b = dd.dream_u8(img), dd.dream_u8(img, guide)
    assert a.dtype == b.dtype == torch.uint8 and a.shape == b.shape == img.shape and not torch.equal(a, b)


def test_tiled_engine_refuses_a_guide(inc_cpu):
    t = TiledDeepDream(inc_cpu, DreamSettings(octaves=1, iterations=1), tile=64)
    with pytest.raises(ValueError, match="guide is not supported by the tiled engine"):
        t.run(_rand((1, 100, 100, 3), 9), _rand((1, 80, 80, 3), 10))
    with pytest.raises(ValueError, match="guide is not supported by the tiled engine"):
        t.dream_u8(torch.zeros(1, 100, 100, 3, dtype=torch.uint8), torch.zeros(1, 80, 80, 3, dtype=torch.uint8))


# --------------------------------------------------------------------------- GPU
def _torch_tail(ref, x, guide, split):
    """The torch-tail engine ``ref`` on the sub-batches the fused engine runs (DeepDream.run splits a batch
    into ``split`` sub-batches, the torch-tail path never does). The network's input-gradient kernels round
    differently at another batch size, and a normalized one-step update turns one 16-bit ulp of a peak gradient
    value into more than the bound below; measured on an MI355X, 2 x 150 x 150, one step, no taps, the
    torch-tail step on the whole batch against ITSELF on the two images one by one: 3.9e-4 guided (6.9e-5
    unguided), and exactly that figure for the fused step against the whole-batch torch tail, while on equal
    batches fused and torch-tail differ by 1.2e-7. So the reference runs on the fused engine's sub-batches."""
    if guide.shape[0] == 1:
        return torch.cat([ref.run(xc, guide) for xc in x.chunk(split)])
    return torch.cat([ref.run(xc, gc) for xc, gc in zip(x.chunk(split), guide.chunk(split))])


def _guided_pairs(net, x, guide, layers=None):
    """The bounds of test_gpu_fused_step_equals_unfused (tests/test_deepdream.py) on the guided pair: fused
    step (guide_match as loss tap / root) against the torch-tail step (dd.fused = False: guide_core through
    autograd), eager and graph-replayed."""
    for max_loss in (None, 1e-9):  # 1e-9: every image stops at its first step (device-side flag)
        for iters, octs in ((1, 1), (3, 2)):
            s = DreamSettings(iterations=iters, octaves=octs, max_loss=max_loss)
            if layers:
                s.layers = dict(layers)
            ref = DeepDream(net, s, use_graphs=False)
            ref.fused = False
            want = _torch_tail(ref, x, guide, DeepDream(net, s).split)
            got = {}
            for graphs in (False, True):
                for taps in (False, True):
                    deepdream_mod.TAPS = taps
                    try:
                        dd = DeepDream(net, s, use_graphs=graphs)
                        assert dd.fused
                        got[graphs, taps] = r = dd.run(x, guide)
                    finally:
                        deepdream_mod.TAPS = True
                    d = float((r - want).abs().max())
                    if max_loss is not None or (iters == 1 and not taps):
                        print(f"guided max_loss={max_loss} iters={iters} graphs={graphs} taps={taps}: max diff {d:.3g}")
                        assert d < 1e-4, (max_loss, graphs, taps)
                    elif iters == 1:  # loss taps sum the loss gradient in fp32 (one rounding, not two)
                        c = _cos(r - x, want - x)
                        print(f"guided iters=1 graphs={graphs} taps={taps}: cos {c:.6f} max diff {d:.3g}")
                        assert c > 0.9999 and d < 1e-2, (graphs, taps)
                    else:  # later steps feed 16-bit-rounded inputs to a chaotic map: same dream direction
                        c = _cos(r - x, want - x)
                        print(f"guided iters={iters} graphs={graphs} taps={taps}: cos {c:.4f}")
                        assert c > 0.9, (max_loss, graphs, taps)
            # the captured graph replays exactly the eager fused steps
            assert (got[True, True] - got[False, True]).abs().max() < 1e-3, (max_loss, iters)
            if max_loss is None:
                assert (want - x).abs().max() > 1e-3


@pytest.mark.gpu
def test_gpu_guided_fused_step_equals_unfused(native_lib):
    net = InceptionV3(0).build("cuda")
    _guided_pairs(net, _rand((2, 150, 150, 3), 6).cuda(), _rand((2, 120, 160, 3), 7).cuda())


@pytest.mark.gpu
def test_gpu_guided_fused_step_equals_unfused_resnet_fp16(native_lib):
    net = ResNet50(0).build("cuda", torch.float16)
    x, guide = _rand((2, 128, 128, 3), 4), _rand((1, 100, 100, 3), 5)
    x = x.to(torch.float16).float().cuda()
    s = DreamSettings(layers=dict(RESNET_LAYERS), iterations=1, octaves=1, max_loss=None)
    ref = DeepDream(net, s, use_graphs=False)
    assert ref.dtype == torch.float16
    ref.fused = False
    want = _torch_tail(ref, x, guide.cuda(), DeepDream(net, s).split)
    for graphs in (False, True):
        r = DeepDream(net, s, use_graphs=graphs).run(x, guide.cuda())
        c, d = _cos(r - x, want - x), float((r - want).abs().max())
        print(f"guided resnet fp16 graphs={graphs}: cos {c:.6f} max diff {d:.3g}")
        assert c > 0.9999 and d < 1e-2, graphs
    assert (want - x).abs().max() > 1e-3


@pytest.mark.gpu
def test_gpu_guided_graph_replay_equals_eager(native_lib):
    net = InceptionV3(0).build("cuda")
    s = DreamSettings(iterations=3, octaves=2)
    x, guide = _rand((2, 150, 150, 3), 3).cuda(), _rand((1, 200, 170, 3), 4).cuda()
    eager = DeepDream(net, s, use_graphs=False).run(x, guide)
    dd = DeepDream(net, s, use_graphs=True)
    graph = dd.run(x, guide)
    assert (eager - graph).abs().max() < 1e-3
    assert (graph - x).abs().max() > 1e-3
    # a replay reads the guide of THIS run: another guide through the same cached graphs
    guide2 = _rand((1, 200, 170, 3), 5).cuda()
    n = len(dd._graphs)
    again = dd.run(x, guide2)
    assert len(dd._graphs) == n, "a second guided run of the same shapes captured new graphs"
    assert (again - DeepDream(net, s, use_graphs=False).run(x, guide2)).abs().max() < 1e-3
    assert (again - graph).abs().max() > 1e-3


@pytest.mark.gpu
def test_gpu_unguided_after_guided_does_not_leak_the_guide(native_lib):
    """An unguided run on an engine that has run guided equals an unguided run on a fresh engine:
    the guided graphs live under their own cache keys."""
    net = InceptionV3(0).build("cuda")
    s = DreamSettings(iterations=2, octaves=2)
    x, guide = _rand((2, 150, 150, 3), 8).cuda(), _rand((2, 120, 120, 3), 9).cuda()
    fresh = DeepDream(net, s).run(x)
    dd = DeepDream(net, s)
    guided = dd.run(x, guide)
    after = dd.run(x)
    assert (after - fresh).abs().max() < 1e-3  # (the bound of graph replay against eager)
    assert (guided - fresh).abs().max() > 1e-2
    assert (dd.run(x, guide) - guided).abs().max() < 1e-3  # and back: the guided graphs still are the guided ones
