"""Laplacian-pyramid gradient normalisation in the engine (engine/deepdream.py: DreamSettings.lap_levels): the
torch tail on the CPU, and on the GPU the fused step with the dream_lap kernels against the torch-tail step,
graph replay against eager, the graph / state cache key, and lapnorm together with a guide."""
import pytest
import torch

import deconv_api_amd.engine.deepdream as deepdream_mod
from deconv_api_amd.engine.deepdream import DeepDream, DreamSettings, TiledDeepDream
from deconv_api_amd.models.inception_v3 import InceptionV3
from deconv_api_amd.ops import lapnorm
from deconv_api_amd.ops.autograd import premasked_grads


@pytest.fixture(scope="module")
def inc_cpu():
    return InceptionV3(0).build("cpu")


def _rand(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm()))


# --------------------------------------------------------------------------- CPU
def test_loss_and_grad_applies_the_reference(inc_cpu):
    """loss_and_grad with lap_levels = the raw input gradient, lap-normalised by the torch reference, divided by
    its mean magnitude; the loss is untouched and the gradient differs from the plain one."""
    x = _rand((2, 100, 110, 3), 1)
    dd = DeepDream(inc_cpu, DreamSettings(lap_levels=3))
    loss, g = dd.loss_and_grad(x)
    xin = dd._net_input(x).requires_grad_(True)
    with premasked_grads():
        acts = inc_cpu.forward(xin, list(dd.s.layers))
    (raw,) = torch.autograd.grad(dd.loss(acts).sum(), xin)
    want = lapnorm.normalize_ref(raw[..., :3].float(), 3)
    want = want / want.abs().mean(dim=(1, 2, 3), keepdim=True).clamp_min(1e-7)
    assert torch.equal(g, want)
    loss0, g0 = DeepDream(inc_cpu, DreamSettings()).loss_and_grad(x)
    assert torch.equal(loss, loss0) and _cos(g, g0) < 0.9
    # what lapnorm is for: the share of the step in the lowest band grows
    low = lambda t: float(lapnorm.split_ref(t, 3)[0].square().sum() / t.square().sum())  # noqa: E731
    assert low(g) > 10 * low(g0)


def test_run_with_lap_levels_differs_from_plain(inc_cpu):
    x = _rand((1, 100, 100, 3), 2)
    plain = DeepDream(inc_cpu, DreamSettings(octaves=2, iterations=2)).run(x)
    lap = DeepDream(inc_cpu, DreamSettings(octaves=2, iterations=2, lap_levels=4)).run(x)
    assert lap.shape == x.shape and torch.isfinite(lap).all()
    assert (lap - x).abs().max() > 1e-3 and (lap - plain).abs().max() > 1e-3
    for bad in (-1, 6, 2.0, True):
        with pytest.raises(ValueError, match="lap_levels"):
            DeepDream(inc_cpu, DreamSettings(octaves=1, iterations=1, lap_levels=bad)).run(x)


def test_tiled_engine_refuses_lap_levels(inc_cpu):
    t = TiledDeepDream(inc_cpu, DreamSettings(octaves=1, iterations=1, lap_levels=2), tile=64)
    with pytest.raises(ValueError, match="lap_levels is not supported by the tiled engine"):
        t.run(_rand((1, 100, 100, 3), 3))
    with pytest.raises(ValueError, match="lap_levels is not supported by the tiled engine"):
        t.dream_u8(torch.zeros(1, 100, 100, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="lap_levels is not supported by the tiled engine"):
        next(t.octave_steps(_rand((1, 100, 100, 3), 3)))


# --------------------------------------------------------------------------- GPU
def _torch_tail(ref, x, split, guide=None):
    """The torch-tail engine on the sub-batches the fused engine runs (see tests/test_dream_guide.py:_torch_tail:
    the network's input-gradient kernels round differently at another batch size)."""
    if guide is None:
        return torch.cat([ref.run(xc) for xc in x.chunk(split)])
    return torch.cat([ref.run(xc, guide) for xc in x.chunk(split)])


@pytest.mark.gpu
def test_gpu_lap_fused_step_equals_unfused(native_lib):
    """One fused step with lap_levels = 4 (lap_split / lap_merge kernels between the network's backward and
    dream_update) against the torch-tail step (the torch reference, rounded to the engine's dtype like the fused
    16-bit gradient), with the bounds of test_gpu_fused_step_equals_unfused (tests/test_deepdream.py), eager and
    graph-replayed, with and without loss taps."""
    net = InceptionV3(0).build("cuda")
    x = _rand((2, 150, 150, 3), 6).cuda()
    for max_loss in (None, 1e-9):  # 1e-9: every image stops at its first step (device-side flag)
        s = DreamSettings(iterations=1, octaves=1, max_loss=max_loss, lap_levels=4)
        ref = DeepDream(net, s, use_graphs=False)
        ref.fused = False
        want = _torch_tail(ref, x, DeepDream(net, s).split)
        got = {}
        for graphs in (False, True):
            for taps in (False, True):
                deepdream_mod.TAPS = taps
                try:
                    dd = DeepDream(net, s, use_graphs=graphs)
                    assert dd.fused
                    got[graphs, taps] = r = dd.run(x)
                finally:
                    deepdream_mod.TAPS = True
                d = float((r - want).abs().max())
                c = _cos(r - x, want - x) if max_loss is None else 1.0
                print(f"lap max_loss={max_loss} graphs={graphs} taps={taps}: max diff {d:.3g} cos {c:.6f}")
                if max_loss is not None or not taps:
                    assert d < 1e-4, (max_loss, graphs, taps)
                else:  # loss taps sum the loss gradient in fp32 (one rounding, not two)
                    assert c > 0.9999 and d < 1e-2, (graphs, taps)
        assert (got[True, True] - got[False, True]).abs().max() < 1e-3, max_loss
        if max_loss is None:
            assert (want - x).abs().max() > 1e-3
            plain = DeepDream(net, DreamSettings(iterations=1, octaves=1, max_loss=None)).run(x)
            assert (plain - want).abs().max() > 1e-3  # lapnorm changes the step


@pytest.mark.gpu
def test_gpu_lap_graph_replay_equals_eager(native_lib):
    net = InceptionV3(0).build("cuda")
    s = DreamSettings(iterations=3, octaves=2, lap_levels=4)
    x = _rand((2, 150, 150, 3), 3).cuda()
    eager = DeepDream(net, s, use_graphs=False).run(x)
    dd = DeepDream(net, s, use_graphs=True)
    graph = dd.run(x)
    d = float((eager - graph).abs().max())
    print(f"lap graph vs eager: max diff {d:.3g}")
    assert d < 1e-3 and (graph - x).abs().max() > 1e-3
    n = len(dd._graphs)
    again = dd.run(x)
    assert len(dd._graphs) == n, "a second run of the same shapes captured new graphs"
    assert (again - graph).abs().max() < 1e-3


@pytest.mark.gpu
def test_gpu_plain_after_lap_is_the_fresh_engines_result(native_lib):
    """A dream with lap_levels = 4 and then one with 0 on the same engine and shape: the second equals a fresh
    engine's result bit for bit (lap_levels is part of the state / graph cache key), and going back to 4 finds
    the lapnorm graphs again."""
    net = InceptionV3(0).build("cuda")
    x = _rand((2, 150, 150, 3), 8).cuda()
    fresh = DeepDream(net, DreamSettings(iterations=2, octaves=2)).run(x)
    dd = DeepDream(net, DreamSettings(iterations=2, octaves=2, lap_levels=4))
    lap = dd.run(x)
    n = len(dd._graphs)
    dd.s.lap_levels = 0
    after = dd.run(x)
    print(f"plain after lap vs fresh: max diff {float((after - fresh).abs().max()):.3g}")
    assert len(dd._graphs) == 2 * n
    assert torch.equal(after, fresh)
    assert (lap - fresh).abs().max() > 1e-2
    dd.s.lap_levels = 4
    assert (dd.run(x) - lap).abs().max() < 1e-3 and len(dd._graphs) == 2 * n


@pytest.mark.gpu
def test_gpu_guided_lap_runs(native_lib):
    """Guide and lapnorm together: the fused step against the torch tail (one step, no taps: the bound above),
    and it differs from either alone."""
    net = InceptionV3(0).build("cuda")
    x, guide = _rand((2, 150, 150, 3), 4).cuda(), _rand((1, 120, 160, 3), 5).cuda()
    s = DreamSettings(iterations=1, octaves=1, max_loss=None, lap_levels=4)
    ref = DeepDream(net, s, use_graphs=False)
    ref.fused = False
    dd = DeepDream(net, s)
    want = _torch_tail(ref, x, dd.split, guide)
    got = dd.run(x, guide)
    d, c = float((got - want).abs().max()), _cos(got - x, want - x)
    print(f"guided lap: max diff {d:.3g} cos {c:.6f}")
    assert torch.isfinite(got).all() and c > 0.9999 and d < 1e-2
    assert (got - dd.run(x)).abs().max() > 1e-3
    s0 = DreamSettings(iterations=1, octaves=1, max_loss=None)
    assert (got - DeepDream(net, s0).run(x, guide)).abs().max() > 1e-3
